// fx_fastq_trim.hpp -- FASTQ read trimming and trimmed-record output on the resident stream for gfx950 (MI355X, wave64).
// Extension: the reference has no trimming and writes no records other than verbatim copies (Read.raw, read.c:124-150).
//
// Both passes read the `rlen` bytes at `soff` and at `qoff` of the read table -- the bytes k_fastq_fetch returns, a byte
// past the end of the stream reads as 0.  Everything is integer and exact; the definition is the one of include/fxgpu.h.
//
//   k_fq_trim<NW>   the lane-group layout of k_fq_read_stats: lpr lanes per read, 64 / lpr reads side by side per wave, one
//        16-byte piece of each line per lane (qc_load16), the table row fetched one iteration ahead, `ids` makes it a
//        gather.  The host picks lpr = ceil(longest read / 16), so a read of up to 1024 bytes lies in the registers of its
//        lane group at once and every step below is a few cross-lane operations on it; the steps run in their fixed order,
//        each ends in one minimum / maximum down the lane group that is handed back to all its lanes.  A step that was
//        not asked for is skipped by a wave-uniform branch (the adapter step by the template argument).
//          adapter (NW = 16-letter words of the adapter, 0: none)  a piece is packed to 2 bits per base ((b >> 1) & 3:
//            A 0, C 1, T 2, G 3) plus one "not A C G T" bit per base, both spread over a 32-bit word; the NW pieces behind
//            a lane's own come from its neighbours by ds_bpermute.  An offset then costs, per word, two v_alignbit (the
//            window of codes and of flags), an XOR against the packed adapter (kernel arguments, SGPRs), the mask of the
//            letters that count (not N, inside the overlap) and a popcount.
//          5' / 3' quality  a 16-bit mask "byte >= threshold" per piece (the borrow of a packed 16-bit subtraction on the
//            even and odd bytes), cut to the interval, first / last set bit, group minimum / maximum of the position.
//          sliding window  the sum of a piece by v_sad_u8, an exclusive scan of the sums across the lane group: with
//            we = 16 k + r the window that starts at a lane's first byte sums to P[p + we] - P[p], the difference of the
//            scan value (plus the first r bytes) of the lane k further on and the lane's own -- a window that spans lanes
//            costs one ds_bpermute.  The lane's other 15 windows follow by adding the byte that enters (the 16 bytes at
//            p + we, one unaligned load that hits the cache: the neighbours loaded them) and dropping the one that leaves.
//        A read longer than 16 * lpr (only when the longest read has more than 1024 bytes) is walked by lane 0 of its
//        group byte by byte with the same rules: exact, slow, rare.
//   k_fq_format_count   one lane per query: the interval is checked against the read (first offender -> atomicMin), the
//        record's size is header + 2 x kept + 5, or 0 for a read shorter than min_len.  k_sscan_sums / k_sscan_top /
//        k_sscan_apply (fx_search.hpp) give the exclusive offsets, the total and the number of records kept.
//   k_fq_format_emit    one lane group per record: header, sequence slice, "\n+\n", quality slice, "\n" copied to the
//        record's offset -- up to the first 16-byte boundary of the destination byte by byte, then 16-byte stores fed by
//        unaligned 16-byte loads, then the tail.  No atomics, nothing sorted.
#pragma once
#include "fx_fastq_qc.hpp"

namespace fx {

struct TrimPar {
    int phred;
    int64_t clip_front, clip_tail;
    int alen, min_overlap;                   // alen = 0: no adapter
    int64_t err_num, err_den;
    uint32_t acode[4], acare[4];             // 2 bits per letter: the code; bit 0 of the pair: the letter counts (not N)
    int front_thr, tail_thr;                 // RAW byte thresholds phred + qual, capped at 256; < 0: not asked
    int win_len;                             // 0: not asked
    int64_t win_num, win_den;
};

constexpr int TRIM_NONE = 0x7FFFFFFF;

// a value down the lane group and back to every lane of it
template <class Op>
__device__ __forceinline__ int trim_group_all(int v, int lane, int grp, int sub, int lpr, int p2, Op op) {
    v = qc_group_reduce(v, lane, sub, lpr, p2, op);
    return __shfl(v, grp * lpr, 64);
}

// bit t set: byte t of the piece is >= thr (thr in 0..256)
__device__ __forceinline__ uint32_t trim_ge_mask16(const uint4 &v, int thr) {
    const uint32_t thr2 = (uint32_t)thr * 0x00010001u, w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t ev = __builtin_amdgcn_perm(0u, w[k], 0x0C020C00u), od = __builtin_amdgcn_perm(0u, w[k], 0x0C030C01u);
        const uint32_t ge = ((ev | 0x80008000u) - thr2) & 0x80008000u, go = ((od | 0x80008000u) - thr2) & 0x80008000u;
        m |= (((ge >> 15) & 1u) | ((go >> 14) & 2u) | ((ge >> 29) & 4u) | ((go >> 28) & 8u)) << (4 * k);
    }
    return m;
}
// bits lo..hi-1 of a 16-bit piece mask: the bytes of the piece at p that lie in [a, b)
__device__ __forceinline__ uint32_t trim_range16(int p, int a, int b) {
    const int lo = min(max(a - p, 0), 16), hi = min(max(b - p, 0), 16);
    return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}
// the first `m` letters (two bits each) of word k of a packed window
__device__ __forceinline__ uint32_t trim_len_mask(int m, int k) {
    const int mk = m - 16 * k;
    return mk >= 16 ? 0xFFFFFFFFu : mk <= 0 ? 0u : (1u << (2 * mk)) - 1u;
}

// One read by one lane, byte by byte: the definition as it stands.  For reads that do not fit their lane group.
__device__ __noinline__ void trim_serial(const uint8_t *__restrict__ data, int64_t n_bytes, int64_t so, int64_t qo, int64_t L,
                                         const TrimPar &P, int64_t *o_a, int64_t *o_b) {
    auto ldb = [&](int64_t off) -> uint32_t { return off >= 0 && off < n_bytes ? (uint32_t)data[off] : 0u; };
    int64_t a = min(P.clip_front, L), b = max(a, L - P.clip_tail);
    if (P.alen > 0) {
        for (int64_t j = a; j < b; ++j) {
            const int64_t m = min((int64_t)P.alen, b - j);
            if (m < P.min_overlap) break;
            int64_t mm = 0;
            for (int k = 0; k < (int)m; ++k) {
                const uint32_t c = ldb(so + j + k), sh = 2 * (k & 15);
                const uint32_t care = (P.acare[k >> 4] >> sh) & 1u, code = (P.acode[k >> 4] >> sh) & 3u;
                const bool exact = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                mm += care && (!exact || ((c >> 1) & 3u) != code) ? 1 : 0;
            }
            if (mm * P.err_den <= P.err_num * m) { b = j; break; }
        }
    }
    if (P.front_thr >= 0)
        while (a < b && (int)ldb(qo + a) < P.front_thr) ++a;
    if (P.win_len > 0 && b > a) {
        const int64_t we = min((int64_t)P.win_len, b - a);
        const unsigned __int128 rhs = (unsigned __int128)(uint64_t)we * (uint64_t)(P.win_num + (int64_t)P.phred * P.win_den);
        uint64_t sum = 0;
        for (int64_t k = 0; k < we; ++k) sum += ldb(qo + a + k);
        for (int64_t j = a;; ++j) {
            if ((unsigned __int128)sum * (uint64_t)P.win_den < rhs) { b = j; break; }
            if (j + we >= b) break;
            sum += ldb(qo + j + we);
            sum -= ldb(qo + j);
        }
    }
    if (P.tail_thr >= 0)
        while (b > a && (int)ldb(qo + b - 1) < P.tail_thr) --b;
    *o_a = a; *o_b = b;
}

template <int NW>
__global__ __launch_bounds__(BLOCK) void k_fq_trim(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                  const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                  const int64_t *__restrict__ qoff, const int64_t *__restrict__ ids, int64_t nq,
                                                  int lpr, TrimPar P, int64_t *__restrict__ o_start, int64_t *__restrict__ o_end) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    const bool any_q = P.front_thr >= 0 || P.win_len > 0 || P.tail_thr >= 0;
    const int p = sub * 16;                                    // this lane's piece: bytes p .. p + 15 of the read
    auto imin = [](int x, int y) { return x < y ? x : y; };
    auto imax = [](int x, int y) { return x > y ? x : y; };
    struct Row { int64_t n, so, qo; };
    auto get_row = [&](int64_t q) -> Row {                    // the table row of query q, one iteration ahead of its bytes
        Row r{0, 0, 0};
        if (live && q < nq) {
            const int64_t id = ids ? ids[q] : q;
            r.n = rlen[id]; r.so = soff[id] - gbase; r.qo = qoff[id] - gbase;
        }
        return r;
    };
    int64_t q = wave * ngrp + grp;
    Row nxt = get_row(q);
    for (; q - grp < nq; q += stride) {                       // wave-uniform trip count
        const Row row = nxt;
        nxt = get_row(q + stride);
        const int64_t L = row.n > 0 ? row.n : 0;
        const bool fits = L <= 16 * (int64_t)lpr;             // the whole read lies in the lane group's registers
        const bool mine = fits && p < L;
        uint4 vs = make_uint4(0, 0, 0, 0), vq = make_uint4(0, 0, 0, 0);
        if (NW > 0 && mine) vs = qc_load16(data, row.so + p, n_bytes);
        if (any_q && mine) vq = qc_load16(data, row.qo + p, n_bytes);
        const int Li = fits ? (int)L : 0;
        int a = (int)min(P.clip_front, (int64_t)Li);
        int b = (int)max((int64_t)a, (int64_t)Li - P.clip_tail);
        // ---- 2: 3' adapter
        if constexpr (NW > 0) {
            const uint32_t s[4] = {vs.x, vs.y, vs.z, vs.w};
            uint32_t cw[NW + 1], iw[NW + 1];
            cw[0] = 0; iw[0] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t z = zero_bytes(s[k] ^ __builtin_amdgcn_perm(QC_EX_HI, QC_EX_LO, (s[k] >> 1) & 0x07070707u));
                const uint32_t x = (s[k] >> 1) & 0x03030303u, y = (~z >> 7) & 0x01010101u;
                cw[0] |= ((x | (x >> 6) | (x >> 12) | (x >> 18)) & 0xFFu) << (8 * k);
                iw[0] |= ((y | (y >> 6) | (y >> 12) | (y >> 18)) & 0x55u) << (8 * k);
            }
#pragma unroll
            for (int k = 1; k <= NW; ++k) {                   // letters past the read's end are cut off by the overlap mask
                cw[k] = (uint32_t)__shfl((int)cw[0], lane + k, 64);
                iw[k] = (uint32_t)__shfl((int)iw[0], lane + k, 64);
            }
            int cand = TRIM_NONE;
            if (p + 16 > a && p < b && b - p >= P.min_overlap) {
                auto offsets = [&](auto full_tag) {
                    constexpr bool FULL = decltype(full_tag)::value;      // every offset of the piece sees the whole adapter
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int j = p + t, m = FULL ? P.alen : imin(P.alen, b - j);
                        uint32_t mm = 0;
#pragma unroll
                        for (int k = 0; k < NW; ++k) {
                            const uint32_t c = t ? __builtin_amdgcn_alignbit(cw[k + 1], cw[k], 2 * t) : cw[k];
                            const uint32_t v = t ? __builtin_amdgcn_alignbit(iw[k + 1], iw[k], 2 * t) : iw[k];
                            const uint32_t d = c ^ P.acode[k];
                            uint32_t x = (((d | (d >> 1)) & 0x55555555u) | v) & P.acare[k];
                            if (!FULL) x &= trim_len_mask(m, k);
                            mm += __popc(x);
                        }
                        const bool ok = j >= a && m >= P.min_overlap && (int64_t)mm * P.err_den <= P.err_num * (int64_t)m;
                        if (ok) cand = imin(cand, j);
                    }
                };
                if (b - p - 15 >= P.alen) offsets(std::true_type{});
                else offsets(std::false_type{});
            }
            cand = trim_group_all(cand, lane, grp, sub, lpr, p2, imin);
            if (cand < b) b = cand;
        }
        // ---- 3: 5' end
        if (P.front_thr >= 0) {
            const uint32_t m = trim_ge_mask16(vq, P.front_thr) & trim_range16(p, a, b);
            int cand = m ? p + (int)__builtin_ctz(m) : TRIM_NONE;
            cand = trim_group_all(cand, lane, grp, sub, lpr, p2, imin);
            a = imin(cand, b);
        }
        // ---- 4: sliding window
        if (P.win_len > 0) {
            const uint32_t w[4] = {vq.x, vq.y, vq.z, vq.w};
            const int we = imax(imin(P.win_len, b - a), 1), k = we >> 4, r = we & 15;
            uint32_t ps = 0, hs = 0;
            uint32_t head[4] = {vq.x, vq.y, vq.z, vq.w};
            fq_keep_first(head, r, 0u);
#pragma unroll
            for (int i = 0; i < 4; ++i) { ps = __builtin_amdgcn_sad_u8(w[i], 0u, ps); hs = __builtin_amdgcn_sad_u8(head[i], 0u, hs); }
            uint32_t inc = ps;                                 // inclusive scan of the piece sums across the lane group
            for (int d = 1; d < lpr; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
                if (sub >= d) inc += o;
            }
            const uint32_t E = inc - ps;                       // P[p]
            const uint32_t tot = (uint32_t)__shfl((int)inc, grp * lpr + lpr - 1, 64);
            uint32_t far_p = (uint32_t)__shfl((int)(E + hs), lane + k, 64);          // P[p + we], from the lane k further on
            if (sub + k >= lpr) far_p = tot;                   // the window ends with the last piece (r = 0), or is not a window of the read
            int cand = TRIM_NONE;
            const int tlo = imax(a - p, 0), thi = imin(b - we - p, 15);
            if (b > a && tlo <= thi) {
                const uint4 vf = qc_load16(data, row.qo + p + we, n_bytes);
                const uint32_t f[4] = {vf.x, vf.y, vf.z, vf.w};
                const uint64_t rhs = (uint64_t)we * (uint64_t)(P.win_num + (int64_t)P.phred * P.win_den);
                uint32_t D = far_p - E;                        // the sum of q[j .. j + we) at j = p
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    if (t >= tlo && t <= thi && (uint64_t)D * (uint64_t)P.win_den < rhs) cand = imin(cand, p + t);
                    D += (f[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                    D -= (w[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                }
            }
            cand = trim_group_all(cand, lane, grp, sub, lpr, p2, imin);
            if (cand < b) b = cand;
        }
        // ---- 5: 3' end
        if (P.tail_thr >= 0) {
            const uint32_t m = trim_ge_mask16(vq, P.tail_thr) & trim_range16(p, a, b);
            int cand = m ? p + 32 - (int)__builtin_clz(m) : -1;
            cand = trim_group_all(cand, lane, grp, sub, lpr, p2, imax);
            b = cand < 0 ? a : cand;
        }
        if (live && sub == 0 && q < nq) {
            int64_t ra = a, rb = b;
            if (!fits) trim_serial(data, n_bytes, row.so, row.qo, L, P, &ra, &rb);
            o_start[q] = ra; o_end[q] = rb;
        }
    }
}

// ------------------------------------------------------------------ formatted records
struct FmtLdCnt {                             // bytes of the record, "the record is there"
    const int64_t *p;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = p[i]; v[1] = p[i] > 0; }
};

__global__ __launch_bounds__(BLOCK) void k_fq_format_count(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                          const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                          const int32_t *__restrict__ dlen, const int64_t *__restrict__ ids, int64_t nq,
                                                          const int64_t *__restrict__ start, const int64_t *__restrict__ end, int64_t min_len,
                                                          int64_t *__restrict__ cnt, unsigned long long *__restrict__ bad) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    const int64_t id = ids ? ids[q] : q, L = rlen[id] > 0 ? rlen[id] : 0;
    const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
    if (a < 0 || a > b || b > L) { atomicMin(bad, (unsigned long long)q); cnt[q] = 0; return; }
    int64_t hl = dlen[id] > 0 ? dlen[id] : 0;
    const int64_t last = soff[id] - gbase - 2;                // the header's last byte: one trailing '\r' is not part of it
    if (hl > 0 && last >= 0 && last < n_bytes && data[last] == 13) --hl;
    cnt[q] = b - a < min_len ? 0 : hl + 2 * (b - a) + 5;
}

// len bytes of the stream from src on (a byte outside the stream is 0) to dst, by the lanes sub, sub + lpr, ... of a group
__device__ __forceinline__ void fmt_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ data, int64_t src, int64_t len,
                                         int64_t n_bytes, int sub, int lpr) {
    auto ldb = [&](int64_t off) -> uint8_t { return off >= 0 && off < n_bytes ? data[off] : (uint8_t)0; };
    const int64_t head = min((int64_t)((16 - ((uintptr_t)dst & 15)) & 15), len);
    for (int64_t i = sub; i < head; i += lpr) dst[i] = ldb(src + i);
    const int64_t nb = (len - head) >> 4;
    for (int64_t c = sub; c < nb; c += lpr)
        *reinterpret_cast<uint4 *>(dst + head + 16 * c) = qc_load16(data, src + head + 16 * c, n_bytes);
    const int64_t t0 = head + 16 * nb;
    for (int64_t i = t0 + sub; i < len; i += lpr) dst[i] = ldb(src + i);
}

__global__ __launch_bounds__(BLOCK) void k_fq_format_emit(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                         const int64_t *__restrict__ soff, const int64_t *__restrict__ qoff,
                                                         const int32_t *__restrict__ dlen, const int64_t *__restrict__ ids, int64_t nq,
                                                         const int64_t *__restrict__ start, const int64_t *__restrict__ off, int lpr,
                                                         uint8_t *__restrict__ out) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t q = wave * ngrp + grp;
    if (grp >= ngrp || q >= nq) return;
    const int64_t o = off[q], size = off[q + 1] - o;
    if (size <= 0) return;                                    // dropped
    const int64_t id = ids ? ids[q] : q;
    const int64_t a = start ? start[q] : 0;
    const int64_t so = soff[id] - gbase, qo = qoff[id] - gbase;
    int64_t hl = dlen[id] > 0 ? dlen[id] : 0;
    const int64_t ho = so - hl - 1, last = so - 2;
    if (hl > 0 && last >= 0 && last < n_bytes && data[last] == 13) --hl;      // as the count pass did
    const int64_t kk = (size - hl - 5) >> 1;                  // the kept bases: size = header + 2 x kept + 5
    uint8_t *d = out + o;
    fmt_copy(d, data, ho, hl, n_bytes, sub, lpr);
    fmt_copy(d + hl + 1, data, so + a, kk, n_bytes, sub, lpr);
    fmt_copy(d + hl + kk + 4, data, qo + a, kk, n_bytes, sub, lpr);
    if (sub == 0) {
        d[hl] = '\n'; d[hl + 1 + kk] = '\n'; d[hl + 2 + kk] = '+'; d[hl + 3 + kk] = '\n'; d[hl + 2 * kk + 4] = '\n';
    }
}

}  // namespace fx
