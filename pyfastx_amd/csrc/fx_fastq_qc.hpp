// fx_fastq_qc.hpp -- FASTQ quality control on the resident stream for gfx950 (MI355X, wave64): per-read statistics, read
// selection and the per-cycle profile.  Extension: the reference answers whole-file questions only (fastq.c:715-753).
//
// All three read the `rlen` bytes at `soff` and at `qoff` of the read table -- the bytes k_fastq_fetch returns, a byte past
// the end of the stream reads as 0 -- and follow no line rule of their own.  Base classes are those of the composition:
// upper-case A C G T, every other byte is "other".  Everything is integer and exact.
//
//   k_fq_read_stats<false>   lpr lanes per read (the host picks ceil(mean read length / 16), as for k_fastq_comp), 64 / lpr
//        reads side by side per wave, 16 bytes of each line per lane and step.  Quality: the byte sum by v_sad_u8, minimum /
//        maximum by packed 16-bit min / max on the even and odd bytes, "below the threshold" as the borrow of a packed 16-bit
//        subtraction.  Sequence: (b >> 1) & 7 picks the letter that code stands for through v_perm_b32; the bytes equal to it
//        are A C G T, and bit 1 of those says G or C.  A piece is masked to the bytes inside its line (no byte is read
//        twice: sums and counts, unlike k_fastq_comp's minima, would not survive it).  The partial results go down the lane
//        group by ds_bpermute and lane 0 of the group stores the row.  `ids` makes it a gather; the row goes to the query's slot.
//   k_fq_read_stats<true>    the same body; instead of the row the lane evaluates the selection predicate in int64 and
//        stores one byte.  k_sscan_sums / k_sscan_top (fx_search.hpp) turn the bytes into per-chunk offsets and the total,
//        k_fq_select_emit writes the ids of a chunk at its offset in read order: no atomics, nothing sorted.
//   k_fq_cycle_hist          one LANE per CYCLE: a wave owns 64 consecutive cycles and walks reads; lane j loads byte j of
//        the quality line and of the sequence line (64 consecutive bytes per wave-instruction) and adds to ITS OWN row of the
//        wave's histogram in LDS.  No two lanes ever add to one counter, so the handful of quality values real files use
//        costs nothing: there is no same-address contention to plan for, and no atomic is needed to be correct -- ds_add_u32
//        without a return value is used because it measured faster than ds_read / add / ds_write on the lane's own word
//        (9.8 against 10.4 ms for 20 M reads).  Rows are 101 counters (quality bytes 32..127, then A C G T other), two 16-bit
//        counters per word, 51 words per cycle -- an odd stride, so the 64 lanes fall into distinct banks -- 13 KiB per wave,
//        51 KiB per workgroup, three workgroups per CU.  A wave flushes its rows to the global int64 counters (one atomic
//        per non-zero counter) before any 16-bit counter can wrap -- after 65535 reads -- and at its end; the grid is the
//        resident waves, so that is once or a few times per wave.  A quality byte outside 32..127 goes to its global
//        counter directly.  More cycles than one tile: the waves are dealt over the tiles, each tile's waves share the reads
//        -- and each tile's waves read the whole read table, so the table traffic grows with cycles / 64.
#pragma once
#include "fx_fastq.hpp"
#include "fx_search.hpp"

namespace fx {

struct QcCols { int64_t *length, *qsum; int16_t *qmin, *qmax; int32_t *n_low, *n_gc, *n_other; };
// selection criteria; a bound < 0 (a denominator of 0) is one that was not asked for
struct QcSel { int64_t min_len, max_len, mq_num, mq_den, lf_num, lf_den, max_other; };

constexpr uint32_t QC_EX_LO = 0x47544341u, QC_EX_HI = 0x80808080u;     // codes 0..3: 'A' 'C' 'T' 'G'; 4..7: 0x80, whose own code is 0

// 16 bytes at data[p, p + 16) at any alignment; a byte outside [0, n_bytes) reads as 0
__device__ __forceinline__ uint4 qc_load16(const uint8_t *__restrict__ data, int64_t p, int64_t n_bytes) {
    if (p >= 0 && p + 16 <= n_bytes) return *reinterpret_cast<const uint4_u *>(data + p);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; ++k)
        if (p + k >= 0 && p + k < n_bytes) w[k >> 2] |= (uint32_t)data[p + k] << ((k & 3) * 8);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// down the lane group to its lane 0 (any group size lpr <= 64; p2 = the power of two at or above lpr, halved)
template <class T, class Op>
__device__ __forceinline__ T qc_group_reduce(T v, int lane, int sub, int lpr, int p2, Op op) {
    for (int d = p2; d > 0; d >>= 1) {
        T o;
        if constexpr (sizeof(T) == 8) o = (T)shfl64((long long)v, lane + d);
        else o = (T)__shfl((int)v, lane + d, 64);
        if (sub + d < lpr) v = op(v, o);
    }
    return v;
}

template <bool SELECT>
__global__ __launch_bounds__(BLOCK) void k_fq_read_stats(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                        const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                        const int64_t *__restrict__ qoff, const int64_t *__restrict__ ids, int64_t nq,
                                                        int phred, int thr, int lpr, QcCols out, QcSel sel, uint8_t *__restrict__ pass) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr, step = 16 * lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    const uint32_t thr2 = (uint32_t)thr * 0x00010001u;       // thr in 0..256
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
        uint64_t sum = 0;
        uint32_t mn = 0x00FF00FFu, mx = 0u, nlow = 0, nacgt = 0, ngc = 0;
        for (int64_t p = (int64_t)sub * 16; p < L; p += step) {
            const uint4 vq = qc_load16(data, row.qo + p, n_bytes), vs = qc_load16(data, row.so + p, n_bytes);
            const int keep = L - p < 16 ? (int)(L - p) : 16;
            uint32_t lo[4] = {vq.x, vq.y, vq.z, vq.w}, hi[4] = {vq.x, vq.y, vq.z, vq.w}, s[4] = {vs.x, vs.y, vs.z, vs.w};
            if (keep < 16) { fq_keep_first(lo, keep, 0xFFFFFFFFu); fq_keep_first(hi, keep, 0u); fq_keep_first(s, keep, 0u); }
            uint32_t psum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                psum = __builtin_amdgcn_sad_u8(hi[k], 0u, psum);
                const uint32_t ev = __builtin_amdgcn_perm(0u, lo[k], 0x0C020C00u), od = __builtin_amdgcn_perm(0u, lo[k], 0x0C030C01u);
                mn = pk_min_u16(mn, pk_min_u16(ev, od));
                mx = pk_max_u16(mx, pk_max_u16(__builtin_amdgcn_perm(0u, hi[k], 0x0C020C00u), __builtin_amdgcn_perm(0u, hi[k], 0x0C030C01u)));
                // bit 15 of (0x8000 + b - thr) stays set exactly when b >= thr; no borrow leaves a 16-bit half
                nlow += 4 - __popc((((ev | 0x80008000u) - thr2) & 0x80008000u)) - __popc((((od | 0x80008000u) - thr2) & 0x80008000u));
                const uint32_t z = zero_bytes(s[k] ^ __builtin_amdgcn_perm(QC_EX_HI, QC_EX_LO, (s[k] >> 1) & 0x07070707u));
                nacgt += __popc(z);
                ngc += __popc(z & (s[k] << 6));               // bit 1 of an exact letter: set for C and G
            }
            sum += psum;
        }
        int qmin = (int)min(mn & 0xFFFFu, mn >> 16), qmax = (int)max(mx & 0xFFFFu, mx >> 16);
        sum = qc_group_reduce(sum, lane, sub, lpr, p2, [](uint64_t a, uint64_t b) { return a + b; });
        qmin = qc_group_reduce(qmin, lane, sub, lpr, p2, [](int a, int b) { return a < b ? a : b; });
        qmax = qc_group_reduce(qmax, lane, sub, lpr, p2, [](int a, int b) { return a > b ? a : b; });
        nlow = qc_group_reduce(nlow, lane, sub, lpr, p2, [](uint32_t a, uint32_t b) { return a + b; });
        nacgt = qc_group_reduce(nacgt, lane, sub, lpr, p2, [](uint32_t a, uint32_t b) { return a + b; });
        ngc = qc_group_reduce(ngc, lane, sub, lpr, p2, [](uint32_t a, uint32_t b) { return a + b; });
        if (live && sub == 0 && q < nq) {
            // the bytes a partial piece was padded with (0xFF) are below a threshold of 256 only: every byte is, then
            const int64_t n_low = thr >= 256 ? L : (int64_t)nlow, n_other = L - (int64_t)nacgt;
            const int64_t qsum = (int64_t)sum - (int64_t)phred * L;
            if (SELECT) {
                bool ok = true;
                if (sel.min_len >= 0) ok = ok && L >= sel.min_len;
                if (sel.max_len >= 0) ok = ok && L <= sel.max_len;
                if (sel.mq_den > 0) ok = ok && qsum * sel.mq_den >= sel.mq_num * L;
                if (sel.lf_den > 0) ok = ok && n_low * sel.lf_den <= sel.lf_num * L;
                if (sel.max_other >= 0) ok = ok && n_other <= sel.max_other;
                pass[q] = ok ? 1 : 0;
            } else {
                out.length[q] = L; out.qsum[q] = qsum;
                out.qmin[q] = (int16_t)(L > 0 ? qmin - phred : 0); out.qmax[q] = (int16_t)(L > 0 ? qmax - phred : 0);
                out.n_low[q] = (int32_t)n_low; out.n_gc[q] = (int32_t)ngc; out.n_other[q] = (int32_t)n_other;
            }
        }
    }
}

struct QcLdPass {
    const uint8_t *p;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = p[i]; }
};
// the ids of the reads of one chunk that passed, from the chunk's offset on (sums: what k_sscan_top left), in read order
__global__ __launch_bounds__(BLOCK) void k_fq_select_emit(const uint8_t *__restrict__ pass, int64_t n, const int64_t *__restrict__ sums,
                                                         int64_t *__restrict__ out) {
    __shared__ int64_t lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * SRCH_CHUNK + (int64_t)threadIdx.x * SRCH_PER;
    int64_t s = 0;
    for (int i = 0; i < SRCH_PER; ++i)
        if (i0 + i < n) s += pass[i0 + i];
    int64_t tot;
    int64_t at = block_incl_scan64(s, lds, &tot) - s + sums[blockIdx.x];
    for (int i = 0; i < SRCH_PER && i0 + i < n; ++i)
        if (pass[i0 + i]) out[at++] = i0 + i;
}

constexpr int QC_QLO = 32, QC_QBINS = 96;                    // quality bytes 32..127 are counted in LDS
constexpr int QC_BINS = QC_QBINS + 5, QC_ROW = 51;           // + A C G T other; 16-bit counters, two per word
constexpr int QC_U = 32;                                     // reads a wave has in flight per pass
constexpr int QC_FLUSH = 65535;                              // reads a wave may count before a 16-bit counter could wrap

__global__ __launch_bounds__(BLOCK) void k_fq_cycle_hist(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                        const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                        const int64_t *__restrict__ qoff, int64_t n_reads, int cycles, int n_tiles,
                                                        unsigned long long *__restrict__ qual, unsigned long long *__restrict__ base) {
    __shared__ uint32_t hist_all[BLOCK / 64][64 * QC_ROW];
    const int lane = lane_id(), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *row = hist_all[wv] + lane * QC_ROW;             // this lane's counters: no other lane touches them
    for (int w = 0; w < QC_ROW; ++w) row[w] = 0;
    const int64_t wave = (int64_t)blockIdx.x * (BLOCK / 64) + wv;
    const int64_t nwaves = (int64_t)gridDim.x * (BLOCK / 64), share = nwaves / n_tiles;       // waves per tile (the host makes it >= 1)
    if (wave >= share * n_tiles) return;
    const int tile = (int)(wave % n_tiles);
    const int64_t cyc = (int64_t)tile * 64 + lane;            // the cycle this lane counts
    const bool mine = cyc < cycles;
    auto flush = [&]() {
        if (!mine) return;
        for (int w = 0; w < QC_ROW; ++w) {
            const uint32_t v = row[w];
            if (!v) continue;
            row[w] = 0;
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const uint32_t c = hlf ? v >> 16 : v & 0xFFFFu;
                const int b = 2 * w + hlf;
                if (!c) continue;
                if (b < QC_QBINS) atomicAdd(&qual[cyc * 256 + QC_QLO + b], (unsigned long long)c);
                else atomicAdd(&base[cyc * 5 + (b - QC_QBINS)], (unsigned long long)c);
            }
        }
    };
    // QC_U reads per pass.  Their rows come by three vector loads (lane u asks for read i + u), one pass ahead of their
    // bytes, and reach the other lanes through v_readlane; the 2 * QC_U byte loads of a pass are unconditional (a lane
    // without a byte there reads byte 0 of the stream and drops it) and all in flight before the first is counted.
    auto rows = [&](int64_t i0, int64_t &l, int64_t &so, int64_t &qo) {
        const int64_t k = i0 + lane;
        const bool ok = lane < QC_U && k < n_reads;
        const int64_t kk = ok ? k : 0;
        l = ok ? rlen[kk] : 0; so = soff[kk] - gbase; qo = qoff[kk] - gbase;
    };
    auto lane64 = [](int64_t v, int u) -> int64_t {
        return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), u) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, u));
    };
    int since = 0;
    const int64_t stride = share * QC_U;
    int64_t i = (wave / n_tiles) * QC_U, nl, nso, nqo;
    rows(i, nl, nso, nqo);
    for (; i < n_reads; i += stride) {
        const int64_t cl = nl, cso = nso, cqo = nqo;
        rows(i + stride, nl, nso, nqo);
        if (since + QC_U > QC_FLUSH) { flush(); since = 0; }
        uint8_t qb[QC_U], sb[QC_U];
        uint32_t has_m = 0, q_in = 0, s_in = 0;                // per read of the pass: this lane counts it; its byte lies inside the stream
        static_assert(QC_U <= 32, "one bit per read of a pass");
#pragma unroll
        for (int u = 0; u < QC_U; ++u) {                      // every v_readlane of the pass is here, with all lanes active
            const int64_t pq = lane64(cqo, u) + cyc, ps = lane64(cso, u) + cyc;
            const bool has = mine && cyc < lane64(cl, u), qin = has && pq >= 0 && pq < n_bytes, sin_ = has && ps >= 0 && ps < n_bytes;
            has_m |= (uint32_t)has << u; q_in |= (uint32_t)qin << u; s_in |= (uint32_t)sin_ << u;
            qb[u] = data[qin ? pq : 0];
            sb[u] = data[sin_ ? ps : 0];
        }
#pragma unroll
        for (int u = 0; u < QC_U; ++u) {
            if (!((has_m >> u) & 1u)) continue;
            const uint32_t q = (q_in >> u) & 1u ? qb[u] : 0u, c = (s_in >> u) & 1u ? sb[u] : 0u;      // past the end: 0
            const uint32_t qi = q - QC_QLO;
            if (qi < (uint32_t)QC_QBINS) atomicAdd(&row[qi >> 1], 1u << (16 * (qi & 1)));      // ds_add_u32, nothing returned
            else atomicAdd(&qual[cyc * 256 + q], 1ull);       // outside the fast range: straight to its counter
            const int bi = QC_QBINS + (c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4);
            atomicAdd(&row[bi >> 1], 1u << (16 * (bi & 1)));
        }
        since += QC_U;
    }
    flush();
}

}  // namespace fx
