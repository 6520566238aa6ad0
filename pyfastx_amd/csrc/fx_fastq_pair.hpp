// fx_fastq_pair.hpp -- paired-end FASTQ on two resident streams for gfx950 (MI355X, wave64): the overlap of the mates of a pair,
// what survives adapter read-through, the merged fragment records.  Extension: the reference reads one file at a time and has
// no counterpart.
//
// Pair i is read i of stream 1 and read i of stream 2; s1, q1, L1 and s2, q2, L2 are the bytes k_fastq_fetch returns for them (a
// byte past the end of a stream reads as 0).  Everything is integer and exact; the definition is the one of include/fxgpu.h:
// diagonal d puts letter k of the reverse complement of read 2 under s1[k + d], the diagonals are tried in the order 0, 1, ...,
// L1 - 1, -1, -2, ..., -(L2 - 1) and the first accepted one is the pair's.
//
//   k_fp_overlap   the lane-group layout of k_fq_trim: lpr = ceil(longest read of either stream / 16) lanes per pair, 64 / lpr
//        pairs side by side per wave, the table rows of both streams fetched one iteration ahead, `ids` makes it a gather.
//        Lane `sub` loads bytes 16 sub .. 16 sub + 15 of s1, and the 16 bytes of s2 that END at L2 - 16 sub (one unaligned
//        load), reversed: letters 16 sub .. 16 sub + 15 of the reverse complement but for the complement itself.  Both pieces
//        are packed as k_fq_trim packs its piece -- 2 bits per base ((b >> 1) & 3: A 0, C 1, T 2, G 3), where the complement
//        is an XOR with 2, plus a "not A C G T" bit per base -- and stored to LDS, 16 bytes per lane, so that the pair lies in
//        its lane group's 4 x lpr words.  The lanes of a group split the diagonals: lane `sub` takes the forward diagonals
//        16 sub .. 16 sub + 15 (overlaps of at most L1 - 16 sub letters: lpr - sub words) and the backward diagonals
//        -(16 (lpr - 1 - sub)) .. -(16 (lpr - 1 - sub) + 15) (at most sub + 1 words), lpr + 1 words in all for every lane.  The
//        16 diagonals of a set share their words: per word of the set's longest overlap a lane reads four words from LDS, and
//        each diagonal costs two v_alignbit (the window of codes and of flags), an XOR, the fold of the two bits of a letter
//        with the flags of both mates and a popcount.  Nothing is masked: a letter past the end of its read carries the "not
//        A C G T" flag, so the letters of a word that lie outside a diagonal's overlap all count as mismatches, and their
//        number -- known from the lengths -- is taken off at the end.  A set whose longest overlap is below min_overlap is
//        not walked at all.  The first accepted diagonal of a lane, as (position in the trial order) << 16 | mismatches, goes
//        down the lane group in one minimum; lane 0 writes the five columns.
//        A pair with a read longer than 16 * lpr (only when a stream's longest read exceeds 1024) is walked by lane 0 of its
//        group byte by byte from the definition: exact, slow, rare.
//   k_fp_merge_count   one lane per query: diag against the two lengths (first offender -> atomicMin), the size of the merged
//        record: header + 2 x fragment + 5, or 0.  k_sscan_sums / k_sscan_top / k_sscan_apply (fx_search.hpp) give the
//        exclusive offsets, the total and the number of records.
//   k_fp_merge_emit    one lane group per record: the header of read 1, the consensus sequence, "\n+\n", the consensus quality,
//        "\n".  The stretches only read 1 covers are copied as k_fq_format_emit copies; every other 16 letters of the
//        fragment are one lane's: 16-byte pieces of s1, q1 and of the reversed s2, q2 (the complement through the table of
//        k_fastq_fetch in LDS), the rule of the definition byte by byte in registers, one store of up to 16 bytes each for the
//        sequence and the quality.  No atomics, nothing sorted.
#pragma once
#include "fx_fastq_trim.hpp"

namespace fx {

constexpr int32_t PAIR_NONE = INT32_MIN;                     // FX_PAIR_NONE

struct PairSrc { const uint8_t *data; int64_t base, n; const int64_t *rlen, *soff, *qoff; const int32_t *dlen; };      // one mate's stream and table
struct PairPar { int min_overlap, max_diff; int64_t err_num, err_den; };
struct PairCols { int32_t *diag, *overlap, *mism; int64_t *end1, *end2; };

// the 16 bytes of v in reverse order
__device__ __forceinline__ uint4 pair_rev16(const uint4 &v) {
    return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}
// a piece as k_fq_trim packs it: 2 bits per letter, and bit 0 of the pair set for a byte that is not A C G T -- and for every
// byte from `keep` (0..16) on: a letter past the end of its read matches nothing
__device__ __forceinline__ void pair_pack16(const uint4 &v, int keep, uint32_t *code, uint32_t *inv) {
    const uint32_t s[4] = {v.x, v.y, v.z, v.w};
    uint32_t c = 0, i = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t z = zero_bytes(s[k] ^ __builtin_amdgcn_perm(QC_EX_HI, QC_EX_LO, (s[k] >> 1) & 0x07070707u));
        const uint32_t x = (s[k] >> 1) & 0x03030303u, y = (~z >> 7) & 0x01010101u;
        c |= ((x | (x >> 6) | (x >> 12) | (x >> 18)) & 0xFFu) << (8 * k);
        i |= ((y | (y >> 6) | (y >> 12) | (y >> 18)) & 0x55u) << (8 * k);
    }
    *code = c; *inv = i | (0x55555555u & ~trim_len_mask(keep, 0));
}

// "accepted": the rule of the definition for an overlap of m letters with mm mismatches
__device__ __forceinline__ bool pair_accepts(const PairPar &P, int64_t m, int64_t mm) {
    return m >= P.min_overlap && mm <= P.max_diff && mm * P.err_den <= P.err_num * m;
}

// The 16 diagonals ws * 16 + t of one direction: letter k of y against letter k + 16 ws + t of x, over the first m_t =
// min(mbase - t, mcap) letters.  x and y are the lpr packed words of the two mates in LDS (code, flag).  No letter is masked:
// the nw words of the set's longest overlap are walked whole for every t, and the 16 nw - m_t letters of them that lie
// outside diagonal t's overlap are past the end of x or of y, flagged, and counted -- so they are taken off again at the
// end.  (The word behind x's last counts as flagged throughout.)  -> the smallest (key0 + t) << 16 | mismatches over the
// accepted t >= t_min, or TRIM_NONE.
__device__ __forceinline__ int pair_walk(const uint32_t *xc, const uint32_t *xi, const uint32_t *yc, const uint32_t *yi, int lpr, int ws,
                                         int mbase, int mcap, int t_min, int key0, const PairPar &P) {
    const int mmax = mbase < mcap ? mbase : mcap;             // the overlap of t = 0, the longest of the set
    if (mmax < P.min_overlap || mmax <= 0) return TRIM_NONE;
    const int nw = (mmax + 15) >> 4;
    uint32_t mm[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) mm[t] = 0;
    uint32_t x0c = xc[ws], x0i = xi[ws];
    for (int w = 0; w < nw; ++w) {
        const bool behind = ws + w + 1 >= lpr;
        const uint32_t x1c = behind ? 0u : xc[ws + w + 1], x1i = behind ? 0x55555555u : xi[ws + w + 1], y = yc[w], yv = yi[w];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t c = t ? __builtin_amdgcn_alignbit(x1c, x0c, 2 * t) : x0c;
            const uint32_t v = t ? __builtin_amdgcn_alignbit(x1i, x0i, 2 * t) : x0i;
            const uint32_t d = c ^ y;
            mm[t] += __popc(((d | (d >> 1)) & 0x55555555u) | v | yv);
        }
        x0c = x1c; x0i = x1i;
    }
    int best = TRIM_NONE;
#pragma unroll
    for (int t = 15; t >= 0; --t) {
        const int m = mbase - t < mcap ? mbase - t : mcap;
        const int miss = (int)mm[t] - (16 * nw - m);          // (m < 1: no diagonal, refused below whatever this is)
        if (t >= t_min && pair_accepts(P, m, miss)) best = ((key0 + t) << 16) | miss;
    }
    return best;
}

// the columns of a pair from its diagonal
__device__ __forceinline__ void pair_store(const PairCols &out, int64_t q, int64_t L1, int64_t L2, bool found, int64_t d, int64_t mm) {
    const int64_t lo = d > 0 ? d : 0, hi = min(L1, d + L2);
    out.diag[q] = found ? (int32_t)d : PAIR_NONE;
    out.overlap[q] = found ? (int32_t)(hi - lo) : 0;
    out.mism[q] = found ? (int32_t)mm : 0;
    out.end1[q] = found && d < 0 ? min(L1, L2 + d) : L1;
    out.end2[q] = found && d < 0 ? L2 + d : L2;
}

// One pair by one lane, byte by byte: the definition as it stands.  For pairs that do not fit their lane group.
__device__ __forceinline__ void pair_serial(const PairSrc &A, const PairSrc &B, int64_t so1, int64_t so2, int64_t L1, int64_t L2,
                                         const PairPar &P, const PairCols &out, int64_t q) {
    auto ld = [](const PairSrc &S, int64_t off) -> uint32_t { return off >= 0 && off < S.n ? (uint32_t)S.data[off] : 0u; };
    auto exact = [](uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
    const int64_t n_diag = L1 + (L2 > 0 ? L2 - 1 : 0);
    for (int64_t i = 0; i < n_diag; ++i) {
        const int64_t d = i < L1 ? i : -(i - L1 + 1);
        const int64_t lo = d > 0 ? d : 0, hi = min(L1, d + L2), m = hi - lo;
        if (m < P.min_overlap) continue;
        int64_t mm = 0;
        for (int64_t j = lo; j < hi; ++j) {
            const uint32_t x = ld(A, so1 + j), y = ld(B, so2 + L2 - 1 - (j - d));
            mm += exact(x) && exact(y) && ((x >> 1) & 3u) == (((y >> 1) & 3u) ^ 2u) ? 0 : 1;
        }
        if (pair_accepts(P, m, mm)) { pair_store(out, q, L1, L2, true, d, mm); return; }
    }
    pair_store(out, q, L1, L2, false, 0, 0);
}

__global__ __launch_bounds__(BLOCK) void k_fp_overlap(PairSrc A, PairSrc B, const int64_t *__restrict__ ids, int64_t nq, int lpr, PairPar P,
                                                     PairCols out) {
    __shared__ uint32_t words[BLOCK / 64][4][64];              // per wave: codes and flags of s1, of the reverse complement of s2
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *c1 = words[wv][0], *i1 = words[wv][1], *c2 = words[wv][2], *i2 = words[wv][3];
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    const int p = sub * 16;                                    // this lane's piece: letters p .. p + 15 of either mate
    const int g0 = grp * lpr;                                  // the group's first word
    auto imin = [](int x, int y) { return x < y ? x : y; };
    struct Row { int64_t n1, so1, n2, so2; };
    auto get_row = [&](int64_t q) -> Row {                    // the table rows of query q, one iteration ahead of their bytes
        Row r{0, 0, 0, 0};
        if (live && q < nq) {
            const int64_t id = ids ? ids[q] : q;
            r.n1 = A.rlen[id]; r.so1 = A.soff[id] - A.base;
            r.n2 = B.rlen[id]; r.so2 = B.soff[id] - B.base;
        }
        return r;
    };
    int64_t q = wave * ngrp + grp;
    Row nxt = get_row(q);
    for (; q - grp < nq; q += stride) {                       // wave-uniform trip count
        const Row row = nxt;
        nxt = get_row(q + stride);
        const int64_t L1 = row.n1 > 0 ? row.n1 : 0, L2 = row.n2 > 0 ? row.n2 : 0;
        const bool fits = L1 <= 16 * (int64_t)lpr && L2 <= 16 * (int64_t)lpr;        // the whole pair lies in the lane group's words
        uint4 v1 = make_uint4(0, 0, 0, 0), v2 = make_uint4(0, 0, 0, 0);
        if (fits && p < L1) v1 = qc_load16(A.data, row.so1 + p, A.n);
        if (fits && p < L2) v2 = pair_rev16(qc_load16(B.data, row.so2 + L2 - 16 - p, B.n));     // (bytes before the read: letters past L2, outside every overlap)
        uint32_t cw1, iw1, cw2, iw2;
        pair_pack16(v1, fits ? (int)min(max(L1 - p, (int64_t)0), (int64_t)16) : 0, &cw1, &iw1);
        pair_pack16(v2, fits ? (int)min(max(L2 - p, (int64_t)0), (int64_t)16) : 0, &cw2, &iw2);
        __builtin_amdgcn_wave_barrier();                      // (the iteration before has read its words)
        c1[lane] = cw1; i1[lane] = iw1; c2[lane] = cw2 ^ 0xAAAAAAAAu; i2[lane] = iw2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int best = TRIM_NONE;
        const int Li1 = fits ? (int)L1 : 0, Li2 = fits ? (int)L2 : 0;
        if (live && fits) {
            // forward: d = 16 sub + t, read 1 shifted against the reverse complement; its place in the trial order is d
            // backward: d = -(16 wb + t), wb = lpr - 1 - sub, the reverse complement shifted against read 1; its place is L1 - 1 - d
            // (d = -0 is no diagonal of its own).  One body for both: the two mates change roles.
#pragma nounroll
            for (int back = 0; back < 2; ++back) {
                const int ws = back ? lpr - 1 - sub : sub, Lx = back ? Li2 : Li1, Ly = back ? Li1 : Li2;
                const uint32_t *xc = (back ? c2 : c1) + g0, *xi = (back ? i2 : i1) + g0, *yc = (back ? c1 : c2) + g0, *yi = (back ? i1 : i2) + g0;
                best = imin(best, pair_walk(xc, xi, yc, yi, lpr, ws, Lx - 16 * ws, Ly, back && ws == 0 ? 1 : 0, back ? Li1 - 1 + 16 * ws : 16 * ws, P));
            }
        }
        best = qc_group_reduce(best, lane, sub, lpr, p2, imin);
        if (live && sub == 0 && q < nq) {
            if (!fits) pair_serial(A, B, row.so1, row.so2, L1, L2, P, out, q);
            else {
                const int key = best >> 16;
                pair_store(out, q, L1, L2, best != TRIM_NONE, key < Li1 ? key : -(key - (Li1 - 1)), best & 0xFFFF);
            }
        }
    }
}

// ------------------------------------------------------------------ merged records
// the header of a read as k_fq_format_count cuts it: dlen bytes, without one trailing '\r'
__device__ __forceinline__ int64_t pair_header_len(const PairSrc &A, int64_t id) {
    int64_t hl = A.dlen[id] > 0 ? A.dlen[id] : 0;
    const int64_t last = A.soff[id] - A.base - 2;
    if (hl > 0 && last >= 0 && last < A.n && A.data[last] == 13) --hl;
    return hl;
}

__global__ __launch_bounds__(BLOCK) void k_fp_merge_count(PairSrc A, PairSrc B, const int64_t *__restrict__ ids, int64_t nq,
                                                         const int32_t *__restrict__ diag, int64_t min_len, int64_t *__restrict__ cnt,
                                                         unsigned long long *__restrict__ bad) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    const int64_t id = ids ? ids[q] : q, L1 = A.rlen[id] > 0 ? A.rlen[id] : 0, L2 = B.rlen[id] > 0 ? B.rlen[id] : 0;
    const int32_t dg = diag[q];
    if (dg == PAIR_NONE) { cnt[q] = 0; return; }
    const int64_t d = dg;
    if (d < -(L2 - 1) || d > L1 - 1) { atomicMin(bad, (unsigned long long)q); cnt[q] = 0; return; }
    const int64_t F = d >= 0 ? max(L1, d + L2) : L2 + d;
    cnt[q] = F < min_len ? 0 : pair_header_len(A, id) + 2 * F + 5;
}

__global__ __launch_bounds__(BLOCK) void k_fp_merge_emit(PairSrc A, PairSrc B, const int64_t *__restrict__ ids, int64_t nq,
                                                        const int32_t *__restrict__ diag, const int64_t *__restrict__ off, int lpr,
                                                        uint8_t *__restrict__ out) {
    __shared__ uint8_t lut[256];                              // the complement of k_fastq_fetch
    build_comp_lut(lut);
    __syncthreads();
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t q = wave * ngrp + grp;
    if (grp >= ngrp || q >= nq) return;
    const int64_t o = off[q], size = off[q + 1] - o;
    if (size <= 0) return;                                    // not merged, or dropped
    const int64_t id = ids ? ids[q] : q, d = diag[q];
    const int64_t L1 = A.rlen[id] > 0 ? A.rlen[id] : 0, L2 = B.rlen[id] > 0 ? B.rlen[id] : 0;
    const int64_t so1 = A.soff[id] - A.base, qo1 = A.qoff[id] - A.base, so2 = B.soff[id] - B.base, qo2 = B.qoff[id] - B.base;
    const int64_t hl = pair_header_len(A, id);                // as the count pass did
    const int64_t F = (size - hl - 5) >> 1;                   // the fragment: size = header + 2 x fragment + 5
    uint8_t *dh = out + o, *ds = dh + hl + 1, *dq = ds + F + 3;
    fmt_copy(dh, A.data, so1 - (A.dlen[id] > 0 ? A.dlen[id] : 0) - 1, hl, A.n, sub, lpr);
    const int64_t lo = d > 0 ? d : 0, hi = min(L1, d + L2);    // [lo, hi): both mates; below lo: read 1 alone
    int64_t to = F;                                           // [hi, to): read 2 alone
    if (lo > 0) {
        fmt_copy(ds, A.data, so1, lo, A.n, sub, lpr);
        fmt_copy(dq, A.data, qo1, lo, A.n, sub, lpr);
    }
    if (d >= 0 && L1 > hi) {                                  // read 2 lies inside read 1: read 1 alone again from hi on
        fmt_copy(ds + hi, A.data, so1 + hi, L1 - hi, A.n, sub, lpr);
        fmt_copy(dq + hi, A.data, qo1 + hi, L1 - hi, A.n, sub, lpr);
        to = hi;
    }
    const int64_t npc = (to - lo + 15) >> 4;
    for (int64_t c = sub; c < npc; c += lpr) {
        const int64_t f0 = lo + 16 * c, k0 = f0 - d;          // letters f0 .. f0 + 15 of the fragment: k0 .. of the reverse complement
        const int len = (int)min((int64_t)16, to - f0);
        const int both = (int)min(max(hi - f0, (int64_t)0), (int64_t)16);          // the first `both` of them have read 1 as well
        uint4 vx = make_uint4(0, 0, 0, 0), va = vx;
        if (both > 0) { vx = qc_load16(A.data, so1 + f0, A.n); va = qc_load16(A.data, qo1 + f0, A.n); }
        const uint4 vy = pair_rev16(qc_load16(B.data, so2 + L2 - 16 - k0, B.n)), vb = pair_rev16(qc_load16(B.data, qo2 + L2 - 16 - k0, B.n));
        const uint32_t x[4] = {vx.x, vx.y, vx.z, vx.w}, a[4] = {va.x, va.y, va.z, va.w}, b[4] = {vb.x, vb.y, vb.z, vb.w};
        const uint32_t y[4] = {lut4(lut, vy.x), lut4(lut, vy.y), lut4(lut, vy.z), lut4(lut, vy.w)};
        uint32_t rs[4] = {0, 0, 0, 0}, rq[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int sh = 8 * (t & 3);
            const uint32_t xb = (x[t >> 2] >> sh) & 0xFFu, ab = (a[t >> 2] >> sh) & 0xFFu, yb = (y[t >> 2] >> sh) & 0xFFu, bb = (b[t >> 2] >> sh) & 0xFFu;
            uint32_t s = yb, ql = bb;
            if (t < both) {
                if (xb == yb) { s = xb; ql = ab > bb ? ab : bb; }
                else if (ab >= bb) { s = xb; ql = ab; }
            }
            rs[t >> 2] |= s << sh; rq[t >> 2] |= ql << sh;
        }
        store_low_bytes(ds + f0, make_uint4(rs[0], rs[1], rs[2], rs[3]), len);
        store_low_bytes(dq + f0, make_uint4(rq[0], rq[1], rq[2], rq[3]), len);
    }
    if (sub == 0) {
        dh[hl] = '\n'; ds[F] = '\n'; ds[F + 1] = '+'; ds[F + 2] = '\n'; dq[F] = '\n';
    }
}

}  // namespace fx
