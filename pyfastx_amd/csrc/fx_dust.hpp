// fx_dust.hpp -- low-complexity sequence by the DUST triplet score for gfx950 (MI355X, wave64): the windowed mask of the
// resident FASTA table (fx_fasta_low_complexity) and the per-read columns of the resident FASTQ table (fx_fastq_complexity).
// Extension: the reference has no such call.  The definition is the one of include/fxgpu.h; this is the WINDOWED form (a whole
// qualifying window is masked), not sdust's perfect intervals.
//
// Letters fold as in fx_kmer.hpp (kmer_code): A a 0, C c 1, G g 2, T t 3, every other kept byte invalid.  A triplet is valid
// when its three letters are; its code is 16 a + 4 b + c.
//
// FASTA.  The run layout of fx_search.hpp and the interval driver of fx_annot.hpp's class runs: one lane per 256-byte run of
// the selected records.  The lane keeps the last 64 letters (two bits each, 128 bits) and their validity (64 bits), shifted
// per kept byte as fx_pwm.hpp keeps its history; the triplet that enters the window is the low six bits after the shift, the
// one that leaves it the six bits at 2 (W - 3) before the shift -- both shifts are uniform over the wave.  The 64 counters of
// the window (each <= 62) are bytes in LDS, four codes to a word, word (code >> 2) * BLOCK + thread: every lane of a wave on a
// bank of its own, 16 KiB per workgroup, cleared by the lane that owns them.  Rolling score: leaving y: S -= --c[y]; entering
// x: S += c[x]++; n beside them; the window that ends at e qualifies, f(e), iff n >= 2 and 10 S > T (n - 1).
//
//   Carry.  g(e) = "some f in (e - W, e]" is a counter of the steps since the last qualifying end, capped at W.  The masked
//   intervals are exactly the maximal runs of g shifted left by W - 1: a position with g = 0 plays the part of class runs'
//   "letter outside the set" -- the packed word per run, the scan of "has an outside position", the list and an_open_start are
//   those of fx_annot.hpp as they are.  The outside position o that ends a run of g that began behind the outside position p
//   closes [max(0, p + 2 - W), o - W + 1): g(o - 1) = 1 and g(o) = 0 say that the last qualifying end is o - W.  The end of
//   the text closes an open one at L - since, since = the steps behind the last qualifying end; the run that holds the
//   letter L - 1 owns that close (not the record's last run: with a cut at slen the letter may lie many runs earlier) and
//   stores `since` in a word of its own.
//   Warm-up.  g at a run's first byte depends on f of the W - 1 letters in front of it, and those on the W - 1 letters in
//   front of them: a warm-up over 2 W - 2 kept bytes (dust_warm: run_warm in 16-byte chunks).  A warm-up that starts inside the record sees windows shorter than the
//   real ones on its first W - 1 steps (seven A there would qualify although their real window of 64 does not): their f is
//   ignored.  One that starts at the record's first letter -- the run begins fewer than 2 W - 2 letters into the record --
//   sees exactly the short windows of the definition and ignores nothing.
//
// FASTQ (k_fq_complexity).  The lane groups of k_fq_read_stats: lpr lanes per read, a 16-byte piece per lane and step, the two
// bytes in front of the piece from one more load (the neighbour lane's piece: it hits the cache).  The 64 counters of a group
// are 32-bit words in LDS, cleared by the group before each read; a lane adds 1 for every valid triplet that ENDS in its piece
// by a returning ds_add and sums what comes back: each insertion returns the count it found, so the total is
// sum c (c - 1) / 2 in whatever order the lanes arrive, and no counter can wrap below 2^32 letters.  n_diff compares every
// byte with the one in front of it.  The sums go down the group by qc_group_reduce (64-bit for dust_sum).
#pragma once
#include "fx_annot.hpp"
#include "fx_kmer.hpp"

namespace fx {

constexpr int DUST_MIN_W = 4, DUST_MAX_W = 64, DUST_MAX_T = 1000;
constexpr int DUST_LDS_WORDS = 16 * BLOCK;                 // 64 byte counters per lane

struct DustArg {
    int W, T;                             // window in letters, threshold in tenths
    int64_t min_len;
};

// byte address of counter `code` of this thread in the workgroup's table
__device__ __forceinline__ uint32_t dust_at(uint32_t code) { return ((((code >> 2) * BLOCK) + threadIdx.x) << 2) | (code & 3u); }

// the interval a run of g over [cur, o) stands for, o the outside position behind it: is it a row?
__device__ __forceinline__ int64_t dust_start(const DustArg &A, int64_t cur) { return max(cur + 1 - A.W, (int64_t)0); }
__device__ __forceinline__ bool dust_row(const DustArg &A, int64_t cur, int64_t o) {
    return o > cur && (o - A.W + 1) - dust_start(A, cur) >= A.min_len;
}
// the run holds the last letter of the text (R.L > 0: exactly one run of a record does)
__device__ __forceinline__ bool dust_owns_end(const SearchPlan &P, const RankIndex &X, const AnRun &R, int64_t q) {
    const int64_t g = X.run0[R.r] + (q - P.run0[R.k]), limit = R.L - R.base;
    return limit > 0 && X.pref[g + 1] - X.pref[g] >= limit;
}

// run_warm of fx_search.hpp -- the last `need` kept bytes of [b, lo), or all of them, in order to step(c) -- in aligned
// 16-byte chunks: back from lo counting the kept bytes of every chunk until they suffice, then forward over the same chunks
// (they hit the cache), the kept bytes too many skipped.  With up to 126 kept bytes to warm up on, the byte loads of run_warm
// were 256 of a lane's 272 load instructions, every one of them 64 cache lines wide across the wave.
template <class S>
__device__ __forceinline__ void dust_warm(const SearchPlan &P, int64_t b, int64_t lo, int need, S &&step) {
    if (lo <= b) return;
    int have = 0;
    int64_t c = (lo - 1) & ~(int64_t)15;
    for (;; c -= 16) {
        const int s = (int)max(b - c, (int64_t)0), t = (int)min(lo - c, (int64_t)16);      // [c + s, c + t) lies in [b, lo): t > s
        const uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
        have += __popc(an_kept16(v, ((1u << t) - 1u) & ~((1u << s) - 1u)));
        if (have >= need || c <= b) break;
    }
    int skip = have > need ? have - need : 0;
    run_walk(P, max(c, b), lo, [&](uint32_t ch) {
        if (skip > 0) --skip;
        else step(ch);
    });
}

// Walk the kept bytes of one run in front of the cut after the warm-up: outside(i) for every one (i: kept index) whose g is 0.
// cnt: the workgroup's table, this lane's counters zero.  -> since at the last letter walked (W: g = 0, also when none was).
template <class F>
__device__ __forceinline__ uint32_t dust_walk(const SearchPlan &P, const DustArg &A, const AnRun &R, uint8_t *cnt, F &&outside) {
    const int W = A.W;
    const int64_t limit = R.L - R.base;
    if (limit <= 0) return (uint32_t)W;
    const int out_sh = 2 * (W - 3), val_sh = W - 3;         // the leaving triplet: letters W - 1, W - 2, W - 3 behind the newest
    uint64_t h0 = 0, h1 = 0, valid = 0;
    uint32_t S = 0, n = 0;
    int since = W, ignore = R.base >= 2 * W - 2 ? W - 1 : 0;
    auto step = [&](uint32_t c) {
        if (((valid >> val_sh) & 7u) == 7u) {
            const uint32_t y = (uint32_t)(out_sh < 64 ? (h0 >> out_sh) | (h1 << (64 - out_sh)) : h1 >> (out_sh - 64)) & 63u;
            uint8_t *p = cnt + dust_at(y);
            const uint32_t v = (uint32_t)*p - 1u;
            *p = (uint8_t)v;
            S -= v;
            --n;
        }
        const uint32_t code = kmer_code(c);
        h1 = (h1 << 2) | (h0 >> 62);
        h0 = (h0 << 2) | (code & 3u);
        valid = (valid << 1) | (code <= 3u ? 1u : 0u);
        if ((valid & 7u) == 7u) {
            uint8_t *p = cnt + dust_at((uint32_t)h0 & 63u);
            const uint32_t v = *p;
            *p = (uint8_t)(v + 1u);
            S += v;
            ++n;
        }
        bool f = n >= 2u && 10u * S > (uint32_t)A.T * (n - 1u);
        if (ignore > 0) { --ignore; f = false; }
        since = f ? 0 : min(since + 1, W);
    };
    dust_warm(P, R.b, R.lo, 2 * W - 2, step);
    int64_t kidx = 0;
    run_walk(P, R.lo, R.hi, [&](uint32_t c) {
        if (kidx < limit) {
            step(c);
            if (since >= W) outside(kidx);
        }
        ++kidx;
    });
    return (uint32_t)since;
}
__device__ __forceinline__ uint8_t *dust_clear(uint32_t *lds) {
#pragma unroll
    for (int j = 0; j < 16; ++j) lds[j * BLOCK + threadIdx.x] = 0;      // the lane's own words: nothing to wait for
    return reinterpret_cast<uint8_t *>(lds);
}

// packed[q]: the word of k_an_runs_count with "outside" = g is 0; since[q]: what dust_walk returns
__global__ __launch_bounds__(BLOCK) void k_dust_count(SearchPlan P, RankIndex X, DustArg A, uint32_t *__restrict__ packed, uint32_t *__restrict__ since) {
    __shared__ uint32_t lds[DUST_LDS_WORDS];
    uint8_t *cnt = dust_clear(lds);
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const AnRun R = an_run(P, X, q);
    uint32_t closes = 0, first = AN_NOFIRST, behind = 0;
    since[q] = dust_walk(P, A, R, cnt, [&](int64_t i) {
        if (first == AN_NOFIRST) first = (uint32_t)i;
        else closes += dust_row(A, R.base + behind, R.base + i) ? 1u : 0u;
        behind = (uint32_t)i + 1u;
    });
    packed[q] = an_runs_pack(closes, first, behind);
}
// adds what the scan decides: the row the run's first outside position closes and the one the end of the text closes
__global__ __launch_bounds__(BLOCK) void k_dust_close(SearchPlan P, RankIndex X, DustArg A, const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                      const uint32_t *__restrict__ since, uint32_t *__restrict__ packed) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const AnRun R = an_run(P, X, q);
    const uint32_t w = packed[q], first = (w >> 8) & 511u, behind = (w >> 17) & 511u;
    int64_t cur = an_open_start(P, X, R, q, packed, NZ, list);
    uint32_t closes = w & 255u;
    if (first != AN_NOFIRST) {
        closes += dust_row(A, cur, R.base + first) ? 1u : 0u;
        cur = R.base + behind;
    }
    if (dust_owns_end(P, X, R, q) && since[q] < (uint32_t)A.W) closes += (R.L - since[q]) - dust_start(A, cur) >= A.min_len ? 1u : 0u;
    packed[q] = (w & ~255u) | closes;
}
// the runs that close something walk again and store their rows at O[q] (exclusive prefix of the counts)
__global__ __launch_bounds__(BLOCK) void k_dust_emit(SearchPlan P, RankIndex X, DustArg A, const uint32_t *__restrict__ packed, const int64_t *__restrict__ NZ,
                                                     const int64_t *__restrict__ list, const int64_t *__restrict__ O, int64_t *__restrict__ o_rec,
                                                     int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop) {
    __shared__ uint32_t lds[DUST_LDS_WORDS];
    uint8_t *cnt = dust_clear(lds);
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs || !(packed[q] & 255u)) return;
    const AnRun R = an_run(P, X, q);
    int64_t cur = an_open_start(P, X, R, q, packed, NZ, list), o = O[q];
    const int64_t o_end = O[q + 1];
    auto put = [&](int64_t stop) {
        const int64_t start = dust_start(A, cur);
        if (stop - start >= A.min_len && o < o_end) { o_rec[o] = R.r; o_start[o] = start; o_stop[o] = stop; ++o; }
    };
    const uint32_t since = dust_walk(P, A, R, cnt, [&](int64_t i) {
        if (R.base + i > cur) put(R.base + i - A.W + 1);
        cur = R.base + i + 1;
    });
    if (dust_owns_end(P, X, R, q) && since < (uint32_t)A.W) put(R.L - since);
}

// ------------------------------------------------------------------ FASTQ
struct DustCols { int64_t *length, *dust_sum; int32_t *n_triplets, *n_diff; };

// Queries [0, nq); start / end null: whole reads.  Dynamic LDS: 64 words per lane group of the workgroup.
__global__ __launch_bounds__(BLOCK) void k_fq_complexity(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes, const int64_t *__restrict__ rlen,
                                                        const int64_t *__restrict__ soff, const int64_t *__restrict__ ids, int64_t nq,
                                                        const int64_t *__restrict__ start, const int64_t *__restrict__ end, int lpr, DustCols out) {
    extern __shared__ __align__(16) uint32_t dust_lds[];
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    uint32_t *tab = dust_lds + ((int)(threadIdx.x >> 6) * ngrp + (live ? grp : 0)) * 64;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    for (int64_t q = wave * ngrp + grp; q - grp < nq; q += stride) {              // wave-uniform trip count
        uint32_t nt = 0, nd = 0;
        uint64_t S = 0;
        int64_t a = 0, b = 0;
        // the group's table: cleared by its lanes, then added to by them; a group lies in one wave, whose LDS operations keep
        // their order -- the fences keep the compiler from moving them across
        if (live) for (int j = sub; j < 64; j += lpr) tab[j] = 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (live && q < nq) {
            const int64_t id = ids ? ids[q] : q;
            const int64_t L = rlen[id] > 0 ? rlen[id] : 0, so = soff[id] - gbase;
            a = start ? start[q] : 0;
            b = end ? end[q] : L;
            for (int64_t p = (int64_t)sub * 16; p < b; p += (int64_t)lpr * 16) {
                if (p + 16 <= a) continue;
                uint32_t c0 = KMER_INVALID, c1 = KMER_INVALID, prev = 0;
                if (p > a) {                                 // the two bytes in front of the piece, from `a` on
                    const uint4 pv = qc_load16(data, so + p - 16, n_bytes);
                    prev = pv.w >> 24;
                    c1 = kmer_code(prev);
                    if (p - 2 >= a) c0 = kmer_code((pv.w >> 16) & 0xFFu);
                }
                const uint4 cv = qc_load16(data, so + p, n_bytes);
                const uint32_t w[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (p + i < a || p + i >= b) continue;
                    const uint32_t ch = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu, c = kmer_code(ch);
                    if (p + i > a) nd += ch != prev ? 1u : 0u;
                    if ((c0 | c1 | c) <= 3u) {
                        S += atomicAdd(&tab[16 * c0 + 4 * c1 + c], 1u);
                        ++nt;
                    }
                    c0 = c1; c1 = c; prev = ch;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        nt = qc_group_reduce(nt, lane, sub, lpr, p2, [](uint32_t x, uint32_t y) { return x + y; });
        nd = qc_group_reduce(nd, lane, sub, lpr, p2, [](uint32_t x, uint32_t y) { return x + y; });
        S = qc_group_reduce(S, lane, sub, lpr, p2, [](uint64_t x, uint64_t y) { return x + y; });
        if (live && sub == 0 && q < nq) {
            out.length[q] = b - a; out.dust_sum[q] = (int64_t)S;
            out.n_triplets[q] = (int32_t)nt; out.n_diff[q] = (int32_t)nd;
        }
    }
}

}  // namespace fx
