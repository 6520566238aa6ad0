// fx_search.hpp -- every overlapping hit of one pattern (1..64 bases) on the sequence bytes of the resident FASTA table
// (fx_fasta_search).  Extension: the reference answers one question of this kind, the first hit in one record
// (Sequence.search, sequence.c:519-558, str.find on the host copy of the record).
//
// Layout.  Every selected record's byte range [boff, boff + blen) is cut at the 256-byte blocks of the stream: a RUN is the
// part of one record inside one block, and one lane owns one run.  Runs are numbered record by record (run0[k] = first run
// of selected record k, a device scan), so a lane finds its record by a binary search over run0, never reads a header byte
// and never parses '>'.  Inside its run the lane drops bytes 10 / 13 / 32 (what k_fetch drops) and runs a bit-parallel
// Shift-And automaton over the kept bytes, both strands in the same step: with L <= 32 the two 32-bit states share one
// 64-bit word (bit 32 is set by the "| 1" of the reverse half, so the carry out of the forward half never matters), longer
// patterns keep two 64-bit words.  Before its run the lane warms the state up on the L - 1 kept bytes in front of it (or
// fewer, at the record's boff): the state after them is exactly the state a single walk over the record would have.
//
// Passes.  k_hits_count: per run, hits on + and - and the kept bytes (one 32-bit word).  A device scan of the kept
// counts gives each run's first base (segmented at the records' first runs: record-local positions, whatever the line
// layout).  k_hits_fix: the rare record whose kept bytes outnumber slen (the cut of `seq`) has the run that crosses the
// cut counted again and the runs behind it emptied.  A scan of the hit counts gives every run's output offset and the
// total; the host reads only the totals.  k_hits_emit: only the runs that have hits (a compacted list) walk again and
// store (record, start, strand) at their offsets -- file order comes from the layout, no sort, no atomic.  The three kernels
// are templates on a FORM (below): ExactForm here, and those of fx_search_approx, fx_search_edit, fx_pwm and fx_minimizer.
#pragma once
#include "fx_kernels.hpp"

namespace fx {

constexpr int SRCH_RUN = 256;                              // raw bytes of the stream per lane (one aligned block)
constexpr int SRCH_PER = 16;                               // elements per thread of the scan kernels
constexpr int SRCH_CHUNK = BLOCK * SRCH_PER;
constexpr unsigned SRCH_NONE = 0xFFFFFFFFu;

struct SearchPlan {
    const uint8_t *base;          // the blob minus its misalignment: 16-byte aligned; stream byte x is base[x + mis]
    int64_t mis, n;               // misalignment of the blob, bytes of the stream
    const int64_t *boff, *blen, *slen;
    const int64_t *sel;           // record id of selected slot k (null: k itself)
    int64_t n_sel;
    const int64_t *run0;          // first run of slot k, n_sel + 1 entries (after the plan scan)
    int64_t n_runs;
    int plen;
    const ulonglong2 *masks;      // [256]: Shift-And masks of each byte value, .x forward pattern, .y reverse pattern
};

// address-space extent [b, e) of the bytes of record r (blen over-counts by one when the stream lacks a final newline)
__device__ __forceinline__ void srch_extent(const SearchPlan &P, int64_t r, int64_t &b, int64_t &e) {
    b = P.boff[r] + P.mis;
    e = min(P.boff[r] + P.blen[r], P.n) + P.mis;
}
__device__ __forceinline__ int64_t srch_nruns(int64_t b, int64_t e) { return e > b ? (e - 1) / SRCH_RUN - b / SRCH_RUN + 1 : 0; }
__device__ __forceinline__ int64_t srch_rec(const SearchPlan &P, int64_t k) { return P.sel ? P.sel[k] : k; }

__device__ __forceinline__ bool srch_space(uint32_t c) { return c == 10u || c == 13u || c == 32u; }

// The LDS copy of the masks: narrow (L <= 32): .x = forward | reverse << 32; wide: as given.
template <bool WIDE>
__device__ __forceinline__ void srch_load_tab(const SearchPlan &P, ulonglong2 *tab) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        const ulonglong2 m = P.masks[i];
        tab[i] = WIDE ? m : make_ulonglong2(m.x | (m.y << 32), 0ull);
    }
}

// ------------------------------------------------------------------ the skeleton of every walk over the windows of a run
// Warm-up: back from lo over `need` kept bytes (at most to the record's first byte b), then every kept byte from there to lo,
// in order, to step(c).
template <class S>
__device__ __forceinline__ void run_warm(const SearchPlan &P, int64_t b, int64_t lo, int need, S &&step) {
    int64_t ws = lo;
    while (need > 0 && ws > b) {
        --ws;
        need -= srch_space(P.base[ws]) ? 0 : 1;
    }
    for (int64_t p = ws; p < lo; ++p) {
        const uint32_t c = P.base[p];
        if (!srch_space(c)) step(c);
    }
}

// Every kept byte of the raw bytes [lo, hi), in order, to f(c): aligned 16-byte chunks, the first and the last one masked.
template <class F>
__device__ __forceinline__ void run_walk(const SearchPlan &P, int64_t lo, int64_t hi, F &&f) {
    auto feed = [&](uint32_t x, bool live) {
        if (!live || srch_space(x)) return;
        f(x);
    };
    int64_t c = lo & ~(int64_t)15;
    uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
    for (; c < hi; c += 16) {
        const uint4 cur = v;
        if (c + 16 < hi) v = *reinterpret_cast<const uint4 *>(P.base + c + 16);     // the next chunk in flight while this one is walked
        const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
        if (c >= lo && c + 16 <= hi) {
#pragma unroll
            for (int i = 0; i < 16; ++i) feed((w[i >> 2] >> (8 * (i & 3))) & 0xFFu, true);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) feed((w[i >> 2] >> (8 * (i & 3))) & 0xFFu, c + i >= lo && c + i < hi);
        }
    }
}

// run_walk that hands f(c, at) the address of the byte as well (P.base[at] is c).  A copy, not a wrapper of or under run_walk:
// with one body for both, the kernels that stand on run_walk compile to other code.
template <class F>
__device__ __forceinline__ void run_walk_at(const SearchPlan &P, int64_t lo, int64_t hi, F &&f) {
    auto feed = [&](uint32_t x, bool live, int64_t at) {
        if (!live || srch_space(x)) return;
        f(x, at);
    };
    int64_t c = lo & ~(int64_t)15;
    uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
    for (; c < hi; c += 16) {
        const uint4 cur = v;
        if (c + 16 < hi) v = *reinterpret_cast<const uint4 *>(P.base + c + 16);
        const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
        if (c >= lo && c + 16 <= hi) {
#pragma unroll
            for (int i = 0; i < 16; ++i) feed((w[i >> 2] >> (8 * (i & 3))) & 0xFFu, true, c + i);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) feed((w[i >> 2] >> (8 * (i & 3))) & 0xFFu, c + i >= lo && c + i < hi, c + i);
        }
    }
}

// Walk one run: raw bytes [lo, hi) of the address space, after a warm-up on the L - 1 kept bytes in front of it.  Kept bytes
// whose local index (0 at lo) is below `limit` may end a hit; hits go to on_hit(kidx, fwd, rev).  -> kept bytes in [lo, hi).
template <bool WIDE, class F>
__device__ __forceinline__ uint32_t srch_walk(const SearchPlan &P, const ulonglong2 *tab, int64_t b, int64_t lo, int64_t hi,
                                              int64_t limit, F &&on_hit) {
    const int L = P.plen;
    uint64_t Df = 0, Dr = 0;
    auto step = [&](uint32_t c) {
        if (WIDE) {
            Df = ((Df << 1) | 1ull) & tab[c].x;
            Dr = ((Dr << 1) | 1ull) & tab[c].y;
        } else {
            Df = ((Df << 1) | 0x100000001ull) & tab[c].x;
        }
    };
    run_warm(P, b, lo, L - 1, step);
    const int shf = L - 1, shr = WIDE ? L - 1 : 31 + L;
    int64_t kidx = 0;
    run_walk(P, lo, hi, [&](uint32_t c) {
        step(c);
        const uint32_t f = (uint32_t)(Df >> shf) & 1u, r = (uint32_t)((WIDE ? Dr : Df) >> shr) & 1u;
        if ((f | r) && kidx < limit) on_hit(kidx, f, r);
        ++kidx;
    });
    return (uint32_t)kidx;
}

// geometry of run g of slot k: record id r, record start b, run bytes [lo, hi) -- all address space
__device__ __forceinline__ void srch_run(const SearchPlan &P, int64_t g, int64_t k, int64_t &r, int64_t &b, int64_t &lo, int64_t &hi) {
    r = srch_rec(P, k);
    int64_t e;
    srch_extent(P, r, b, e);
    const int64_t blk = (b & ~(int64_t)(SRCH_RUN - 1)) + (g - P.run0[k]) * SRCH_RUN;
    lo = max(b, blk);
    hi = min(e, blk + SRCH_RUN);
}
__device__ __forceinline__ int64_t srch_slot(const SearchPlan &P, int64_t g) { return upper_bound(P.run0, P.n_sel + 1, g) - 1; }

// per run: hits on + (bits 0..8), on - (9..17), kept bytes (18..26)
__device__ __forceinline__ uint32_t srch_pack(uint32_t hp, uint32_t hm, uint32_t kept) { return hp | (hm << 9) | (kept << 18); }

// ------------------------------------------------------------------ the three passes of every window-hit form
// A FORM is a small trivially copyable struct, a kernel argument, that says what the families of window hits differ in and
// nothing else (ExactForm below, ApproxForm, EditForm, PwmForm, MzForm in the headers on top of this one):
//   table(P)                                   its table in LDS, loaded and synced (every thread of the block calls it) -> tab
//   walk<ROWS>(P, tab, b, lo, hi, limit, on)   its walk over one run: on(kidx, Win w) for every window that may be a row and
//                                              ends at a kept byte in front of `limit` (ROWS: what a row stores is wanted too)
//                                              -> kept bytes in [lo, hi)
//   plus(w), minus(w)                          the window is a row on '+', on '-'
//   first(P, base), pos(first, kidx, w)        a row's position; base: the record-local index of the run's first kept byte
//   Col, COL, col(w, minus)                    the type of its own column, whether it has one, its value for the row of a strand
//   AT                                         a row stores w.at, the address of its last byte, too
//   ONE                                        a window is a row on exactly one strand
// The kernels own the rest: the run geometry, the packed word, the cut, base, the offset Pp[g] + Pm[g] and the order '+' before
// '-'.
template <bool WIDE>
struct ExactForm {
    struct Win { uint32_t f, r; };
    using Col = uint8_t;
    static constexpr bool COL = false, AT = false, ONE = false;
    __device__ __forceinline__ const ulonglong2 *table(const SearchPlan &P) const {
        __shared__ ulonglong2 tab[256];
        srch_load_tab<WIDE>(P, tab);
        __syncthreads();
        return tab;
    }
    template <bool ROWS, class F>
    __device__ __forceinline__ uint32_t walk(const SearchPlan &P, const ulonglong2 *tab, int64_t b, int64_t lo, int64_t hi, int64_t limit,
                                             F &&on) const {
        return srch_walk<WIDE>(P, tab, b, lo, hi, limit, [&](int64_t kidx, uint32_t f, uint32_t rv) { on(kidx, Win{f, rv}); });
    }
    __device__ __forceinline__ uint32_t plus(const Win &w) const { return w.f; }
    __device__ __forceinline__ uint32_t minus(const Win &w) const { return w.r; }
    __device__ __forceinline__ int64_t first(const SearchPlan &P, int64_t base) const { return base - P.plen + 1; }
    __device__ __forceinline__ int64_t pos(int64_t first, int64_t kidx, const Win &) const { return first + kidx; }
    __device__ __forceinline__ Col col(const Win &, bool) const { return 0; }
};

template <class Form>
__global__ __launch_bounds__(BLOCK) void k_hits_count(SearchPlan P, Form F, uint32_t *__restrict__ packed) {
    auto *tab = F.table(P);
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= P.n_runs) return;
    int64_t r, b, lo, hi;
    srch_run(P, g, srch_slot(P, g), r, b, lo, hi);
    uint32_t hp = 0, hm = 0;
    const uint32_t kept = F.template walk<false>(P, tab, b, lo, hi, INT64_MAX, [&](int64_t, const typename Form::Win &w) { hp += F.plus(w); hm += F.minus(w); });
    packed[g] = srch_pack(hp, hm, kept);
}

// The cut at slen of selected record s: where its kept bytes run past slen, f(g, base, slen) for every run from the one that
// crosses the cut on, base: the run's first kept byte.  K: exclusive prefix of the kept counts (n_runs + 1).
template <class F>
__device__ __forceinline__ void srch_cut(const SearchPlan &P, const int64_t *K, int64_t s, F &&f) {
    const int64_t g0 = P.run0[s], g1 = P.run0[s + 1];
    const int64_t slen = P.slen[srch_rec(P, s)];
    if (g0 == g1 || K[g1] - K[g0] <= slen) return;
    int64_t lo_g = g0, hi_g = g1 - 1;                        // first run whose kept bytes end past slen
    while (lo_g < hi_g) { const int64_t m = (lo_g + hi_g) >> 1; if (K[m + 1] - K[g0] > slen) hi_g = m; else lo_g = m + 1; }
    for (int64_t g = lo_g; g < g1; ++g) {
        const int64_t base = K[g] - K[g0];
        f(g, base, slen);
    }
}

// One lane per selected record: the run that crosses the cut is counted again with the cut and the runs behind it lose their
// rows.
template <class Form>
__global__ __launch_bounds__(BLOCK) void k_hits_fix(SearchPlan P, Form F, const int64_t *__restrict__ K, uint32_t *__restrict__ packed) {
    auto *tab = F.table(P);
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= P.n_sel) return;
    srch_cut(P, K, s, [&](int64_t g, int64_t base, int64_t slen) {
        uint32_t hp = 0, hm = 0;
        const uint32_t kept = (packed[g] >> 18) & 511u;
        if (base < slen && (packed[g] & 0x3FFFFu)) {
            int64_t r, b, lo, hi;
            srch_run(P, g, s, r, b, lo, hi);
            F.template walk<false>(P, tab, b, lo, hi, slen - base, [&](int64_t, const typename Form::Win &w) { hp += F.plus(w); hm += F.minus(w); });
        }
        packed[g] = srch_pack(hp, hm, kept);
    });
}

// list[NZ[g]] = g for every run with a hit (NZ: exclusive prefix of "has a hit")
__global__ __launch_bounds__(BLOCK) void k_search_list(const uint32_t *__restrict__ packed, const int64_t *__restrict__ NZ, int64_t n_runs,
                                                       int64_t *__restrict__ list) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g < n_runs && (packed[g] & 0x3FFFFu)) list[NZ[g]] = g;
}

// The runs of the list walk again and store their rows at Pp[g] + Pm[g] (exclusive prefixes of the + and - counts): by
// position, '+' before '-' at the same position.  Record-local positions: the run's first kept byte (K, segmented) + the kept
// index, moved by the form.  o_col / o_at: the form's column and the address column, where it has them.
template <class Form>
__global__ __launch_bounds__(BLOCK) void k_hits_emit(SearchPlan P, Form F, const int64_t *__restrict__ list, int64_t n_list,
                                                     const int64_t *__restrict__ K, const int64_t *__restrict__ Pp,
                                                     const int64_t *__restrict__ Pm, int64_t *__restrict__ o_rec,
                                                     int64_t *__restrict__ o_pos, int64_t *__restrict__ o_at,
                                                     uint8_t *__restrict__ o_strand, typename Form::Col *__restrict__ o_col) {
    auto *tab = F.table(P);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_list) return;
    const int64_t g = list[i], k = srch_slot(P, g);
    int64_t r, b, lo, hi;
    srch_run(P, g, k, r, b, lo, hi);
    const int64_t base = K[g] - K[P.run0[k]];
    const int64_t first = F.first(P, base);
    int64_t o = Pp[g] + Pm[g];
    F.template walk<true>(P, tab, b, lo, hi, P.slen[r] - base, [&](int64_t kidx, const typename Form::Win &w) {
        auto put = [&](bool minus) {
            o_rec[o] = r;
            o_pos[o] = F.pos(first, kidx, w);
            if constexpr (Form::AT) o_at[o] = w.at;
            o_strand[o] = minus ? '-' : '+';
            if constexpr (Form::COL) o_col[o] = F.col(w, minus);
            ++o;
        };
        if constexpr (Form::ONE) put(F.minus(w));
        else {
            if (F.plus(w)) put(false);
            if (F.minus(w)) put(true);
        }
    });
}

// per selected record: hits on + and - (differences of the run prefixes at the records' first runs)
__global__ __launch_bounds__(BLOCK) void k_search_rec_counts(const int64_t *__restrict__ run0, int64_t n_sel, const int64_t *__restrict__ Pp,
                                                             const int64_t *__restrict__ Pm, int64_t *__restrict__ counts) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n_sel) return;
    const int64_t g0 = run0[k], g1 = run0[k + 1];
    counts[2 * k] = Pp[g1] - Pp[g0];
    counts[2 * k + 1] = Pm[g1] - Pm[g0];
}

// ------------------------------------------------------------------ int64 scans of C components at once
// Loaders: ld(i, v) fills v[0..C) for element i.
struct SrchLdRuns {                       // runs of selected record k
    SearchPlan P;
    __device__ void operator()(int64_t k, int64_t *v) const { int64_t b, e; srch_extent(P, srch_rec(P, k), b, e); v[0] = srch_nruns(b, e); }
};
struct SrchLdKept {
    const uint32_t *p;
    __device__ void operator()(int64_t g, int64_t *v) const { v[0] = (p[g] >> 18) & 511u; }
};
struct SrchLdHits {                       // + hits, - hits, "has a hit"
    const uint32_t *p;
    __device__ void operator()(int64_t g, int64_t *v) const { const uint32_t w = p[g]; v[0] = w & 511u; v[1] = (w >> 9) & 511u; v[2] = (w & 0x3FFFFu) != 0; }
};

__device__ __forceinline__ int64_t wave_incl_scan64(int64_t v) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int lo = __shfl_up((int)(v & 0xFFFFFFFFll), d, 64), hi = __shfl_up((int)(v >> 32), d, 64);
        const int64_t t = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
        if (lane >= d) v += t;
    }
    return v;
}
// inclusive scan over the block (BLOCK = 4 waves); *total = the block's sum.  lds: 4 words.
__device__ __forceinline__ int64_t block_incl_scan64(int64_t v, int64_t *lds, int64_t *total) {
    const int w = threadIdx.x >> 6;
    v = wave_incl_scan64(v);
    __syncthreads();
    if (lane_id() == 63) lds[w] = v;
    __syncthreads();
    int64_t add = 0;
    for (int j = 0; j < w; ++j) add += lds[j];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    return v + add;
}

template <int C, class Ld>
__global__ __launch_bounds__(BLOCK) void k_sscan_sums(Ld ld, int64_t n, int64_t *__restrict__ sums) {
    __shared__ int64_t lds[4];
    int64_t s[C];
    for (int c = 0; c < C; ++c) s[c] = 0;
    const int64_t c0 = (int64_t)blockIdx.x * SRCH_CHUNK;
    for (int i = 0; i < SRCH_PER; ++i) {
        const int64_t idx = c0 + (int64_t)i * BLOCK + threadIdx.x;
        if (idx < n) { int64_t v[C]; ld(idx, v); for (int c = 0; c < C; ++c) s[c] += v[c]; }
    }
    for (int c = 0; c < C; ++c) {
        int64_t tot;
        (void)block_incl_scan64(s[c], lds, &tot);
        if (threadIdx.x == 0) sums[(int64_t)blockIdx.x * C + c] = tot;
    }
}
// one block: sums[nch][C] -> exclusive prefixes in place; totals[C]
template <int C>
__global__ __launch_bounds__(BLOCK) void k_sscan_top(int64_t *__restrict__ sums, int64_t nch, int64_t *__restrict__ totals) {
    __shared__ int64_t lds[4];
    int64_t carry[C];
    for (int c = 0; c < C; ++c) carry[c] = 0;
    for (int64_t b0 = 0; b0 < nch; b0 += BLOCK) {
        const int64_t i = b0 + threadIdx.x;
        for (int c = 0; c < C; ++c) {
            const int64_t v = i < nch ? sums[i * C + c] : 0;
            int64_t tot;
            const int64_t inc = block_incl_scan64(v, lds, &tot);
            if (i < nch) sums[i * C + c] = carry[c] + inc - v;
            carry[c] += tot;
        }
    }
    if (threadIdx.x == 0) for (int c = 0; c < C; ++c) totals[c] = carry[c];
}
// out + c * (n + 1): exclusive prefix of component c, n + 1 entries (the last = the total)
template <int C, class Ld>
__global__ __launch_bounds__(BLOCK) void k_sscan_apply(Ld ld, int64_t n, const int64_t *__restrict__ sums, int64_t *__restrict__ out) {
    __shared__ int64_t lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * SRCH_CHUNK + (int64_t)threadIdx.x * SRCH_PER;
    int64_t s[C];
    for (int c = 0; c < C; ++c) s[c] = 0;
    for (int i = 0; i < SRCH_PER; ++i)
        if (i0 + i < n) { int64_t v[C]; ld(i0 + i, v); for (int c = 0; c < C; ++c) s[c] += v[c]; }
    int64_t run[C];
    for (int c = 0; c < C; ++c) {
        int64_t tot;
        run[c] = block_incl_scan64(s[c], lds, &tot) - s[c] + sums[(int64_t)blockIdx.x * C + c];
    }
    for (int i = 0; i < SRCH_PER && i0 + i < n; ++i) {
        int64_t v[C];
        ld(i0 + i, v);
        for (int c = 0; c < C; ++c) {
            out[c * (n + 1) + i0 + i] = run[c];
            run[c] += v[c];
            if (i0 + i == n - 1) out[c * (n + 1) + n] = run[c];
        }
    }
}

}  // namespace fx
