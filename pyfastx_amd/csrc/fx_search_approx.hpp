// fx_search_approx.hpp -- every window of L kept letters that differs from one pattern (1..64 letters) at no more than d
// positions (Hamming distance, substitutions only), with its distance, on the sequence bytes of the resident FASTA table
// (fx_fasta_search_approx).  Extension of fx_search.hpp: the run layout, the per-run word, the scans, the cut at slen and the
// run list are that header's, unchanged; what is new is the automaton and the mismatch column.
//
// Automaton.  Shift-And with d + 1 state words R_0 .. R_d.  M[c]: the mask of byte c (fx_search.hpp), X: the anchored
// positions (no mismatch allowed there), sh(R) = (R << 1) | 1, R_j the words before the step:
//     R_0' = sh(R_0) & M[c]
//     R_j' = (sh(R_j) & M[c]) | (sh(R_{j-1}) & ~X)                j = 1..d
// Bit i of R_j is set exactly when the last i + 1 kept letters match the pattern's first i + 1 letters with at most j
// mismatches, none of them at an anchored position.  The levels are nested (R_j is a subset of R_{j+1}), so the count pass
// tests bit L - 1 of R_d alone, and the distance of a hit is the number of levels below d whose bit L - 1 is clear.
//
// Warm-up.  Bit i after a step is a function of the last i + 1 kept letters and of nothing else: it comes from bit i - 1 of
// the step before (or from the constant 1 at i = 0), and ~X is cut to the L positions of the pattern, so no bit at or above
// L is ever set.  The hit test reads bit L - 1, that is the last L letters; the state a run starts from holds bits 0..L - 2,
// that is the last L - 1 letters.  Walking the L - 1 kept bytes in front of the run from the zero state (fewer at the
// record's boff, where a single walk over the record starts from zero too) therefore gives exactly the state of a single
// walk, for every level: the warm-up rule of fx_search.hpp is exact as it stands.
//
// Forms.  L <= 32: both strands in one 64-bit word per level, forward in the low half, reverse in the high half;
// sh(R) = (R << 1) | 0x100000001 -- the carry out of bit 31 lands on bit 32, which is set anyway -- and X = forward anchor |
// mirrored anchor << 32: 2 VGPRs per level.  L > 32: one word per strand and level, 4 VGPRs per level.  The '-' strand is
// searched with the reverse pattern, so its anchor is the mirror: position j becomes L - 1 - j.
//
// Levels in registers.  The kernels are templates on the level count NLEV (1, 2, 3, 5, 9), fully unrolled, every index a
// compile-time constant; a call runs the smallest NLEV >= d + 1.  The NLEV - 1 - d spare levels sit at the bottom and get no
// injection from the level below them (their ~X is 0): they repeat R_0, and level NLEV - 1 is R_d.
#pragma once
#include <type_traits>

#include "fx_search.hpp"

namespace fx {

struct ApproxArg {
    uint64_t nxf, nxr;            // positions where a mismatch may fall (bits 0..L-1 minus the anchor; 0: strand not searched):
                                  // narrow: nxf = forward | reverse << 32 (nxr unused); wide: forward, reverse
    int d;                        // mismatches allowed
};

template <bool WIDE> using asrch_tab_t = std::conditional_t<WIDE, ulonglong2, uint64_t>;

// The LDS copy of the masks: narrow: forward | reverse << 32; wide: as given.
template <bool WIDE>
__device__ __forceinline__ void asrch_load_tab(const SearchPlan &P, asrch_tab_t<WIDE> *tab) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        const ulonglong2 m = P.masks[i];
        if constexpr (WIDE) tab[i] = m; else tab[i] = m.x | (m.y << 32);
    }
}

// srch_walk (run_warm and run_walk of fx_search.hpp) with the d + 1 levels: hits go to on_hit(kidx, fwd, rev, dist_fwd, dist_rev) (the distances only under DIST,
// and only that of a strand that hit means anything).  -> kept bytes in [lo, hi).
template <bool WIDE, int NLEV, bool DIST, class F>
__device__ __forceinline__ uint32_t asrch_walk(const SearchPlan &P, const ApproxArg &A, const asrch_tab_t<WIDE> *tab, int64_t b, int64_t lo,
                                               int64_t hi, int64_t limit, F &&on_hit) {
    const int L = P.plen;
    const int spare = NLEV - 1 - A.d;                        // levels 0..spare repeat R_0
    uint64_t Rf[NLEV], Rr[NLEV], nf[NLEV], nr[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; ++i) {
        Rf[i] = Rr[i] = 0;
        nf[i] = i > spare ? A.nxf : 0ull;
        nr[i] = i > spare ? A.nxr : 0ull;
    }
    auto step = [&](uint32_t c) {                            // top level first: level i still sees level i - 1 from before the step
        if constexpr (WIDE) {
            const ulonglong2 m = tab[c];
#pragma unroll
            for (int i = NLEV - 1; i > 0; --i) {
                Rf[i] = (((Rf[i] << 1) | 1ull) & m.x) | (((Rf[i - 1] << 1) | 1ull) & nf[i]);
                Rr[i] = (((Rr[i] << 1) | 1ull) & m.y) | (((Rr[i - 1] << 1) | 1ull) & nr[i]);
            }
            Rf[0] = ((Rf[0] << 1) | 1ull) & m.x;
            Rr[0] = ((Rr[0] << 1) | 1ull) & m.y;
        } else {
            const uint64_t m = tab[c];
#pragma unroll
            for (int i = NLEV - 1; i > 0; --i)
                Rf[i] = (((Rf[i] << 1) | 0x100000001ull) & m) | (((Rf[i - 1] << 1) | 0x100000001ull) & nf[i]);
            Rf[0] = ((Rf[0] << 1) | 0x100000001ull) & m;
        }
    };
    run_warm(P, b, lo, L - 1, step);
    const int shf = L - 1, shr = WIDE ? L - 1 : 31 + L;
    int64_t kidx = 0;
    run_walk(P, lo, hi, [&](uint32_t c) {
        step(c);
        const uint32_t f = (uint32_t)(Rf[NLEV - 1] >> shf) & 1u, r = (uint32_t)((WIDE ? Rr[NLEV - 1] : Rf[NLEV - 1]) >> shr) & 1u;
        if ((f | r) && kidx < limit) {
            uint32_t df = 0, dr = 0;
            if constexpr (DIST) {
#pragma unroll
                for (int i = 0; i < NLEV - 1; ++i) {         // levels spare..NLEV-2 are R_0..R_{d-1}
                    const uint32_t on = i >= spare ? 1u : 0u;
                    df += on & ~(uint32_t)(Rf[i] >> shf) & 1u;
                    dr += on & ~(uint32_t)((WIDE ? Rr[i] : Rf[i]) >> shr) & 1u;
                }
            }
            on_hit(kidx, f, r, df, dr);
        }
        ++kidx;
    });
    return (uint32_t)kidx;
}

// The form of the three passes (k_hits_count / _fix / _emit of fx_search.hpp): the level words, the mismatch column.
template <bool WIDE, int NLEV>
struct ApproxForm {
    struct Win { uint32_t f, r, df, dr; };
    using Col = uint8_t;
    static constexpr bool COL = true, AT = false, ONE = false;
    ApproxArg A;
    __device__ __forceinline__ const asrch_tab_t<WIDE> *table(const SearchPlan &P) const {
        __shared__ asrch_tab_t<WIDE> tab[256];
        asrch_load_tab<WIDE>(P, tab);
        __syncthreads();
        return tab;
    }
    template <bool ROWS, class F>
    __device__ __forceinline__ uint32_t walk(const SearchPlan &P, const asrch_tab_t<WIDE> *tab, int64_t b, int64_t lo, int64_t hi, int64_t limit,
                                             F &&on) const {
        return asrch_walk<WIDE, NLEV, ROWS>(P, A, tab, b, lo, hi, limit,
                                            [&](int64_t kidx, uint32_t f, uint32_t rv, uint32_t df, uint32_t dr) { on(kidx, Win{f, rv, df, dr}); });
    }
    __device__ __forceinline__ uint32_t plus(const Win &w) const { return w.f; }
    __device__ __forceinline__ uint32_t minus(const Win &w) const { return w.r; }
    __device__ __forceinline__ int64_t first(const SearchPlan &P, int64_t base) const { return base - P.plen + 1; }
    __device__ __forceinline__ int64_t pos(int64_t first, int64_t kidx, const Win &) const { return first + kidx; }
    __device__ __forceinline__ Col col(const Win &w, bool minus) const { return (uint8_t)(minus ? w.dr : w.df); }
};

}  // namespace fx
