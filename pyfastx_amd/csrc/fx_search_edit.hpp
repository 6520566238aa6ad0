// fx_search_edit.hpp -- every place where one pattern (1..64 letters) ends within k edits (Levenshtein distance: substitutions,
// insertions and deletions, 1 each) on the sequence bytes of the resident FASTA table, with its distance and the start of its
// shortest span (fx_fasta_search_edit).  Extension of fx_search.hpp the way fx_search_approx.hpp is one: the run layout, the
// per-run word, the scans, the cut at slen and the run list are that header's, unchanged; what is new is the automaton, the
// filter of the rows and the pass that finds the starts.
//
// Automaton.  Myers' bit-vector form of Sellers' column: D[i] = the least distance between the pattern's first i letters and a
// stretch of text that ends at the current letter (D[0] = 0: a stretch may begin anywhere).  Pv / Mv hold the vertical
// differences D[i] - D[i-1] = +1 / -1 at bit i - 1, `score` is D[L].  Before the record's first letter D[i] = i: Pv = the L low
// bits, Mv = 0, score = L.  One step per kept byte c, Eq = M[c] (the mask table of fx_search.hpp), mask = the L low bits,
// top = 1 << (L - 1):
//     Xv = Eq | Mv                       Xh = ((((Eq & Pv) + Pv) ^ Pv) | Eq) & mask
//     Ph = (Mv | ~(Xh | Pv)) & mask      Mh = Pv & Xh
//     score += (Ph & top) != 0           score -= (Mh & top) != 0
//     Ph = (Ph << 1) & mask              Mh = (Mh << 1) & mask
//     Pv = (Mh | ~(Xv | Ph)) & mask      Mv = Ph & Xv
// A letter is an END when score <= k afterwards, and score is its `edits`; k is compared at run time, there is one kernel for
// every budget.  A strand that is not searched has an empty table: score stays L > k.
//
// Warm-up.  A stretch within k edits of the pattern has at most L + k letters, so whether a letter is an end, and its edits
// when it is one, is a function of the last L + k kept letters: min(score, k + 1) after a walk that starts from the state
// above L + k kept bytes in front of the run (fewer at the record's boff, where a single walk over the record starts from that
// state too) equals that of the single walk.  Above k the two may differ, and nothing reads a score above k.  The L - 1 bytes
// of fx_search.hpp are not enough here: a site with an insertion reaches further back than L letters.
//
// Forms.  L <= 32: a 32-bit Pv / Mv per strand, so the add never carries from one strand into the other; the two strands'
// masks share one 64-bit LDS entry (the narrow table of fx_search_approx.hpp).  L > 32: 64-bit words.
//
// Rows.  k_hits_emit with EditForm stores per end the record, the stop (the run's first base from K + the kept index + 1), the strand,
// the edits and the byte address of the end letter, by (record, stop), '+' before '-' at one stop.  report = best:
// k_esearch_best flags the ends that are the leftmost minimum of their dip -- the neighbour on the same strand, one letter to
// either side, lies within two rows because at most one row of the other strand sits between them -- and a scan of the flags
// gives the list of the rows that stay.  k_esearch_start: one lane per row that stays walks back from the end letter over at
// most L + k kept bytes, never in front of boff, and steps the same column ANCHORED at the end (row 0 grows by one per letter:
// Ph = ((Ph << 1) | 1) & mask) with the reversed pattern (bit j of M[c] read as position L - 1 - j): after m letters score =
// the distance between the pattern and the last m letters.  The first m whose score is the row's edits is the shortest span,
// start = stop - m; m = 0 never is, since edits <= k < L.
#pragma once
#include <type_traits>

#include "fx_search_approx.hpp"

namespace fx {

template <bool WIDE> using esrch_word_t = std::conditional_t<WIDE, uint64_t, uint32_t>;

// One strand's column.  carry: 0 for the search (a stretch may begin anywhere), 1 for the anchored form of the start pass.
template <class W>
struct EdCol {
    W Pv, Mv;
    int score;
    __device__ __forceinline__ EdCol(W mask, int L) : Pv(mask), Mv(0), score(L) {}
    __device__ __forceinline__ void step(W Eq, W mask, W top, W carry) {
        const W Xv = Eq | Mv;
        const W Xh = ((((Eq & Pv) + Pv) ^ Pv) | Eq) & mask;
        W Ph = (Mv | ~(Xh | Pv)) & mask;
        W Mh = Pv & Xh;
        score += (Ph & top) ? 1 : 0;
        score -= (Mh & top) ? 1 : 0;
        Ph = ((Ph << 1) | carry) & mask;
        Mh = (Mh << 1) & mask;
        Pv = (Mh | ~(Xv | Ph)) & mask;
        Mv = Ph & Xv;
    }
};

// srch_walk with the two columns: after a warm-up on the L + k kept bytes in front of the run, the ends among the kept bytes
// whose local index is below `limit` go to on_end(kidx, address of the byte, end on +, end on -, edits on +, edits on -) (the
// edits of a strand that has no end there mean nothing).  -> kept bytes in [lo, hi).
template <bool WIDE, class F>
__device__ __forceinline__ uint32_t esrch_walk(const SearchPlan &P, int k, const asrch_tab_t<WIDE> *tab, int64_t b, int64_t lo, int64_t hi,
                                               int64_t limit, F &&on_end) {
    using W = esrch_word_t<WIDE>;
    const int L = P.plen;
    const W mask = (W)(~(W)0 >> ((int)sizeof(W) * 8 - L)), top = (W)1 << (L - 1);
    EdCol<W> f(mask, L), r(mask, L);
    auto step = [&](uint32_t c) {
        if constexpr (WIDE) {
            const ulonglong2 m = tab[c];
            f.step(m.x, mask, top, 0);
            r.step(m.y, mask, top, 0);
        } else {
            const uint64_t m = tab[c];
            f.step((uint32_t)m, mask, top, 0);
            r.step((uint32_t)(m >> 32), mask, top, 0);
        }
    };
    run_warm(P, b, lo, L + k, step);
    int64_t kidx = 0;
    run_walk_at(P, lo, hi, [&](uint32_t c, int64_t at) {
        step(c);
        const bool ef = f.score <= k, er = r.score <= k;
        if ((ef | er) && kidx < limit) on_end(kidx, at, ef, er, (uint32_t)f.score, (uint32_t)r.score);
        ++kidx;
    });
    return (uint32_t)kidx;
}

// The form of the three passes (k_hits_count / _fix / _emit of fx_search.hpp): a row is an END, by stop (the run's first base
// from K + the kept index + 1), with its edits and the address of the end letter (address space of the plan: P.base[at] is the
// letter), for k_esearch_start.
template <bool WIDE>
struct EditForm {
    struct Win { int64_t at; bool ef, er; uint32_t df, dr; };
    using Col = uint8_t;
    static constexpr bool COL = true, AT = true, ONE = false;
    int k;
    __device__ __forceinline__ const asrch_tab_t<WIDE> *table(const SearchPlan &P) const {
        __shared__ asrch_tab_t<WIDE> tab[256];
        asrch_load_tab<WIDE>(P, tab);
        __syncthreads();
        return tab;
    }
    template <bool ROWS, class F>
    __device__ __forceinline__ uint32_t walk(const SearchPlan &P, const asrch_tab_t<WIDE> *tab, int64_t b, int64_t lo, int64_t hi, int64_t limit,
                                             F &&on) const {
        return esrch_walk<WIDE>(P, k, tab, b, lo, hi, limit,
                                [&](int64_t kidx, int64_t at, bool ef, bool er, uint32_t df, uint32_t dr) { on(kidx, Win{at, ef, er, df, dr}); });
    }
    __device__ __forceinline__ bool plus(const Win &w) const { return w.ef; }
    __device__ __forceinline__ bool minus(const Win &w) const { return w.er; }
    __device__ __forceinline__ int64_t first(const SearchPlan &, int64_t base) const { return base; }
    __device__ __forceinline__ int64_t pos(int64_t first, int64_t kidx, const Win &) const { return first + kidx + 1; }
    __device__ __forceinline__ Col col(const Win &w, bool minus) const { return (uint8_t)(minus ? w.dr : w.df); }
};

// report = best: keep[i] = 1 where end i is the leftmost minimum of its dip -- the end one letter to the left on the same
// strand (if there is one) has more edits, the one to the right (if there is one) has no fewer.  Rows of one record and strand
// whose stops differ by one are at most two rows apart.  The record id tells the records apart even where a selection names
// one record twice: between a row of the first copy and a row with a larger stop of the second lie that row's own twin and
// the first row's, so they are three rows apart or more.
__global__ __launch_bounds__(BLOCK) void k_esearch_best(const int64_t *__restrict__ rec, const int64_t *__restrict__ stop,
                                                        const uint8_t *__restrict__ strand, const uint8_t *__restrict__ edits, int64_t n,
                                                        uint8_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rec[i], s = stop[i];
    const uint8_t st = strand[i];
    const int d = edits[i];
    auto neighbour = [&](int dir) {                          // its edits, or -1 where that letter is no end
        for (int j = 1; j <= 2; ++j) {
            const int64_t q = i + dir * j;
            if (q < 0 || q >= n) break;
            if (rec[q] == r && strand[q] == st && stop[q] == s + dir) return (int)edits[q];
        }
        return -1;
    };
    const int left = neighbour(-1), right = neighbour(1);
    keep[i] = (left < 0 || left > d) && (right < 0 || right >= d);
}
struct EdLdKeep {                         // rows kept on +, on -
    const uint8_t *keep, *strand;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = keep[i] && strand[i] == '+'; v[1] = keep[i] && strand[i] == '-'; }
};
// per selected record: rows kept on + and on -.  The ends of slot s are the rows Pp[g] + Pm[g] of its runs; F: the exclusive
// prefixes of EdLdKeep, two arrays of n + 1.
__global__ __launch_bounds__(BLOCK) void k_esearch_rec_counts(const int64_t *__restrict__ run0, int64_t n_sel, const int64_t *__restrict__ Pp,
                                                              const int64_t *__restrict__ Pm, const int64_t *__restrict__ F, int64_t n,
                                                              int64_t *__restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_sel) return;
    const int64_t a = Pp[run0[s]] + Pm[run0[s]], e = Pp[run0[s + 1]] + Pm[run0[s + 1]];
    counts[2 * s] = F[e] - F[a];
    counts[2 * s + 1] = F[n + 1 + e] - F[n + 1 + a];
}

// One lane per row that stays (pos: their indices among the ends; null: every end): the start of the shortest span with the
// row's edits, and the row at its place in the answer.
__global__ __launch_bounds__(BLOCK) void k_esearch_start(SearchPlan P, int k, const int64_t *__restrict__ pos, int64_t n_rows,
                                                         const int64_t *__restrict__ e_rec, const int64_t *__restrict__ e_stop,
                                                         const int64_t *__restrict__ e_at, const uint8_t *__restrict__ e_strand,
                                                         const uint8_t *__restrict__ e_edits, int64_t *__restrict__ o_rec,
                                                         int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop,
                                                         uint8_t *__restrict__ o_strand, uint8_t *__restrict__ o_edits) {
    __shared__ ulonglong2 tab[256];
    srch_load_tab<true>(P, tab);
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_rows) return;
    const int64_t i = pos ? pos[j] : j;
    const int64_t r = e_rec[i], b = P.boff[r] + P.mis;
    const bool minus = e_strand[i] == '-';
    const int L = P.plen, d = e_edits[i];
    const uint64_t mask = ~0ull >> (64 - L), top = 1ull << (L - 1);
    EdCol<uint64_t> col(mask, L);
    int best = L, best_m = 0;
    int64_t p = e_at[i];                                     // a kept byte at or behind b
    for (int m = 1; m <= L + k; ++m) {
        const ulonglong2 t = tab[P.base[p]];
        col.step(__brevll(minus ? t.y : t.x) >> (64 - L), mask, top, 1);
        if (col.score < best) { best = col.score; best_m = m; }
        if (best <= d) break;
        do --p; while (p >= b && srch_space(P.base[p]));     // the kept byte in front of it
        if (p < b) break;
    }
    o_rec[j] = r; o_start[j] = e_stop[i] - best_m; o_stop[j] = e_stop[i]; o_strand[j] = e_strand[i]; o_edits[j] = (uint8_t)d;
}

}  // namespace fx
