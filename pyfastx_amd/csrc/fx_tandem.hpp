// fx_tandem.hpp -- perfect tandem repeats (microsatellites) of period 1..8 on the sequence bytes of the resident FASTA table
// (fx_fasta_tandem_repeats).  Extension: the reference has no repeat search; MISA / TRF users slice the genome on the host.
//
// Definition.  The text of a record is what fx_search.hpp walks (bytes 10 / 13 / 32 dropped, cut at slen).  Letters fold to
// A C G T = 0..3 whatever their case; every other byte is invalid and equals nothing.  A repeat of period p is a MAXIMAL
// interval [a, b) of valid letters with t[j] == t[j - p] for every j in [a + p, b), at least max(2 p, p * min_copies[p],
// min_len) long, whose motif t[a : a + p] is primitive (p is the smallest period of the interval).  These are the maximal
// repetitions of stringology with a bounded period: repeats of different periods may overlap and all are reported.
//
// One walk decides everything.  Per period the walk keeps the start of the stretch that is open; letter j BREAKS period p
// when it is invalid or differs from t[j - p] (a letter in front of the record or an invalid one differs from everything).
// A break closes [start_p, j) and opens the next stretch at j - p + 1, moved behind the last invalid letter (at j + 1 when j
// itself is invalid).  The closed stretch is not primitive exactly when a proper divisor q of p has start_q <= start_p at
// that point, so divisors of the periods asked for are tracked too.  Its motif is the last p letters rotated by
// (b - a) mod p: the walk never reads back to a.  The eight compares are one XOR of the history word (eight 4-bit fields,
// the last eight letters) with the letter written into every field.
//
// Passes, in the shape of the class runs of fx_annot.hpp: one lane per 256-byte run of the selected records, geometry and the
// cut from the rank index.
//   k_td_count   fills the history from the (at most 8) kept bytes in front of the run, never past the record's boff, and runs
//                the same walk over them: a start inside those letters is known exactly, one further back is "far" (-8).
//                Over its own letters it notes per tracked period the first break, the start open behind the last break and,
//                for every break after the first, whether a row closes there: that stretch began inside the run or the
//                letters in front, so its length is known, and a divisor's start is either exact or far, which is enough.
//                The row a period's FIRST break closes waits for the carry; only the verdict of the divisors that broke
//                earlier in the same run is noted (one bit), since their starts are gone afterwards.
//   carry        per period a scan of "has a break" (the eight components of k_sscan_*<8>) and the compacted list of those
//                runs (k_td_list): the stretch open at a run's entry starts where the last earlier breaking run of the same
//                record left it, or at 0 -- it may span any number of runs.
//   k_td_close   adds the row of every period's first break (length from the carried start; not primitive when the noted bit
//                is set or a divisor without an earlier break in the run carries a start at or before it) and, in the run
//                that holds the last letter in front of the cut, what the end of the text closes.
//   offsets      one scan of the counts; the host reads the total only.
//   k_td_emit    the runs that close something walk again, now from the exact carried starts, and store (record, start,
//                stop, period, motif) at their offsets: ordered by record, stop, period -- no sort, no atomic.
#pragma once
#include "fx_annot.hpp"

namespace fx {

constexpr int TD_MAXP = 8;                                 // longest period; also the letters of history in front of a run
constexpr uint32_t TD_EACH = 0x11111111u;                  // bit 4 (p - 1): period p
constexpr uint32_t TD_NOFIRST = 511u;
constexpr uint32_t TD_BAD = 4u;                            // the code of an invalid letter (differs from 0..3 in every XOR)

struct TdArg {
    int64_t thr[TD_MAXP];         // a stretch of period p qualifies from this length on: max(2 p, p * min_copies, min_len)
    int32_t slot[TD_MAXP];        // row of period p in the per-run arrays (tracked periods only)
    uint32_t track4, search4;     // bit 4 (p - 1): period p is walked / its rows are reported
};
__device__ __forceinline__ bool td_has(uint32_t m4, int p) { return (m4 >> (4 * (p - 1))) & 1u; }

// per run and tracked period: kept index of the first break (bits 0..8, TD_NOFIRST: none), 8 + the start that is open at the
// run's end relative to its first letter (9..17), "a divisor that broke earlier in the run covers the first break" (18)
__device__ __forceinline__ uint32_t td_pack(uint32_t first, int open, uint32_t covered) {
    return first | ((uint32_t)(open + TD_MAXP) << 9) | (covered << 18);
}
__device__ __forceinline__ uint32_t td_first(uint32_t w) { return w & 511u; }
__device__ __forceinline__ int64_t td_open(uint32_t w) { return (int64_t)((w >> 9) & 511u) - TD_MAXP; }

__device__ __forceinline__ uint32_t td_code(uint32_t ch) {
    const uint32_t f = ch & 0xDFu;
    return f == 'A' ? 0u : f == 'C' ? 1u : f == 'G' ? 2u : f == 'T' ? 3u : TD_BAD;
}

// geometry of selected run q; end: the run holds the last letter in front of the cut (what the end of the text closes is
// closed there -- runs behind the cut are never walked)
struct TdRun : AnRun { bool end; };
__device__ __forceinline__ TdRun td_run(const SearchPlan &P, const RankIndex &X, int64_t q) {
    TdRun R;
    static_cast<AnRun &>(R) = an_run(P, X, q);
    const int64_t g = X.run0[R.r] + (q - P.run0[R.k]);
    R.end = R.base < R.L && R.L <= R.base + (X.pref[g + 1] - X.pref[g]);
    return R;
}

// The walk's state; positions are relative to the run's first letter (T: int in the count pass, int64 where starts are exact).
template <class T> struct TdState {
    T start[TD_MAXP], lastinv;            // start of the open stretch per period; the last invalid letter
    uint32_t hist;                        // field f = the letter f + 1 places back
};
// some proper divisor of p has a stretch open that began at or before sp
template <class T> __device__ __forceinline__ bool td_covered(const TdState<T> &S, int p, T sp) {
    bool k = false;
#pragma unroll
    for (int d = 1; d <= TD_MAXP / 2; ++d) k |= d < p && p % d == 0 && S.start[d - 1] <= sp;
    return k;
}
// One letter at position x.  en4: the periods whose letter p places back is known.  brk(p, x) for every tracked period it
// breaks, in ascending p, all of them before any start moves (a divisor that breaks at the same letter still counts).
template <class T, class F>
__device__ __forceinline__ void td_step(const TdArg &A, TdState<T> &S, uint32_t code, T x, uint32_t en4, F &&brk) {
    const bool valid = code != TD_BAD;
    const uint32_t d = S.hist ^ (code * TD_EACH);
    const uint32_t bm = (valid ? (d | (d >> 1) | (d >> 2)) & en4 : TD_EACH) & A.track4;
    if (bm) {
#pragma unroll
        for (int p = 1; p <= TD_MAXP; ++p)
            if (td_has(bm, p)) brk(p, x);
        const T behind = S.lastinv + 1;
#pragma unroll
        for (int p = 1; p <= TD_MAXP; ++p)
            if (td_has(bm, p)) S.start[p - 1] = valid ? max((T)(x - p + 1), behind) : x + 1;
    }
    if (!valid) S.lastinv = x;
    S.hist = (S.hist << 4) | code;
}
// The state at the run's entry, as far as the (at most 8) letters in front of it tell: the history, and every start that lies
// inside them; a start further back stays at -8 ("far": at or before that letter).  A run within 8 letters of the record's
// start knows everything (letters in front of the record are invalid).
template <class T> __device__ __forceinline__ void td_warm(const SearchPlan &P, const TdArg &A, const TdRun &R, TdState<T> &S) {
    const bool head = R.base <= TD_MAXP;
#pragma unroll
    for (int p = 0; p < TD_MAXP; ++p) S.start[p] = head ? (T)-R.base : (T)-TD_MAXP;
    S.lastinv = head ? (T)(-R.base - 1) : (T)(-TD_MAXP - 1);
    S.hist = TD_BAD * TD_EACH;
    if (R.L - R.base <= 0) return;                          // behind the cut: nothing is walked
    int64_t ws = R.lo;
    int w = 0;
    while (w < TD_MAXP && ws > R.b) {
        --ws;
        w += srch_space(P.base[ws]) ? 0 : 1;
    }
    int x = -w;
    for (int64_t a = ws; a < R.lo; ++a) {
        const uint32_t ch = P.base[a];
        if (srch_space(ch)) continue;
        const int known = x + TD_MAXP;                      // letters of the window in front of this one
        td_step(A, S, td_code(ch), (T)x, head ? TD_EACH : (1u << (4 * known)) - 1u, [](int, T) {});
        ++x;
    }
}
// The kept bytes of the run in front of the cut, in order.
template <class T, class F>
__device__ __forceinline__ void td_walk(const SearchPlan &P, const TdArg &A, const TdRun &R, TdState<T> &S, F &&brk) {
    const int lim = (int)min(R.L - R.base, (int64_t)SRCH_RUN);
    int kidx = 0;
    for (int64_t c = R.lo & ~(int64_t)15; c < R.hi && kidx < lim; c += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t four = w[i];
#pragma unroll 1
            for (int j = 0; j < 4; ++j, four >>= 8) {
                const uint32_t ch = four & 0xFFu;
                const int64_t a = c + 4 * i + j;
                if (a < R.lo || a >= R.hi || srch_space(ch) || kidx >= lim) continue;
                td_step(A, S, td_code(ch), (T)kidx, TD_EACH, brk);
                ++kidx;
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_td_count(SearchPlan P, RankIndex X, TdArg A, uint32_t *__restrict__ pk, uint32_t *__restrict__ closes) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const TdRun R = td_run(P, X, q);
    TdState<int> S;
    td_warm(P, A, R, S);
    uint32_t first[TD_MAXP], covered = 0, n = 0;
#pragma unroll
    for (int p = 0; p < TD_MAXP; ++p) first[p] = TD_NOFIRST;
    td_walk(P, A, R, S, [&](int p, int x) __attribute__((always_inline)) {
        const int sp = S.start[p - 1];
        if (first[p - 1] == TD_NOFIRST) {
            first[p - 1] = (uint32_t)x;
            bool k = false;
#pragma unroll
            for (int d = 1; d <= TD_MAXP / 2; ++d) k |= d < p && p % d == 0 && first[d - 1] < (uint32_t)x && S.start[d - 1] <= sp;
            covered |= (k ? 1u : 0u) << (p - 1);
        } else if (td_has(A.search4, p) && x - sp >= A.thr[p - 1] && !td_covered(S, p, sp)) {
            ++n;
        }
    });
#pragma unroll
    for (int p = 1; p <= TD_MAXP; ++p)
        if (td_has(A.track4, p)) pk[A.slot[p - 1] * P.n_runs + q] = td_pack(first[p - 1], S.start[p - 1], (covered >> (p - 1)) & 1u);
    closes[q] = n;
}

struct TdLdBreak {                        // per period: "the run has a break"
    const uint32_t *pk;
    int64_t n_runs;
    int32_t slot[TD_MAXP];
    uint32_t track4;
    __device__ void operator()(int64_t q, int64_t *v) const {
#pragma unroll
        for (int p = 1; p <= TD_MAXP; ++p) v[p - 1] = td_has(track4, p) && td_first(pk[slot[p - 1] * n_runs + q]) != TD_NOFIRST;
    }
};
struct TdLdCloses {
    const uint32_t *p;
    __device__ void operator()(int64_t q, int64_t *v) const { v[0] = p[q]; }
};
// per tracked period: list[NZ[q]] = q for every run with a break (NZ: component p - 1 of the scan, n_runs + 1 entries each)
__global__ __launch_bounds__(BLOCK) void k_td_list(TdArg A, const uint32_t *__restrict__ pk, const int64_t *__restrict__ NZ, int64_t n_runs,
                                                   int64_t *__restrict__ list) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_runs) return;
#pragma unroll
    for (int p = 1; p <= TD_MAXP; ++p) {
        if (!td_has(A.track4, p)) continue;
        const int64_t row = A.slot[p - 1] * n_runs;
        if (td_first(pk[row + q]) != TD_NOFIRST) list[row + NZ[(p - 1) * (n_runs + 1) + q]] = q;
    }
}
// where the stretch of period p that is open at the entry of run q starts: where the last earlier breaking run of the same
// record left it, or at 0
__device__ __forceinline__ int64_t td_open_start(const SearchPlan &P, const RankIndex &X, const TdArg &A, const TdRun &R, int64_t q, int p,
                                                 const uint32_t *__restrict__ pk, const int64_t *__restrict__ NZ,
                                                 const int64_t *__restrict__ list) {
    const int64_t nz = NZ[(p - 1) * (P.n_runs + 1) + q], row = A.slot[p - 1] * P.n_runs;
    if (nz == 0) return 0;
    const int64_t pr = list[row + nz - 1];
    if (pr < P.run0[R.k]) return 0;
    const int64_t g0 = X.run0[R.r], g = g0 + (pr - P.run0[R.k]);
    return X.pref[g] - X.pref[g0] + td_open(pk[row + pr]);
}

__global__ __launch_bounds__(BLOCK) void k_td_close(SearchPlan P, RankIndex X, TdArg A, const uint32_t *__restrict__ pk,
                                                    const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                    uint32_t *__restrict__ closes) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const TdRun R = td_run(P, X, q);
    uint32_t w[TD_MAXP];
    int64_t cs[TD_MAXP];                                    // the starts carried into the run
#pragma unroll
    for (int p = 1; p <= TD_MAXP; ++p) {
        const bool t = td_has(A.track4, p);
        w[p - 1] = t ? pk[A.slot[p - 1] * P.n_runs + q] : TD_NOFIRST;
        cs[p - 1] = t ? td_open_start(P, X, A, R, q, p, pk, NZ, list) : 0;
    }
    uint32_t n = closes[q];
#pragma unroll
    for (int p = 1; p <= TD_MAXP; ++p) {
        const uint32_t first = td_first(w[p - 1]);
        if (!td_has(A.search4, p) || first == TD_NOFIRST) continue;
        bool k = (w[p - 1] >> 18) & 1u;
#pragma unroll
        for (int d = 1; d <= TD_MAXP / 2; ++d) k |= d < p && p % d == 0 && td_first(w[d - 1]) >= first && cs[d - 1] <= cs[p - 1];
        n += R.base + first - cs[p - 1] >= A.thr[p - 1] && !k ? 1u : 0u;
    }
    if (R.end) {
        int64_t a[TD_MAXP];                                 // the starts open at the end of the text
#pragma unroll
        for (int p = 0; p < TD_MAXP; ++p) a[p] = td_first(w[p]) != TD_NOFIRST ? R.base + td_open(w[p]) : cs[p];
#pragma unroll
        for (int p = 1; p <= TD_MAXP; ++p) {
            if (!td_has(A.search4, p)) continue;
            bool k = false;
#pragma unroll
            for (int d = 1; d <= TD_MAXP / 2; ++d) k |= d < p && p % d == 0 && a[d - 1] <= a[p - 1];
            n += R.L - a[p - 1] >= A.thr[p - 1] && !k ? 1u : 0u;
        }
    }
    closes[q] = n;
}

// t[a : a + p] from the last p letters in front of b = a + len: 2 bits a letter, the first most significant
__device__ __forceinline__ uint32_t td_motif(uint32_t hist, int p, int64_t len) {
    const int m = (int)(len % p);
    uint32_t v = 0;
    for (int i = 0; i < p; ++i) {
        const int idx = i - m + (i < m ? p : 0);            // place of t[a + i] among t[b - p : b)
        v = (v << 2) | ((hist >> (4 * (p - 1 - idx))) & 3u);
    }
    return v;
}

__global__ __launch_bounds__(BLOCK) void k_td_emit(SearchPlan P, RankIndex X, TdArg A, const uint32_t *__restrict__ pk,
                                                   const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                   const uint32_t *__restrict__ closes, const int64_t *__restrict__ O,
                                                   int64_t *__restrict__ o_rec, int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop,
                                                   uint8_t *__restrict__ o_period, uint32_t *__restrict__ o_motif) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs || !closes[q]) return;
    const TdRun R = td_run(P, X, q);
    TdState<int64_t> S;
    td_warm(P, A, R, S);
#pragma unroll
    for (int p = 1; p <= TD_MAXP; ++p)
        if (td_has(A.track4, p)) S.start[p - 1] = td_open_start(P, X, A, R, q, p, pk, NZ, list) - R.base;
    int64_t o = O[q];
    const int64_t o_end = O[q + 1];
    auto put = [&](int p, int64_t x) __attribute__((always_inline)) {
        const int64_t sp = S.start[p - 1];
        if (!td_has(A.search4, p) || x - sp < A.thr[p - 1] || td_covered(S, p, sp) || o >= o_end) return;
        o_rec[o] = R.r;
        o_start[o] = R.base + sp;
        o_stop[o] = R.base + x;
        o_period[o] = (uint8_t)p;
        o_motif[o] = td_motif(S.hist, p, x - sp);
        ++o;
    };
    td_walk(P, A, R, S, put);
    if (R.end) {
#pragma unroll
        for (int p = 1; p <= TD_MAXP; ++p) put(p, R.L - R.base);
    }
}

}  // namespace fx
