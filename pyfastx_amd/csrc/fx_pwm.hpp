// fx_pwm.hpp -- every window of W kept letters (1..64) whose score under one position weight matrix reaches a threshold, on
// both strands, with its score, and the best window of every record (fx_fasta_pwm_scan, fx_fasta_pwm_best), on the sequence
// bytes of the resident FASTA table.  Extension of fx_search.hpp: the run layout, the per-run word, the scans, the cut at slen
// and the run list are that header's, unchanged; what is new is the per-letter state, the score tables in LDS, the score
// column and the per-record maximum.
//
// Text and letters.  The text is the one fx_fasta_search walks.  A C G T in either case and U / u (= T) are the codes 0..3;
// every other kept byte is INVALID: a window that holds one has no score on either strand.  mat[j][c]: the weight of code c at
// position j of the motif.  The '+' score of the window x[s .. s + W) is sum_j mat[j][x[s + j]]; its '-' score is the score of
// its reverse complement, sum_j mat[W - 1 - j][3 - x[s + j]].  All of it int32: |score| <= 64 * 32767 < 2^21.
//
// State.  Per lane a HISTORY of the 2-bit codes of the last 64 letters, newest in the low bits (one 64-bit word while
// W <= 32, two beyond), and CNT, the number of consecutive valid letters that end here, saturating at 64.  An invalid letter
// sets CNT to 0 (what it pushes into the history is never read: a window is scored only when CNT >= W, and then its W newest
// history entries are all codes of valid letters).
//
// Warm-up.  The test at a letter reads the last W letters: CNT >= W and the W newest history entries.  The state a run starts
// from has to answer for the last W - 1 of them.  Walking the W - 1 kept bytes in front of the run from the empty state (fewer
// at the record's boff, where a single walk over the record starts empty too) gives exactly their codes in the history, and
// CNT = min(true CNT, W - 1): where the true count is larger, all W - 1 bytes are valid, and W - 1 + i >= W holds at the i-th
// letter of the run exactly when the true count says so; where it is smaller the invalid letter lies inside the W - 1 bytes
// and the count is the true one.  The warm-up rule of fx_search.hpp is exact as it stands.
//
// Score tables.  G = ceil(W / 4) tables of 256 entries in LDS: entry [g][code8] = {forward partial, reverse partial} of the
// history positions 4g .. 4g + 3 holding the four codes of code8 (position p of the history is position W - 1 - p of the
// window; the positions >= W of a ragged last group add 0).  Per scorable letter G reads of 8 bytes at (history >> 8g) & 255
// and two adds each; one read serves both strands, so the strand that was not asked for costs one add per read and is left
// in.  G * 2 KiB of LDS, 32 KiB at W = 64.  The kernels are templates on G (1..16), the loop over the groups fully unrolled;
// G > 8 is the two-word form.
//
// Best.  k_pwm_best packs the best scorable window of a run (larger score, then smaller start) into one 64-bit key per
// strand, (score + 2^23) << 40 | (2^40 - 1 - start), and reduces the keys per (record, strand) with a 64-bit atomicMax in
// global memory; 0 means "no scorable window".  A block whose lanes all belong to one record reduces in the block first (wave
// shuffles, then LDS) and sends one atomic per strand.  A maximum does not depend on the order it is taken in.
#pragma once
#include "fx_search.hpp"

namespace fx {

constexpr int32_t PWM_NEVER = INT32_MAX;                   // the threshold of a strand that is not searched
constexpr int PWM_START_BITS = 40;
constexpr int64_t PWM_BIAS = (int64_t)1 << 23;

struct PwmArg {
    const int2 *tab;              // [G][256]: .x forward partial, .y reverse partial
    int32_t thr_f, thr_r;         // a window hits on + (-) when its score is >= thr_f (thr_r); PWM_NEVER: strand not searched
};

template <int G> constexpr int pwm_lds() { return G ? G * 256 : 1; }
template <int G>
__device__ __forceinline__ void pwm_load_tab(const PwmArg &A, int2 *tab) {
    for (int i = threadIdx.x; i < G * 256; i += blockDim.x) tab[i] = A.tab[i];
}

__device__ __forceinline__ unsigned long long pwm_key(int32_t score, int64_t start) {
    return ((unsigned long long)(score + PWM_BIAS) << PWM_START_BITS) | (unsigned long long)((((int64_t)1 << PWM_START_BITS) - 1) - start);
}

// srch_walk (run_warm and run_walk of fx_search.hpp) with the history: every scorable window that ends at a kept byte whose local index (0 at lo) is below `limit`
// goes to on_win(kidx, score on +, score on -).  G = 0: nothing is scored, the kept bytes are counted.  -> kept bytes in [lo, hi).
template <int G, class F>
__device__ __forceinline__ uint32_t pwm_walk(const SearchPlan &P, const int2 *tab, int64_t b, int64_t lo, int64_t hi, int64_t limit,
                                             F &&on_win) {
    constexpr bool WIDE = G > 8;
    const int W = P.plen;
    uint64_t h0 = 0, h1 = 0;
    int cnt = 0;
    auto step = [&](uint32_t c) {
        const uint32_t v = (c & 0xDFu) - 0x41u;              // 'A'..'U' -> 0..20
        const bool ok = v <= 20u && ((0x180045u >> v) & 1u); // A C G T U
        const uint32_t q = (c >> 1) & 3u;                    // A 0, C 1, T / U 2, G 3
        if (WIDE) h1 = (h1 << 2) | (h0 >> 62);
        h0 = (h0 << 2) | (q ^ (q >> 1));
        cnt = ok ? min(cnt + 1, 64) : 0;
    };
    run_warm(P, b, lo, W - 1, step);
    int64_t kidx = 0;
    run_walk(P, lo, hi, [&](uint32_t c) {
        step(c);
        if (G > 0 && cnt >= W && kidx < limit) {
            int32_t sf = 0, sr = 0;
            uint64_t t = h0;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g == 8) t = h1;
                const int2 e = tab[g * 256 + (int)(t & 0xFFu)];
                t >>= 8;
                sf += e.x;
                sr += e.y;
            }
            on_win(kidx, sf, sr);
        }
        ++kidx;
    });
    return (uint32_t)kidx;
}

// The form of the three passes (k_hits_count / _fix / _emit of fx_search.hpp): the thresholds decide what is a row, the score
// is its column.  G = 0: the kept bytes alone (what k_pwm_best needs before it can place the cut).
template <int G>
struct PwmForm {
    struct Win { int32_t sf, sr; };
    using Col = int32_t;
    static constexpr bool COL = true, AT = false, ONE = false;
    PwmArg A;
    __device__ __forceinline__ const int2 *table(const SearchPlan &) const {
        __shared__ int2 tab[pwm_lds<G>()];
        pwm_load_tab<G>(A, tab);
        __syncthreads();
        return tab;
    }
    template <bool ROWS, class F>
    __device__ __forceinline__ uint32_t walk(const SearchPlan &P, const int2 *tab, int64_t b, int64_t lo, int64_t hi, int64_t limit, F &&on) const {
        return pwm_walk<G>(P, tab, b, lo, hi, limit, [&](int64_t kidx, int32_t sf, int32_t sr) { on(kidx, Win{sf, sr}); });
    }
    __device__ __forceinline__ uint32_t plus(const Win &w) const { return w.sf >= A.thr_f ? 1u : 0u; }
    __device__ __forceinline__ uint32_t minus(const Win &w) const { return w.sr >= A.thr_r ? 1u : 0u; }
    __device__ __forceinline__ int64_t first(const SearchPlan &P, int64_t base) const { return base - P.plen + 1; }
    __device__ __forceinline__ int64_t pos(int64_t first, int64_t kidx, const Win &) const { return first + kidx; }
    __device__ __forceinline__ Col col(const Win &w, bool minus) const { return minus ? w.sr : w.sf; }
};

__device__ __forceinline__ unsigned long long pwm_wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(v & 0xFFFFFFFFull), d, 64), hi = (unsigned)__shfl_xor((int)(v >> 32), d, 64);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        v = t > v ? t : v;
    }
    return v;
}

// per run the best scorable window of each strand in front of the cut, as a key (pwm_key); keys[2 * k + s] = the maximum over
// the runs of selected record k (0: none; the caller zeroes keys).  K: exclusive prefix of the kept counts (n_runs + 1).
template <int G>
__global__ __launch_bounds__(BLOCK) void k_pwm_best(SearchPlan P, PwmArg A, const int64_t *__restrict__ K, unsigned long long *__restrict__ keys) {
    __shared__ int2 tab[pwm_lds<G>()];
    __shared__ int64_t ends[2];                              // the slots of the block's first and last run
    __shared__ unsigned long long red[2][BLOCK / 64];
    pwm_load_tab<G>(A, tab);
    __syncthreads();
    const int64_t g0 = (int64_t)blockIdx.x * BLOCK, g = g0 + threadIdx.x;
    const int64_t g_last = min(g0 + BLOCK, P.n_runs) - 1;
    int64_t k = -1;
    unsigned long long kf = 0, kr = 0;
    if (g <= g_last) {
        k = srch_slot(P, g);
        int64_t r, b, lo, hi;
        srch_run(P, g, k, r, b, lo, hi);
        const int64_t base = K[g] - K[P.run0[k]];
        const int64_t first = base - P.plen + 1;
        int32_t bf = INT32_MIN, br = INT32_MIN;
        int64_t pf = 0, pr = 0;
        pwm_walk<G>(P, tab, b, lo, hi, P.slen[r] - base, [&](int64_t kidx, int32_t sf, int32_t sr) {
            if (sf > bf) { bf = sf; pf = kidx; }             // strictly larger: the earliest start keeps a tie
            if (sr > br) { br = sr; pr = kidx; }
        });
        if (bf != INT32_MIN) {                               // a scorable window has a score on both strands
            if (A.thr_f != PWM_NEVER) kf = pwm_key(bf, first + pf);
            if (A.thr_r != PWM_NEVER) kr = pwm_key(br, first + pr);
        }
        if (g == g0) ends[0] = k;
        if (g == g_last) ends[1] = k;
    }
    __syncthreads();
    if (ends[0] != ends[1]) {                                // records meet inside the block: every run for itself
        if (kf) atomicMax(&keys[2 * k], kf);
        if (kr) atomicMax(&keys[2 * k + 1], kr);
        return;
    }
    kf = pwm_wave_max(kf);
    kr = pwm_wave_max(kr);
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = kf; red[1][threadIdx.x >> 6] = kr; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long m = 0;
        for (int w = 0; w < BLOCK / 64; ++w) m = red[threadIdx.x][w] > m ? red[threadIdx.x][w] : m;
        if (m) atomicMax(&keys[2 * ends[0] + threadIdx.x], m);
    }
}

}  // namespace fx
