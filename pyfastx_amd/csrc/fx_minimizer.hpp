// fx_minimizer.hpp -- the (w, k) minimizers of the records of the resident FASTA table (fx_fasta_minimizers): of every w
// consecutive k-mers the smallest one, each distinct choice once, with its strand and its code.  Extension: the reference has
// no k-mer of any kind.  The run layout, the per-run word, the scans, the cut at slen and the run list are those of
// fx_search.hpp, the rolling code is KmerRoll<uint64_t> of fx_kmer.hpp; what is new is the sliding minimum and its carry
// across run boundaries.
//
// Definition (include/fxgpu.h has it in full).  Position p of a record holds the k-mer seq[p .. p + k); it is VALID when all
// its letters are ACGTacgt (kmer_code).  code = min(fw, rc) (canonical; strand '-' when rc < fw) or fw; key = code (lex) or
// mz_mix(code) (hash), a bijection of the 2k-bit words, so equal keys mean equal codes.  Window j holds the positions
// j .. j + w - 1; its SELECTION is the leftmost position with the smallest key among its valid ones.  The rows are the
// distinct selections of a record's windows.  Selections never move left as j grows, so the rows are the windows whose
// selection exists and differs from that of the window in front: a lane emits in order, without a sort.
//
// Ownership.  A lane owns the windows whose LAST k-mer ENDS at a kept byte of its run (kept index i: the window's last
// position is i - k + 1, its first i - k - w + 2).  It emits at i iff the window exists, has a selection, and the window that
// ends at i - 1 has none or another one.  The start of a row may therefore lie in the run in front:
// start = base + i - (k - 1) - age, base the record-local index of the run's first kept byte (the segmented prefix K).
//
// State, all of it a function of the last w + k - 1 kept bytes (fewer at the record's first byte):
//   roll       fw, rc and the count of valid letters in a row (capped at k)
//   ring       the keys of the last w positions, MZ_NONE for a position without a valid k-mer: one column of 64-bit words per
//              lane in LDS, laid out [slot][thread], so the lanes of a wave sit on distinct bank pairs whatever their slots
//   mn, age    the smallest key of the ring and how many positions back its leftmost holder lies.  A new key takes over only
//              when strictly smaller (the leftmost keeps a tie); when the holder leaves the window (age == w) the lane reads
//              its w ring slots again, oldest first.  mn == MZ_NONE: no valid k-mer in the window, no selection.
//   hist       the strand bits of the last 32 positions (bit a: a positions back)
//   fed        kept bytes fed, capped at w + k - 1: a k-mer exists from k on, a window from w + k - 1 on
// Carry.  The lane warms up on the w + k - 1 kept bytes in front of its run (run_warm; fewer at the record's boff, where a
// single walk starts empty too).  After them roll, ring, (mn, age) and fed are those of a single walk over the record: the
// oldest of the last w positions' k-mers begins at the first warm-up byte, the k - 1 slots fed before it hold MZ_NONE and
// have left the ring by then, and (mn, age) is at every step the leftmost minimum of the ring by construction.  The window
// that ends at the last warm-up byte is the "window in front" of the run's first one.
//
// LDS: BLOCK * w * 8 bytes of dynamic shared memory, 20 KiB at w = 10, 64 KiB at w = 32; no slot is read before it was
// written (a holder that ages out was set w steps ago, and every step writes one slot).
#pragma once
#include "fx_kmer.hpp"

namespace fx {

constexpr int MZ_MAX_K = 31, MZ_MAX_W = 32;
constexpr uint64_t MZ_NONE = ~0ull;                          // no key: every key is below 4^31

// key = mz_mix(code) on 2k-bit words, m = 4^k - 1: multiply by 2^21 - 1 and subtract 1, xorshift 24, multiply by 265,
// xorshift 14, multiply by 21, xorshift 28, multiply by 2^31 + 1 -- every step a bijection modulo 2^(2k)
__device__ __forceinline__ uint64_t mz_mix(uint64_t x, uint64_t m) {
    x = (~x + (x << 21)) & m; x ^= x >> 24;
    x = (x + (x << 3) + (x << 8)) & m; x ^= x >> 14;
    x = (x + (x << 2) + (x << 4)) & m; x ^= x >> 28;
    x = (x + (x << 31)) & m;
    return x;
}
// the steps undone last to first: the odd multipliers by their inverses modulo 2^64, y = x ^ (x >> s) by x = y ^ (y >> s) ^ (y >> 2s) ..
__device__ __forceinline__ uint64_t mz_unmix(uint64_t x, uint64_t m) {
    x = (x * 0x3FFFFFFF80000001ull) & m;
    x ^= (x >> 28) ^ (x >> 56);
    x = (x * 0xCF3CF3CF3CF3CF3Dull) & m;
    x ^= (x >> 14) ^ (x >> 28) ^ (x >> 42) ^ (x >> 56);
    x = (x * 0xD38FF08B1C03DD39ull) & m;
    x ^= (x >> 24) ^ (x >> 48);
    x = ((x + 1) * 0x7FFFFBFFFFDFFFFFull) & m;
    return x;
}

// Walk one run: raw bytes [lo, hi) of a record that begins at b, after the warm-up.  ring: this lane's column (slot s at
// ring[s * BLOCK]).  Every row owned by a kept byte whose local index (0 at lo) is below `limit` goes to
// on_row(kidx, age, minus, key): age positions back from the window's last one, minus = 1 for strand '-'.  -> kept bytes in [lo, hi).
template <bool CANON, bool LEX, class F>
__device__ __forceinline__ uint32_t mz_walk(const SearchPlan &P, int k, int w, uint64_t *ring, int64_t b, int64_t lo, int64_t hi, int64_t limit,
                                            F &&on_row) {
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    const int sh = 2 * (k - 1), need = w + k - 1;
    KmerRoll<uint64_t, CANON> st;
    uint64_t mn = MZ_NONE;
    uint32_t hist = 0;
    int age = 0, head = 0, fed = 0;
    auto step = [&](uint32_t c) -> bool {                    // -> the window that ends here is a row
        const bool p_has = fed >= need && mn != MZ_NONE;     // the window in front: has a selection, p_age back from its end
        const int p_age = age;
        st.step(kmer_code(c), k, mask, sh);
        const uint64_t code = st.value();
        const uint64_t key = st.v >= k ? (LEX ? code : mz_mix(code, mask)) : MZ_NONE;
        ring[head * BLOCK] = key;
        hist = (hist << 1) | (CANON && st.rc < st.fw ? 1u : 0u);
        if (key < mn || mn == MZ_NONE) { mn = key; age = 0; }
        else if (++age >= w) {                               // the holder has left: the last w keys again, oldest first
            mn = MZ_NONE;                                    // (one dependent read per slot; eight reads in flight at a time,
            int s = head;                                    // with the slots past w masked, measured 15 - 23 % slower)
            for (int a = w - 1; a >= 0; --a) {
                s = s + 1 == w ? 0 : s + 1;
                const uint64_t q = ring[s * BLOCK];
                if (q < mn) { mn = q; age = a; }
            }
        }
        head = head + 1 == w ? 0 : head + 1;
        fed = fed < need ? fed + 1 : need;
        return fed >= need && mn != MZ_NONE && !(p_has && age == p_age + 1);
    };
    run_warm(P, b, lo, need, [&](uint32_t c) { (void)step(c); });
    uint32_t kidx = 0;
    run_walk(P, lo, hi, [&](uint32_t c) {
        if (step(c) && (int64_t)kidx < limit) on_row(kidx, age, (hist >> age) & 1u, mn);
        ++kidx;
    });
    return kidx;
}

// per run: the packed word of fx_search.hpp (srch_pack): rows on '+', rows on '-', kept bytes (at most 256 rows in all)
template <bool CANON, bool LEX>
__global__ __launch_bounds__(BLOCK) void k_mz_count(SearchPlan P, int k, int w, uint32_t *__restrict__ packed) {
    extern __shared__ __align__(16) uint64_t mz_ring[];
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= P.n_runs) return;
    int64_t r, b, lo, hi;
    srch_run(P, g, srch_slot(P, g), r, b, lo, hi);
    uint32_t hp = 0, hm = 0;
    const uint32_t kept = mz_walk<CANON, LEX>(P, k, w, mz_ring + threadIdx.x, b, lo, hi, INT64_MAX,
                                              [&](uint32_t, int, uint32_t minus, uint64_t) { hp += 1u - minus; hm += minus; });
    packed[g] = srch_pack(hp, hm, kept);
}

// The cut at slen, as k_search_fix makes it: one lane per selected record; where the kept bytes run past slen, the run that
// crosses the cut is counted again with the cut and the runs behind it lose their rows.  A window that ends in front of the
// cut reads nothing behind it.
template <bool CANON, bool LEX>
__global__ __launch_bounds__(BLOCK) void k_mz_fix(SearchPlan P, int k, int w, const int64_t *__restrict__ K, uint32_t *__restrict__ packed) {
    extern __shared__ __align__(16) uint64_t mz_ring[];
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= P.n_sel) return;
    const int64_t g0 = P.run0[s], g1 = P.run0[s + 1];
    const int64_t slen = P.slen[srch_rec(P, s)];
    if (g0 == g1 || K[g1] - K[g0] <= slen) return;
    int64_t lo_g = g0, hi_g = g1 - 1;                        // first run whose kept bytes end past slen
    while (lo_g < hi_g) { const int64_t m = (lo_g + hi_g) >> 1; if (K[m + 1] - K[g0] > slen) hi_g = m; else lo_g = m + 1; }
    for (int64_t g = lo_g; g < g1; ++g) {
        const int64_t base = K[g] - K[g0];
        uint32_t hp = 0, hm = 0;
        const uint32_t kept = (packed[g] >> 18) & 511u;
        if (base < slen && (packed[g] & 0x3FFFFu)) {
            int64_t r, b, lo, hi;
            srch_run(P, g, s, r, b, lo, hi);
            mz_walk<CANON, LEX>(P, k, w, mz_ring + threadIdx.x, b, lo, hi, slen - base,
                                [&](uint32_t, int, uint32_t minus, uint64_t) { hp += 1u - minus; hm += minus; });
        }
        packed[g] = srch_pack(hp, hm, kept);
    }
}

// The runs of the list walk again and store their rows at Pp[g] + Pm[g], by start: record, start, strand and the code.
template <bool CANON, bool LEX>
__global__ __launch_bounds__(BLOCK) void k_mz_emit(SearchPlan P, int k, int w, const int64_t *__restrict__ list, int64_t n_list,
                                                   const int64_t *__restrict__ K, const int64_t *__restrict__ Pp,
                                                   const int64_t *__restrict__ Pm, int64_t *__restrict__ o_rec,
                                                   int64_t *__restrict__ o_start, uint8_t *__restrict__ o_strand,
                                                   uint64_t *__restrict__ o_code) {
    extern __shared__ __align__(16) uint64_t mz_ring[];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_list) return;
    const int64_t g = list[i], s = srch_slot(P, g);
    int64_t r, b, lo, hi;
    srch_run(P, g, s, r, b, lo, hi);
    const int64_t base = K[g] - K[P.run0[s]];
    const int64_t first = base - (k - 1);
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    int64_t o = Pp[g] + Pm[g];
    mz_walk<CANON, LEX>(P, k, w, mz_ring + threadIdx.x, b, lo, hi, P.slen[r] - base, [&](uint32_t kidx, int age, uint32_t minus, uint64_t key) {
        o_rec[o] = r;
        o_start[o] = first + kidx - age;
        o_strand[o] = minus ? '-' : '+';
        o_code[o] = LEX ? key : mz_unmix(key, mask);
        ++o;
    });
}

}  // namespace fx
