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

// The form of the three passes (k_hits_count / _fix / _emit of fx_search.hpp): no table, the lanes' rings in dynamic LDS; a
// window is a row on one strand, its position lies `age` in front of the window's last k-mer, its column is the code.  A
// window that ends in front of the cut reads nothing behind it.
template <bool CANON, bool LEX>
struct MzForm {
    struct Win { int age; uint32_t minus; uint64_t key; };
    using Col = uint64_t;
    static constexpr bool COL = true, AT = false, ONE = true;
    int k, w;
    __device__ __forceinline__ uint64_t *table(const SearchPlan &) const {
        extern __shared__ __align__(16) uint64_t mz_ring[];
        return mz_ring + threadIdx.x;
    }
    template <bool ROWS, class F>
    __device__ __forceinline__ uint32_t walk(const SearchPlan &P, uint64_t *ring, int64_t b, int64_t lo, int64_t hi, int64_t limit, F &&on) const {
        return mz_walk<CANON, LEX>(P, k, w, ring, b, lo, hi, limit,
                                   [&](uint32_t kidx, int age, uint32_t minus, uint64_t key) { on(kidx, Win{age, minus, key}); });
    }
    __device__ __forceinline__ uint32_t plus(const Win &x) const { return 1u - x.minus; }
    __device__ __forceinline__ uint32_t minus(const Win &x) const { return x.minus; }
    __device__ __forceinline__ int64_t first(const SearchPlan &, int64_t base) const { return base - (k - 1); }
    __device__ __forceinline__ int64_t pos(int64_t first, int64_t kidx, const Win &x) const { return first + kidx - x.age; }
    __device__ __forceinline__ Col col(const Win &x, bool) const { return LEX ? x.key : mz_unmix(x.key, ((uint64_t)1 << (2 * k)) - 1); }
};

}  // namespace fx
