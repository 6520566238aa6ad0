// fx_kmer.hpp -- dense k-mer spectra (1 <= k <= 13) of the resident FASTA and FASTQ streams for gfx950 (MI355X, wave64).
// Extension: the reference counts single letters only (composition); the definition is the one of include/fxgpu.h.
//
// Codes.  A / a 0, C / c 1, G / g 2, T / t 3, the first base of a window the most significant digit; every other byte is
// invalid and a window that holds one is not counted.  A lane keeps a rolling state over the kept bytes it walks: the
// forward code (shift in two bits, mask to 2k), the code of the reverse complement (shift out two bits, the complement in
// at the top) and the number of valid bases in a row, capped at k -- a window counts when that number is k.  Canonical
// counting takes the smaller of the two codes, so a window that is its own reverse complement counts once.
//
// FASTA (k_kmer_fasta): the run layout of fx_search.hpp as it is -- one lane per run (the part of one record inside one
//   256-byte block), the record found by a binary search over run0.  The warm-up over the k - 1 kept bytes in front of
//   the run comes from ONE 16-byte load of the bytes in front of it (a run that does not begin its record begins at a
//   block boundary, so the load is aligned and lies inside the record when the record began 16 bytes earlier); only when
//   those 16 bytes hold fewer than k - 1 kept ones (blank lines, a short line) or reach in front of the record does the
//   lane go back byte by byte as srch_walk does.  The pass ignores the cut at slen and stores the kept bytes of every run;
//   after the scan of the kept counts k_kmer_fix -- one lane per selected record, idle unless the record's kept bytes
//   outnumber slen -- takes the windows that end past the cut off again (an add of -1).
// FASTQ (k_kmer_fastq): the lane groups of k_fq_read_stats -- lpr lanes per read, one 16-byte piece per lane and step; a lane
//   counts the windows that END in its piece and warms up on the last k - 1 <= 12 bytes of the piece in front (one more
//   16-byte load; it hits the cache, the neighbour lane loads the same bytes).  A read longer than 16 * lpr is covered by
//   further steps of the same lanes.  Bytes in front of `start` are skipped, so no window begins before it.
// Both walks (kmer_walk, kmer_fq_pieces) and the rolling state are templates on the code word: the sparse table and the screen
//   (fx_kmer_table.hpp, fx_kmer_screen.hpp, k <= 31) run the same code with 64-bit words and a warm-up of up to 32 bytes.
//
// Counters.  Every lane first aggregates: it remembers the last two distinct codes and how often it has met each, and
// only a third code makes it add the older pair.  A single-letter run (one code) and a dinucleotide run (two codes that
// alternate) therefore cost no counter update at all while they last; a repeat of period 3 or more alternates more codes
// than the lane remembers and adds for every window.  Random bases pay a compare and a select per window.
//   k <= KMER_LDS_K  a 16 KiB table of 32-bit counters per workgroup in LDS (ds_add_u32), 4096 >> 2k copies of it (at most
//        64), the copy chosen by the lane: at k = 1..3 every lane of a wave has a copy of its own.  A workgroup adds the
//        non-zero sums of its copies to the int64 table when it is done.  No counter wraps: the host launches at most
//        2^31 windows' worth of runs (2^23 runs of 256 bytes) or reads (queries x longest read) per kernel.
//        Per-record rows (kmer_profile): a workgroup whose 256 runs lie in one record counts in LDS and adds to that row
//        after the step; one that spans records adds to the rows in global memory directly.
//   k >  KMER_LDS_K  one no-return 64-bit atomic add per aggregated code on the int64 table in global memory.
#pragma once
#include "fx_search.hpp"
#include "fx_fastq_qc.hpp"

namespace fx {

constexpr int KMER_MAX_K = 13;
constexpr int KMER_LDS_K = 6;                               // largest k whose table lives in LDS (and of the per-record rows)
constexpr int KMER_LDS_WORDS = 1 << (2 * KMER_LDS_K);       // 4096 counters, 16 KiB
constexpr int64_t KMER_MAX_WINDOWS = (int64_t)1 << 31;      // per kernel launch: what keeps a 32-bit counter from wrapping
constexpr uint32_t KMER_INVALID = 4u;

// A / a 0, C / c 1, G / g 2, T / t 3, anything else KMER_INVALID
__device__ __forceinline__ uint32_t kmer_code(uint32_t c) {
    const uint32_t u = c & 0xDFu, x = (u >> 1) & 3u;         // x: A 0, C 1, T 2, G 3 (QC_EX_LO holds the letters in this order)
    return u == ((QC_EX_LO >> (8 * x)) & 0xFFu) ? x ^ (x >> 1) : KMER_INVALID;
}

// Word: uint32_t holds the codes of the dense form (k <= 13), uint64_t those of the table and the screen (k <= 31)
template <class Word, bool CANON>
struct KmerRoll {
    Word fw = 0, rc = 0;
    int v = 0;                                               // valid bases in a row, capped at k
    __device__ __forceinline__ void step(uint32_t code, int k, Word mask, int sh) {
        if (code > 3u) { v = 0; return; }
        fw = ((fw << 2) | code) & mask;
        if (CANON) rc = (rc >> 2) | ((Word)(3u - code) << sh);
        v = v < k ? v + 1 : k;
    }
    __device__ __forceinline__ Word value() const { return CANON ? (fw < rc ? fw : rc) : fw; }
};

// the last two distinct codes of a lane and their counts; add(code, n) is called when a third one pushes the older out
struct KmerAgg {
    uint32_t c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu, n0 = 0, n1 = 0;
    template <class Add> __device__ __forceinline__ void put(uint32_t code, Add &&add) {
        if (code == c0) ++n0;
        else if (code == c1) ++n1;
        else {
            if (n1) add(c1, n1);
            c1 = c0; n1 = n0; c0 = code; n0 = 1;
        }
    }
    template <class Add> __device__ __forceinline__ void flush(Add &&add) {
        if (n0) add(c0, n0);
        if (n1) add(c1, n1);
        n0 = n1 = 0; c0 = c1 = 0xFFFFFFFFu;
    }
};

// Walk one run: raw bytes [lo, hi) of the address space of a record that begins at b.  Every valid window that ends at a
// kept byte whose local index (0 at lo) lies in [from, limit) goes to on_win(code).  -> kept bytes in [lo, hi).
template <class Word, bool CANON, class F>
__device__ __forceinline__ uint32_t kmer_walk(const SearchPlan &P, int k, int64_t b, int64_t lo, int64_t hi, int64_t from, int64_t limit,
                                              F &&on_win) {
    const Word mask = ((Word)1 << (2 * k)) - 1;
    const int sh = 2 * (k - 1);
    KmerRoll<Word, CANON> st;
    auto step = [&](uint32_t c) { st.step(kmer_code(c), k, mask, sh); };
    if (k > 1 && lo > b) {                                   // warm-up on the k - 1 kept bytes in front of the run
        int kept = 0;
        const int64_t reach = (sizeof(Word) == 4 || k - 1 <= 12) ? 16 : 32;    // one aligned load, or two (a 32-bit code has k <= 13)
        if ((lo & 15) == 0 && lo - reach >= b) {
            for (int64_t q = lo - reach; q < lo; q += 16) {
                const uint4 pv = *reinterpret_cast<const uint4 *>(P.base + q);
                const uint32_t w[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                    if (!srch_space(c)) { step(c); ++kept; }
                }
            }
        }
        if (kept < k - 1) {                                  // white space hides them, or the record begins inside the reach
            st = KmerRoll<Word, CANON>();
            run_warm(P, b, lo, k - 1, step);
        }
    }
    uint32_t kidx = 0;                                       // 32 bits: a bound the caller passes as a constant costs no compare
    run_walk(P, lo, hi, [&](uint32_t c) {
        step(c);
        if (st.v >= k && (int64_t)kidx >= from && (int64_t)kidx < limit) on_win(st.value());
        ++kidx;
    });
    return kidx;
}

// The pieces of one lane of a FASTQ query: lane `sub` of the lpr lanes of a read whose bytes begin at data[so] takes the bytes
// [p, p + 16) of the read, p = 16 sub, 16 (sub + lpr), ...  Every valid window of [a, b) that ENDS in such a piece -- at a byte of
// [a + k - 1, b) -- goes to on_win(code); the state is warmed up on the k - 1 bytes in front of the piece, from `a` on: they lie
// in the piece in front (k - 1 <= 16) or in the two in front.
template <class Word, bool CANON, class F>
__device__ __forceinline__ void kmer_fq_pieces(const uint8_t *__restrict__ data, int64_t so, int64_t n_bytes, int64_t a, int64_t b, int sub,
                                               int lpr, int k, F &&on_win) {
    constexpr bool DENSE = sizeof(Word) == 4;                // k - 1 <= 12: one piece in front, its first 4 bytes never
    const Word mask = ((Word)1 << (2 * k)) - 1;
    const int sh = 2 * (k - 1);
    for (int64_t p = (int64_t)sub * 16; p < b; p += (int64_t)lpr * 16) {
        if (p + 16 <= a + k - 1) continue;
        KmerRoll<Word, CANON> st;
        if (k > 1 && p > a) {
            const int64_t ws = max(a, p - (k - 1));
            for (int64_t f = (DENSE || k - 1 <= 16) ? p - 16 : p - 32; f < p; f += 16) {
                if (f + 16 <= ws) continue;
                const uint4 pv = qc_load16(data, so + f, n_bytes);
                const uint32_t w[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int i = DENSE ? 4 : 0; i < 16; ++i)
                    if (f + i >= ws) st.step(kmer_code((w[i >> 2] >> (8 * (i & 3))) & 0xFFu), k, mask, sh);
            }
        }
        const uint4 cv = qc_load16(data, so + p, n_bytes);
        const uint32_t w[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (p + i < a || p + i >= b) continue;
            st.step(kmer_code((w[i >> 2] >> (8 * (i & 3))) & 0xFFu), k, mask, sh);
            if (st.v >= k) on_win(st.value());
        }
    }
}

// ------------------------------------------------------------------ the LDS table of a workgroup
__device__ __forceinline__ void kmer_lds_clear(uint32_t *lds) {
    for (int i = threadIdx.x; i < KMER_LDS_WORDS; i += blockDim.x) lds[i] = 0;
}
__device__ __forceinline__ int kmer_lds_copies(int k) { const int c = KMER_LDS_WORDS >> (2 * k); return c < 64 ? c : 64; }
// the sums of the copies, where not zero, added to dst[0 .. 4^k); the table is left cleared.  Between two __syncthreads.
__device__ __forceinline__ void kmer_lds_flush(uint32_t *lds, int k, unsigned long long *__restrict__ dst) {
    const int n = 1 << (2 * k), copies = kmer_lds_copies(k);
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        unsigned long long s = 0;
        for (int c = 0; c < copies; ++c) { s += lds[(c << (2 * k)) + e]; lds[(c << (2 * k)) + e] = 0; }
        if (s) atomicAdd(dst + e, s);
    }
}

// MODE 0: one spectrum, table in LDS (k <= KMER_LDS_K).  1: one spectrum, table in global memory.  2: one row per selected
// record (k <= KMER_LDS_K).  Runs [g_begin, g_end), at most KMER_MAX_WINDOWS / 256 of them; packed[g] = the run's kept bytes
// in the form SrchLdKept reads.
template <bool CANON, int MODE>
__global__ __launch_bounds__(BLOCK) void k_kmer_fasta(SearchPlan P, int k, int64_t g_begin, int64_t g_end,
                                                     unsigned long long *__restrict__ table, uint32_t *__restrict__ packed) {
    __shared__ uint32_t lds[MODE == 1 ? 1 : KMER_LDS_WORDS];
    const int kb = 2 * k;
    const uint32_t mine = MODE == 1 ? 0u : (uint32_t)(lane_id() & (kmer_lds_copies(k) - 1)) << kb;
    if (MODE != 1) { kmer_lds_clear(lds); __syncthreads(); }
    for (int64_t g = g_begin + (int64_t)blockIdx.x * BLOCK + threadIdx.x; g - threadIdx.x < g_end; g += (int64_t)gridDim.x * BLOCK) {
        bool one = MODE == 0;                                // the workgroup's runs of this step lie in one record
        int64_t slot = -1;
        if (MODE == 2) {
            const int64_t g_first = g - threadIdx.x, g_last = min(g_first + BLOCK, g_end) - 1;
            const int64_t k_first = srch_slot(P, g_first), k_last = srch_slot(P, g_last);
            one = k_first == k_last;
            slot = k_first;
        }
        if (g < g_end) {
            if (MODE != 2 || !one) slot = srch_slot(P, g);
            int64_t r, b, lo, hi;
            srch_run(P, g, slot, r, b, lo, hi);
            unsigned long long *row = MODE == 2 ? table + (slot << kb) : table;
            auto add = [&](uint32_t code, uint32_t n) {
                if (MODE == 1 || !one) atomicAdd(row + code, (unsigned long long)n);
                else atomicAdd(&lds[mine + code], n);
            };
            KmerAgg agg;
            const uint32_t kept = kmer_walk<uint32_t, CANON>(P, k, b, lo, hi, 0, INT64_MAX, [&](uint32_t code) { agg.put(code, add); });
            agg.flush(add);
            packed[g] = srch_pack(0, 0, kept);
        }
        if (MODE == 2) {                                     // block-uniform: every lane computed the same `one`
            __syncthreads();
            if (one) kmer_lds_flush(lds, k, table + (slot << kb));
            __syncthreads();
        }
    }
    if (MODE == 0) { __syncthreads(); kmer_lds_flush(lds, k, table); }
}

// One lane per selected record: where the kept bytes run past slen, the windows that end at or behind the cut are taken
// off again.  K: exclusive prefix of the kept counts (n_runs + 1).  row_stride: 4^k for per-record rows, else 0.
template <bool CANON>
__global__ __launch_bounds__(BLOCK) void k_kmer_fix(SearchPlan P, int k, const int64_t *__restrict__ K, int64_t row_stride,
                                                   unsigned long long *__restrict__ table) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= P.n_sel) return;
    unsigned long long *row = table + s * row_stride;
    srch_cut(P, K, s, [&](int64_t g, int64_t base, int64_t slen) {
        int64_t r, b, lo, hi;
        srch_run(P, g, s, r, b, lo, hi);
        kmer_walk<uint32_t, CANON>(P, k, b, lo, hi, max(slen - base, (int64_t)0), INT64_MAX, [&](uint32_t code) { atomicAdd(row + code, ~0ull); });
    });
}

// ------------------------------------------------------------------ FASTQ
// first query whose interval lies outside 0 <= start <= end <= rlen -> *bad (atomicMin)
__global__ __launch_bounds__(BLOCK) void k_kmer_fq_check(const int64_t *__restrict__ rlen, const int64_t *__restrict__ ids, int64_t nq,
                                                        const int64_t *__restrict__ start, const int64_t *__restrict__ end,
                                                        unsigned long long *__restrict__ bad) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq) return;
    const int64_t id = ids ? ids[q] : q, L = rlen[id] > 0 ? rlen[id] : 0;
    if (start[q] < 0 || start[q] > end[q] || end[q] > L) atomicMin(bad, (unsigned long long)q);
}

// Queries [q_begin, q_end); start / end null: whole reads.  LDS: the table of the workgroup in LDS (k <= KMER_LDS_K).
template <bool CANON, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_kmer_fastq(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                     const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                     const int64_t *__restrict__ ids, int64_t q_begin, int64_t q_end,
                                                     const int64_t *__restrict__ start, const int64_t *__restrict__ end, int lpr, int k,
                                                     unsigned long long *__restrict__ table) {
    __shared__ uint32_t lds[LDS ? KMER_LDS_WORDS : 1];
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const int kb = 2 * k;
    const uint32_t mine = LDS ? (uint32_t)(lane & (kmer_lds_copies(k) - 1)) << kb : 0u;
    if (LDS) { kmer_lds_clear(lds); __syncthreads(); }
    auto add = [&](uint32_t code, uint32_t n) {
        if (LDS) atomicAdd(&lds[mine + code], n);
        else atomicAdd(table + code, (unsigned long long)n);
    };
    KmerAgg agg;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    for (int64_t q = q_begin + wave * ngrp + grp; grp < ngrp && q < q_end; q += stride) {
        const int64_t id = ids ? ids[q] : q;
        const int64_t L = rlen[id] > 0 ? rlen[id] : 0, so = soff[id] - gbase;
        const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
        kmer_fq_pieces<uint32_t, CANON>(data, so, n_bytes, a, b, sub, lpr, k, [&](uint32_t code) { agg.put(code, add); });
    }
    agg.flush(add);
    if (LDS) { __syncthreads(); kmer_lds_flush(lds, k, table); }
}

}  // namespace fx
