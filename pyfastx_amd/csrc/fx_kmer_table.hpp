// fx_kmer_table.hpp -- sparse k-mer tables (1 <= k <= 31) of the resident FASTA and FASTQ streams for gfx950 (MI355X, wave64).
// Extension: the definition is the one of fx_kmer.hpp / include/fxgpu.h; where the dense form keeps 4^k counters, this one
// returns the codes that occur, ascending, each with its exact count.  DESIGN.md 4.6.
//
// Codes.  2k <= 62 bits: KmerRoll of fx_kmer.hpp with 64-bit words (forward code masked to 2k bits, the complement shifted in
// at bit 2(k - 1) <= 60).  The dense kernels keep their 32-bit registers.
//
// Walks.  The stream is walked once for a histogram and once per partition for the codes:
//   k_kt_kept   one lane per run: its kept bytes (the form SrchLdKept reads).  Their scan K gives every run the kept index
//               it starts at, so that no walk produces a window that ends at or behind slen -- a sorted list cannot take a
//               window off again with an add of -1 as k_kmer_fix does.
//   k_kt_fasta  one lane per run as k_kmer_fasta: kmer_walk of fx_kmer.hpp with 64-bit words and an upper bound on the kept
//               index.  The warm-up over the k - 1 <= 30 kept bytes in front of a run comes from one (k - 1 <= 12) or two
//               aligned 16-byte loads; where they hold fewer than k - 1 kept bytes or reach in front of the record the lane
//               goes back byte by byte.
//   k_kt_fastq  the lane groups of k_kmer_fastq and its pieces (kmer_fq_pieces); the warm-up reads the k - 1 bytes in front of a
//               piece from the one or two 16-byte pieces there.
//   EMIT = false: the top min(2k, 12) bits of every counted code go to a 16 KiB table of 32-bit counters in LDS (a lane adds a
//               bin when the next window falls into another one), the table to 4096 int64 bins when the workgroup is done.
//   EMIT = true:  codes in [lo, hi) are stored at a cursor in global memory: the lanes of a wave that have one ballot, the
//               first of them adds their number to the cursor, every one stores at its rank.  The order is lost; the sort
//               that follows does not need it.  The bins give the number of codes exactly, `cap` guards the buffer anyway.
//
// Reduction.  The sorted keys become (code, count) by head flags, a scan (k_sscan_sums / k_sscan_top of fx_search.hpp with the
// loaders below) and a compaction (k_kt_compact): the heads' positions first -- a run of equal keys may span any number of
// tiles, its length is the distance to the next head --, then the entries whose count reaches min_count.
// Fold (a bin above the capacity, taken in position sub-chunks): the running list and the sub-chunk's list are laid back to
// back (k_kt_concat), sorted by code with the row as value, and summed by code -- a code has at most one row in either list.
#pragma once
#include "fx_kmer.hpp"

namespace fx {

constexpr int KT_MAX_K = 31;
constexpr int KT_BIN_BITS = 12;                             // the partitions are ranges of the top min(2k, 12) bits of a code
constexpr int KT_BINS = 1 << KT_BIN_BITS;
static_assert(KT_BINS == KMER_LDS_WORDS, "the histogram uses the LDS table of the dense form");

// where the windows of a walk go
struct KtArgs {
    int shift;                                               // code >> shift = its bin
    unsigned long long *bins;                                // EMIT = false: KT_BINS counters
    uint64_t lo, hi;                                         // EMIT = true: codes in [lo, hi) ...
    uint64_t *out;                                           // ... are stored here, at most cap of them,
    unsigned long long *cursor;                              // ... at this cursor
    uint64_t cap;
};

struct KtHist {                                              // the last bin of a lane and how often it has met it
    uint32_t *lds;
    int shift;
    uint32_t bin = 0, n = 0;
    __device__ __forceinline__ void put(uint64_t code) {
        const uint32_t b = (uint32_t)(code >> shift);
        if (b == bin) { ++n; return; }
        if (n) atomicAdd(&lds[bin], n);
        bin = b; n = 1;
    }
    __device__ __forceinline__ void flush() { if (n) atomicAdd(&lds[bin], n); n = 0; }
};
struct KtEmit {
    KtArgs a;
    __device__ __forceinline__ void put(uint64_t code) {
        const bool in = code >= a.lo && code < a.hi;
        const uint64_t m = __ballot(in);                     // the lanes that walk a window in this step and have a code of the range
        if (!in) return;
        const int lane = lane_id();
        unsigned long long base = 0;
        if (lane == __ffsll((unsigned long long)m) - 1) base = atomicAdd(a.cursor, (unsigned long long)__popcll(m));
        const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);       // the first lane in here is the one that added
        const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        const uint64_t pos = (((uint64_t)bhi << 32) | blo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < a.cap) a.out[pos] = code;
    }
    __device__ __forceinline__ void flush() {}
};
template <bool EMIT> using KtSink = std::conditional_t<EMIT, KtEmit, KtHist>;

// the workgroup's table -> the bins, where not zero; the table is left cleared.  Between two __syncthreads.
__device__ __forceinline__ void kt_lds_flush(uint32_t *lds, unsigned long long *__restrict__ bins) {
    for (int e = threadIdx.x; e < KT_BINS; e += blockDim.x) {
        const uint32_t s = lds[e];
        lds[e] = 0;
        if (s) atomicAdd(bins + e, (unsigned long long)s);
    }
}

// packed[g] = the kept bytes of run g, as srch_pack lays them.  A loop of its own, not run_walk: a count does not depend on the
// order of the bytes, so every load of the run may be in flight at once (measured at half the time of the one-ahead walk).
__global__ __launch_bounds__(BLOCK) void k_kt_kept(SearchPlan P, uint32_t *__restrict__ packed) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= P.n_runs) return;
    int64_t r, b, lo, hi;
    srch_run(P, g, srch_slot(P, g), r, b, lo, hi);
    uint32_t kept = 0;
    for (int64_t c = lo & ~(int64_t)15; c < hi; c += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            kept += (c + i >= lo && c + i < hi && !srch_space((w[i >> 2] >> (8 * (i & 3))) & 0xFFu)) ? 1u : 0u;
    }
    packed[g] = srch_pack(0, 0, kept);
}

// Runs [g_begin, g_end), grid-stride; K: exclusive prefix of the kept bytes of the runs (n_runs + 1).
template <bool CANON, bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_kt_fasta(SearchPlan P, int k, int64_t g_begin, int64_t g_end, const int64_t *__restrict__ K, KtArgs A) {
    __shared__ uint32_t lds[EMIT ? 1 : KT_BINS];
    if (!EMIT) { kmer_lds_clear(lds); __syncthreads(); }
    for (int64_t g = g_begin + (int64_t)blockIdx.x * BLOCK + threadIdx.x; g < g_end; g += (int64_t)gridDim.x * BLOCK) {
        const int64_t slot = srch_slot(P, g);
        int64_t r, b, lo, hi;
        srch_run(P, g, slot, r, b, lo, hi);
        const int64_t limit = P.slen[r] - (K[g] - K[P.run0[slot]]);          // windows may end at the kept bytes of the run below it
        if (limit <= 0) continue;
        KtSink<EMIT> sink{};
        if constexpr (EMIT) sink.a = A; else { sink.lds = lds; sink.shift = A.shift; }
        kmer_walk<uint64_t, CANON>(P, k, b, lo, hi, 0, limit, [&](uint64_t code) { sink.put(code); });
        sink.flush();
    }
    if (!EMIT) { __syncthreads(); kt_lds_flush(lds, A.bins); }
}

// Queries [q_begin, q_end); start / end null: whole reads.  The lanes and pieces of k_kmer_fastq, 64-bit words.
template <bool CANON, bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_kt_fastq(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                   const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                   const int64_t *__restrict__ ids, int64_t q_begin, int64_t q_end,
                                                   const int64_t *__restrict__ start, const int64_t *__restrict__ end, int lpr, int k, KtArgs A) {
    __shared__ uint32_t lds[EMIT ? 1 : KT_BINS];
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    if (!EMIT) { kmer_lds_clear(lds); __syncthreads(); }
    KtSink<EMIT> sink{};
    if constexpr (EMIT) sink.a = A; else { sink.lds = lds; sink.shift = A.shift; }
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    for (int64_t q = q_begin + wave * ngrp + grp; grp < ngrp && q < q_end; q += stride) {
        const int64_t id = ids ? ids[q] : q;
        const int64_t L = rlen[id] > 0 ? rlen[id] : 0, so = soff[id] - gbase;
        const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
        kmer_fq_pieces<uint64_t, CANON>(data, so, n_bytes, a, b, sub, lpr, k, [&](uint64_t code) { sink.put(code); });
    }
    sink.flush();
    if (!EMIT) { __syncthreads(); kt_lds_flush(lds, A.bins); }
}

// ------------------------------------------------------------------ sorted keys -> (code, count)
// Loaders of the scans (one component): "a run of equal keys begins here", "the run behind head j has min_count keys",
// "row j of the folded list has min_count".
struct KtLdHead {
    const uint64_t *k;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0; }
};
__device__ __forceinline__ int64_t kt_run_len(const uint32_t *S, int64_t j, int64_t nd, int64_t n) { return (j + 1 < nd ? (int64_t)S[j + 1] : n) - (int64_t)S[j]; }
struct KtLdKeep {
    const uint32_t *S;
    int64_t nd, n, m;
    __device__ void operator()(int64_t j, int64_t *v) const { v[0] = kt_run_len(S, j, nd, n) >= m ? 1 : 0; }
};
struct KtLdGe {
    const int64_t *c;
    int64_t m;
    __device__ void operator()(int64_t j, int64_t *v) const { v[0] = c[j] >= m ? 1 : 0; }
};
// What the compaction does with element i whose flag is set and that is number j among them.
struct KtPutStart {                                          // head i of the sorted keys -> S[j]
    uint32_t *S;
    __device__ void operator()(int64_t i, int64_t j) const { S[j] = (uint32_t)i; }
};
struct KtPutEntry {                                          // kept head j -> entry jj of the table
    const uint64_t *keys;
    const uint32_t *S;
    int64_t nd, n;
    uint64_t *codes;
    int64_t *counts;
    __device__ void operator()(int64_t j, int64_t jj) const { codes[jj] = keys[S[j]]; counts[jj] = kt_run_len(S, j, nd, n); }
};
struct KtPutFold {                                           // head i of the sorted rows of two lists -> row j of the folded list
    const uint64_t *keys;
    const uint32_t *rows;
    const int64_t *W;
    int64_t n;
    uint64_t *codes;
    int64_t *counts;
    __device__ void operator()(int64_t i, int64_t j) const {
        int64_t c = W[rows[i]];
        if (i + 1 < n && keys[i + 1] == keys[i]) c += W[rows[i + 1]];       // a code has at most one row in either list
        codes[j] = keys[i];
        counts[j] = c;
    }
};
struct KtPutCopy {
    const uint64_t *k;
    const int64_t *c;
    uint64_t *codes;
    int64_t *counts;
    __device__ void operator()(int64_t j, int64_t jj) const { codes[jj] = k[j]; counts[jj] = c[j]; }
};

// The chunks of k_sscan_sums: sums[blk] = flagged elements in front of chunk blk (after k_sscan_top).
template <class Ld, class Put>
__global__ __launch_bounds__(BLOCK) void k_kt_compact(Ld ld, int64_t n, const int64_t *__restrict__ sums, Put put) {
    __shared__ int64_t lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * SRCH_CHUNK + (int64_t)threadIdx.x * SRCH_PER;
    uint32_t flags = 0;
    for (int i = 0; i < SRCH_PER; ++i)
        if (i0 + i < n) { int64_t v; ld(i0 + i, &v); flags |= v ? 1u << i : 0u; }
    const int64_t s = __popc(flags);
    int64_t tot;
    int64_t j = block_incl_scan64(s, lds, &tot) - s + sums[blockIdx.x];
    for (int i = 0; i < SRCH_PER; ++i)
        if ((flags >> i) & 1u) put(i0 + i, j++);
}

// keys / W / rows [0, nr + ns) = the running list then the sub-chunk's list, rows = 0, 1, 2, ...
__global__ __launch_bounds__(BLOCK) void k_kt_concat(const uint64_t *__restrict__ rk, const int64_t *__restrict__ rc, int64_t nr,
                                                    const uint64_t *__restrict__ sk, const int64_t *__restrict__ sc, int64_t ns,
                                                    uint64_t *__restrict__ keys, int64_t *__restrict__ W, uint32_t *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nr + ns) return;
    keys[i] = i < nr ? rk[i] : sk[i - nr];
    W[i] = i < nr ? rc[i] : sc[i - nr];
    rows[i] = (uint32_t)i;
}

}  // namespace fx
