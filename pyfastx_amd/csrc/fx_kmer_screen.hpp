// fx_kmer_screen.hpp -- k-mer screening of the resident FASTA and FASTQ streams against a device k-mer set (1 <= k <= 31) for
// gfx950 (MI355X, wave64).  Extension: the definition -- alphabet, code of a window, canonical form, the windows of a selection --
// is the one of fx_kmer_table.hpp / include/fxgpu.h; where the table kernels sort the codes they meet, these look every one of
// them up in a set and count, per read or record, the valid windows and the hits.  DESIGN.md 4.7.
//
// The set.  An open-addressing hash set of 64-bit codes in device memory.  A code has 2k <= 62 bits, so ~0 marks an empty slot.
// slots = a power of two, at least 2n and at least KS_MIN_SLOTS: the load is at most 0.5 and a probe chain always ends at an
// empty slot.  The home slot of a code is the top log2(slots) bits of code * KS_MUL (an odd constant); chains are linear and
// wrap at the table's end.
//   k_ks_check    one lane per given code: inside [0, 4^k), canonical where the set is -- before anything is kept.
//   k_ks_insert   one lane per code: atomicCAS(slot, empty, code) along the chain; reading back the code itself means it is
//                 there already, so duplicates in the input are tolerated and membership does not depend on the order.
//   ks_probe      from the home slot on until the code (1) or an empty slot (0); all 64 bits are compared.
// Two forms of the probing kernels, chosen by the host from `slots`:
//   LDS = true    slots <= KS_LDS_SLOTS (an image of at most 64 KiB, at most KS_LDS_KEYS = 4096 codes: adapters, primers, PhiX
//                 at small k).  Every workgroup copies the image with coalesced 16-byte loads once (dynamic LDS of exactly the
//                 image's size, so two workgroups of the largest image fit the 160 KiB of a CU and more of a smaller one) and
//                 probes with 8-byte LDS reads.
//   LDS = false   8-byte loads from global memory.
//
// Walks.
//   k_ks_fastq    the lane groups of k_kt_fastq and the pieces of kmer_fq_pieces (fx_kmer.hpp), start / end intervals and reads
//                 longer than 16 * lpr included; a lane counts its valid windows and its hits, qc_group_reduce brings the lanes
//                 of a group together and its first lane stores n_windows[q], n_hits[q] (int32): no atomics, no cursor.
//   k_ks_fasta    one lane per run as k_kt_fasta, kmer_walk with limit = slen - kept bytes in front of the run (k_kt_kept and its
//                 scan come first), so nothing behind the cut at slen counts.  A lane adds its two sums to the int64 pair of its
//                 row -- the position of its record in the selection, so a record listed twice has two rows -- with one 64-bit
//                 atomicAdd each, left out when zero; the rows are zeroed first.
//   k_ks_pass     the screen's predicate per query from the two columns; the passing positions then come from the scan and
//                 k_fq_select_emit of fx_fastq_qc.hpp.
//   k_ks_contains one lane per queried code -> 0 or 1.
#pragma once
#include "fx_kmer_table.hpp"

namespace fx {

constexpr uint64_t KS_EMPTY = ~0ull;
constexpr uint64_t KS_MUL = 0x9E3779B97F4A7C15ull;           // odd: 2^64 / the golden ratio
constexpr int KS_MIN_LOG2 = 6;                               // at least 64 slots
constexpr int KS_LDS_LOG2 = 13;                              // the LDS form: at most 8192 slots = 64 KiB
constexpr int64_t KS_MIN_SLOTS = 1 << KS_MIN_LOG2, KS_LDS_SLOTS = 1 << KS_LDS_LOG2, KS_LDS_KEYS = KS_LDS_SLOTS / 2;
constexpr int64_t KS_MAX_KEYS = (int64_t)1 << 31;

struct KsView {                                              // the set as the kernels take it
    const uint64_t *slots;
    int log2;                                                // slots = 1 << log2, KS_MIN_LOG2 <= log2 <= 32
};

__device__ __forceinline__ uint32_t ks_home(uint64_t code, int log2) { return (uint32_t)((code * KS_MUL) >> (64 - log2)); }

// 1 when `code` (never KS_EMPTY) is in the table, which lies in LDS or in global memory
template <class T>
__device__ __forceinline__ uint32_t ks_probe(const T *__restrict__ tab, int log2, uint64_t code) {
    const uint32_t mask = (uint32_t)((1ull << log2) - 1ull);
    for (uint32_t i = ks_home(code, log2);; i = (i + 1u) & mask) {
        const uint64_t s = tab[i];
        if (s == code) return 1u;
        if (s == KS_EMPTY) return 0u;
    }
}

// the image of a table of at most KS_LDS_SLOTS slots -> LDS, 16 bytes per lane and step.  Followed by __syncthreads.
__device__ __forceinline__ void ks_lds_fill(const KsView &S, uint64_t *lds) {
    const int n2 = 1 << (S.log2 - 1);
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(S.slots);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(lds);
    for (int i = threadIdx.x; i < n2; i += blockDim.x) dst[i] = src[i];
}

// *bad = index of the first code outside [0, 4^k) or, in a canonical set, above its reverse complement's
__global__ __launch_bounds__(BLOCK) void k_ks_check(const int64_t *__restrict__ codes, int64_t n, int k, int canon, unsigned long long *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = (uint64_t)codes[i];
    bool ok = c < (1ull << (2 * k));
    if (ok && canon) {
        uint64_t rc = 0, f = c;
        for (int j = 0; j < k; ++j) { rc = (rc << 2) | (3ull - (f & 3ull)); f >>= 2; }
        ok = c <= rc;
    }
    if (!ok) atomicMin(bad, (unsigned long long)i);
}

__global__ __launch_bounds__(BLOCK) void k_ks_insert(const int64_t *__restrict__ codes, int64_t n, unsigned long long *__restrict__ slots, int log2) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long c = (unsigned long long)codes[i];
    const uint32_t mask = (uint32_t)((1ull << log2) - 1ull);
    for (uint32_t s = ks_home(c, log2);; s = (s + 1u) & mask) {
        const unsigned long long was = atomicCAS(slots + s, (unsigned long long)KS_EMPTY, c);
        if (was == KS_EMPTY || was == c) return;             // kept now, or there already
    }
}

// out[i] = 1 where codes[i] is in the set; a value outside [0, 4^k) is in no set
__global__ __launch_bounds__(BLOCK) void k_ks_contains(KsView S, int k, const int64_t *__restrict__ codes, int64_t n, uint8_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = (uint64_t)codes[i];
    out[i] = c < (1ull << (2 * k)) ? (uint8_t)ks_probe(S.slots, S.log2, c) : (uint8_t)0;
}

// Queries [0, nq); start / end null: whole reads.  The lanes and pieces of k_kt_fastq, the wave-uniform trip count of
// k_fq_read_stats (the lanes of a group meet in qc_group_reduce).
template <bool CANON, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_ks_fastq(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                   const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                   const int64_t *__restrict__ ids, int64_t nq, const int64_t *__restrict__ start,
                                                   const int64_t *__restrict__ end, int lpr, int k, KsView S,
                                                   int32_t *__restrict__ n_windows, int32_t *__restrict__ n_hits) {
    extern __shared__ __align__(16) uint64_t ks_lds[];
    if (LDS) { ks_lds_fill(S, ks_lds); __syncthreads(); }
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    for (int64_t q = wave * ngrp + grp; q - grp < nq; q += stride) {              // wave-uniform trip count
        uint32_t nw = 0, nh = 0;
        if (live && q < nq) {
            const int64_t id = ids ? ids[q] : q;
            const int64_t L = rlen[id] > 0 ? rlen[id] : 0, so = soff[id] - gbase;
            const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
            kmer_fq_pieces<uint64_t, CANON>(data, so, n_bytes, a, b, sub, lpr, k, [&](uint64_t code) {
                ++nw;
                nh += LDS ? ks_probe(ks_lds, S.log2, code) : ks_probe(S.slots, S.log2, code);
            });
        }
        nw = qc_group_reduce(nw, lane, sub, lpr, p2, [](uint32_t x, uint32_t y) { return x + y; });
        nh = qc_group_reduce(nh, lane, sub, lpr, p2, [](uint32_t x, uint32_t y) { return x + y; });
        if (live && sub == 0 && q < nq) { n_windows[q] = (int32_t)nw; n_hits[q] = (int32_t)nh; }
    }
}

// Runs [0, n_runs), grid-stride; K: exclusive prefix of the kept bytes of the runs (n_runs + 1); acc: n_sel rows of
// (windows, hits), zeroed.
template <bool CANON, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_ks_fasta(SearchPlan P, int k, const int64_t *__restrict__ K, KsView S, unsigned long long *__restrict__ acc) {
    extern __shared__ __align__(16) uint64_t ks_lds[];
    if (LDS) { ks_lds_fill(S, ks_lds); __syncthreads(); }
    for (int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x; g < P.n_runs; g += (int64_t)gridDim.x * BLOCK) {
        const int64_t slot = srch_slot(P, g);
        int64_t r, b, lo, hi;
        srch_run(P, g, slot, r, b, lo, hi);
        const int64_t limit = P.slen[r] - (K[g] - K[P.run0[slot]]);          // windows may end at the kept bytes of the run below it
        if (limit <= 0) continue;
        unsigned long long nw = 0, nh = 0;
        kmer_walk<uint64_t, CANON>(P, k, b, lo, hi, 0, limit, [&](uint64_t code) {
            ++nw;
            nh += LDS ? ks_probe(ks_lds, S.log2, code) : ks_probe(S.slots, S.log2, code);
        });
        if (nw) atomicAdd(acc + 2 * slot, nw);
        if (nh) atomicAdd(acc + 2 * slot + 1, nh);
    }
}

// acc rows -> the two int64 columns
__global__ __launch_bounds__(BLOCK) void k_ks_split(const unsigned long long *__restrict__ acc, int64_t n, int64_t *__restrict__ n_windows,
                                                   int64_t *__restrict__ n_hits) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    n_windows[i] = (int64_t)acc[2 * i];
    n_hits[i] = (int64_t)acc[2 * i + 1];
}

// pass[q] = (n_hits >= min_hits and n_hits * den >= num * n_windows) != invert; den = 0: the ratio is not asked.  int64: the
// columns are below 2^31, num and den at most 10^9.
__global__ __launch_bounds__(BLOCK) void k_ks_pass(const int32_t *__restrict__ n_windows, const int32_t *__restrict__ n_hits, int64_t n,
                                                  int64_t min_hits, int64_t num, int64_t den, int invert, uint8_t *__restrict__ pass) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const int64_t w = n_windows[q], h = n_hits[q];
    bool ok = h >= min_hits;
    if (den > 0) ok = ok && h * den >= num * w;
    pass[q] = (ok != (invert != 0)) ? 1 : 0;
}

}  // namespace fx
