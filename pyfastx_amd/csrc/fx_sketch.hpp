// fx_sketch.hpp -- MinHash and FracMinHash sketches of the records of the resident FASTA table and of the reads of the resident
// FASTQ table (fx_fasta_sketch, fx_fastq_sketch), and the all-pairs comparison of two sketches (fx_sketch_compare).
// Extension: the reference has no k-mer of any kind.  DESIGN.md 4.17.
//
// Definition (include/fxgpu.h has it in full).  The windows are those of the k-mer tables: valid letters ACGTacgt, across line
// ends, never across records, never past slen; FASTQ: the windows of s[start:end].  key = mz_mix(code) with code = min(fw, rc)
// (canonical) or fw: a bijection of the 2k-bit words, so a threshold on the key is a uniform sample of the distinct k-mers.  A set
// keeps the distinct keys below max_key, and with size > 0 the `size` smallest of them, ascending.
//
// Filter pass (FASTA).  The run layout of fx_search.hpp: one lane per run and the walk of the k-mer tables (kmer_walk: the warm-up
// on k - 1 letters from one or two aligned loads, run_warm where they do not reach, then run_walk), one KmerRoll<uint64_t, CANON>.
// A lane owns the k-mers that END at a kept byte of its run and keeps those whose key lies below T[slot], the threshold of the
// run's set (slot: the selected record, or 0 when pooled), read once per run.  No ring, no LDS.
//   k_sk_count  rows per run (at most 256: bits 0..8 of the packed word of srch_pack) and its kept bytes
//   k_sk_fix    the cut at slen once the kept-byte scan is there, as k_hits_fix makes it
//   k_sk_emit   (slot, key) rows at the run's offset of the row scan; they never leave the device
// A set that is not `active` (final in an earlier round) is not walked: its lanes leave after the binary search over run0.
// Filter pass (FASTQ).  The lane groups and pieces of k_kt_fastq with one pooled slot: a count of the keys below T[0], then the
// keys at a cursor (a ballot per step, one atomic per wave), in no order -- the sort does not need one.
//
// Rounds.  size > 0 with a large max_key must not emit every window.  Round 0 gives a set the threshold
// 4^k * oversample * size / windows (at most max_key); a set is final when it holds `size` distinct keys below its threshold or
// when the threshold is max_key; the others get theirs times 8, saturating, and are walked again alone.  The keys below a
// threshold are the same whatever the round, so no result depends on oversample.
//
// Sort and reduce.  Rows by the low bits(max_key - 1) key bits with the slot as the 32-bit value (radix_sort_rows), then a stable
// pass over (rank << 32) | slot by the slot bits (radix_sort_keys) and a gather: rows by (slot, key).  Heads (a row that differs
// from the one in front) are compacted, a binary search per set over the heads' slots gives the sets' bounds, and the sets that
// are final move their first `size` keys to the result.
//
// Comparison.  k_sk_compare: one wave per pair of sets.  Lanes take 64 consecutive keys of A, each lane finds the lower bound of
// its key in B (from the lower bound of the chunk in front on), a ballot gives the shared flags and their prefix, the union rank
// of A[p] is p + lower_bound - shared_below, and the loop stops once a rank reaches the limit.
#pragma once
#include "fx_kmer.hpp"
#include "fx_minimizer.hpp"

namespace fx {

constexpr int SK_MAX_K = 31;
constexpr int SK_MAX_OVERSAMPLE = 64;
constexpr int64_t SK_MAX_ROWS = ((int64_t)1 << 31) - 1;      // the sort's limit

__device__ __forceinline__ int64_t sk_set_of(const SearchPlan &P, int pooled, int64_t slot) { return pooled ? 0 : slot; }

// Walk one run (kmer_walk): raw bytes [lo, hi) of a record that begins at b, after the warm-up on k - 1 letters.  Every valid k-mer that
// ends at a kept byte whose local index (0 at lo) is below `limit` and whose key is below T goes to on_key(key).
// -> kept bytes in [lo, hi).
template <bool CANON, class F>
__device__ __forceinline__ uint32_t sk_walk(const SearchPlan &P, int k, uint64_t T, int64_t b, int64_t lo, int64_t hi, int64_t limit, F &&on_key) {
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1;
    return kmer_walk<uint64_t, CANON>(P, k, b, lo, hi, 0, limit, [&](uint64_t code) {
        const uint64_t key = mz_mix(code, mask);
        if (key < T) on_key(key);
    });
}

// per run: rows (bits 0..8), kept bytes (18..26).  Every set is active in round 0, so the kept bytes of every run are stored
// there; a later round only clears the rows of a run whose set is final.
template <bool CANON>
__global__ __launch_bounds__(BLOCK) void k_sk_count(SearchPlan P, int k, int pooled, const uint64_t *__restrict__ T, const uint8_t *__restrict__ active,
                                                    uint32_t *__restrict__ packed) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= P.n_runs) return;
    const int64_t slot = srch_slot(P, g), set = sk_set_of(P, pooled, slot);
    if (!active[set]) { packed[g] &= ~0x3FFFFu; return; }
    int64_t r, b, lo, hi;
    srch_run(P, g, slot, r, b, lo, hi);
    uint32_t rows = 0;
    const uint32_t kept = sk_walk<CANON>(P, k, T[set], b, lo, hi, INT64_MAX, [&](uint64_t) { ++rows; });
    packed[g] = srch_pack(rows, 0, kept);
}

// The cut at slen, as k_hits_fix makes it: one lane per selected record.
template <bool CANON>
__global__ __launch_bounds__(BLOCK) void k_sk_fix(SearchPlan P, int k, int pooled, const uint64_t *__restrict__ T, const int64_t *__restrict__ K,
                                                  uint32_t *__restrict__ packed) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= P.n_sel) return;
    srch_cut(P, K, s, [&](int64_t g, int64_t base, int64_t slen) {
        uint32_t rows = 0;
        const uint32_t kept = (packed[g] >> 18) & 511u;
        if (base < slen && (packed[g] & 0x3FFFFu)) {
            int64_t r, b, lo, hi;
            srch_run(P, g, s, r, b, lo, hi);
            sk_walk<CANON>(P, k, T[sk_set_of(P, pooled, s)], b, lo, hi, slen - base, [&](uint64_t) { ++rows; });
        }
        packed[g] = srch_pack(rows, 0, kept);
    });
}

struct SkLdRows {                                            // rows of run g
    const uint32_t *p;
    __device__ void operator()(int64_t g, int64_t *v) const { v[0] = p[g] & 511u; }
};

// The runs that have rows walk again and store them at R[g] (exclusive prefix of the rows): n_rows rows in all.
template <bool CANON>
__global__ __launch_bounds__(BLOCK) void k_sk_emit(SearchPlan P, int k, int pooled, const uint64_t *__restrict__ T, const uint32_t *__restrict__ packed,
                                                   const int64_t *__restrict__ K, const int64_t *__restrict__ R, int64_t n_rows,
                                                   uint64_t *__restrict__ o_key, uint32_t *__restrict__ o_set) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= P.n_runs || !(packed[g] & 511u)) return;
    const int64_t slot = srch_slot(P, g), set = sk_set_of(P, pooled, slot);
    int64_t r, b, lo, hi;
    srch_run(P, g, slot, r, b, lo, hi);
    const int64_t base = K[g] - K[P.run0[slot]];
    int64_t o = R[g];
    const int64_t end = min(R[g + 1], n_rows);               // (a row more than the count saw would land in the next run's: never stored)
    sk_walk<CANON>(P, k, T[set], b, lo, hi, P.slen[r] - base, [&](uint64_t key) {
        if (o < end) { o_key[o] = key; if (o_set) o_set[o] = (uint32_t)set; }
        ++o;
    });
}

// ------------------------------------------------------------------ windows of the sets, thresholds, rounds
// W[set] += the letters of the selected records (an upper bound of their windows; what the first threshold is sized by)
__global__ __launch_bounds__(BLOCK) void k_sk_letters_fa(SearchPlan P, int pooled, unsigned long long *__restrict__ W) {
    __shared__ int64_t lds[4];
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t n = s < P.n_sel ? max(P.slen[srch_rec(P, s)], (int64_t)0) : 0;
    if (!pooled) { if (s < P.n_sel) W[s] = (unsigned long long)n; return; }
    int64_t tot;
    (void)block_incl_scan64(n, lds, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(W, (unsigned long long)tot);
}
__global__ __launch_bounds__(BLOCK) void k_sk_letters_fq(const int64_t *__restrict__ rlen, const int64_t *__restrict__ ids, int64_t nq,
                                                         const int64_t *__restrict__ start, const int64_t *__restrict__ end,
                                                         unsigned long long *__restrict__ W) {
    __shared__ int64_t lds[4];
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    int64_t n = 0;
    if (q < nq) {
        const int64_t id = ids ? ids[q] : q;
        n = start ? end[q] - start[q] : max(rlen[id], (int64_t)0);
    }
    int64_t tot;
    (void)block_incl_scan64(n, lds, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(W, (unsigned long long)tot);
}

// round 0: T[set] = max_key without a size, else about 4^k * oversample * size / windows, at least 1 and at most max_key
__global__ __launch_bounds__(BLOCK) void k_sk_thresh(const unsigned long long *__restrict__ W, int64_t n_sets, int k, uint64_t max_key, int64_t size,
                                                     int oversample, uint64_t *__restrict__ T, uint8_t *__restrict__ active,
                                                     int64_t *__restrict__ cnt) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_sets) return;
    uint64_t t = max_key;
    if (size > 0) {
        const double want = ldexp((double)oversample * (double)size, 2 * k) / (double)max(W[s], 1ull);
        if (want < (double)max_key) t = (uint64_t)want + 1;
        if (t > max_key) t = max_key;
    }
    T[s] = t;
    active[s] = 1;
    cnt[s] = 0;
}

// rows by key, slots beside them -> (rank << 32) | slot; and back: the keys and slots by (slot, key)
__global__ __launch_bounds__(BLOCK) void k_sk_pack(const uint32_t *__restrict__ set, int64_t n, uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = ((uint64_t)i << 32) | set[i];
}
__global__ __launch_bounds__(BLOCK) void k_sk_gather(const uint64_t *__restrict__ ranked, const uint64_t *__restrict__ key, int64_t n,
                                                     uint64_t *__restrict__ o_key, uint32_t *__restrict__ o_set) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t w = ranked[i];
    o_key[i] = key[w >> 32];
    o_set[i] = (uint32_t)w;
}

// "row i differs from the row in front" (set: null with one set), and what the compaction does with head i, number j
struct SkLdHead {
    const uint64_t *key;
    const uint32_t *set;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = (i == 0 || key[i] != key[i - 1] || (set && set[i] != set[i - 1])) ? 1 : 0; }
};
struct SkPutHead {
    const uint64_t *key;
    const uint32_t *set;
    uint64_t *o_key;
    uint32_t *o_set;
    __device__ void operator()(int64_t i, int64_t j) const { o_key[j] = key[i]; if (set) o_set[j] = set[i]; }
};

// seg[s] = first of the nd distinct rows (by set) whose set is >= s, s = 0 .. n_sets
__global__ __launch_bounds__(BLOCK) void k_sk_bounds(const uint32_t *__restrict__ set, int64_t nd, int64_t n_sets, int64_t *__restrict__ seg) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s > n_sets) return;
    if (!set) { seg[s] = s == 0 ? 0 : nd; return; }
    int64_t lo = 0, hi = nd;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if ((int64_t)set[m] < s) lo = m + 1; else hi = m; }
    seg[s] = lo;
}

// A set of this round is final with `size` distinct keys, or at the largest threshold; another one gets its threshold times 8
// and adds itself to *left.  now[s] = 1 for the sets that became final here, cnt[s] = the keys they keep.
__global__ __launch_bounds__(BLOCK) void k_sk_decide(const int64_t *__restrict__ seg, int64_t n_sets, uint64_t max_key, int64_t size,
                                                     uint64_t *__restrict__ T, uint8_t *__restrict__ active, uint8_t *__restrict__ now,
                                                     int64_t *__restrict__ cnt, unsigned long long *__restrict__ left) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_sets) return;
    now[s] = 0;
    if (!active[s]) return;
    const int64_t c = seg[s + 1] - seg[s];
    if (size == 0 || c >= size || T[s] >= max_key) {
        cnt[s] = size > 0 && c > size ? size : c;
        active[s] = 0;
        now[s] = 1;
    } else {
        T[s] = T[s] > (max_key >> 3) ? max_key : min(T[s] << 3, max_key);
        atomicAdd(left, 1ull);
    }
}

// "distinct row j goes to the result": its set became final in this round and it is among the set's first `size`
struct SkLdTake {
    const uint32_t *set;
    const int64_t *seg;
    const uint8_t *now;
    int64_t size;
    __device__ void operator()(int64_t j, int64_t *v) const {
        const int64_t s = set ? set[j] : 0;
        v[0] = (now[s] && (size == 0 || j - seg[s] < size)) ? 1 : 0;
    }
};
struct SkLdCnt {
    const int64_t *c;
    __device__ void operator()(int64_t s, int64_t *v) const { v[0] = c[s]; }
};

// ------------------------------------------------------------------ FASTQ: one pooled slot
// Queries [q_begin, q_end); start / end null: whole reads.  EMIT = false: *cursor += the keys below T[0]; EMIT = true: the keys
// themselves at the cursor, at most cap of them.
template <bool CANON, bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_sk_fastq(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes, const int64_t *__restrict__ rlen,
                                                    const int64_t *__restrict__ soff, const int64_t *__restrict__ ids, int64_t q_begin, int64_t q_end,
                                                    const int64_t *__restrict__ start, const int64_t *__restrict__ end, int lpr, int k,
                                                    const uint64_t *__restrict__ T, uint64_t *__restrict__ out, uint64_t cap,
                                                    unsigned long long *__restrict__ cursor) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr;
    const uint64_t mask = ((uint64_t)1 << (2 * k)) - 1, t = T[0];
    unsigned long long mine = 0;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    for (int64_t q = q_begin + wave * ngrp + grp; grp < ngrp && q < q_end; q += stride) {
        const int64_t id = ids ? ids[q] : q;
        const int64_t L = rlen[id] > 0 ? rlen[id] : 0, so = soff[id] - gbase;
        const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
        kmer_fq_pieces<uint64_t, CANON>(data, so, n_bytes, a, b, sub, lpr, k, [&](uint64_t code) {
            const uint64_t key = mz_mix(code, mask);
            if (!EMIT) { mine += key < t ? 1u : 0u; return; }
            const bool in = key < t;
            const uint64_t m = __ballot(in);                 // the lanes that walk a window in this step and keep its key
            if (!in) return;
            unsigned long long base = 0;
            if (lane == __ffsll((unsigned long long)m) - 1) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
            const uint64_t pos = (((uint64_t)bhi << 32) | blo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) out[pos] = key;
        });
    }
    if (!EMIT && mine) atomicAdd(cursor, mine);
}

// ------------------------------------------------------------------ a sketch from host arrays: the checks
// Element i < n_sets: off[i] <= off[i + 1] and, with a size, at most `size` keys.  Element n_sets + j: key j lies below max_key and
// above the key in front of it in its set.  The first element that fails -> *bad (atomicMin).
__global__ __launch_bounds__(BLOCK) void k_sk_check(const int64_t *__restrict__ off, int64_t n_sets, const uint64_t *__restrict__ keys, int64_t n_keys,
                                                    uint64_t max_key, int64_t size, unsigned long long *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_sets) {
        const int64_t a = off[i], b = off[i + 1];
        if (a < 0 || b < a || b > n_keys || (size > 0 && b - a > size)) atomicMin(bad, (unsigned long long)i);
        return;
    }
    const int64_t j = i - n_sets;
    if (j >= n_keys) return;
    int64_t s = upper_bound(off, n_sets + 1, j) - 1;         // (offsets that do not ascend are reported by the lanes above)
    s = s < 0 ? 0 : (s >= n_sets ? n_sets - 1 : s);
    const bool first = off[s] == j;
    if (keys[j] >= max_key || (!first && j > 0 && keys[j - 1] >= keys[j])) atomicMin(bad, (unsigned long long)i);
}

// ------------------------------------------------------------------ comparison
struct SkSide {
    const uint64_t *keys;
    const int64_t *off;
    const int64_t *sel;                                      // the sets that take part (null: all), n of them
    int64_t n;
};
__device__ __forceinline__ int64_t sk_lower(const uint64_t *__restrict__ a, int64_t lo, int64_t hi, uint64_t x) {
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (a[m] < x) lo = m + 1; else hi = m; }
    return lo;
}

// One wave per pair (i, j) of the selected sets: shared[i * B.n + j], total[i * B.n + j] as include/fxgpu.h defines them.
__global__ __launch_bounds__(BLOCK) void k_sk_compare(SkSide A, SkSide B, int64_t limit, uint64_t max_key, int64_t *__restrict__ shared,
                                                      int64_t *__restrict__ total) {
    const int lane = lane_id();
    const int64_t n_pairs = A.n * B.n;
    const int64_t wave0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * BLOCK) >> 6;
    for (int64_t pair = wave0; pair < n_pairs; pair += n_waves) {
        const int64_t i = pair / B.n, j = pair - i * B.n;
        const int64_t sa = A.sel ? A.sel[i] : i, sb = B.sel ? B.sel[j] : j;
        const uint64_t *a = A.keys + A.off[sa], *b = B.keys + B.off[sb];
        int64_t na = A.off[sa + 1] - A.off[sa], nb = B.off[sb + 1] - B.off[sb];
        if (max_key) { na = sk_lower(a, 0, na, max_key); nb = sk_lower(b, 0, nb, max_key); }
        int64_t in_both = 0, in_limit = 0, from = 0;         // shared keys met; those of them inside the limit; no key of B in front of `from` matters any more
        bool full = false;                                   // a rank has reached the limit
        for (int64_t p0 = 0; p0 < na && !full; p0 += 64) {
            const int64_t p = p0 + lane;
            const bool live = p < na;
            const uint64_t x = live ? a[p] : 0;
            const int64_t lb = live ? sk_lower(b, from, nb, x) : nb;
            const bool hit = live && lb < nb && b[lb] == x;
            const uint64_t m = __ballot(hit);
            const int64_t rank = p + lb - (in_both + (int64_t)__popcll(m & ((1ull << lane) - 1ull)));
            const bool inside = limit == 0 || rank < limit;
            in_limit += (int64_t)__popcll(__ballot(hit && inside));
            in_both += (int64_t)__popcll(m);
            full = __ballot(live && !inside) != 0;
            from = (int64_t)(((uint64_t)(uint32_t)__shfl((int)(lb >> 32), 63, 64) << 32) | (uint32_t)__shfl((int)(lb & 0xFFFFFFFFll), 63, 64));
            // (it is used by the next chunk only, and then all lanes of this one are live)
        }
        if (lane == 0) {
            const int64_t all = na + nb - in_both;           // |U| when the loop ran to the end
            shared[pair] = in_limit;
            total[pair] = full ? limit : (limit > 0 && all > limit ? limit : all);
        }
    }
}

}  // namespace fx
