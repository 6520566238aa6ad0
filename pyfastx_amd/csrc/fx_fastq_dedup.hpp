// fx_fastq_dedup.hpp -- exact duplicate-read detection on the resident FASTQ stream for gfx950 (MI355X, wave64).  Extension: the
// definition -- the key of a query, "duplicate", first[q], the reverse-complement rule -- stands in include/fxgpu.h.  DESIGN.md 4.8.
//
// A round works on m elements (the first round: every query; a later one: the ascending list of the queries the round before
// left unresolved):
//   k_dd_hash     lpr lanes per element in the lane groups, pieces and wave-uniform trip count of k_fq_read_stats.  A piece is
//                 16 bytes RELATIVE TO `a` (the key's first byte), the last one zeroed behind `b`: what a lane folds does not
//                 depend on where the key lies in memory.  Piece j becomes dd_fold(piece, j, seed), a 64-bit value; the values of
//                 all pieces are ADDED (lanes first, then qc_group_reduce), so neither lpr nor the number of steps shows in the
//                 sum; dd_finish mixes the length in.  REVCOMP: the lane also folds the pieces of rc(key) -- piece j of it is the
//                 byte-reversed, complemented piece that ends at b - 16 j -- and the stored fingerprint is the smaller of the two.
//   (sort)        radix_sort_rows of fx_sort.hip over the fingerprint's bits, value = the element's index: stable, so the head of
//                 a run of equal fingerprints is its smallest position.
//   k_dd_rank     head flags -> group rank of every element and the heads' indices (the chunk offsets come from k_sscan_sums /
//                 k_sscan_top with KtLdHead, as in the reduction of fx_kmer_table.hpp).
//   k_dd_verify   one lane group per sorted element that is no head: its key against the head's, length first, then 16-byte
//                 pieces with a group-OR of "differs"; REVCOMP: where that differs, against the pieces of rc(head).  Equal:
//                 first[q] = the head's position.  Different (two keys, one fingerprint): the element's flag is set, it goes to
//                 the next round, and -- where the group sizes are asked for -- the run's counter of such elements gets one
//                 atomicAdd.  Heads resolve to themselves.
//   k_dd_copies   copies[head] = length of its run - the elements of the run that did not resolve.  Run-length arithmetic: the
//                 20 000 copies of one read cost no atomic at all; atomics only count collisions.
//   k_dd_pass / k_dd_gather   the dedup predicate per query, and the copies of the selected positions.
#pragma once
#include "fx_fastq_qc.hpp"
#include "fx_kmer_table.hpp"

namespace fx {

constexpr uint64_t DD_C1 = 0x9E3779B97F4A7C15ull, DD_C2 = 0xC2B2AE3D27D4EB4Full, DD_C3 = 0x165667B19E3779F9ull, DD_C4 = 0xD6E8FEB86659FD93ull;
constexpr int64_t DD_MAX_QUERIES = (int64_t)1 << 31;        // the sort's values and offsets are 32-bit

// the finalizer of splitmix64: a bijection of 64 bits
__host__ __device__ __forceinline__ uint64_t dd_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ uint64_t dd_seed(int64_t round) { return dd_mix((uint64_t)(round + 1) * DD_C4); }
__device__ __forceinline__ uint64_t dd_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// piece j of a key under `seed`: the piece's index goes into the words it is multiplied under
__device__ __forceinline__ uint64_t dd_fold(const uint32_t (&x)[4], int64_t j, uint64_t seed) {
    const uint64_t kj = seed + (uint64_t)(j + 1) * DD_C1;
    const uint64_t lo = ((uint64_t)x[1] << 32) | x[0], hi = ((uint64_t)x[3] << 32) | x[2];
    uint64_t u = (lo ^ kj) * DD_C2, t = (hi ^ dd_rotl(kj, 31)) * DD_C3;
    u ^= u >> 29;
    return dd_mix(u + dd_rotl(t, 23));
}
__device__ __forceinline__ uint64_t dd_finish(uint64_t sum, int64_t len, uint64_t seed) { return dd_mix(sum + (uint64_t)len * DD_C4 + seed); }

// A<->T, C<->G, a<->t, c<->g in every byte of w; any other byte stays.  Without its case bit a letter of a pair differs from
// its partner by 0x15 (A, T) or 0x04 (C, G).
__device__ __forceinline__ uint32_t dd_complement(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t at = (zero_bytes(u ^ 0x41414141u) | zero_bytes(u ^ 0x54545454u)) >> 7;
    const uint32_t cg = (zero_bytes(u ^ 0x43434343u) | zero_bytes(u ^ 0x47474747u)) >> 7;
    return w ^ (at * 0x15u) ^ (cg * 0x04u);
}

// The key of a query: len bytes from data + at.
struct DdKey { int64_t at, len; };
// bytes [p, p + 16) of the key, zero behind its end (p < len)
__device__ __forceinline__ void dd_piece(const uint8_t *__restrict__ data, int64_t n_bytes, const DdKey &k, int64_t p, uint32_t (&x)[4]) {
    const uint4 v = qc_load16(data, k.at + p, n_bytes);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    if (k.len - p < 16) fq_keep_first(x, (int)(k.len - p), 0u);
}
// bytes [p, p + 16) of the key's reverse complement: the 16 bytes that end at len - p, reversed and complemented; what lies in
// front of the key's first byte ends up behind the end and is zeroed
__device__ __forceinline__ void dd_piece_rc(const uint8_t *__restrict__ data, int64_t n_bytes, const DdKey &k, int64_t p, uint32_t (&x)[4]) {
    const uint4 v = qc_load16(data, k.at + k.len - p - 16, n_bytes);
    x[0] = dd_complement(__builtin_bswap32(v.w)); x[1] = dd_complement(__builtin_bswap32(v.z));
    x[2] = dd_complement(__builtin_bswap32(v.y)); x[3] = dd_complement(__builtin_bswap32(v.x));
    if (k.len - p < 16) fq_keep_first(x, (int)(k.len - p), 0u);
}

// The queries as the kernels take them: element j of a round is query list[j] (list null: j), its read ids[q] (ids null: q).
struct DdQueries {
    const int64_t *rlen, *soff, *ids, *start, *end;
    const uint32_t *list;
    int64_t gbase;
    __device__ __forceinline__ int64_t query(int64_t j) const { return list ? (int64_t)list[j] : j; }
    __device__ __forceinline__ DdKey key(int64_t q) const {
        const int64_t id = ids ? ids[q] : q;
        const int64_t L = rlen[id] > 0 ? rlen[id] : 0;
        const int64_t a = start ? start[q] : 0, b = end ? end[q] : L;
        return DdKey{soff[id] - gbase + a, b - a};
    }
};

// Elements [0, m): keys[j] = the fingerprint of element j under `seed`, cut to the bits of `mask`; vals[j] = j.
template <bool REVCOMP>
__global__ __launch_bounds__(BLOCK) void k_dd_hash(const uint8_t *__restrict__ data, int64_t n_bytes, DdQueries Q, int64_t m, int lpr, uint64_t seed,
                                                  uint64_t mask, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr, step = 16 * lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    auto get_key = [&](int64_t j) -> DdKey {                  // the key of element j, one iteration ahead of its bytes
        return live && j < m ? Q.key(Q.query(j)) : DdKey{0, 0};
    };
    int64_t j = wave * ngrp + grp;
    DdKey nxt = get_key(j);
    for (; j - grp < m; j += stride) {                        // wave-uniform trip count
        const DdKey key = nxt;
        nxt = get_key(j + stride);
        uint64_t hf = 0, hr = 0;
        for (int64_t p = (int64_t)sub * 16; p < key.len; p += step) {
            uint32_t x[4];
            dd_piece(data, n_bytes, key, p, x);
            hf += dd_fold(x, p >> 4, seed);
            if (REVCOMP) {
                dd_piece_rc(data, n_bytes, key, p, x);
                hr += dd_fold(x, p >> 4, seed);
            }
        }
        hf = qc_group_reduce(hf, lane, sub, lpr, p2, [](uint64_t a, uint64_t b) { return a + b; });
        if (REVCOMP) hr = qc_group_reduce(hr, lane, sub, lpr, p2, [](uint64_t a, uint64_t b) { return a + b; });
        if (live && sub == 0 && j < m) {
            uint64_t f = dd_finish(hf, key.len, seed);
            if (REVCOMP) { const uint64_t r = dd_finish(hr, key.len, seed); f = r < f ? r : f; }
            keys[j] = f & mask;
            vals[j] = (uint32_t)j;
        }
    }
}

// The chunks of k_sscan_sums over KtLdHead{keys}: G[i] = the rank of the run element i lies in, S[rank] = the index of its head.
__global__ __launch_bounds__(BLOCK) void k_dd_rank(const uint64_t *__restrict__ keys, int64_t m, const int64_t *__restrict__ sums,
                                                  uint32_t *__restrict__ G, uint32_t *__restrict__ S) {
    __shared__ int64_t lds[4];
    const int64_t i0 = (int64_t)blockIdx.x * SRCH_CHUNK + (int64_t)threadIdx.x * SRCH_PER;
    uint32_t flags = 0;
    for (int i = 0; i < SRCH_PER; ++i)
        if (i0 + i < m && (i0 + i == 0 || keys[i0 + i] != keys[i0 + i - 1])) flags |= 1u << i;
    const int64_t s = __popc(flags);
    int64_t tot;
    int64_t r = block_incl_scan64(s, lds, &tot) - s + sums[blockIdx.x];      // heads in front of element i0
    for (int i = 0; i < SRCH_PER && i0 + i < m; ++i) {
        if ((flags >> i) & 1u) S[r++] = (uint32_t)(i0 + i);
        G[i0 + i] = (uint32_t)(r - 1);                        // (element 0 is a head: r >= 1 from there on)
    }
}

// Sorted elements [0, m): vals[i] = the element's index in the round, G / S as k_dd_rank left them.  first[q] of every element
// that resolves; flag[j] = 1 where element j does not; unres (may be null): per run, the elements that did not.
template <bool REVCOMP>
__global__ __launch_bounds__(BLOCK) void k_dd_verify(const uint8_t *__restrict__ data, int64_t n_bytes, DdQueries Q, int64_t m, int lpr,
                                                    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ G, const uint32_t *__restrict__ S,
                                                    int64_t *__restrict__ first, uint8_t *__restrict__ flag, uint32_t *__restrict__ unres) {
    const int lane = lane_id(), grp = lane / lpr, sub = lane - grp * lpr, ngrp = 64 / lpr, step = 16 * lpr;
    const bool live = grp < ngrp;
    int p2 = 1;
    while (p2 < lpr) p2 <<= 1;
    p2 >>= 1;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t stride = (((int64_t)gridDim.x * BLOCK) >> 6) * ngrp;
    const auto either = [](uint32_t a, uint32_t b) { return a | b; };
    for (int64_t i = wave * ngrp + grp; i - grp < m; i += stride) {              // wave-uniform trip count
        const bool act = live && i < m;
        bool head = true;
        int64_t j = 0, q = 0, qh = 0;
        uint32_t run = 0, diff = 0;
        DdKey x{0, 0}, y{0, 0};
        if (act) {
            run = G[i];
            const int64_t ih = S[run];
            j = vals[i]; q = Q.query(j);
            head = ih == i;
            if (!head) {
                qh = Q.query(vals[ih]);
                x = Q.key(q); y = Q.key(qh);
                diff = x.len != y.len ? 1u : 0u;
                for (int64_t p = (int64_t)sub * 16; !diff && p < x.len; p += step) {
                    uint32_t u[4], v[4];
                    dd_piece(data, n_bytes, x, p, u);
                    dd_piece(data, n_bytes, y, p, v);
                    diff = ((u[0] ^ v[0]) | (u[1] ^ v[1]) | (u[2] ^ v[2]) | (u[3] ^ v[3])) ? 1u : 0u;
                }
            }
        }
        diff = qc_group_reduce(diff, lane, sub, lpr, p2, either);
        if (REVCOMP) {
            const uint32_t again = (uint32_t)__shfl((int)diff, lane - sub, 64);   // what the group's first lane knows now
            uint32_t drc = 0;
            if (act && !head && again) {
                drc = x.len != y.len ? 1u : 0u;
                for (int64_t p = (int64_t)sub * 16; !drc && p < x.len; p += step) {
                    uint32_t u[4], v[4];
                    dd_piece(data, n_bytes, x, p, u);
                    dd_piece_rc(data, n_bytes, y, p, v);
                    drc = ((u[0] ^ v[0]) | (u[1] ^ v[1]) | (u[2] ^ v[2]) | (u[3] ^ v[3])) ? 1u : 0u;
                }
            }
            drc = qc_group_reduce(drc, lane, sub, lpr, p2, either);
            diff &= drc;
        }
        if (act && sub == 0) {
            if (!diff) first[q] = head ? q : qh;
            else if (unres) atomicAdd(&unres[run], 1u);
            flag[j] = diff ? 1 : 0;
        }
    }
}

// copies[q of head r] = the length of run r - its unresolved elements; *nd = the number of runs
__global__ __launch_bounds__(BLOCK) void k_dd_copies(const uint32_t *__restrict__ S, const int64_t *__restrict__ nd, int64_t m,
                                                    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ list,
                                                    const uint32_t *__restrict__ unres, uint32_t *__restrict__ copies) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x, n = *nd;
    if (r >= n) return;
    const uint32_t j = vals[S[r]];
    copies[list ? list[j] : j] = (uint32_t)(kt_run_len(S, r, n, m) - (int64_t)unres[r]);
}

// What the compaction does with unresolved element j, number jj among them: the query it stands for goes to the next list.
struct DdPutList {
    const uint32_t *list;
    uint32_t *next;
    __device__ void operator()(int64_t j, int64_t jj) const { next[jj] = list ? list[j] : (uint32_t)j; }
};

// pass[q] = "q is the first occurrence of its group and the group has min_copies..max_copies members" (max_copies < 0: not asked)
__global__ __launch_bounds__(BLOCK) void k_dd_pass(const int64_t *__restrict__ first, const uint32_t *__restrict__ copies, int64_t n,
                                                  int64_t min_copies, int64_t max_copies, uint8_t *__restrict__ pass) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    bool ok = first[q] == q;
    if (ok) { const int64_t c = copies[q]; ok = c >= min_copies && (max_copies < 0 || c <= max_copies); }
    pass[q] = ok ? 1 : 0;
}
__global__ __launch_bounds__(BLOCK) void k_dd_gather(const int64_t *__restrict__ pos, int64_t n, const uint32_t *__restrict__ copies,
                                                    int64_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k < n) out[k] = (int64_t)copies[pos[k]];
}

}  // namespace fx
