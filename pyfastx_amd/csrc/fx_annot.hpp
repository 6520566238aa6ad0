// fx_annot.hpp -- composition of intervals and of windows, and the maximal runs of a letter class, on the sequence bytes of
// the resident FASTA table (fx_fasta_region_counts, fx_fasta_window_counts, fx_fasta_class_runs).  Regions replace the
// reference's slice-then-count on the host (sequence.c:562-749: composition, gc_content, gc_skew of a Sequence); windows and
// class runs are extensions.
//
// Text and classes.  The text of a record is what fx_search.hpp walks: the bytes of [boff, boff + blen) with 10 / 13 / 32
// dropped, cut at slen.  Seven counters: A C G T N (either case), other (every other kept byte, U included), masked (kept
// bytes in a..z, overlapping the first six).
//
// Rank index (k_an_rank + one 8-component scan).  The run layout of fx_search.hpp over ALL records: a run is the part of one
// record inside one aligned 256-byte block of the stream.  A group of 16 lanes owns one run: lane j loads the 16 bytes
// [blk + 16 j, blk + 16 j + 16) -- one coalesced 256-byte row per group -- and classifies them four at a time with SWAR
// compares (no branch per byte); the seven 9-bit fields kept A C G T N masked (each <= 256) share one 64-bit word, summed over
// the group with four xor-shuffles.  The multi-component scan of fx_search.hpp turns the words into eight exclusive int64
// prefixes per run -- kept, A, C, G, T, N, other = kept - (A + .. + N), masked -- 64 bytes per 256-byte run, a quarter of the
// stream beside it, kept on the handle with run0 (first run of every record).
//
// Regions (k_an_region).  A group of 16 lanes per (record, start, stop): the run that holds base `start` by a binary search
// over the kept prefix between the record's first and last run, the same for `stop`; the group reads each of those two runs
// once (256 raw bytes, coalesced) and counts the classes of its first t kept bytes; lanes 0..6 subtract the prefixes of their
// column.  Nothing else of the record is read, whatever the region's length.  Windows are regions made on the device
// (k_an_windows: slot from a scan of the per-record window counts).
//
// Class runs.  One lane per run of the SELECTED records walks its bytes against a 256-bit set (LDS).  k_an_runs_count notes,
// per run, the first and the last letter outside the set and the intervals closed between two such letters inside the run.
// What is open at a run's entry starts behind the last outside letter of an earlier run of the same record: a scan of "has an
// outside letter" and the compacted list of those runs name that run for every run (the stretch may span thousands of runs),
// no max-scan needed because positions only grow along a record.  k_an_runs_close adds the interval the run's first outside
// letter closes and, in a record's last run, the one the end of the text closes; a scan of the counts gives the offsets;
// k_an_runs_emit walks the runs that close something again and stores (record, start, stop) -- ordered by the layout, no sort,
// no atomic.  Kept bytes behind slen are never looked at: an interval reaching the cut ends at slen.
#pragma once
#include "fx_search.hpp"

namespace fx {

constexpr int AN_NCOL = 7;                                 // A C G T N other masked
constexpr int AN_NPREF = 8;                                // kept + the seven
constexpr int AN_LPR = 16;                                 // lanes per run (16 bytes each)
constexpr int AN_GROUPS = BLOCK / AN_LPR;                  // runs / queries a workgroup takes

// ------------------------------------------------------------------ SWAR over four bytes
// 0x80 in every byte of v that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t an_zero(uint32_t v) {
    const uint32_t t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | v | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t an_eq(uint32_t v, uint32_t c) { return an_zero(v ^ (c * 0x01010101u)); }
// 0x80 in every byte of v that lies in 'a'..'z'
__device__ __forceinline__ uint32_t an_lower(uint32_t v) {
    const uint32_t l = v & 0x7F7F7F7Fu;
    return (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u) & ~v & 0x80808080u;       // low 7 bits >= 0x61 and < 0x7B, bit 7 clear
}
// bits 0..3 of nib -> 0x80 of bytes 0..3
__device__ __forceinline__ uint32_t an_spread(uint32_t nib) { return (((nib & 15u) * 0x00204081u) & 0x01010101u) << 7; }
// 0x80 flags of bytes 0..3 -> bits 0..3
__device__ __forceinline__ uint32_t an_gather(uint32_t f) { return (((f >> 7) * 0x00204081u) >> 21) & 15u; }

// the seven fields of one word: kept, A, C, G, T, N, masked at bits 9 * i
__device__ __forceinline__ uint64_t an_field(uint32_t n, int i) { return (uint64_t)n << (9 * i); }
__device__ __forceinline__ uint32_t an_get(uint64_t w, int i) { return (uint32_t)(w >> (9 * i)) & 511u; }

// 16 bytes, of which those whose bit is set in live16 are inside the run -> bits of the kept ones (not 10 / 13 / 32)
__device__ __forceinline__ uint32_t an_kept16(const uint4 &q, uint32_t live16) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) k |= an_gather(~(an_eq(w[i], 10u) | an_eq(w[i], 13u) | an_eq(w[i], 32u)) & 0x80808080u) << (4 * i);
    return k & live16;
}
// the packed class counts of the bytes of q whose bit is set in take16 (a subset of the kept ones)
__device__ __forceinline__ uint64_t an_classify16(const uint4 &q, uint32_t take16) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t n[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t m = an_spread(take16 >> (4 * i)), f = w[i] & ~0x20202020u;      // f: case folded (only X and x fold onto X)
        n[0] += __popc(an_eq(f, 'A') & m);
        n[1] += __popc(an_eq(f, 'C') & m);
        n[2] += __popc(an_eq(f, 'G') & m);
        n[3] += __popc(an_eq(f, 'T') & m);
        n[4] += __popc(an_eq(f, 'N') & m);
        n[5] += __popc(an_lower(w[i]) & m);
    }
    return an_field(__popc(take16), 0) | an_field(n[0], 1) | an_field(n[1], 2) | an_field(n[2], 3) | an_field(n[3], 4) | an_field(n[4], 5) |
           an_field(n[5], 6);
}
__device__ __forceinline__ uint64_t an_shfl_xor64(uint64_t v, int d) {
    const int lo = __shfl_xor((int)(uint32_t)v, d, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
// sum over the 16 lanes of a group (fields never overflow: a run has at most 256 bytes)
__device__ __forceinline__ uint64_t an_group_sum(uint64_t v) {
#pragma unroll
    for (int d = 1; d < AN_LPR; d <<= 1) v += an_shfl_xor64(v, d);
    return v;
}
// this lane's 16 bytes of the run [lo, hi) inside the block at blk: the bytes (zero when none is inside) and which are inside
__device__ __forceinline__ uint4 an_load16(const SearchPlan &P, int64_t blk, int sub, int64_t lo, int64_t hi, uint32_t *live16) {
    const int64_t c = blk + 16 * sub;
    const int s = (int)min(max(lo - c, (int64_t)0), (int64_t)16), t = (int)min(max(hi - c, (int64_t)0), (int64_t)16);
    *live16 = t > s ? ((1u << t) - 1u) & ~((1u << s) - 1u) : 0u;
    return *live16 ? *reinterpret_cast<const uint4 *>(P.base + c) : make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------ rank index
// words[g] = the packed counts of run g; one group of 16 lanes per run
__global__ __launch_bounds__(BLOCK) void k_an_rank(SearchPlan P, uint64_t *__restrict__ words) {
    const int sub = threadIdx.x & (AN_LPR - 1);
    const int64_t g = (int64_t)blockIdx.x * AN_GROUPS + (threadIdx.x / AN_LPR);
    uint64_t w = 0;
    if (g < P.n_runs) {                                     // (a whole group leaves or stays: the shuffles below see all 16)
        int64_t r, b, lo, hi;
        srch_run(P, g, srch_slot(P, g), r, b, lo, hi);
        uint32_t live;
        const uint4 q = an_load16(P, lo & ~(int64_t)(SRCH_RUN - 1), sub, lo, hi, &live);
        w = an_classify16(q, an_kept16(q, live));
    }
    w = an_group_sum(w);
    if (g < P.n_runs && sub == 0) words[g] = w;
}
struct AnLdRank {                          // kept, A, C, G, T, N, other, masked
    const uint64_t *p;
    __device__ void operator()(int64_t g, int64_t *v) const {
        const uint64_t w = p[g];
        int64_t named = 0;
        v[0] = an_get(w, 0);
        for (int i = 1; i <= 5; ++i) { v[i] = an_get(w, i); named += v[i]; }
        v[6] = v[0] - named;
        v[7] = an_get(w, 6);
    }
};

// The index as the kernels take it: run0 over all records, pref + c * (n_runs + 1) = exclusive prefix of component c.
struct RankIndex {
    const int64_t *run0, *pref;
    int64_t n_runs;
};

// ------------------------------------------------------------------ regions
// position pos (0..slen) of record r with runs [g0, g1): the packed counts of the first t kept bytes of the run g that holds
// it (summed over the group), *run = g.  g0 == g1 (a record without bytes): nothing, *run = g0.
__device__ __forceinline__ uint64_t an_partial(const SearchPlan &P, const RankIndex &X, int64_t r, int64_t g0, int64_t g1, int64_t pos,
                                               int sub, int64_t *run) {
    *run = g0;
    if (g0 == g1) return 0;
    const int64_t *K = X.pref, k0 = K[g0];
    int64_t a = g0, z = g1 - 1;                             // last run whose first base is <= pos
    while (a < z) { const int64_t m = (a + z + 1) >> 1; if (K[m] - k0 <= pos) a = m; else z = m - 1; }
    *run = a;
    const int64_t t = pos - (K[a] - k0);
    if (t <= 0) return 0;                                   // (uniform over the group)
    int64_t b, e;
    srch_extent(P, r, b, e);
    const int64_t blk = (b & ~(int64_t)(SRCH_RUN - 1)) + (a - g0) * SRCH_RUN;
    uint32_t live;
    const uint4 q = an_load16(P, blk, sub, max(b, blk), min(e, blk + SRCH_RUN), &live);
    uint32_t kept = an_kept16(q, live);
    // kept bytes in the lanes below this one: an inclusive scan over the group, minus the lane's own
    int cnt = __popc(kept), inc = cnt;
#pragma unroll
    for (int d = 1; d < AN_LPR; d <<= 1) { const int o = __shfl_up(inc, d, AN_LPR); if (sub >= d) inc += o; }
    const int64_t room = t - (inc - cnt);                   // of this lane's kept bytes, the first `room` count
    if (room <= 0) kept = 0;
    else if (room < cnt) {
        uint32_t rest = kept;
        for (int i = 0; i < (int)room; ++i) rest &= rest - 1;       // drop the lowest `room` set bits: what remains is behind the cut
        kept &= ~rest;
    }
    return an_group_sum(an_classify16(q, kept));
}
__device__ __forceinline__ int64_t an_column(uint64_t w, int col) {             // column 0..6 of a packed word
    if (col == 5) return (int64_t)an_get(w, 0) - an_get(w, 1) - an_get(w, 2) - an_get(w, 3) - an_get(w, 4) - an_get(w, 5);
    return an_get(w, col < 5 ? col + 1 : 6);
}

// counts[i * 7 + c] of query i; a query outside the table or its record: zeros and atomicMin(bad, i)
__global__ __launch_bounds__(BLOCK) void k_an_region(SearchPlan P, RankIndex X, int64_t n_rec, const int64_t *__restrict__ id,
                                                     const int64_t *__restrict__ qa, const int64_t *__restrict__ qb, int64_t n,
                                                     int64_t *__restrict__ counts, unsigned long long *__restrict__ bad) {
    const int sub = threadIdx.x & (AN_LPR - 1);
    const int64_t i = (int64_t)blockIdx.x * AN_GROUPS + (threadIdx.x / AN_LPR);
    if (i >= n) return;                                     // (whole groups)
    const int64_t r = id[i], x = qa[i], y = qb[i];
    const bool ok = r >= 0 && r < n_rec && x >= 0 && y >= x && y <= P.slen[r];
    if (!ok) {
        if (sub == 0) atomicMin(bad, (unsigned long long)i);
        if (sub < AN_NCOL) counts[i * AN_NCOL + sub] = 0;
        return;
    }
    const int64_t g0 = X.run0[r], g1 = X.run0[r + 1];
    int64_t ga, gb;
    const uint64_t wa = an_partial(P, X, r, g0, g1, x, sub, &ga), wb = an_partial(P, X, r, g0, g1, y, sub, &gb);
    if (sub < AN_NCOL) {
        const int64_t *pc = X.pref + (int64_t)(sub + 1) * (X.n_runs + 1);
        counts[i * AN_NCOL + sub] = x == y ? 0 : (pc[gb] + an_column(wb, sub)) - (pc[ga] + an_column(wa, sub));
    }
}

// windows of selected record k: [j step, min(j step + window, slen)) for j step < slen; without `partial` only the whole ones
struct AnLdWindows {
    const int64_t *slen, *sel;
    int64_t window, step;
    int partial;
    __device__ void operator()(int64_t k, int64_t *v) const {
        const int64_t s = slen[sel ? sel[k] : k];
        v[0] = partial ? (s > 0 ? (s - 1) / step + 1 : 0) : (s >= window ? (s - window) / step + 1 : 0);
    }
};
// window i -> (record, start, stop): its record from the scan of the counts (woff: n_sel + 1)
__global__ __launch_bounds__(BLOCK) void k_an_windows(const int64_t *__restrict__ slen, const int64_t *__restrict__ sel, int64_t n_sel,
                                                      const int64_t *__restrict__ woff, int64_t window, int64_t step, int64_t n,
                                                      int64_t *__restrict__ o_rec, int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t k = upper_bound(woff, n_sel + 1, i) - 1, r = sel ? sel[k] : k, a = (i - woff[k]) * step;
    o_rec[i] = r;
    o_start[i] = a;
    o_stop[i] = a + min(window, slen[r] - a);
}

// ------------------------------------------------------------------ class runs
// P: the plan over the SELECTED records (run q of slot k); X: the index over all records, in whose numbering that run is
// X.run0[r] + (q - P.run0[k]).
struct RunsArg {
    const uint32_t *set;                  // 8 words: bit c = byte value c is in the class
    int64_t min_len;
};
constexpr uint32_t AN_NOFIRST = 511u;
// per run: intervals it closes (bits 0..7), kept index of its first outside letter (8..16, AN_NOFIRST: none), kept index
// behind its last outside letter (17..25, 0: none)
__device__ __forceinline__ uint32_t an_runs_pack(uint32_t closes, uint32_t first, uint32_t behind) { return closes | (first << 8) | (behind << 17); }

// geometry of selected run q: record, record-local position of its first kept byte, length L of the record's text
struct AnRun { int64_t k, r, b, lo, hi, base, L; bool last; };
__device__ __forceinline__ AnRun an_run(const SearchPlan &P, const RankIndex &X, int64_t q) {
    AnRun R;
    R.k = srch_slot(P, q);
    srch_run(P, q, R.k, R.r, R.b, R.lo, R.hi);
    const int64_t g0 = X.run0[R.r], g = g0 + (q - P.run0[R.k]);
    R.base = X.pref[g] - X.pref[g0];
    R.L = min(P.slen[R.r], X.pref[X.run0[R.r + 1]] - X.pref[g0]);
    R.last = q + 1 == P.run0[R.k + 1];
    return R;
}
// The kept bytes of the run in front of the cut, in order: outside(i) for every one that is not in the set (i: kept index).
template <class F>
__device__ __forceinline__ void an_runs_walk(const SearchPlan &P, const uint32_t *set, const AnRun &R, F &&outside) {
    const int64_t limit = R.L - R.base;
    if (limit <= 0) return;
    int64_t kidx = 0;
    for (int64_t c = R.lo & ~(int64_t)15; c < R.hi && kidx < limit; c += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t ch = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            const bool kept = c + i >= R.lo && c + i < R.hi && !srch_space(ch) && kidx < limit;
            if (kept && !((set[ch >> 5] >> (ch & 31u)) & 1u)) outside(kidx);
            kidx += kept ? 1 : 0;
        }
    }
}
__device__ __forceinline__ void an_load_set(const RunsArg &A, uint32_t *set) {
    if (threadIdx.x < 8) set[threadIdx.x] = A.set[threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void k_an_runs_count(SearchPlan P, RankIndex X, RunsArg A, uint32_t *__restrict__ packed) {
    __shared__ uint32_t set[8];
    an_load_set(A, set);
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const AnRun R = an_run(P, X, q);
    uint32_t closes = 0, first = AN_NOFIRST, behind = 0;
    an_runs_walk(P, set, R, [&](int64_t i) {
        if (first == AN_NOFIRST) first = (uint32_t)i;
        else closes += i - (int64_t)behind >= A.min_len ? 1u : 0u;
        behind = (uint32_t)i + 1u;
    });
    packed[q] = an_runs_pack(closes, first, behind);
}
struct AnLdOutside {                      // "the run has a letter outside the set"
    const uint32_t *p;
    __device__ void operator()(int64_t q, int64_t *v) const { v[0] = ((p[q] >> 8) & 511u) != AN_NOFIRST; }
};
struct AnLdCloses {
    const uint32_t *p;
    __device__ void operator()(int64_t q, int64_t *v) const { v[0] = p[q] & 255u; }
};
// list[NZ[q]] = q for every run with a letter outside the set
__global__ __launch_bounds__(BLOCK) void k_an_runs_list(const uint32_t *__restrict__ packed, const int64_t *__restrict__ NZ, int64_t n_runs,
                                                        int64_t *__restrict__ list) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q < n_runs && ((packed[q] >> 8) & 511u) != AN_NOFIRST) list[NZ[q]] = q;
}
// where the stretch that is open at the entry of run q starts: behind the last outside letter of an earlier run of the
// same record, or at 0
__device__ __forceinline__ int64_t an_open_start(const SearchPlan &P, const RankIndex &X, const AnRun &R, int64_t q,
                                                 const uint32_t *__restrict__ packed, const int64_t *__restrict__ NZ,
                                                 const int64_t *__restrict__ list) {
    const int64_t nz = NZ[q];
    if (nz == 0) return 0;
    const int64_t p = list[nz - 1];
    if (p < P.run0[R.k]) return 0;
    const int64_t g0 = X.run0[R.r], g = g0 + (p - P.run0[R.k]);
    return X.pref[g] - X.pref[g0] + ((packed[p] >> 17) & 511u);
}
// adds what the scan decides: the interval the run's first outside letter closes, and in a record's last run the one the
// end of the text closes
__global__ __launch_bounds__(BLOCK) void k_an_runs_close(SearchPlan P, RankIndex X, RunsArg A, const int64_t *__restrict__ NZ,
                                                         const int64_t *__restrict__ list, uint32_t *__restrict__ packed) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const AnRun R = an_run(P, X, q);
    const uint32_t w = packed[q], first = (w >> 8) & 511u, behind = (w >> 17) & 511u;
    int64_t cur = an_open_start(P, X, R, q, packed, NZ, list);
    uint32_t closes = w & 255u;
    if (first != AN_NOFIRST) {
        closes += R.base + first - cur >= A.min_len ? 1u : 0u;
        cur = R.base + behind;
    }
    if (R.last) closes += R.L - cur >= A.min_len ? 1u : 0u;
    packed[q] = (w & ~255u) | closes;
}
// the runs that close something walk again and store their intervals at O[q] (exclusive prefix of the counts)
__global__ __launch_bounds__(BLOCK) void k_an_runs_emit(SearchPlan P, RankIndex X, RunsArg A, const uint32_t *__restrict__ packed,
                                                        const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                        const int64_t *__restrict__ O, int64_t *__restrict__ o_rec,
                                                        int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop) {
    __shared__ uint32_t set[8];
    an_load_set(A, set);
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs || !(packed[q] & 255u)) return;
    const AnRun R = an_run(P, X, q);
    int64_t cur = an_open_start(P, X, R, q, packed, NZ, list), o = O[q];
    const int64_t o_end = O[q + 1];
    auto put = [&](int64_t stop) {
        if (stop - cur >= A.min_len && o < o_end) { o_rec[o] = R.r; o_start[o] = cur; o_stop[o] = stop; ++o; }
    };
    an_runs_walk(P, set, R, [&](int64_t i) { put(R.base + i); cur = R.base + i + 1; });
    if (R.last) put(R.L);
}

}  // namespace fx
