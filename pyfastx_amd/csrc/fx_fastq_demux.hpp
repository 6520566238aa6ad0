// fx_fastq_demux.hpp -- barcode demultiplexing on the resident FASTQ stream for gfx950 (MI355X, wave64).
// Extension: the reference has no counterpart.  Everything is integer and exact; the definition is the one of include/fxgpu.h.
//
//   k_fq_demux   ONE LANE PER QUERY (not the lane groups of k_fq_trim: a window is at most 32 letters).  The lane fetches its
//        table row and finds, per segment, where slot 0 of its window lies in the stream and which slots exist:
//          5' / 3'   soff + off, or soff + L - off - len; the slots inside [0, L).
//          header    the 80 bytes in front of the sequence line's newline come by five 16-byte loads (qc_load16); one
//                    trailing '\r' is taken off; eq_mask16 turns them into an 80-bit mask of ':' and one of '+'.  Only the
//                    last min(|H|, 66) bytes of the header count: no ':' there means no ':' at all or a field of more than
//                    65 bytes -- every slot ABSENT either way.  The highest ':' bit starts the field, the lowest '+' bit
//                    above it ends part 0 and starts part 1.
//        The window itself is two unaligned 16-byte loads at slot 0 (they hit the lines the header pieces or the row's
//        neighbours brought in), packed as k_fq_trim packs a piece: 2 bits per letter ((b >> 1) & 3) plus one "not A C G T"
//        bit per letter, both spread over a 32-bit word; the flag is also set for an ABSENT slot, so it mismatches every
//        letter that counts.  The packed sheet -- per sample and segment two code and two care words, packed on the host as
//        TrimPar::acode / acare -- is read from device memory with a wave-uniform index (scalar loads); one sample costs per
//        word (one when no segment has more than 16 letters: the template argument) an XOR, the pair-OR and mask, a
//        popcount, then two compares and the best / second / index update in registers.  Bins are counted in a per-workgroup LDS histogram of n_samples + 2 words, whose non-zero entries go to
//        the int64 counters by one global atomic each.  With want_order the lane also writes its (bin, position) row for the
//        sort.
//   k_fq_demux_bins    one workgroup: the exclusive scan of the counters -> bin_off (n_samples + 3 entries).
//   k_fq_demux_order   the positions the stable radix sort (fx_sort.hpp: radix_sort_rows on the bin key) left, widened to int64.
#pragma once
#include "fx_fastq_trim.hpp"

namespace fx {

constexpr int DEMUX_MAX_SAMPLES = 4096, DEMUX_MAX_LEN = 32;
constexpr int DEMUX_SEQ5 = 0, DEMUX_SEQ3 = 1, DEMUX_HEADER = 2;
constexpr int DEMUX_NONE = -1, DEMUX_AMBIGUOUS = -2;
constexpr int DEMUX_HDR_BYTES = 80, DEMUX_HDR_LOOK = 66;     // bytes loaded in front of the newline; bytes of the header that count
constexpr int DEMUX_SET_WORDS = 8;                           // per sample: segment 0 code[2], care[2], segment 1 code[2], care[2]

struct DemuxPar {
    int n_seg, n_samples, margin;
    int src[2], off[2], len[2], mm[2];
};
struct DemuxOut {
    int32_t *sample, *dist, *second;
    unsigned long long *counts;                              // n_samples + 2
    uint64_t *key;                                           // want_order: the bin of query q, and q itself
    uint32_t *val;
};

typedef unsigned __int128 demux_u128;
__device__ __forceinline__ demux_u128 demux_below(int b) { return ((demux_u128)1 << b) - 1; }       // bits 0 .. b-1, 0 <= b <= 80
__device__ __forceinline__ int demux_top_bit(demux_u128 m) {                                         // m != 0
    const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
    return hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
}
__device__ __forceinline__ int demux_low_bit(demux_u128 m) {                                         // m != 0
    const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
    return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi);
}

// 16 bytes -> their 2-bit codes and their "not A C G T" flags (bit 0 of each pair), as k_fq_trim packs a piece
__device__ __forceinline__ void demux_pack16(const uint4 &v, uint32_t *code, uint32_t *flag) {
    const uint32_t s[4] = {v.x, v.y, v.z, v.w};
    uint32_t c = 0, f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t z = zero_bytes(s[k] ^ __builtin_amdgcn_perm(QC_EX_HI, QC_EX_LO, (s[k] >> 1) & 0x07070707u));
        const uint32_t x = (s[k] >> 1) & 0x03030303u, y = (~z >> 7) & 0x01010101u;
        c |= ((x | (x >> 6) | (x >> 12) | (x >> 18)) & 0xFFu) << (8 * k);
        f |= ((y | (y >> 6) | (y >> 12) | (y >> 18)) & 0x55u) << (8 * k);
    }
    *code = c; *flag = f;
}

template <bool WIDE>                                         // WIDE: a segment has more than 16 letters, the second word of a window counts
__global__ __launch_bounds__(BLOCK) void k_fq_demux(const uint8_t *__restrict__ data, int64_t gbase, int64_t n_bytes,
                                                   const int64_t *__restrict__ rlen, const int64_t *__restrict__ soff,
                                                   const int32_t *__restrict__ dlen, const int64_t *__restrict__ ids, int64_t nq,
                                                   DemuxPar P, const uint32_t *__restrict__ set, DemuxOut out) {
    __shared__ uint32_t hist[DEMUX_MAX_SAMPLES + 2];
    const int nb = P.n_samples + 2;
    for (int b = threadIdx.x; b < nb; b += BLOCK) hist[b] = 0;
    __syncthreads();
    const bool any_hdr = P.src[0] == DEMUX_HEADER || (P.n_seg > 1 && P.src[1] == DEMUX_HEADER);
    for (int64_t q0 = (int64_t)blockIdx.x * BLOCK; q0 < nq; q0 += (int64_t)gridDim.x * BLOCK) {       // the same trips for every lane
        const int64_t q = q0 + threadIdx.x;
        const bool live = q < nq;
        int64_t L = 0, so = 0;
        int hl = 0;
        if (live) {
            const int64_t id = ids ? ids[q] : q;
            L = rlen[id] > 0 ? rlen[id] : 0;
            so = soff[id] - gbase;
            hl = dlen[id] > 0 ? dlen[id] : 0;
        }
        // ---- the header's index field: where part 0 and part 1 start among the 80 bytes that end at the newline, and how long they are
        int part_at[2] = {0, 0}, part_len[2] = {0, 0};
        if (any_hdr && live && hl > 0) {
            demux_u128 colon = 0, plus = 0;
            uint32_t last = 0;
#pragma unroll
            for (int k = 0; k < DEMUX_HDR_BYTES / 16; ++k) {
                const uint4 v = qc_load16(data, so - 1 - DEMUX_HDR_BYTES + 16 * k, n_bytes);
                colon |= (demux_u128)eq_mask16(v, 0x3A3A3A3Au) << (16 * k);
                plus |= (demux_u128)eq_mask16(v, 0x2B2B2B2Bu) << (16 * k);
                last = v.w >> 24;
            }
            int te = DEMUX_HDR_BYTES;                         // one past the header's last byte
            if (last == 13) { --te; --hl; }                   // one trailing '\r' is not part of it
            const int look = hl < DEMUX_HDR_LOOK ? hl : DEMUX_HDR_LOOK;
            const demux_u128 in_hdr = demux_below(te) & ~demux_below(te - look);
            colon &= in_hdr;
            if (colon != 0) {
                const int tc = demux_top_bit(colon);          // the field is bytes tc + 1 .. te - 1: at most 65
                plus &= in_hdr & ~demux_below(tc + 1);
                const int tp = plus != 0 ? demux_low_bit(plus) : te;
                part_at[0] = tc + 1; part_len[0] = tp - tc - 1;
                part_at[1] = tp + 1; part_len[1] = tp < te ? te - tp - 1 : 0;
            }
        }
        // ---- the windows: codes and flags of up to 32 slots per segment
        uint32_t cw[2][2] = {{0, 0}, {0, 0}}, fw[2][2] = {{0x55555555u, 0x55555555u}, {0x55555555u, 0x55555555u}};
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (g >= P.n_seg) break;
            const int len = P.len[g];
            int64_t at;                                       // the stream offset of slot 0
            int lo = 0, hi;                                   // the slots lo .. hi - 1 exist
            if (P.src[g] == DEMUX_HEADER) {
                const int part = P.off[g] ? 1 : 0;
                at = so - 1 - DEMUX_HDR_BYTES + (part ? part_at[1] : part_at[0]);
                hi = min(len, part ? part_len[1] : part_len[0]);
            } else if (P.src[g] == DEMUX_SEQ5) {
                at = so + P.off[g];
                hi = (int)max((int64_t)0, min((int64_t)len, L - P.off[g]));
            } else {
                const int64_t p0 = L - P.off[g] - len;        // slot j is s[p0 + j]; p0 + len <= L
                at = so + p0;
                lo = (int)min((int64_t)len, max((int64_t)0, -p0));
                hi = len;
            }
            if (live && hi > lo) {
                demux_pack16(qc_load16(data, at, n_bytes), &cw[g][0], &fw[g][0]);
                if (hi > 16) demux_pack16(qc_load16(data, at + 16, n_bytes), &cw[g][1], &fw[g][1]);
#pragma unroll
                for (int k = 0; k < 2; ++k)                   // an ABSENT slot mismatches like a byte that is no letter
                    fw[g][k] |= 0x55555555u & ~(trim_len_mask(hi, k) & ~trim_len_mask(lo, k));
            }
        }
        // ---- the sheet, sample by sample: the index is the same in every lane
        int best = TRIM_NONE, second = TRIM_NONE, idx = DEMUX_NONE;
#pragma unroll 4
        for (int s = 0; s < P.n_samples; ++s) {               // (unrolled: the scalar loads of four samples are in flight together)
            const uint32_t *w = set + (size_t)s * DEMUX_SET_WORDS;
            auto dist_of = [&](int g) -> int {
                const uint32_t d0 = cw[g][0] ^ w[4 * g];
                int d = __popc((((d0 | (d0 >> 1)) & 0x55555555u) | fw[g][0]) & w[4 * g + 2]);
                if constexpr (WIDE) {
                    const uint32_t d1 = cw[g][1] ^ w[4 * g + 1];
                    d += __popc((((d1 | (d1 >> 1)) & 0x55555555u) | fw[g][1]) & w[4 * g + 3]);
                }
                return d;
            };
            const int t0 = dist_of(0), t1 = P.n_seg > 1 ? dist_of(1) : 0;
            const bool pass = (t0 <= P.mm[0]) & (t1 <= P.mm[1]);                  // (one segment: t1 = 0 passes any budget)
            const int t = t0 + t1;
            const bool better = pass & (t < best);
            second = better ? best : (pass & (t < second)) ? t : second;
            idx = better ? s : idx;
            best = better ? t : best;
        }
        if (live) {
            int smp = idx, d = best, d2 = second;
            if (best == TRIM_NONE) { smp = DEMUX_NONE; d = -1; d2 = -1; }
            else if (second == TRIM_NONE) d2 = -1;
            else if (second - best < P.margin) smp = DEMUX_AMBIGUOUS;
            out.sample[q] = smp; out.dist[q] = d; out.second[q] = d2;
            const int bin = smp >= 0 ? smp : smp == DEMUX_NONE ? P.n_samples : P.n_samples + 1;
            atomicAdd(&hist[bin], 1u);
            if (out.key) { out.key[q] = (uint64_t)bin; out.val[q] = (uint32_t)q; }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += BLOCK)
        if (hist[b]) atomicAdd(&out.counts[b], (unsigned long long)hist[b]);
}

// one workgroup: bin_off[k] = the queries of the bins in front of bin k, k = 0 .. nb (nb <= DEMUX_MAX_SAMPLES + 2)
__global__ __launch_bounds__(BLOCK) void k_fq_demux_bins(const unsigned long long *__restrict__ counts, int nb, int64_t *__restrict__ bin_off) {
    __shared__ int64_t lds[4];
    constexpr int PER = (DEMUX_MAX_SAMPLES + 2 + BLOCK - 1) / BLOCK;
    const int b0 = threadIdx.x * PER;
    int64_t s = 0;
    for (int i = 0; i < PER; ++i)
        if (b0 + i < nb) s += (int64_t)counts[b0 + i];
    int64_t tot;
    int64_t run = block_incl_scan64(s, lds, &tot) - s;
    for (int i = 0; i < PER && b0 + i < nb; ++i) {
        bin_off[b0 + i] = run;
        run += (int64_t)counts[b0 + i];
    }
    if (threadIdx.x == 0) bin_off[nb] = tot;
}

__global__ __launch_bounds__(BLOCK) void k_fq_demux_order(const uint32_t *__restrict__ val, int64_t n, int64_t *__restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) order[i] = (int64_t)val[i];
}

}  // namespace fx
