// BGZF written on the device: a deflate encoder, one workgroup per member.
// Extension: the reference writes nothing compressed.
//
// Member m carries the input bytes [m * 65280, min(n, (m + 1) * 65280)) (htslib's block size) and refers to nothing outside
// itself: 18 bytes of header (1f 8b 08 04, mtime 0, XFL 0, OS ff, XLEN 6, "BC", SLEN 2, BSIZE - 1), one deflate stream with
// one block, the CRC-32 of the payload, ISIZE.  65280 + 5 (stored-block header) + 26 <= 65536: a member can always be stored.
//
//   k_bgzf_store     level 0: header, a stored block, ISIZE, straight to the packed place (member m begins at m * 65311).
//   k_bgzf_deflate   levels 1 and 2: one workgroup of 512 lanes per member, the payload and the position tables in LDS.
//        histogram   the bytes of the payload (LDS adds): the literal counts of level 1, the literal prices of level 2
//                    (8 * log2(n / count), at least one bit).
//        parse       level 2, in lock step over windows of 512 positions: every lane looks its position up in two tables
//                    (a hash of 8 bytes, then one of 4; entry = the largest earlier position with that hash, +1) and, failing
//                    both, tries distance 1; a candidate is compared byte by byte (lengths 4..258, distances 1..32768, never
//                    past the member's end) and kept when its estimated price (7 + 5 bits and the extra bits) is below the
//                    prices of the literals it replaces.  Only after a barrier are the window's positions entered (LDS
//                    atomicMax), so a look-up sees earlier windows alone and the tables never depend on the order the waves
//                    ran in.  Wave 0 then walks the window greedily by ballot: from the first position the last match left
//                    free to the next lane that has a match, over it, and so on; a window without one is 512 literals in
//                    8 steps.  Every lane reads off whether it begins a chosen match, lies under one or is a literal,
//                    writes its token word to the workgroup's scratch (one word per position) and counts its symbols.
//        codes       symbols ranked by (count, symbol) by all lanes; one lane merges (two queues), reads the depths, limits
//                    them (15; 7 for the code-length code) by moving leaves down until Kraft holds with equality, gives the
//                    longest lengths to the rarest symbols and numbers the codes canonically.  One used distance code, or
//                    none, is sent as a single code of length 1.
//        emit        bits per token, a workgroup scan over 128 positions per lane, and every lane ORs its tokens into the LDS
//                    words the payload lay in (cleared by the pass itself first); Huffman codes bit-reversed, extra bits as
//                    they are, into an LSB-first stream.  A member whose coded form is not smaller than n + 5 is stored.
//                    The member goes to its slot of 65536 bytes in a staging buffer, its size to sizes[m].
//   k_bgzf_crc_put   one wave per member: the CRC-32 of the payload (crc_member of fx_inflate.hpp, the tables k_bgzf_crc uses),
//                    written in front of ISIZE.
//   k_bgzf_pack      after the scan of the sizes: slot m -> member_off[m] (bytes up to the destination's first 16-byte
//                    boundary, 16-byte stores fed by unaligned loads, the tail).
// Nothing in here depends on what memory held before: LDS tables and counters are cleared per member, token words are written
// for every position before they are read, and the slots are read only as far as sizes[m] says.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fx_kernels.hpp"
#include "fx_inflate.hpp"

namespace fx {

constexpr int DFL_MEMBER = 65280, DFL_SLOT = 65536, DFL_STORED = DFL_MEMBER + 31;     // payload of a member; its slot; a full stored member
constexpr int DFL_THREADS = 512, DFL_PER_LANE = 128;                                 // DFL_THREADS * DFL_PER_LANE >= DFL_MEMBER
constexpr int DFL_HASH_BITS = 13;
constexpr int DFL_MIN_MATCH = 4, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768;
constexpr uint32_t DFL_LIT = 0x10000u;                      // token: 0 under a match; DFL_LIT | byte; (length << 16) | (distance - 1)
static_assert(DFL_THREADS * DFL_PER_LANE >= DFL_MEMBER && DFL_MEMBER + 5 + 26 <= DFL_SLOT, "a member fits its lanes and its slot");

__host__ __device__ __forceinline__ void dfl_len_code(int len, int *code, int *nextra, int *extra) {   // length 3..258 -> code 0..28 (symbol 257 + code)
    const int l = len - 3;
    if (len == 258) { *code = 28; *nextra = 0; *extra = 0; return; }
    if (l < 8) { *code = l; *nextra = 0; *extra = 0; return; }
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    *code = 4 * e + 4 + ((l >> e) & 3); *nextra = e; *extra = l & ((1 << e) - 1);
}
__host__ __device__ __forceinline__ void dfl_dist_code(int dm1, int *code, int *nextra, int *extra) {   // distance - 1 in 0..32767 -> code 0..29
    if (dm1 < 4) { *code = dm1; *nextra = 0; *extra = 0; return; }
    const int lg = 31 - __builtin_clz((unsigned)dm1), e = lg - 1;
    *code = 2 * lg + ((dm1 >> e) & 1); *nextra = e; *extra = dm1 & ((1 << e) - 1);
}

// The BGZF header of a member of `total` bytes, by the first 18 lanes.
__device__ __forceinline__ void dfl_header(uint8_t *slot, int total, int t) {
    if (t >= 18) return;
    const uint8_t fixed[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    slot[t] = t < 16 ? fixed[t] : (uint8_t)((total - 1) >> (8 * (t - 16)));
}
// A stored block (BFINAL, BTYPE 00, LEN, NLEN, the bytes) and ISIZE behind the CRC's place; the member is 31 + n bytes.
__device__ __forceinline__ void dfl_stored(uint8_t *slot, const uint8_t *__restrict__ src, int n, int t, int nt) {
    dfl_header(slot, n + 31, t);
    if (t < 5) slot[18 + t] = t == 0 ? 1 : (uint8_t)((t < 3 ? n : ~n) >> (8 * ((t - 1) & 1)));
    if (t < 4) slot[18 + 5 + n + 4 + t] = (uint8_t)(n >> (8 * t));
    uint8_t *o = slot + 23;
    for (int i = t; i < n; i += nt) o[i] = src[i];
}

__global__ __launch_bounds__(BLOCK) void k_bgzf_store(const uint8_t *__restrict__ src, int64_t n, int64_t nmem, uint8_t *__restrict__ dst,
                                                      int64_t *__restrict__ member_off) {
    for (int64_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        const int len = (int)min((int64_t)DFL_MEMBER, n - m * DFL_MEMBER);
        dfl_stored(dst + m * DFL_STORED, src + m * DFL_MEMBER, len, threadIdx.x, BLOCK);
        if (threadIdx.x == 0) {
            member_off[m] = m * DFL_STORED;
            if (m == nmem - 1) member_off[nmem] = m * DFL_STORED + len + 31;
        }
    }
}

// Bits ORed into 32-bit LDS words that the pass cleared: the first and last word of a lane's stretch are shared with its neighbours.
struct DflBits {
    uint32_t *w;
    uint32_t wi;
    uint64_t acc;
    int nb;
    __device__ __forceinline__ void init(uint32_t *words, uint32_t bit) { w = words; wi = bit >> 5; nb = (int)(bit & 31u); acc = 0; }
    __device__ __forceinline__ void put(uint32_t v, int n) {                         // n <= 28
        acc |= (uint64_t)v << nb;
        nb += n;
        if (nb >= 32) { atomicOr(&w[wi++], (uint32_t)acc); acc >>= 32; nb -= 32; }
    }
    __device__ __forceinline__ void flush() { if ((uint32_t)acc) atomicOr(&w[wi], (uint32_t)acc); }
};

// What the code construction works in (LDS).
struct DflHuffWork {
    uint32_t nodef[2 * 288];                                // count of every node: the leaves in rank order, then the merges
    uint16_t par[2 * 288];                                  // parent, then depth
    int cnt[33];                                            // leaves per code length (indexed at run time: LDS, not scratch memory)
    uint32_t next[17];                                      // next canonical code per length
};
// The symbols with a count, ascending by (count, symbol), into srt; -> how many.  Every lane of the workgroup calls it (nsym <= DFL_THREADS).
__device__ __forceinline__ int dfl_rank(const uint32_t *freq, int nsym, uint16_t *srt) {
    const int s = threadIdx.x;
    const uint32_t f = s < nsym ? freq[s] : 0u;
    if (f) {
        int r = 0;
        for (int j = 0; j < nsym; ++j) { const uint32_t g = freq[j]; r += g && (g < f || (g == f && j < s)); }
        srt[r] = (uint16_t)s;
    }
    return __syncthreads_count(f != 0);
}
// One lane: code lengths (at most `limit`) and canonical codes, bit-reversed, of the u ranked symbols; lens of the others 0.
__host__ __device__ inline void dfl_huff(const uint32_t *freq, int nsym, const uint16_t *srt, int u, int limit, uint8_t *lens, uint16_t *codes, DflHuffWork *W) {
    for (int s = 0; s < nsym; ++s) { lens[s] = 0; codes[s] = 0; }
    if (u == 0) return;
    if (u == 1) { lens[srt[0]] = 1; return; }               // (code 0)
    for (int i = 0; i < u; ++i) W->nodef[i] = freq[srt[i]];
    int leaf = 0, head = u;                                  // next unused leaf; next unused merge (merges u .. u + k - 1 exist)
    for (int k = 0; k < u - 1; ++k) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool take_leaf = leaf < u && (head >= u + k || W->nodef[leaf] <= W->nodef[head]);
            const int node = take_leaf ? leaf++ : head++;
            sum += W->nodef[node];
            W->par[node] = (uint16_t)(u + k);
        }
        W->nodef[u + k] = sum;
    }
    int *const cnt = W->cnt;
    for (int i = 0; i <= 32; ++i) cnt[i] = 0;
    W->par[2 * u - 2] = 0;                                  // the root's depth; a parent's index is above its children's
    for (int node = 2 * u - 3; node >= 0; --node) {
        const int d = W->par[W->par[node]] + 1;
        W->par[node] = (uint16_t)d;
        if (node < u) cnt[d < limit ? d : limit]++;
    }
    // Over-long leaves were cut to `limit`, which overfills the code.  One step: the deepest leaf above the last level goes
    // down one level and takes a leaf of the last level as its sibling; Kraft's sum, in units of 2^-limit, falls by one.
    // It began at 2^limit or above (cutting only adds) and ends at exactly 2^limit: a complete code.
    uint32_t total = 0;
    for (int i = 1; i <= limit; ++i) total += (uint32_t)cnt[i] << (limit - i);
    while (total > (1u << limit)) {
        cnt[limit]--;
        for (int i = limit - 1; i >= 1; --i)
            if (cnt[i]) { cnt[i]--; cnt[i + 1] += 2; break; }
        total--;
    }
    int at = 0;                                              // the rarest symbols take the longest codes
    for (int len = limit; len >= 1; --len)
        for (int c = 0; c < cnt[len]; ++c) lens[srt[at++]] = (uint8_t)len;
    uint32_t *const next = W->next;                          // (cnt holds the leaves per length; none of length 0)
    uint32_t code = 0;
    cnt[0] = 0;
    next[0] = 0;
    for (int len = 1; len <= 16; ++len) { code = (code + (uint32_t)cnt[len - 1]) << 1; next[len] = code; }
    for (int s = 0; s < nsym; ++s)
        if (lens[s]) codes[s] = (uint16_t)(__builtin_bitreverse32(next[lens[s]]++) >> (32 - lens[s]));
}

struct DflShared {
    uint32_t pay[DFL_SLOT / 4];                             // the payload; later the coded bits
    uint32_t tab8[1 << DFL_HASH_BITS], tab4[1 << DFL_HASH_BITS];
    uint32_t lfreq[288], dfreq[32], cfreq[32];
    uint16_t lcode[288], dcode[32], ccode[32];
    uint16_t lsrt[288], dsrt[32], csrt[32];
    uint16_t cost8[256];                                    // price of a literal, in eighths of a bit
    uint16_t wlen[DFL_THREADS], wdist[DFL_THREADS];         // the window's matches
    uint16_t rle[320];                                      // the code lengths as code-length symbols: symbol | extra << 8
    unsigned long long wch[DFL_THREADS / 64];               // the window's chosen matches, one bit per position
    uint32_t wsum[DFL_THREADS / 64];
    uint8_t llen[288], dlen[32], clen[32];
    DflHuffWork hw;
    int carry, hlit, hdist, hclen, nrle;
    uint32_t hdr_bits;
};

__device__ __forceinline__ uint32_t dfl_tok_bits(const DflShared &S, uint32_t tok) {
    if (!tok) return 0;
    const int len = (int)(tok >> 16);
    if (len == 1) return S.llen[tok & 255u];
    int lc, le, lx, dc, de, dx;
    dfl_len_code(len, &lc, &le, &lx);
    dfl_dist_code((int)(tok & 0xFFFFu), &dc, &de, &dx);
    return (uint32_t)(S.llen[257 + lc] + le + S.dlen[dc] + de);
}

// A candidate q < p for position p: the bytes it shares with p (at most max_len), what they would cost as literals -> the gain in
// eighths of a bit over a match of that length and distance (<= 0: not worth it), *len.
__device__ __forceinline__ int dfl_try(const uint8_t *pay, const uint16_t *cost8, int p, int q, int max_len, int *len) {
    int L = 0, lit = 0;
    while (L < max_len && pay[q + L] == pay[p + L]) { lit += cost8[pay[p + L]]; ++L; }
    *len = L;
    if (L < DFL_MIN_MATCH) return 0;
    int lc, le, lx, dc, de, dx;
    dfl_len_code(L, &lc, &le, &lx);
    dfl_dist_code(p - q - 1, &dc, &de, &dx);
    return lit - 8 * (7 + le + 5 + de);
}

__global__ __launch_bounds__(DFL_THREADS) void k_bgzf_deflate(const uint8_t *__restrict__ src, int64_t n_bytes, int64_t nmem, int level,
                                                              uint32_t *__restrict__ tok_all, uint8_t *__restrict__ stage,
                                                              int64_t *__restrict__ sizes) {
    __shared__ DflShared S;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint8_t *const pay = reinterpret_cast<uint8_t *>(S.pay);
    uint32_t *const tok = tok_all + (size_t)blockIdx.x * DFL_SLOT;
    for (int64_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        const int n = (int)min((int64_t)DFL_MEMBER, n_bytes - m * DFL_MEMBER);
        const uint8_t *const in = src + m * DFL_MEMBER;
        uint8_t *const slot = stage + m * DFL_SLOT;
        __syncthreads();                                     // (the member before is out of LDS)
        // ---- the payload, the tables and the counters
        if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
            for (int i = t; i < n / 16; i += DFL_THREADS) reinterpret_cast<uint4 *>(S.pay)[i] = reinterpret_cast<const uint4 *>(in)[i];
            for (int i = (n / 16) * 16 + t; i < n; i += DFL_THREADS) pay[i] = in[i];
        } else {
            for (int i = t; i < n; i += DFL_THREADS) pay[i] = in[i];
        }
        for (int i = t; i < (1 << DFL_HASH_BITS); i += DFL_THREADS) { S.tab8[i] = 0; S.tab4[i] = 0; }
        if (t < 288) S.lfreq[t] = 0;
        if (t < 32) { S.dfreq[t] = 0; S.cfreq[t] = 0; }
        if (t == 0) S.carry = 0;
        __syncthreads();
        for (int i = t; i < n; i += DFL_THREADS) atomicAdd(&S.lfreq[pay[i]], 1u);
        __syncthreads();
        if (level >= 2) {
            if (t < 256) {
                const uint32_t f = S.lfreq[t];
                const int c = f ? (int)(8.0f * __log2f((float)n / (float)f) + 0.5f) : 0;
                S.cost8[t] = (uint16_t)(c < 8 ? 8 : c);
            }
            __syncthreads();
            if (t < 256) S.lfreq[t] = 0;
            // ---- the parse, one window of DFL_THREADS positions at a time
            for (int w0 = 0; w0 < n; w0 += DFL_THREADS) {
                const int p = w0 + t;
                const int carry_in = S.carry;
                const bool h8 = p + 8 <= n, h4 = p + 4 <= n;
                uint32_t k8 = 0, k4 = 0;
                int best = 0, best_len = 0, best_q = 0;
                if (h4) {
                    const uint32_t a = (uint32_t)pay[p] | ((uint32_t)pay[p + 1] << 8) | ((uint32_t)pay[p + 2] << 16) | ((uint32_t)pay[p + 3] << 24);
                    k4 = (a * 2654435761u) >> (32 - DFL_HASH_BITS);
                    if (h8) {
                        const uint32_t b = (uint32_t)pay[p + 4] | ((uint32_t)pay[p + 5] << 8) | ((uint32_t)pay[p + 6] << 16) | ((uint32_t)pay[p + 7] << 24);
                        k8 = ((a * 2654435761u) ^ (b * 2246822519u)) * 3266489917u >> (32 - DFL_HASH_BITS);
                    }
                    const int max_len = min(DFL_MAX_MATCH, n - p);
                    const int cand[3] = {h8 ? (int)S.tab8[k8] - 1 : -1, (int)S.tab4[k4] - 1, p - 1};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int q = cand[c];
                        if (q < 0 || p - q > DFL_MAX_DIST || best > 0) continue;      // (the first candidate that pays is taken)
                        int L;
                        const int g = dfl_try(pay, S.cost8, p, q, max_len, &L);
                        if (g > 0) { best = g; best_len = L; best_q = q; }
                    }
                }
                S.wlen[t] = (uint16_t)(best > 0 ? best_len : 0);
                S.wdist[t] = (uint16_t)(best > 0 ? p - best_q - 1 : 0);
                __syncthreads();
                if (h8) atomicMax(&S.tab8[k8], (uint32_t)p + 1u);
                if (h4) atomicMax(&S.tab4[k4], (uint32_t)p + 1u);
                if (wave == 0) {                             // greedy, from the first free position
                    int pos = carry_in;
                    for (int sb = 0; sb < DFL_THREADS / 64; ++sb) {
                        const int base = w0 + sb * 64;
                        const unsigned long long mask = __ballot(S.wlen[sb * 64 + lane] != 0);
                        unsigned long long chosen = 0;
                        for (;;) {
                            const int off = pos > base ? pos - base : 0;
                            if (off >= 64) break;
                            const unsigned long long mm = mask & (~0ull << off);
                            if (!mm) break;
                            const int q = __ffsll((long long)mm) - 1;
                            chosen |= 1ull << q;
                            pos = base + q + S.wlen[sb * 64 + q];
                        }
                        if (lane == 0) S.wch[sb] = chosen;
                    }
                    if (lane == 0) S.carry = pos;
                }
                __syncthreads();
                if (p < n) {
                    uint32_t tk = DFL_LIT | pay[p];
                    if (p < carry_in) tk = 0;
                    else {
                        int qi = -1;                         // the last chosen match at or before this position
                        unsigned long long mm = S.wch[wave] & (~0ull >> (63 - lane));
                        for (int sb = wave; ; ) {
                            if (mm) { qi = sb * 64 + 63 - __clzll((long long)mm); break; }
                            if (--sb < 0) break;
                            mm = S.wch[sb];
                        }
                        if (qi == t) tk = ((uint32_t)S.wlen[t] << 16) | S.wdist[t];
                        else if (qi >= 0 && qi + S.wlen[qi] > t) tk = 0;
                    }
                    tok[p] = tk;
                    if (tk) {
                        const int len = (int)(tk >> 16);
                        if (len == 1) atomicAdd(&S.lfreq[tk & 255u], 1u);
                        else {
                            int lc, le, lx, dc, de, dx;
                            dfl_len_code(len, &lc, &le, &lx);
                            dfl_dist_code((int)(tk & 0xFFFFu), &dc, &de, &dx);
                            atomicAdd(&S.lfreq[257 + lc], 1u);
                            atomicAdd(&S.dfreq[dc], 1u);
                        }
                    }
                }
                __syncthreads();
            }
        } else {
            for (int i = t; i < n; i += DFL_THREADS) tok[i] = DFL_LIT | pay[i];
        }
        if (t == 0) S.lfreq[256] = 1;                        // the end of the block
        __syncthreads();
        // ---- the codes
        const int ul = dfl_rank(S.lfreq, 286, S.lsrt);
        const int ud = dfl_rank(S.dfreq, 30, S.dsrt);
        if (t == 0) {
            dfl_huff(S.lfreq, 286, S.lsrt, ul, 15, S.llen, S.lcode, &S.hw);
            dfl_huff(S.dfreq, 30, S.dsrt, ud, 15, S.dlen, S.dcode, &S.hw);
            if (ud == 0) S.dlen[0] = 1;                      // HDIST sends one code at least: a single code of length 1
            int hlit = 286, hdist = 30;
            while (hlit > 257 && S.llen[hlit - 1] == 0) --hlit;
            while (hdist > 1 && S.dlen[hdist - 1] == 0) --hdist;
            // the hlit + hdist lengths as symbols of the code-length code: 16 repeats the last length 3..6 times, 17 and 18 are 3..10 and 11..138 zeros
            const int tot = hlit + hdist;
            int nr = 0;
            auto cl = [&](int i) { return (int)(i < hlit ? S.llen[i] : S.dlen[i - hlit]); };
            auto emit = [&](int sym, int extra) { S.rle[nr++] = (uint16_t)(sym | (extra << 8)); S.cfreq[sym]++; };
            for (int i = 0; i < tot;) {
                const int v = cl(i);
                int run = 1;
                while (i + run < tot && cl(i + run) == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) { const int r = run < 138 ? run : 138; emit(18, r - 11); run -= r; }
                    if (run >= 3) { emit(17, run - 3); run = 0; }
                } else {
                    emit(v, 0); --run;
                    while (run >= 3) { const int r = run < 6 ? run : 6; emit(16, r - 3); run -= r; }
                }
                for (; run > 0; --run) emit(v, 0);
            }
            S.hlit = hlit; S.hdist = hdist; S.nrle = nr;
        }
        __syncthreads();
        const int uc = dfl_rank(S.cfreq, 19, S.csrt);
        if (t == 0) {
            dfl_huff(S.cfreq, 19, S.csrt, uc, 7, S.clen, S.ccode, &S.hw);
            if (uc == 1) {                                   // the code-length code has to be complete: a second code of length 1 (code 1) that nothing uses
                const int other = S.csrt[0] == 0 ? 1 : 0;
                S.clen[other] = 1;
                S.ccode[other] = S.csrt[0] < other ? 1 : 0;
                S.ccode[S.csrt[0]] = S.csrt[0] < other ? 0 : 1;
            }
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            int hclen = 19;
            while (hclen > 4 && S.clen[order[hclen - 1]] == 0) --hclen;
            uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
            for (int i = 0; i < S.nrle; ++i) {
                const int sym = S.rle[i] & 31;
                bits += S.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
            }
            S.hclen = hclen;
            S.hdr_bits = bits;
        }
        __syncthreads();
        // ---- the bits of every lane's DFL_PER_LANE positions, their offsets
        const int p0 = t * DFL_PER_LANE, p1 = min(n, p0 + DFL_PER_LANE);
        uint32_t mine = 0;
        for (int p = p0; p < p1; p += 4) {                   // (the scratch is read in 16-byte pieces; words past n are not looked at)
            const uint4 v = *reinterpret_cast<const uint4 *>(tok + p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) if (p + k < p1) mine += dfl_tok_bits(S, w[k]);
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += o; }
        if (lane == 63) S.wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < DFL_THREADS / 64; ++k) { const uint32_t s = S.wsum[k]; if (k < wave) before += s; all += s; }
        const uint32_t start = S.hdr_bits + before + incl - mine;
        const uint32_t end_bits = S.hdr_bits + all + S.llen[256];
        const int csize = (int)((end_bits + 7) >> 3);
        const bool coded = csize < n + 5;                    // else a stored block is no larger
        __syncthreads();                                     // (every lane has read what it needs of the payload)
        if (!coded) {
            dfl_stored(slot, in, n, t, DFL_THREADS);
            if (t == 0) sizes[m] = n + 31;
            continue;
        }
        for (int i = t; i < (csize + 3) / 4 + 1; i += DFL_THREADS) S.pay[i] = 0;
        __syncthreads();
        DflBits B;
        if (t == 0) {                                        // the block's header
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            B.init(S.pay, 0);
            B.put(1, 1); B.put(2, 2);                        // BFINAL, BTYPE 10
            B.put((uint32_t)S.hlit - 257, 5); B.put((uint32_t)S.hdist - 1, 5); B.put((uint32_t)S.hclen - 4, 4);
            for (int i = 0; i < S.hclen; ++i) B.put(S.clen[order[i]], 3);
            for (int i = 0; i < S.nrle; ++i) {
                const int sym = S.rle[i] & 31, extra = S.rle[i] >> 8;
                B.put(S.ccode[sym], S.clen[sym]);
                if (sym >= 16) B.put((uint32_t)extra, sym == 16 ? 2 : sym == 17 ? 3 : 7);
            }
            B.flush();
            B.init(S.pay, S.hdr_bits + all);                 // the end of the block
            B.put(S.lcode[256], S.llen[256]);
            B.flush();
        }
        B.init(S.pay, start);
        for (int p = p0; p < p1; p += 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(tok + p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t tk = w[k];
                if (p + k >= p1 || !tk) continue;
                const int len = (int)(tk >> 16);
                if (len == 1) { B.put(S.lcode[tk & 255u], S.llen[tk & 255u]); continue; }
                int lc, le, lx, dc, de, dx;
                dfl_len_code(len, &lc, &le, &lx);
                dfl_dist_code((int)(tk & 0xFFFFu), &dc, &de, &dx);
                B.put((uint32_t)S.lcode[257 + lc] | ((uint32_t)lx << S.llen[257 + lc]), S.llen[257 + lc] + le);
                B.put((uint32_t)S.dcode[dc] | ((uint32_t)dx << S.dlen[dc]), S.dlen[dc] + de);
            }
        }
        B.flush();
        __syncthreads();
        // ---- the member into its slot
        dfl_header(slot, csize + 26, t);
        for (int i = t; i < csize; i += DFL_THREADS) slot[18 + i] = pay[i];
        if (t < 4) slot[18 + csize + 4 + t] = (uint8_t)(n >> (8 * t));
        if (t == 0) sizes[m] = csize + 26;
    }
}

// One wave per member: the CRC-32 of its payload into the four bytes in front of ISIZE.  Member m lies at out + m * stride and is
// sizes[m] bytes long (sizes == nullptr: stored members of a packed level-0 stream, 31 + payload).
__global__ __launch_bounds__(256) void k_bgzf_crc_put(const uint8_t *__restrict__ src, int64_t n_bytes, int64_t nmem, const CrcTables *__restrict__ T,
                                                     uint8_t *__restrict__ out, int64_t stride, const int64_t *__restrict__ sizes) {
    __shared__ uint32_t tab[4][256], sh[CRC_NSH][4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += 256) (&tab[0][0])[i] = (&T->crc[0][0])[i];
    for (int i = threadIdx.x; i < CRC_NSH * 4 * 256; i += 256) (&sh[0][0][0])[i] = (&T->sh[0][0][0])[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t m = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (m >= nmem) return;
    const int64_t n = min((int64_t)DFL_MEMBER, n_bytes - m * DFL_MEMBER);
    const uint32_t crc = crc_member(src + m * DFL_MEMBER, n, tab, sh, T, lane);
    uint8_t *const o = out + m * stride + (sizes ? sizes[m] : n + 31) - 8;
    if (lane < 4) o[lane] = (uint8_t)(crc >> (8 * lane));
}

// Slot m of the staging buffer -> the packed stream at off[m]; one workgroup per member.
__global__ __launch_bounds__(BLOCK) void k_bgzf_pack(const uint8_t *__restrict__ stage, const int64_t *__restrict__ off, int64_t nmem, uint8_t *__restrict__ dst) {
    for (int64_t m = blockIdx.x; m < nmem; m += gridDim.x) {
        const uint8_t *s = stage + m * DFL_SLOT;
        uint8_t *d = dst + off[m];
        const int len = (int)(off[m + 1] - off[m]);
        const int head = min(len, (int)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
        if ((int)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        const int body = (len - head) / 16;
        for (int i = threadIdx.x; i < body; i += BLOCK) *reinterpret_cast<uint4 *>(d + head + 16 * i) = *reinterpret_cast<const uint4_u *>(s + head + 16 * i);
        const int done = head + 16 * body;
        if ((int)threadIdx.x < len - done) d[done + threadIdx.x] = s[done + threadIdx.x];
    }
}

struct DflLdSize {                                          // the scan's loader: bytes of member i
    const int64_t *p;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = p[i]; }
};

}  // namespace fx
