// fx_fasta_format.hpp -- FASTA records written back out from the resident stream for gfx950 (MI355X, wave64): whole
// records or intervals, re-wrapped at a line width, upper-cased, masked, complemented and reversed on the way.
// Extension: the reference writes records only as verbatim copies (Sequence.raw, sequence.c:314-335) and slices one
// interval per call (sequence.c:76-125); the definition is the one of fx_fasta_format_alloc in include/fxgpu.h.
//
//   k_fa_format_mask   one lane per mask row: the record id and the interval against the table, the row against the one
//        before it (sorted by record and start, each beginning at or after the end of the one before); the first offender
//        -> atomicMin.
//   k_fa_format_size   one lane per query.  The id and the interval are checked as k_q_counts_fasta checks them (first
//        offender -> atomicMin); the record's row gives the DESCRIPTOR the emit pass works from: where base 0 of the record
//        lies, the bases per line and the terminator length (sequence.c:498-510), the header's bytes (the record's own:
//        dlen bytes behind '>' without one trailing '\r'; or the caller's), the record's range of mask rows (two binary
//        searches in the id column), the flags, L.  A query the line arithmetic cannot answer exactly -- a record that is
//        not line-regular, fewer than 16 bases per line, a divisor or a coordinate past 32 bits, the edge of the stream, a
//        query an earlier emit pass found white space in -- is marked FLAT and put on a list: its forward letters are
//        despaced into a scratch block by the fetch kernels (flags 0), and k_fa_format_fix takes L from their out_len and
//        points the descriptor at that block as ONE line of L letters.
//   k_fa_format_emit   divided by OUTPUT bytes: a workgroup owns FAF_TILE bytes of the finished buffer, a lane owns four
//        16-byte aligned chunks of it, 4 KiB apart, so that a wave's stores cover 1 KiB at a time.  Two lanes find the
//        tile's first and last query by binary search in dst_off, every lane its chunk's query between the two.  A chunk
//        may hold the end of one record and several whole short ones: the lane walks the output bytes, and a byte is '>',
//        a header byte, a newline ((j - |H| - 2) % (width + 1) == width, or the record's last byte) or letter i of S.  One
//        division places the first byte of a record in the chunk, the rest is counted on: the output column, the letter,
//        its source line and its place in that line (one 32-bit division, guarded by the size pass).  Letter i is read at
//        base + p + elen * (p / bpl), p = start + i -- or, on the reverse strand, start + L - 1 - i --, upper-cased, masked
//        (the row that holds p, or the gap around it, is looked up by binary search and kept until p leaves it),
//        complemented through the LUT (build_comp_lut's table, made once per call by k_fa_format_lut).  A chunk that lies
//        inside the letters of one record that goes by the line arithmetic, with at most one newline in it (lines of 16
//        letters or more), is not walked: its 15 or 16 letters are one ascending run of the source with at most one line
//        end inside, read by two unaligned 16-byte loads merged under a byte mask (as k_fetch_lines reads them),
//        transformed four bytes at a time, byte-swapped on the reverse strand, and the newline is shifted in; a mask row
//        that begins or ends inside the run, FLAT queries and the last 16 + elen bytes of the stream take the walk.  On
//        either way the lane checks what k_fetch_lines checks: a letter that is white space (the walk: one of 10
//        / 13 / 32; the run: any byte up to 32), or a terminator byte between two letters of the query that is none,
//        marks the query dirty -- the host then runs the call again with that query FLAT (for a genome: never).  The 16
//        bytes leave as one aligned store; only the last chunk of the buffer is written byte by byte.  No atomics, nothing
//        sorted.
#pragma once
#include "fx_search.hpp"

namespace fx {

constexpr int FAF_CHUNKS = 4;                               // 16-byte chunks per lane
constexpr int FAF_TILE = BLOCK * 16 * FAF_CHUNKS;           // output bytes per workgroup
constexpr int FAF_FLAT = 0x100;                             // descriptor flag: the letters lie despaced in the scratch block
constexpr int FAF_OWN_HDR = 0x200;                          // descriptor flag: the header is read from the stream
constexpr int FAF_MASK_SOFT = 1, FAF_MASK_HARD = 2, FAF_MASK_UPPER = 3;

struct FaFmtDesc {
    int64_t src;                     // stream offset of base 0 of the record; FLAT: offset of the query's first letter in the scratch block
    int64_t hsrc;                    // the header's first byte: stream offset, or offset in the caller's header bytes
    int64_t a;                       // forward coordinate of the query's first letter
    int64_t m0, m1;                  // the record's mask rows
    int32_t L, hl, bpl, el, flags, pad;
};
static_assert(sizeof(FaFmtDesc) == 64, "one descriptor per 64-byte line");

struct FaFmtTab {
    const int64_t *hoff, *boff, *slen, *llen;
    const int32_t *elen, *reg, *dlen;
    int64_t n_seq;
};
struct FaFmtQ {
    const int64_t *id, *start, *stop;            // id null: records 0..n-1; start null: whole records
    const uint8_t *qflags, *force;               // per-query flags or null; force[k] != 0: FLAT whatever the row says
    const int64_t *hdr_off;                      // null: the record's own header
    const int64_t *mask_id;                      // null: no mask
    int64_t n_mask;
};

// bytes of a record: '>' H '\n', then L letters in lines of W (0: one line), each line ended by '\n'
__device__ __forceinline__ int64_t faf_size(int64_t hl, int64_t L, int64_t width, int64_t min_len) {
    if (L < min_len) return 0;
    const int64_t lines = L == 0 ? 0 : (width == 0 ? 1 : (L + width - 1) / width);
    return hl + 2 + L + lines;
}

struct FafLdSize {                            // bytes of the record, "the record is there", its letters
    const int64_t *cnt;
    const FaFmtDesc *desc;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = cnt[i]; v[1] = cnt[i] > 0; v[2] = cnt[i] > 0 ? desc[i].L : 0; }
};
struct FafLdFlat {                            // letters a FLAT query asks the fetch kernels for
    const int64_t *a, *b;
    __device__ void operator()(int64_t i, int64_t *v) const { v[0] = b[i] - a[i]; }
};

__global__ __launch_bounds__(BLOCK) void k_fa_format_mask(const int64_t *__restrict__ mid, const int64_t *__restrict__ ms,
                                                         const int64_t *__restrict__ me, int64_t n_mask, const int64_t *__restrict__ slen,
                                                         int64_t n_seq, unsigned long long *__restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_mask) return;
    const int64_t id = mid[r], s = ms[r], e = me[r];
    bool ok = id >= 0 && id < n_seq && s >= 0 && s <= e;
    if (ok) ok = e <= slen[id];
    if (ok && r > 0) {
        const int64_t pid = mid[r - 1];
        ok = pid < id || (pid == id && ms[r - 1] <= s && me[r - 1] <= s);
    }
    if (!ok) atomicMin(bad, (unsigned long long)r);
}

__global__ __launch_bounds__(BLOCK) void k_fa_format_size(const uint8_t *__restrict__ data, int64_t n_bytes, FaFmtTab tab, FaFmtQ q, int64_t nq,
                                                         int flags_all, int64_t width, int64_t min_len, FaFmtDesc *__restrict__ desc,
                                                         int64_t *__restrict__ cnt, unsigned long long *__restrict__ bad,
                                                         int64_t *__restrict__ flat_q, int64_t *__restrict__ flat_id, int64_t *__restrict__ flat_a,
                                                         int64_t *__restrict__ flat_b, int *__restrict__ n_flat) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= nq) return;
    FaFmtDesc D;
    D.src = D.hsrc = D.a = D.m0 = D.m1 = 0;
    D.L = D.hl = D.el = D.flags = 0; D.bpl = 1;
    D.pad = 0;
    const int64_t id = q.id ? q.id[k] : k;
    bool ok = id >= 0 && id < tab.n_seq;
    int64_t a = 0, b = 0;
    if (ok) {
        const int64_t sl = tab.slen[id] > 0 ? tab.slen[id] : 0;
        a = q.start ? q.start[k] : 0;
        b = q.stop ? q.stop[k] : sl;
        ok = a >= 0 && b >= a && b - a <= 0x7FFFFFFFll && b <= sl;
    }
    if (!ok) { atomicMin(bad, (unsigned long long)k); desc[k] = D; cnt[k] = 0; return; }
    const int fl = (q.qflags ? (int)q.qflags[k] : flags_all) & 7;
    const int64_t boff = tab.boff[id], llen = tab.llen[id], el = tab.elen[id], take = b - a;
    const int64_t bpl = llen - el;
    // ---- the header
    int64_t hs, hl;
    int own = 0;
    if (q.hdr_off) { hs = q.hdr_off[k]; hl = q.hdr_off[k + 1] - hs; }
    else {
        own = FAF_OWN_HDR;
        hs = tab.hoff[id] + 1;
        hl = tab.dlen[id] > 0 ? tab.dlen[id] : 0;
        if (hs < 0 || hs > n_bytes) { hs = 0; hl = 0; }
        if (hs + hl > n_bytes) hl = n_bytes - hs;
        if (hl > 0 && data[hs + hl - 1] == 13) --hl;          // one trailing '\r' is not part of it
    }
    // ---- the letters: by the line arithmetic where it is exact (what k_fetch_lines asks for), else FLAT
    bool lines = take == 0;
    if (!lines && tab.reg[id] != 0 && bpl >= 16 && bpl < (1ll << 31) && b < (1ll << 31) && (el == 1 || el == 2) && !(q.force && q.force[k])) {
        const uint32_t bpl32 = (uint32_t)bpl;
        const int64_t first = boff + a + el * (int64_t)((uint32_t)a / bpl32);
        const int64_t last = boff + (b - 1) + el * (int64_t)((uint32_t)(b - 1) / bpl32);
        lines = first >= 0 && last < n_bytes;
    }
    D.hsrc = hs; D.hl = (int32_t)hl; D.a = a; D.L = (int32_t)take;
    if (q.mask_id) {                                           // the rows of this record: [lower bound, upper bound) of its id
        int64_t lo = 0, hi = q.n_mask;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (q.mask_id[mid] < id) lo = mid + 1; else hi = mid; }
        D.m0 = lo;
        hi = q.n_mask;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (q.mask_id[mid] <= id) lo = mid + 1; else hi = mid; }
        D.m1 = lo;
    }
    if (lines) {
        D.src = boff; D.bpl = take ? (int32_t)bpl : 1; D.el = (int32_t)el; D.flags = fl | own;
    } else {
        D.src = 0; D.bpl = 0x7FFFFFFF; D.el = 0; D.flags = fl | own | FAF_FLAT;
        const int s = atomicAdd(n_flat, 1);
        flat_q[s] = k; flat_id[s] = id; flat_a[s] = a; flat_b[s] = b;
    }
    desc[k] = D;
    cnt[k] = faf_size(hl, take, width, min_len);
}

// the FLAT queries after their fetch: where their letters lie, how many came (an irregular record can hold fewer than
// stop - start), the size that follows
__global__ __launch_bounds__(BLOCK) void k_fa_format_fix(const int64_t *__restrict__ flat_q, const int64_t *__restrict__ flat_off,
                                                        const int64_t *__restrict__ out_len, int64_t n_flat, int64_t width, int64_t min_len,
                                                        FaFmtDesc *__restrict__ desc, int64_t *__restrict__ cnt) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_flat) return;
    const int64_t k = flat_q[s];
    const int64_t L = out_len[s] > 0 ? out_len[s] : 0;
    desc[k].src = flat_off[s];
    desc[k].L = (int32_t)L;
    cnt[k] = faf_size(desc[k].hl, L, width, min_len);
}

// ---- 16 output bytes at once (the emit pass where a chunk lies inside the letters of one line-arithmetic record)
// 'A'..'Z' -> 'a'..'z' on four bytes, everything else unchanged (upper4's mirror)
__device__ __forceinline__ uint32_t lower4(uint32_t w) {
    const uint32_t x = w & 0x7F7F7F7Fu;
    const uint32_t upper = (x + 0x3F3F3F3Fu) & ~(x + 0x25252525u) & ~w & 0x80808080u;     // 0x41 <= c <= 0x5A
    return w + (upper >> 2);
}
struct B16 { uint64_t lo, hi; };                          // 16 bytes, byte 0 lowest
__device__ __forceinline__ B16 b16_low(int T) {           // the low T bytes (0..16) set
    B16 m;
    m.lo = T >= 8 ? ~0ull : ((1ull << (8 * T)) - 1ull);
    m.hi = T <= 8 ? 0ull : (T >= 16 ? ~0ull : ((1ull << (8 * (T - 8))) - 1ull));
    return m;
}
__device__ __forceinline__ B16 b16_shr(B16 x, int s) {    // down by s bytes (0..15)
    if (s >= 8) { x.lo = x.hi >> (8 * (s - 8)); x.hi = 0; }
    else if (s > 0) { x.lo = (x.lo >> (8 * s)) | (x.hi << (64 - 8 * s)); x.hi >>= 8 * s; }
    return x;
}
template <class F> __device__ __forceinline__ B16 b16_words(B16 x, F f) {    // f on each of the four 32-bit words
    x.lo = (uint64_t)f((uint32_t)x.lo) | ((uint64_t)f((uint32_t)(x.lo >> 32)) << 32);
    x.hi = (uint64_t)f((uint32_t)x.hi) | ((uint64_t)f((uint32_t)(x.hi >> 32)) << 32);
    return x;
}
__device__ __forceinline__ B16 b16_load(const uint8_t *p) {
    const uint4 v = *reinterpret_cast<const uint4_u *>(p);
    return {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
}

// the complement table of the fetch kernels, once per call, for the emit pass to copy into LDS (one workgroup)
__global__ __launch_bounds__(BLOCK) void k_fa_format_lut(uint8_t *__restrict__ comp) {
    __shared__ uint8_t lut[256];
    build_comp_lut(lut);
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += BLOCK) comp[i] = lut[i];
}

__global__ __launch_bounds__(BLOCK) void k_fa_format_emit(const uint8_t *__restrict__ data, int64_t n_bytes, const uint8_t *__restrict__ flat,
                                                         const uint8_t *__restrict__ hdr, const FaFmtDesc *__restrict__ desc,
                                                         const int64_t *__restrict__ off, int64_t nq, int64_t total, int64_t width,
                                                         const int64_t *__restrict__ mstart, const int64_t *__restrict__ mstop, int mask_mode,
                                                         int mask_byte, const uint8_t *__restrict__ comp, uint8_t *__restrict__ out, uint8_t *__restrict__ dirty,
                                                         int *__restrict__ any_dirty) {
    __shared__ uint8_t lut[256];
    __shared__ int64_t s_q[2];
    static_assert(BLOCK == 256, "one LUT entry per lane");
    lut[threadIdx.x] = comp[threadIdx.x];
    const int64_t tile0 = (int64_t)blockIdx.x * FAF_TILE;
    // the last query that begins at or before output byte o (one that holds bytes: the empty ones before it share its offset)
    auto query_at = [&](int64_t o, int64_t lo, int64_t hi) {
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= o) lo = mid; else hi = mid; }
        return lo;
    };
    if (threadIdx.x < 2) {
        const int64_t end = tile0 + FAF_TILE < total ? tile0 + FAF_TILE : total;
        s_q[threadIdx.x] = query_at(threadIdx.x == 0 ? tile0 : end - 1, 0, nq);
    }
    __syncthreads();
    const int64_t q_lo = s_q[0], q_hi = s_q[1];
#pragma unroll 1
    for (int c = 0; c < FAF_CHUNKS; ++c) {
        const int64_t o0 = tile0 + ((int64_t)c * BLOCK + threadIdx.x) * 16;
        if (o0 >= total) break;
        const int nb = total - o0 < 16 ? (int)(total - o0) : 16;
        int64_t k = query_at(o0, q_lo, q_hi + 1);
        uint64_t w_lo = 0, w_hi = 0;
        // ---- the record the lane is in
        int64_t rec0 = off[k], size = off[k + 1] - rec0, j = o0 - rec0;
        FaFmtDesc D = desc[k];
        // ---- the chunk lies inside the letters of one record that goes by the line arithmetic, with at most one newline in it
        // (lines of 16 letters or more, not the record's last byte): its 15 or 16 letters are one ascending run of the source with
        // at most one line end inside (bpl >= 16) -- two unaligned 16-byte loads merged by a byte mask, as k_fetch_lines reads
        // them --, the transforms go over four bytes at a time, the minus strand is a byte swap, the newline is shifted in.
        // Whatever does not fit (a mask row that begins or ends inside, the edge of the stream) takes the byte walk below.
        if (nb == 16 && !(D.flags & FAF_FLAT) && j >= (int64_t)D.hl + 2 && j + 16 < size) {
            const int64_t L = D.L;
            const uint32_t Wf = (uint32_t)(width == 0 || width > L ? L : width);
            if (Wf >= 16) {
                const uint64_t jj = (uint64_t)(j - D.hl - 2), w1 = (uint64_t)Wf + 1;
                const uint64_t line = jj < (1ull << 32) ? (uint64_t)((uint32_t)jj / (uint32_t)w1) : jj / w1;
                const uint32_t colf = (uint32_t)(jj - line * w1);
                const int tn = Wf - colf < 16u ? (int)(Wf - colf) : 16;     // where the newline falls in the chunk (16: nowhere)
                const int nl = tn < 16 ? 15 : 16;                           // letters in the chunk
                const int64_t i0 = (int64_t)(line * Wf) + colf;             // the first of them
                const bool rev = (D.flags & 2) != 0;
                const int64_t ps = rev ? D.a + L - i0 - nl : D.a + i0;      // the run's first forward coordinate
                const uint32_t bplf = (uint32_t)D.bpl, x0 = (uint32_t)ps, ks = x0 / bplf, rs = x0 - ks * bplf;
                const int64_t as = D.src + ps + (int64_t)D.el * ks;
                const int s1 = bplf - rs < (uint32_t)nl ? (int)(bplf - rs) : nl;      // letters in front of the line end
                bool ok = as + D.el + 16 <= n_bytes;
                bool in = false;
                if (ok && mask_mode && D.m1 > D.m0) {                       // one answer for the whole run, or the byte walk
                    int64_t lo = D.m0, hi = D.m1;
                    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (mstop[mid] <= ps) lo = mid + 1; else hi = mid; }
                    if (lo < D.m1 && mstart[lo] <= ps) { in = true; ok = ps + nl <= mstop[lo]; }
                    else ok = lo >= D.m1 || ps + nl <= mstart[lo];
                }
                if (ok) {
                    B16 x = b16_load(data + as);
                    bool bad = false;
                    if (s1 < nl) {
                        const B16 y = b16_load(data + as + D.el), m = b16_low(s1);
                        x.lo = (x.lo & m.lo) | (y.lo & ~m.lo); x.hi = (x.hi & m.hi) | (y.hi & ~m.hi);
                        bad = !is_space3(data[as + s1]) || (D.el == 2 && !is_space3(data[as + s1 + 1]));
                    } else if (rs + (uint32_t)nl == bplf && ps + nl < D.a + L)          // the run ends with its line, letters follow
                        bad = !is_space3(data[as + nl]) || (D.el == 2 && !is_space3(data[as + nl + 1]));
                    if (rs == 0 && ps > D.a)                                           // the run begins a line, letters precede it
                        bad |= !is_space3(data[as - 1]) || (D.el == 2 && !is_space3(data[as - 2]));
                    {
                        const B16 m = b16_low(nl), f = b16_words(x, le20_bytes);
                        bad |= ((f.lo & m.lo) | (f.hi & m.hi)) != 0;
                    }
                    if (bad) { dirty[k] = 1; *any_dirty = 1; }
                    if (D.flags & 1) x = b16_words(x, upper4);
                    if (in) {
                        if (mask_mode == FAF_MASK_HARD) { x.lo = 0x0101010101010101ull * (uint64_t)(uint32_t)mask_byte; x.hi = x.lo; }
                        else if (mask_mode == FAF_MASK_SOFT) x = b16_words(x, lower4);
                        else x = b16_words(x, upper4);
                    }
                    if (D.flags & 4) x = b16_words(x, [&](uint32_t w) { return lut4(lut, w); });
                    if (rev) {
                        const B16 r = {__builtin_bswap64(x.hi), __builtin_bswap64(x.lo)};
                        x = b16_shr(r, 16 - nl);
                    }
                    if (tn < 16) {                                                     // the newline at byte tn, the letters behind it one up
                        const B16 below = b16_low(tn), upto = b16_low(tn + 1);
                        const B16 up = {x.lo << 8, (x.hi << 8) | (x.lo >> 56)};
                        x.lo = (x.lo & below.lo) | (up.lo & ~upto.lo) | (upto.lo & ~below.lo & 0x0A0A0A0A0A0A0A0Aull);
                        x.hi = (x.hi & below.hi) | (up.hi & ~upto.hi) | (upto.hi & ~below.hi & 0x0A0A0A0A0A0A0A0Aull);
                    }
                    *reinterpret_cast<uint4 *>(out + o0) = make_uint4((uint32_t)x.lo, (uint32_t)(x.lo >> 32), (uint32_t)x.hi, (uint32_t)(x.hi >> 32));
                    continue;
                }
            }
        }
        bool fresh = true;                                     // the letter state below is not set up for this record yet
        uint32_t W = 1, col = 0, bpl = 1, r = 0;
        int64_t i = 0, p = 0, addr = 0;
        int64_t m_lo = 1, m_hi = 0;                            // coordinates [m_lo, m_hi) share one answer: masked or not
        bool m_in = false;
#pragma unroll 1
        for (int t = 0; t < nb; ++t, ++j) {
            while (j >= size) {                                // on to the next record that holds bytes
                ++k;
                rec0 = off[k]; size = off[k + 1] - rec0; j = 0;
                if (size > 0) { D = desc[k]; fresh = true; }
            }
            uint32_t ch;
            const int64_t hl = D.hl;
            if (j == 0) ch = '>';
            else if (j <= hl) ch = (D.flags & FAF_OWN_HDR) ? data[D.hsrc + j - 1] : hdr[D.hsrc + j - 1];
            else if (j == hl + 1) ch = '\n';
            else {
                const bool rev = (D.flags & 2) != 0;
                if (fresh) {                                   // place output byte j: line and column, the letter, its source line
                    fresh = false;
                    const int64_t L = D.L;
                    W = (uint32_t)(width == 0 || width > L ? (L > 0 ? L : 1) : width);
                    const uint64_t jj = (uint64_t)(j - hl - 2), w1 = (uint64_t)W + 1;
                    const uint64_t line = jj < (1ull << 32) ? (uint64_t)((uint32_t)jj / (uint32_t)w1) : jj / w1;     // (W + 1 <= 2^31)
                    col = (uint32_t)(jj - line * w1);
                    i = (int64_t)(line * W) + col;
                    const int64_t f = rev ? L - 1 - i : i;
                    p = D.a + f;
                    bpl = (uint32_t)D.bpl;
                    if (D.flags & FAF_FLAT) { r = 0; addr = D.src + f; }
                    else {
                        const uint32_t x = (uint32_t)(p < 0 ? 0 : p), ks = x / bpl;
                        r = x - ks * bpl;
                        addr = D.src + p + (int64_t)D.el * ks;
                    }
                    m_lo = 1; m_hi = 0;
                }
                if (col == W || i >= D.L) { ch = '\n'; col = 0; }
                else {
                    const bool is_flat = (D.flags & FAF_FLAT) != 0;
                    const uint8_t *__restrict__ s = is_flat ? flat : data;
                    ch = s[addr];
                    if (!is_flat) {
                        bool bad = is_space3(ch);
                        // the terminator between this letter and the query's next one
                        const bool line_end = rev ? (r == 0 && i + 1 < D.L) : (r == bpl - 1 && i + 1 < D.L);
                        if (line_end) {
                            const int64_t t0 = rev ? addr - D.el : addr + 1;
                            bad |= !is_space3(data[t0]) || (D.el == 2 && !is_space3(data[t0 + 1]));     // (el is 1 or 2: the size pass)
                        }
                        if (bad) { dirty[k] = 1; *any_dirty = 1; }
                    }
                    if ((D.flags & 1) && ch >= 'a' && ch <= 'z') ch -= 32;
                    if (mask_mode && D.m1 > D.m0) {
                        if (p < m_lo || p >= m_hi) {           // the first row that ends behind p holds it, or the gap in front of that row does
                            int64_t lo = D.m0, hi = D.m1;
                            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (mstop[mid] <= p) lo = mid + 1; else hi = mid; }
                            if (lo < D.m1 && mstart[lo] <= p) { m_in = true; m_lo = mstart[lo]; m_hi = mstop[lo]; }
                            else {
                                m_in = false;
                                m_lo = lo > D.m0 ? mstop[lo - 1] : INT64_MIN;
                                m_hi = lo < D.m1 ? mstart[lo] : INT64_MAX;
                            }
                        }
                        if (m_in) {
                            if (mask_mode == FAF_MASK_HARD) ch = (uint32_t)mask_byte;
                            else if (mask_mode == FAF_MASK_SOFT) { if (ch >= 'A' && ch <= 'Z') ch += 32; }
                            else if (ch >= 'a' && ch <= 'z') ch -= 32;
                        }
                    }
                    if (D.flags & 4) ch = lut[ch];
                    // on to the next letter: one forward, or one back on the reverse strand
                    ++i; ++col;
                    if (is_flat) { if (rev) { --p; --addr; } else { ++p; ++addr; } }
                    else if (rev) {
                        --p;
                        if (r == 0) { r = bpl - 1; addr -= 1 + D.el; } else { --r; --addr; }
                    } else {
                        ++p;
                        if (r == bpl - 1) { r = 0; addr += 1 + D.el; } else { ++r; ++addr; }
                    }
                }
            }
            if (t < 8) w_lo |= (uint64_t)ch << (8 * t);
            else w_hi |= (uint64_t)ch << (8 * (t - 8));
        }
        if (nb == 16) *reinterpret_cast<uint4 *>(out + o0) = make_uint4((uint32_t)w_lo, (uint32_t)(w_lo >> 32), (uint32_t)w_hi, (uint32_t)(w_hi >> 32));
        else
            for (int t = 0; t < nb; ++t) out[o0 + t] = (uint8_t)((t < 8 ? w_lo >> (8 * t) : w_hi >> (8 * (t - 8))) & 0xFF);
    }
}

}  // namespace fx
