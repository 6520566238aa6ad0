// fx_orf.hpp -- open reading frames in all six frames on the sequence bytes of the resident FASTA table (fx_fasta_orfs), and
// table translation of a batch of intervals (fx_fasta_translate_alloc).  Extension: the reference reads no codon; getorf /
// ORFfinder users slice every record to the host and walk it six times.
//
// Definition.  The text of a record is what fx_search.hpp walks (bytes 10 / 13 / 32 dropped, cut at slen); letters fold as in
// fx_tandem.hpp (A C G T = 0..3 whatever their case, every other byte invalid).  A codon at j occupies [j, j + 3), 0 <= j,
// j + 3 <= slen; its index is 16 c0 + 4 c1 + c2 on the forward strand and 16 (3 - c2) + 4 (3 - c1) + (3 - c0) on the reverse
// strand.  A codon with an invalid letter is invalid; otherwise it is STOP, START or OTHER by two 64-bit masks (the stop wins).
// A BREAK is a STOP or an invalid codon.  Per strand and class c = j mod 3 a SEGMENT is a maximal run of consecutive codons
// that are no breaks: from c or the end of a break codon to the start of the next break codon or the end of the last full
// codon of the class.  In forward coordinates the segments of the reverse strand have the same geometry (the reverse
// complement only mirrors them), so one left-to-right walk serves six components (strand, class).  Mode stop reports the
// segment [a, b); mode start reports [s, b) on the forward strand, s the FIRST START codon of the segment, and [a, e) on the
// reverse strand, e the end of the LAST reverse START codon -- the first one of the reverse complement.  A row is kept from
// max(min_len, 3) letters on.
//
// Passes, in the shape of fx_tandem.hpp: one lane per 256-byte run of the selected records, geometry and the cut from the rank
// index.  A codon belongs to the run that holds its LAST letter.
//   k_orf_count  warms a history of two letters from the (at most 2) kept bytes in front of the run, never past the record's
//                boff, classifies the codon that ends at each letter on both strands by two shifts of the masks, and notes per
//                component: the first break and its kind, the place behind the last break and its kind, the START in front
//                of the first break (forward: the first one, reverse: the last one; of the whole run when it has no break)
//                and the START behind the last break (same rule), in 38 bits of one 64-bit word.  A row that a break after
//                the first closes began inside the run: it is counted here.
//   carry        one scan of twelve components (k_sscan_*<12>): "has a break" and "has no break but a START", per component,
//                and the compacted lists of those runs (k_orf_list).  The segment open at a run's entry began behind the last
//                break of the last earlier breaking run of the same record, or at c; it may span any number of runs.  Its
//                START is the one that run noted behind its last break, or that of the first (forward) / last (reverse) listed
//                START run between the two: those runs have no break, so what they noted is inside the segment.
//   k_orf_close  adds the row each component's first break closes and, in the run that holds the last letter in front of the
//                cut, what the end of the text closes (three classes, two strands, at slen - 2 .. slen).
//   offsets      one scan of the counts; the host reads the total only.
//   k_orf_emit   the runs that close something walk again from the exact carried state and store (record, start, stop, frame,
//                flags) at their offsets: ordered by record, the coordinate at which the segment closes, strand -- no sort, no
//                atomic.
//   k_tr_translate  one lane per amino acid of the batch: its query by a binary search over the offsets, three letters of the
//                fetched block (read backwards and complemented as codes on the reverse strand: U and IUPAC letters stay
//                invalid, which the complement table of the fetch would not keep), one byte out.
#pragma once
#include "fx_tandem.hpp"

namespace fx {

constexpr int ORF_NC = 6;                                  // components: 3 * strand + class (the codon's start mod 3)
constexpr uint32_t ORF_NONE = 511u;
enum : uint32_t { ORF_OTHER = 0, ORF_START = 1, ORF_STOP = 2, ORF_INVALID = 3 };

struct OrfArg {
    uint64_t stop[2], start[2];   // bit = forward codon index; [1]: the masks of the reverse strand brought to that index
    int64_t thr;                  // a row is kept from this length on: max(min_len, 3)
    int32_t mode, strands;        // 0 stop to stop, 1 START to stop; bit 0 forward, bit 1 reverse
};

// per run and component: letter index of the first break (bits 0..8, ORF_NONE: none), that break is a STOP (9), the place
// behind the last break relative to the run's first letter (10..18), the last break is a STOP (19), 2 + the codon start of the
// START in front of the first break (20..28, ORF_NONE: none), the same behind the last break (29..37)
__device__ __forceinline__ uint64_t orf_pack(uint32_t first, uint32_t fstop, uint32_t open, uint32_t lstop, uint32_t st_a, uint32_t st_b) {
    return (uint64_t)(first | (fstop << 9) | (open << 10) | (lstop << 19)) | ((uint64_t)st_a << 20) | ((uint64_t)st_b << 29);
}
__device__ __forceinline__ uint32_t orf_first(uint64_t w) { return (uint32_t)w & 511u; }
__device__ __forceinline__ uint32_t orf_fstop(uint64_t w) { return (uint32_t)(w >> 9) & 1u; }
__device__ __forceinline__ int64_t orf_open(uint64_t w) { return (int64_t)((w >> 10) & 511u); }
__device__ __forceinline__ uint32_t orf_lstop(uint64_t w) { return (uint32_t)(w >> 19) & 1u; }
__device__ __forceinline__ uint32_t orf_st_a(uint64_t w) { return (uint32_t)(w >> 20) & 511u; }
__device__ __forceinline__ uint32_t orf_st_b(uint64_t w) { return (uint32_t)(w >> 29) & 511u; }

template <class T> __device__ __forceinline__ T orf_nost();                     // "the segment has no START so far"
template <> __device__ __forceinline__ int orf_nost<int>() { return INT32_MIN; }
template <> __device__ __forceinline__ int64_t orf_nost<int64_t>() { return INT64_MIN; }

// The row of a segment [a, b) of strand s whose START codon (first on +, last on -) begins at st -> kept; [*rs, *re)
template <class T> __device__ __forceinline__ bool orf_row(const OrfArg &A, int s, T a, T st, T b, T *rs, T *re) {
    *rs = a;
    *re = b;
    if (A.mode) {
        if (st == orf_nost<T>()) return false;
        if (s == 0) *rs = st; else *re = st + 3;
    }
    return (int64_t)*re - (int64_t)*rs >= A.thr;             // in 64 bits whatever T: thr is any int64 from 3 on
}

// The walk's state; positions are relative to the run's first letter (T: int in the count pass, int64 where they are exact).
template <class T> struct OrfState {
    T open[ORF_NC], st[ORF_NC];           // left end of the open segment; its first (+) / last (-) START codon
    uint32_t ostop;                       // bit comp: a STOP codon opened the segment
    uint32_t idx, inv;                    // the last three letters: codon index, "one of them is invalid" (a bit a letter)
    int cls, skip;                        // class of the codon that ends at the next letter; letters that end no codon
};
// One letter at position x.  brk(comp, x, kind) for every component whose codon [x - 2, x + 1) is a break, + before -, before
// the state moves.
template <class T, class F> __device__ __forceinline__ void orf_step(const OrfArg &A, OrfState<T> &S, uint32_t code, T x, F &&brk) {
    S.idx = ((S.idx << 2) | (code & 3u)) & 63u;
    S.inv = ((S.inv << 1) | (code >> 2)) & 7u;
    if (x >= (T)S.skip) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!((A.strands >> s) & 1)) continue;
            const uint32_t kind = S.inv ? ORF_INVALID : (A.stop[s] >> S.idx) & 1ull ? ORF_STOP : (A.start[s] >> S.idx) & 1ull ? ORF_START : ORF_OTHER;
            if (kind == ORF_OTHER) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (S.cls != c) continue;
                const int comp = 3 * s + c;
                if (kind == ORF_START) {
                    if (s == 1 || S.st[comp] == orf_nost<T>()) S.st[comp] = x - 2;
                } else {
                    brk(comp, x, kind);
                    S.open[comp] = x + 1;
                    S.st[comp] = orf_nost<T>();
                    S.ostop = (S.ostop & ~(1u << comp)) | ((kind == ORF_STOP ? 1u : 0u) << comp);
                }
            }
        }
    }
    S.cls = S.cls == 2 ? 0 : S.cls + 1;
}
// The two letters in front of the run (at most to the record's boff); the segments as a run at the record's start has them.
template <class T> __device__ __forceinline__ void orf_warm(const SearchPlan &P, const TdRun &R, OrfState<T> &S) {
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) { S.open[comp] = (T)(comp % 3) - (T)R.base; S.st[comp] = orf_nost<T>(); }
    S.ostop = 0;
    S.idx = 0;
    S.inv = 0;
    S.cls = (int)((R.base + 1) % 3);                        // letter 0 ends the codon at base - 2
    S.skip = R.base >= 2 ? 0 : 2 - (int)R.base;
    if (R.L - R.base <= 0) return;                          // behind the cut: nothing is walked
    int64_t ws = R.lo;
    int w = 0;
    while (w < 2 && ws > R.b) {
        --ws;
        w += srch_space(P.base[ws]) ? 0 : 1;
    }
    for (int64_t a = ws; a < R.lo; ++a) {
        const uint32_t ch = P.base[a];
        if (srch_space(ch)) continue;
        const uint32_t code = td_code(ch);
        S.idx = ((S.idx << 2) | (code & 3u)) & 63u;
        S.inv = ((S.inv << 1) | (code >> 2)) & 7u;
    }
}
// The kept bytes of the run in front of the cut, in order.
template <class T, class F>
__device__ __forceinline__ void orf_walk(const SearchPlan &P, const OrfArg &A, const TdRun &R, OrfState<T> &S, F &&brk) {
    const int lim = (int)min(R.L - R.base, (int64_t)SRCH_RUN);
    int kidx = 0;
    for (int64_t c = R.lo & ~(int64_t)15; c < R.hi && kidx < lim; c += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.base + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t four = w[i];
#pragma unroll 1
            for (int j = 0; j < 4; ++j, four >>= 8) {
                const uint32_t ch = four & 0xFFu;
                const int64_t a = c + 4 * i + j;
                if (a < R.lo || a >= R.hi || srch_space(ch) || kidx >= lim) continue;
                orf_step(A, S, td_code(ch), (T)kidx, brk);
                ++kidx;
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_orf_count(SearchPlan P, RankIndex X, OrfArg A, uint64_t *__restrict__ pk, uint32_t *__restrict__ closes) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const TdRun R = td_run(P, X, q);
    OrfState<int> S;
    orf_warm(P, R, S);
    uint32_t first[ORF_NC], fstop = 0, n = 0;
    int st_a[ORF_NC];
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) { first[comp] = ORF_NONE; st_a[comp] = orf_nost<int>(); }
    orf_walk(P, A, R, S, [&](int comp, int x, uint32_t kind) __attribute__((always_inline)) {
        if (first[comp] == ORF_NONE) {
            first[comp] = (uint32_t)x;
            fstop |= (kind == ORF_STOP ? 1u : 0u) << comp;
            st_a[comp] = S.st[comp];
        } else {
            int rs, re;
            n += orf_row(A, comp / 3, S.open[comp], S.st[comp], x - 2, &rs, &re) ? 1u : 0u;
        }
    });
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) {
        const bool brk = first[comp] != ORF_NONE;
        const int a = brk ? st_a[comp] : S.st[comp], b = brk ? S.st[comp] : orf_nost<int>();
        pk[comp * P.n_runs + q] = orf_pack(first[comp], (fstop >> comp) & 1u, brk ? (uint32_t)S.open[comp] : 0u, (S.ostop >> comp) & 1u,
                                           a == orf_nost<int>() ? ORF_NONE : (uint32_t)(a + 2), b == orf_nost<int>() ? ORF_NONE : (uint32_t)(b + 2));
    }
    closes[q] = n;
}

struct OrfLdCarry {                       // per component "the run has a break" (0..5), "it has none, but a START" (6..11)
    const uint64_t *pk;
    int64_t n_runs;
    __device__ void operator()(int64_t q, int64_t *v) const {
#pragma unroll
        for (int comp = 0; comp < ORF_NC; ++comp) {
            const uint64_t w = pk[comp * n_runs + q];
            const bool brk = orf_first(w) != ORF_NONE;
            v[comp] = brk;
            v[ORF_NC + comp] = !brk && orf_st_a(w) != ORF_NONE;
        }
    }
};
struct OrfLdCloses {
    const uint32_t *p;
    __device__ void operator()(int64_t q, int64_t *v) const { v[0] = p[q]; }
};
// per scan component: list[NZ[q]] = q for every run that counts in it (NZ: 12 components of n_runs + 1 entries)
__global__ __launch_bounds__(BLOCK) void k_orf_list(const uint64_t *__restrict__ pk, const int64_t *__restrict__ NZ, int64_t n_runs,
                                                    int64_t *__restrict__ list) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_runs) return;
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) {
        const uint64_t w = pk[comp * n_runs + q];
        const bool brk = orf_first(w) != ORF_NONE;
        if (brk) list[comp * n_runs + NZ[comp * (n_runs + 1) + q]] = q;
        else if (orf_st_a(w) != ORF_NONE) list[(ORF_NC + comp) * n_runs + NZ[(ORF_NC + comp) * (n_runs + 1) + q]] = q;
    }
}

// The segment of component comp that is open at the entry of run q, in positions of the record: its left end, what opened it,
// and its START codon as far as the runs in front of q know it (forward: the first one; reverse: the last one).
struct OrfOpen { int64_t a, st; uint32_t stop; };
__device__ __forceinline__ OrfOpen orf_carry(const SearchPlan &P, const RankIndex &X, const TdRun &R, int64_t q, int comp,
                                             const uint64_t *__restrict__ pk, const int64_t *__restrict__ NZ,
                                             const int64_t *__restrict__ list) {
    const int64_t nr1 = P.n_runs + 1, k0 = P.run0[R.k], g0 = X.run0[R.r], none = orf_nost<int64_t>();
    const int64_t *NB = NZ + comp * nr1, *NS = NZ + (ORF_NC + comp) * nr1;
    const int64_t *bl = list + comp * P.n_runs, *sl = list + (ORF_NC + comp) * P.n_runs;
    auto base_of = [&](int64_t p) { return X.pref[g0 + (p - k0)] - X.pref[g0]; };
    OrfOpen o{comp % 3, none, 0u};
    int64_t from = k0, behind = none;                       // the runs from `from` on have no break; the START behind the break
    const int64_t nb = NB[q];
    if (nb > 0 && bl[nb - 1] >= k0) {
        const int64_t p = bl[nb - 1], pb = base_of(p);
        const uint64_t w = pk[comp * P.n_runs + p];
        o.a = pb + orf_open(w);
        o.stop = orf_lstop(w);
        if (orf_st_b(w) != ORF_NONE) behind = pb + (int64_t)orf_st_b(w) - 2;
        from = p + 1;
    }
    const int64_t s0 = NS[from], s1 = NS[q];                // the listed START runs in [from, q)
    const int64_t r = s0 < s1 ? sl[comp < 3 ? s0 : s1 - 1] : -1;
    const int64_t between = r >= 0 ? base_of(r) + (int64_t)orf_st_a(pk[comp * P.n_runs + r]) - 2 : none;
    if (comp < 3) o.st = behind != none ? behind : between;
    else o.st = between != none ? between : behind;
    return o;
}
// the START of a segment whose part in front of run q has `carried` and whose part inside the run has `own`
__device__ __forceinline__ int64_t orf_join(int s, int64_t carried, int64_t own) {
    const int64_t none = orf_nost<int64_t>();
    return s == 0 ? (carried != none ? carried : own) : (own != none ? own : carried);
}

__global__ __launch_bounds__(BLOCK) void k_orf_close(SearchPlan P, RankIndex X, OrfArg A, const uint64_t *__restrict__ pk,
                                                     const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                     uint32_t *__restrict__ closes) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs) return;
    const TdRun R = td_run(P, X, q);
    const int64_t none = orf_nost<int64_t>();
    uint32_t n = closes[q];
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) {
        const int s = comp / 3, c = comp % 3;
        const uint64_t w = pk[comp * P.n_runs + q];
        const uint32_t first = orf_first(w);
        if (!((A.strands >> s) & 1) || (first == ORF_NONE && !R.end)) continue;
        OrfOpen o = orf_carry(P, X, R, q, comp, pk, NZ, list);
        int64_t rs, re;
        o.st = orf_join(s, o.st, orf_st_a(w) != ORF_NONE ? R.base + (int64_t)orf_st_a(w) - 2 : none);
        if (first != ORF_NONE) {
            n += orf_row(A, s, o.a, o.st, R.base + (int64_t)first - 2, &rs, &re) ? 1u : 0u;
            o.a = R.base + orf_open(w);
            o.st = orf_st_b(w) != ORF_NONE ? R.base + (int64_t)orf_st_b(w) - 2 : none;
        }
        if (R.end && R.L >= c + 3) n += orf_row(A, s, o.a, o.st, R.L - (R.L - c) % 3, &rs, &re) ? 1u : 0u;
    }
    closes[q] = n;
}

__global__ __launch_bounds__(BLOCK) void k_orf_emit(SearchPlan P, RankIndex X, OrfArg A, const uint64_t *__restrict__ pk,
                                                    const int64_t *__restrict__ NZ, const int64_t *__restrict__ list,
                                                    const uint32_t *__restrict__ closes, const int64_t *__restrict__ O,
                                                    int64_t *__restrict__ o_rec, int64_t *__restrict__ o_start, int64_t *__restrict__ o_stop,
                                                    int8_t *__restrict__ o_frame, uint8_t *__restrict__ o_flags) {
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= P.n_runs || !closes[q]) return;
    const TdRun R = td_run(P, X, q);
    const int64_t none = orf_nost<int64_t>();
    OrfState<int64_t> S;
    orf_warm(P, R, S);
#pragma unroll
    for (int comp = 0; comp < ORF_NC; ++comp) {
        if (!((A.strands >> (comp / 3)) & 1)) continue;
        const OrfOpen o = orf_carry(P, X, R, q, comp, pk, NZ, list);
        S.open[comp] = o.a - R.base;
        S.st[comp] = o.st != none ? o.st - R.base : none;
        S.ostop |= o.stop << comp;
    }
    int64_t o = O[q];
    const int64_t o_end = O[q + 1];
    // the segment of comp closes at b (relative); stop: a STOP codon closes it
    auto put = [&](int comp, int64_t b, uint32_t stop) __attribute__((always_inline)) {
        const int s = comp / 3;
        const int64_t st = S.st[comp];
        const uint32_t opened = (S.ostop >> comp) & 1u;
        int64_t rs, re;
        if (!orf_row(A, s, S.open[comp], st, b, &rs, &re) || o >= o_end) return;
        rs += R.base;
        re += R.base;
        o_rec[o] = R.r;
        o_start[o] = rs;
        o_stop[o] = re;
        if (s == 0) {
            o_frame[o] = (int8_t)(1 + rs % 3);
            o_flags[o] = (uint8_t)(stop | (opened << 1) | ((st != none && st + R.base == rs ? 1u : 0u) << 2));
        } else {
            o_frame[o] = (int8_t)-(1 + (R.L - re) % 3);
            o_flags[o] = (uint8_t)(opened | (stop << 1) | ((st != none && st + 3 + R.base == re ? 1u : 0u) << 2));
        }
        ++o;
    };
    orf_walk(P, A, R, S, [&](int comp, int64_t x, uint32_t kind) __attribute__((always_inline)) { put(comp, x - 2, kind == ORF_STOP ? 1u : 0u); });
    if (R.end) {
        for (int64_t b = max(R.L - 2, (int64_t)3); b <= R.L; ++b) {       // the last full codon of class b mod 3 ends at b
            const int cc = (int)(b % 3);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!((A.strands >> s) & 1)) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c == cc) put(3 * s + c, b - R.base, 0u);
            }
        }
    }
}

// ------------------------------------------------------------------ translation
// amino acids of query i: a third of the letters it fetches (cnt: 0 for a query that is not valid)
__global__ __launch_bounds__(BLOCK) void k_tr_counts(const int32_t *__restrict__ cnt, int64_t n, int32_t *__restrict__ cnt3) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) cnt3[i] = cnt[i] / 3;
}
// nt: the letters of the queries at noff (n + 1 entries), forward; out[aoff[k] + i] = amino acid i of query k.  tab: 64 amino
// acids by codon index, then the byte of an invalid codon.
__global__ __launch_bounds__(BLOCK) void k_tr_translate(const uint8_t *__restrict__ nt, const int64_t *__restrict__ noff,
                                                        const int64_t *__restrict__ aoff, const uint8_t *__restrict__ strand, int64_t n,
                                                        const uint8_t *__restrict__ tab, int64_t total, uint8_t *__restrict__ out) {
    __shared__ uint8_t t[65];
    if (threadIdx.x < 65) t[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const int64_t k = upper_bound(aoff, n + 1, i) - 1, a = i - aoff[k], b = noff[k], len = noff[k + 1] - b;
    const bool minus = strand && strand[k];
    const uint8_t *p = nt + b + (minus ? len - 3 - 3 * a : 3 * a);
    uint32_t c0 = td_code(p[0]), c1 = td_code(p[1]), c2 = td_code(p[2]);
    const bool bad = (c0 | c1 | c2) & TD_BAD;
    if (minus) { const uint32_t f = 3u - c0; c0 = 3u - c2; c1 = 3u - c1; c2 = f; }
    out[i] = bad ? t[64] : t[(16u * c0 + 4u * c1 + c2) & 63u];
}

}  // namespace fx
