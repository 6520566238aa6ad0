"""Plain Python truth of the DUST entries (include/fxgpu.h, "low-complexity sequence"): the windowed mask of a text, by brute
force (every window recounted) and in the rolling form, and the per-read columns.  No numpy, nothing of the package."""

CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({c.lower(): i for c, i in list(CODE.items())})


def triplets(seq):
    """code of the triplet at every position p in 0..len - 3, -1 where one of its letters is invalid"""
    out = []
    for p in range(len(seq) - 2):
        a, b, c = (CODE.get(seq[p + i], -1) for i in range(3))
        out.append(16 * a + 4 * b + c if a >= 0 and b >= 0 and c >= 0 else -1)
    return out


def qualifies(n, s, threshold):
    return n >= 2 and 10 * s > threshold * (n - 1)


def _rows(flags, min_len):
    rows, i, n = [], 0, len(flags)
    while i < n:
        if flags[i]:
            j = i
            while j < n and flags[j]:
                j += 1
            if j - i >= min_len:
                rows.append((i, j))
            i = j
        else:
            i += 1
    return rows


def mask_brute(seq, window=64, threshold=20, min_len=1):
    """The definition as written: every window recounted from nothing, the union as one flag per letter."""
    n, tri = len(seq), triplets(seq)
    flags = [False] * n
    for e in range(2, n):
        a = max(0, e - window + 1)
        cnt = {}
        for p in range(a, e - 1):                            # triplets [p, p + 2] wholly inside [a, e]
            if tri[p] >= 0:
                cnt[tri[p]] = cnt.get(tri[p], 0) + 1
        if qualifies(sum(cnt.values()), sum(v * (v - 1) // 2 for v in cnt.values()), threshold):
            for i in range(a, e + 1):
                flags[i] = True
    return _rows(flags, min_len)


def mask(seq, window=64, threshold=20, min_len=1):
    """The rolling form: entering x: S += c[x]++, leaving y: S -= --c[y]; intervals joined as they come."""
    n, tri = len(seq), triplets(seq)
    cnt, s, t, cover = [0] * 64, 0, 0, []
    for e in range(2, n):
        x = tri[e - 2]
        if x >= 0:
            s += cnt[x]
            cnt[x] += 1
            t += 1
        o = e - window                                       # the window begins at e - window + 1: the triplet at o leaves
        if o >= 0 and tri[o] >= 0:
            cnt[tri[o]] -= 1
            s -= cnt[tri[o]]
            t -= 1
        if qualifies(t, s, threshold):
            a, b = max(0, e - window + 1), e + 1
            if cover and a <= cover[-1][1]:
                cover[-1][1] = b
            else:
                cover.append([a, b])
    return [(a, b) for a, b in cover if b - a >= min_len]


def merged(rows):
    """Intervals in any order -> the maximal intervals of their union (touching ones joined)."""
    out = []
    for a, b in sorted(rows):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def mask_multi(seq, windows, threshold=20, min_len=1):
    """Several window lengths: the union of their masks, min_len applied after the join."""
    rows = [r for w in windows for r in mask(seq, w, threshold, 1)]
    return [(a, b) for a, b in merged(rows) if b - a >= min_len]


def read_columns(s):
    """(length, n_triplets, dust_sum, n_diff) of one interval of a read, s a str"""
    cnt = {}
    for x in triplets(s):
        if x >= 0:
            cnt[x] = cnt.get(x, 0) + 1
    return (len(s), sum(cnt.values()), sum(v * (v - 1) // 2 for v in cnt.values()), sum(1 for j in range(len(s) - 1) if s[j] != s[j + 1]))


def dust(dust_sum, n_triplets):
    return 10.0 * dust_sum / (n_triplets - 1) if n_triplets >= 2 else 0.0


def complexity(n_diff, length):
    return n_diff / (length - 1) if length >= 2 else 0.0
