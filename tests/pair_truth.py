"""The definitions of the paired-end entries (include/fxgpu.h: fx_fastq_pair_overlap, fx_fastq_pair_merge_alloc) in plain
Python / numpy, one pair at a time: the overlap of the mates, what survives read-through, the insert, the merged record.
s1, q1, s2, q2 are bytes (or uint8 arrays) as fq[i].seq / fq[i].qual give them."""
import numpy as np

NONE = -2**31

_CODE = np.full(256, -1, dtype=np.int16)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k                                            # the Watson-Crick complement of code c is 3 - c

# the complement table of fx_fastq_fetch's reverse-complement flag: IUPAC pairs, U -> A, case kept, everything else itself
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "CG", "MK", "RY", "VB", "HD"):
    for _x, _y in ((_a, _b), (_b, _a)):
        COMP[ord(_x)] = ord(_y)
        COMP[ord(_x) + 32] = ord(_y) + 32
COMP[ord("U")] = ord("A")
COMP[ord("u")] = ord("a")


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b.astype(np.uint8, copy=False)


def diagonals(L1, L2):
    """The trial order: 0, 1, ..., L1 - 1, -1, -2, ..., -(L2 - 1)."""
    return list(range(0, L1)) + [-e for e in range(1, L2)]


def mismatches_on(s1, s2, d):
    """(m, mm) of diagonal d, letter by letter from the definition."""
    s1, s2 = bytes(s1), bytes(s2)
    L1, L2 = len(s1), len(s2)
    lo, hi = max(0, d), min(L1, d + L2)
    wc = {65: 84, 67: 71, 71: 67, 84: 65}
    mm = 0
    for j in range(lo, hi):
        x, y = s1[j], s2[L2 - 1 - (j - d)]
        if not (x in wc and y in wc and wc[y] == x):
            mm += 1
    return hi - lo, mm


def insert_of(d, L1, L2):
    if d == NONE:
        return -1
    return max(L1, d + L2) if d >= 0 else L2 + d


def overlap_truth(s1, s2, min_overlap=30, max_diff=5, err=(1, 5)):
    """-> dict(diag, overlap, mismatches, end1, end2, insert) of one pair."""
    a, b = _u8(s1), _u8(s2)
    L1, L2 = len(a), len(b)
    ca = _CODE[a]
    cr = _CODE[b[::-1]]
    cr = np.where(cr >= 0, 3 - cr, -1)                        # codes of the reverse complement
    num, den = err
    for d in diagonals(L1, L2):
        lo, hi = max(0, d), min(L1, d + L2)
        m = hi - lo
        if m < min_overlap:
            continue
        x, y = ca[lo:hi], cr[lo - d:hi - d]
        mm = m - int(((x >= 0) & (x == y)).sum())
        if mm <= max_diff and mm * den <= num * m:
            return {"diag": d, "overlap": m, "mismatches": mm, "end1": min(L1, L2 + d) if d < 0 else L1, "end2": L2 + d if d < 0 else L2,
                    "insert": insert_of(d, L1, L2)}
    return {"diag": NONE, "overlap": 0, "mismatches": 0, "end1": L1, "end2": L2, "insert": -1}


def merged_truth(header, s1, q1, s2, q2, d, min_len=0):
    """The merged record of a pair on diagonal d (bytes; b"" for NONE or a fragment shorter than min_len)."""
    s1, q1, s2, q2 = bytes(s1), bytes(q1), bytes(s2), bytes(q2)
    L1, L2 = len(s1), len(s2)
    if d == NONE:
        return b""
    assert -(L2 - 1) <= d <= L1 - 1
    F = insert_of(d, L1, L2)
    if F < min_len:
        return b""
    seq, qual = bytearray(), bytearray()
    for f in range(F):
        k = f - d
        has1, has2 = f < L1, 0 <= k < L2
        assert has1 or has2
        if has2:
            y, b = int(COMP[s2[L2 - 1 - k]]), q2[L2 - 1 - k]
        if has1 and has2:
            x, a = s1[f], q1[f]
            if x == y:
                c, q = x, max(a, b)
            elif a >= b:
                c, q = x, a
            else:
                c, q = y, b
        elif has1:
            c, q = s1[f], q1[f]
        else:
            c, q = y, b
        seq.append(c)
        qual.append(q)
    return bytes(header) + b"\n" + bytes(seq) + b"\n+\n" + bytes(qual) + b"\n"


def revcomp(s):
    return bytes(COMP[_u8(s)[::-1]])
