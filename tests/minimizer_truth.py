"""The oracle of the minimizer tests: a brute-force model of the definition in include/fxgpu.h over fa[i].seq, in Python ints.
It computes the key of every position and, for every window, the leftmost minimum; nothing is rolled, nothing is carried.

keys(seq, k, canonical, order)          -> per position None (no valid k-mer) or (key, strand, code)
truth(seqs, k, w, canonical, order, ids) -> (rows [(record, start, strand, code)], counts int64[n, 2])
lane_rows(seq, k, w, ..., run)          -> the rows of one record as the device's lanes find them: the state machine of
                                           csrc/fx_minimizer.hpp (ring, running minimum and its age, strand history, fed count),
                                           one lane per `run` letters, each warmed up on the w + k - 1 letters in front"""
import numpy as np

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
M64 = (1 << 64) - 1


def mix_int(x, k):
    """The hash order's key, as the definition writes it: unsigned 64-bit words, m = 4**k - 1."""
    m = 4 ** k - 1
    x = ((~x & M64) + ((x << 21) & M64)) & M64 & m
    x ^= x >> 24
    x = (x + ((x << 3) & M64) + ((x << 8) & M64)) & M64 & m
    x ^= x >> 14
    x = (x + ((x << 2) & M64) + ((x << 4) & M64)) & M64 & m
    x ^= x >> 28
    x = (x + ((x << 31) & M64)) & M64 & m
    return x


_FW = str.maketrans("ACGTacgt", "01230123")                    # the base-4 digits of a word, and of its complement
_RC = str.maketrans("ACGTacgt", "32103210")
_VALID = frozenset("ACGTacgt")
NONE = 1 << 64                                               # the key of a position without a valid k-mer: above every key


def keys(seq, k, canonical=True, order="hash"):
    """Per position p of seq[p:p+k]: None, or (key, strand, code).  Every word is read on its own: int(digits, 4)."""
    bad = [i for i, c in enumerate(seq) if c not in _VALID]
    invalid = set(p for i in bad for p in range(max(0, i - k + 1), i + 1))
    out = []
    for p in range(len(seq) - k + 1):
        if p in invalid:
            out.append(None)
            continue
        word = seq[p:p + k]
        fw, rc = int(word.translate(_FW), 4), int(word[::-1].translate(_RC), 4)
        if canonical:
            code, strand = (fw, "+") if fw <= rc else (rc, "-")
        else:
            code, strand = fw, "+"
        out.append((code if order == "lex" else mix_int(code, k), strand, code))
    return out


def record_rows(seq, k, w, canonical=True, order="hash"):
    """[(start, strand, code)] of one record: the distinct selections of its windows, in order."""
    ky = keys(seq, k, canonical, order)
    kk = [NONE if e is None else e[0] for e in ky]
    rows, last = [], None
    for j in range(len(ky) - w + 1):
        win = kk[j:j + w]
        m = min(win)
        if m == NONE:
            continue
        best = j + win.index(m)                              # the leftmost holder of the smallest key
        if best != last:
            assert last is None or best > last               # selections never move left
            rows.append((best, ky[best][1], ky[best][2]))
            last = best
    return rows


def truth(seqs, k, w, canonical=True, order="hash", ids=None):
    sel = range(len(seqs)) if ids is None else sorted(set(int(i) for i in ids))
    rows, counts = [], np.zeros((len(sel), 2), dtype=np.int64)
    for slot, i in enumerate(sel):
        for start, strand, code in record_rows(seqs[i], k, w, canonical, order):
            rows.append((i, start, strand, code))
            counts[slot, 1 if strand == "-" else 0] += 1
    return rows, counts


def lane_rows(seq, k, w, canonical=True, order="hash", run=256):
    """One lane per `run` letters of seq.  A lane owns the windows whose last k-mer ends at a letter of its run and emits at
    letter i iff that window exists, has a selection, and the window that ends at i - 1 has none or another one."""
    need, none = w + k - 1, 1 << 64
    mask = 4 ** k - 1
    rows = []
    for lo in range(0, len(seq), run):
        fw = rc = v = 0
        ring, head, mn, age, hist, fed = [None] * w, 0, none, 0, 0, 0
        for i in range(max(0, lo - need), min(lo + run, len(seq))):
            p_has, p_age = fed >= need and mn != none, age
            c = _CODE.get(seq[i])
            if c is None:
                v = 0
            else:
                fw = ((fw << 2) | c) & mask
                rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
                v = min(v + 1, k)
            code = min(fw, rc) if canonical else fw
            key = none if v < k else code if order == "lex" else mix_int(code, k)
            ring[head] = key
            hist = ((hist << 1) | (1 if canonical and rc < fw else 0)) & 0xFFFFFFFF
            if key < mn or mn == none:
                mn, age = key, 0
            else:
                age += 1
                if age >= w:
                    mn, s = none, head
                    for a in range(w - 1, -1, -1):
                        s = (s + 1) % w
                        assert ring[s] is not None           # no slot is read before it was written
                        if ring[s] < mn:
                            mn, age = ring[s], a
            head = (head + 1) % w
            fed = min(fed + 1, need)
            if i >= lo and fed >= need and mn != none and not (p_has and age == p_age + 1):
                start = i - (k - 1) - age
                rows.append((start, "-" if (hist >> age) & 1 else "+", mn if order == "lex" else _unmix_int(mn, k)))
    return rows


def _unmix_int(x, k):
    m = 4 ** k - 1
    x = (x * pow(2 ** 31 + 1, -1, 1 << 64)) & m
    x ^= (x >> 28) ^ (x >> 56)
    x = (x * pow(21, -1, 1 << 64)) & m
    x ^= (x >> 14) ^ (x >> 28) ^ (x >> 42) ^ (x >> 56)
    x = (x * pow(265, -1, 1 << 64)) & m
    x ^= (x >> 24) ^ (x >> 48)
    x = ((x + 1) * pow(2 ** 21 - 1, -1, 1 << 64)) & m
    return x
