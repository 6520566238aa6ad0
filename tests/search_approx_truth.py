"""The truth Fasta.search_approx is held to: a sliding window over fa[i].seq compared with the pattern letter by letter.
Plain Python / numpy; the match rules are written out here, nothing of pyfastx_amd.search is used (only _lib.revcomp_bytes
for the '-' pattern of an exact search, as Sequence.search makes it)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BASES = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
         "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
        "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}


def degenerate_revcomp(p):
    return "".join(COMP[c] for c in reversed(p.upper()))


def match_table(p, degenerate):
    """ok[j, c]: does text byte c match letter j of p?  Exact: the same byte.  Degenerate: c is an IUPAC letter (either
    case) whose base set lies inside the pattern letter's."""
    ok = np.zeros((len(p), 256), dtype=bool)
    for j, ch in enumerate(p):
        if degenerate:
            want = set(BASES[ch.upper()])
            for t, ts in BASES.items():
                if set(ts) <= want:
                    ok[j, ord(t)] = ok[j, ord(t.lower())] = True
        else:
            ok[j, ord(ch)] = True
    return ok


def anchor_positions(anchor, L):
    if anchor is None:
        return []
    if isinstance(anchor, slice):
        return list(range(*anchor.indices(L)))
    return [int(j) for j in anchor]


def window_distances(s, p, degenerate, held):
    """Per window of len(p) letters of s: the number of mismatching letters, or -1 where a held position mismatches."""
    L = len(p)
    a = np.frombuffer(s.encode("latin-1"), dtype=np.uint8)
    if a.size < L:
        return np.zeros(0, dtype=np.int64)
    win = sliding_window_view(a, L)
    bad = ~match_table(p, degenerate)[np.arange(L), win]                # [windows, L]
    dist = bad.sum(axis=1).astype(np.int64)
    if held:
        dist[bad[:, held].any(axis=1)] = -1
    return dist


def truth(seqs, p, d, anchor=None, strand="both", degenerate=False, rev=None):
    """[(record, start, stop, '+' / '-', mismatches)] by (record, start), '+' first: the windows of every s in seqs within
    d mismatches of p ('+') or of its reverse complement ('-'), none at an anchored position (given for p; mirrored for
    '-').  rev: the '-' pattern, where the caller has it already."""
    L = len(p)
    held = anchor_positions(anchor, L)
    pats = []
    if strand in ("+", "both"):
        pats.append((0, p.upper() if degenerate else p, held))
    if strand in ("-", "both"):
        if rev is None:
            if degenerate:
                rev = degenerate_revcomp(p)
            else:
                from pyfastx_amd import _lib
                rev = _lib.revcomp_bytes(p.encode("latin-1")).decode("latin-1")
        pats.append((1, rev, [L - 1 - j for j in held]))
    rows = []
    for i, s in enumerate(seqs):
        for k, q, h in pats:
            dist = window_distances(s, q, degenerate, h)
            for j in np.nonzero((dist >= 0) & (dist <= d))[0].tolist():
                rows.append((i, j, j + L, k, int(dist[j])))
    rows.sort()
    return [(i, a, b, "+-"[k], m) for i, a, b, k, m in rows]
