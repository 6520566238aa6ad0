"""The truth Fasta.search_edit is held to, and its definition: Sellers' dynamic programme over fa[i].seq, no bit-vector.

D[e] = min over s <= e + 1 of the Levenshtein distance between the pattern and s[s : e + 1] (substitution, insertion and
deletion cost 1 each); e is an END when D[e] <= k.  A row per reported end: stop = e + 1, edits = D[e], start = stop - m
for the smallest span length m in L - k .. L + k whose distance is D[e] (brute force: a plain anchored Levenshtein table
per row, no knowledge of D).  report = "best" keeps end e iff (e - 1 is no end or D[e-1] > D[e]) and (e + 1 is no end or
D[e+1] >= D[e]), per record and strand.  Rows by (record, stop), '+' before '-'.

The table is filled pattern row by pattern row, numpy along the text: with t[j] = min(above-left + mismatch, above + 1)
the in-row term D[i][j-1] + 1 is np.minimum.accumulate(t - arange) + arange.  The match rule and the '-' pattern come from
search_approx_truth.py."""
from functools import lru_cache

import numpy as np

from search_approx_truth import degenerate_revcomp, match_table


def _relax(t):
    """t[..., j] = min over j' <= j of t[..., j'] + (j - j'): steps along the last axis cost 1."""
    ar = np.arange(t.shape[-1], dtype=np.int32)
    return np.minimum.accumulate(t - ar, axis=-1) + ar


@lru_cache(maxsize=64)
def end_distances(s, q, degenerate):
    """D[e] for every letter e of s (int32[len(s)]): the least distance between q and a stretch of s that ends with letter e."""
    a = np.frombuffer(s.encode("latin-1"), dtype=np.uint8)
    ok = match_table(q, degenerate)
    row = np.zeros(a.size + 1, dtype=np.int32)                            # the empty pattern matches the empty stretch anywhere
    for i in range(1, len(q) + 1):
        t = np.empty_like(row)
        t[0] = i
        t[1:] = np.minimum(row[:-1] + ~ok[i - 1, a], row[1:] + 1)
        row = _relax(t)
    row.setflags(write=False)
    return row[1:]


def span_distances(q, degenerate, windows):
    """windows: uint8 [R, M], row r = the M letters in front of (and with) an end, NEWEST FIRST.  -> int32 [R, M + 1]:
    [r, m] = the Levenshtein distance between q and the last m letters (a plain table of the reversed strings, the text as
    its rows' axis: every prefix of the reversed window is a column)."""
    ok = match_table(q, degenerate)
    L = len(q)
    R, M = windows.shape
    row = np.broadcast_to(np.arange(M + 1, dtype=np.int32), (R, M + 1))   # the empty pattern against m letters: m
    for i in range(1, L + 1):
        t = np.empty((R, M + 1), dtype=np.int32)
        t[:, 0] = i
        t[:, 1:] = np.minimum(row[:, :-1] + ~ok[L - i][windows], row[:, 1:] + 1)
        row = _relax(t)
    return row


def best_filter(ends):
    """ends: {e: D[e]} of one record and strand -> the e that report = "best" keeps."""
    return [e for e, d in ends.items()
            if (e - 1 not in ends or ends[e - 1] > d) and (e + 1 not in ends or ends[e + 1] >= d)]


def strand_rows(s, q, k, degenerate, report="all"):
    """[(start, stop, edits)] of one record and one pattern, by stop."""
    L = len(q)
    assert 0 <= k <= min(8, L - 1)
    D = end_distances(s, q, degenerate)
    e = np.nonzero(D <= k)[0]
    if report == "best":
        e = np.array(sorted(best_filter(dict(zip(e.tolist(), D[e].tolist())))), dtype=np.int64)
    else:
        assert report == "all"
    if e.size == 0:
        return []
    a = np.frombuffer(s.encode("latin-1"), dtype=np.uint8)
    M = L + k
    idx = e[:, None] - np.arange(M)[None, :]                              # newest first; in front of the record: nothing
    win = np.where(idx >= 0, a[np.maximum(idx, 0)], 0).astype(np.uint8)
    A = span_distances(q, degenerate, win)
    rows = []
    for r, (end, d) in enumerate(zip(e.tolist(), D[e].tolist())):
        m = next(m for m in range(max(L - k, 1), min(M, end + 1) + 1) if A[r, m] == d)
        rows.append((end + 1 - m, end + 1, d))
    return rows


def truth(seqs, p, k, strand="both", degenerate=False, report="best", rev=None):
    """[(record, start, stop, '+' / '-', edits)] by (record, stop), '+' first.  rev: the '-' pattern, where the caller has it."""
    pats = []
    if strand in ("+", "both"):
        pats.append((0, p.upper() if degenerate else p))
    if strand in ("-", "both"):
        if rev is None:
            if degenerate:
                rev = degenerate_revcomp(p)
            else:
                from pyfastx_amd import _lib
                rev = _lib.revcomp_bytes(p.encode("latin-1")).decode("latin-1")
        pats.append((1, rev))
    rows = []
    for i, s in enumerate(seqs):
        for sid, q in pats:
            rows += [(i, stop, sid, start, d) for start, stop, d in strand_rows(s, q, k, degenerate, report)]
    rows.sort()
    return [(i, start, stop, "+-"[sid], d) for i, stop, sid, start, d in rows]
