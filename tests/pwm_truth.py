"""The numpy oracle of the position weight matrix scan (Fasta.pwm_scan / pwm_counts / pwm_best): windows of W letters of
every record's `seq`, scored with sliding_window_view over the code arrays; a letter that is not A C G T U (either case)
poisons every window that holds it.  Rows in the contract's order: by (record, start), '+' before '-' at one start."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

NO_SCORE = int(np.iinfo(np.int32).min)

_CODE = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def codes(seq):
    """str / bytes -> int64 codes, -1 for a letter that is not A C G T U."""
    b = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    return _CODE[np.frombuffer(b, dtype=np.uint8)]


def window_scores(seq, ints):
    """(valid bool[n], plus int64[n], minus int64[n]) for the n = len(seq) - W + 1 windows of seq (n <= 0: empty arrays)."""
    m = np.asarray(ints, dtype=np.int64)
    W = m.shape[0]
    x = codes(seq)
    if x.size < W:
        z = np.zeros(0, dtype=np.int64)
        return np.zeros(0, dtype=bool), z, z.copy()
    win = sliding_window_view(x, W)                          # [n, W]
    valid = (win >= 0).all(axis=1)
    w = np.where(win >= 0, win, 0)
    j = np.arange(W)
    plus = m[j[None, :], w].sum(axis=1)
    minus = m[(W - 1 - j)[None, :], 3 - w].sum(axis=1)
    return valid, plus, minus


def truth(seqs, ints, min_score, strand="both", ids=None):
    """-> (rows [(id, start, stop, strand, score)], best_scores int64[n_sel, 2], best_starts int64[n_sel, 2]); the rows over the
    ascending distinct ids, the best in the order of ids as given (None: every record)."""
    W = np.asarray(ints).shape[0]
    order = list(range(len(seqs))) if ids is None else [int(i) for i in ids]
    rows = []
    for i in sorted(set(order)):
        valid, plus, minus = window_scores(seqs[i], ints)
        hp = valid & (plus >= min_score) & (strand in ("+", "both"))
        hm = valid & (minus >= min_score) & (strand in ("-", "both"))
        for s in np.nonzero(hp | hm)[0].tolist():
            if hp[s]:
                rows.append((i, s, s + W, "+", int(plus[s])))
            if hm[s]:
                rows.append((i, s, s + W, "-", int(minus[s])))
    bs = np.full((len(order), 2), NO_SCORE, dtype=np.int64)
    bp = np.full((len(order), 2), -1, dtype=np.int64)
    for k, i in enumerate(order):
        valid, plus, minus = window_scores(seqs[i], ints)
        at = np.nonzero(valid)[0]
        if not at.size:
            continue
        for col, (sc, on) in enumerate(((plus, strand in ("+", "both")), (minus, strand in ("-", "both")))):
            if on:
                j = int(np.argmax(sc[at]))                   # the first of the maxima: the smallest start
                bs[k, col], bp[k, col] = int(sc[at][j]), int(at[j])
    return rows, bs, bp
