"""Plain Python truth for the region / window / class-run tests: loops and re.finditer over `seq` strings, nothing shared
with the code under test.  Columns: A C G T N other masked."""
import re

COLUMNS = ("A", "C", "G", "T", "N", "other", "masked")
_COLUMN_OF = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "N": 4, "n": 4}
_LOWER = "abcdefghijklmnopqrstuvwxyz"


def region_counts(seq, a, b):
    """The seven counts of seq[a:b]: A C G T N in either case, other = every other letter (U included), masked = a..z."""
    out = [0] * 7
    for ch in seq[a:b]:
        out[_COLUMN_OF.get(ch, 5)] += 1
        if ch in _LOWER:
            out[6] += 1
    return out


def windows(slen, window, step, partial):
    """[(start, stop)] of the windows [j step, min(j step + window, slen)) with j step < slen; without `partial` only those
    with j step + window <= slen."""
    out, j = [], 0
    while j * step < slen:
        a = j * step
        if partial or a + window <= slen:
            out.append((a, min(a + window, slen)))
        j += 1
    return out


def class_runs(seq, byteset, min_len=1):
    """[(start, stop)] of the maximal stretches of seq whose letters all lie in byteset (bytes / str, used as written), of
    at least min_len letters."""
    if isinstance(byteset, (bytes, bytearray)):
        byteset = bytes(byteset).decode("latin-1")
    rx = re.compile("[" + "".join(re.escape(c) for c in sorted(set(byteset))) + "]+")
    return [(m.start(), m.end()) for m in rx.finditer(seq) if m.end() - m.start() >= min_len]
