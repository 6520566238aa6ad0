"""The definition of exact duplicate detection (Fastq.duplicates / Fastq.dedup) in plain Python: a dict of key -> first position
over the strings a file was written from.  The key of a query is its byte string; with revcomp it is min(key, rc(key)) compared
as byte strings, rc = reversed with A<->T, C<->G, a<->t, c<->g and every other byte mapped to itself.  Never uses the package."""
import numpy as np

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def rc(key):
    return as_bytes(key).translate(_COMP)[::-1]


def canonical(key, revcomp=False):
    key = as_bytes(key)
    return min(key, rc(key)) if revcomp else key


def first_truth(keys, revcomp=False):
    """first[q] = the smallest position whose key is a duplicate of keys[q] -> int64[n]"""
    seen = {}
    first = np.empty(len(keys), dtype=np.int64)
    for q, k in enumerate(keys):
        first[q] = seen.setdefault(canonical(k, revcomp), q)
    return first


def copies_truth(first):
    """copies[q] = the members of the group of q where q is its first occurrence, else 0 -> int64[n]"""
    first = np.asarray(first, dtype=np.int64)
    return np.bincount(first, minlength=first.size).astype(np.int64) if first.size else np.zeros(0, dtype=np.int64)


def dedup_truth(keys, revcomp=False, min_copies=1, max_copies=None):
    """(positions, copies of each) of the first occurrences whose group has min_copies..max_copies members, ascending"""
    first = first_truth(keys, revcomp)
    copies = copies_truth(first)
    ok = (first == np.arange(first.size)) & (copies >= min_copies)
    if max_copies is not None:
        ok &= copies <= max_copies
    pos = np.nonzero(ok)[0].astype(np.int64)
    return pos, copies[pos]


def self_check():
    assert rc("ACGTNacgtn-") == b"-nacgtNACGT" and rc("") == b"" and rc("AAC") == b"GTT"
    assert canonical("TTG", True) == b"CAA" and canonical("TTG") == b"TTG" and canonical("ACGT", True) == b"ACGT"
    keys = ["ACG", "CGT", "ACG", "", "acg", "", "CGT", "ACGA"]
    assert first_truth(keys).tolist() == [0, 1, 0, 3, 4, 3, 1, 7]
    assert first_truth(keys, True).tolist() == [0, 0, 0, 3, 4, 3, 0, 7]          # CGT is rc(ACG); acg is rc(cgt), not rc(CGT)
    assert copies_truth(first_truth(keys)).tolist() == [2, 2, 0, 2, 1, 0, 0, 1]
    pos, cp = dedup_truth(keys)
    assert pos.tolist() == [0, 1, 3, 4, 7] and cp.tolist() == [2, 2, 2, 1, 1]
    pos, cp = dedup_truth(keys, True, min_copies=2)
    assert pos.tolist() == [0, 3] and cp.tolist() == [4, 2]
    pos, cp = dedup_truth(keys, False, 1, 1)
    assert pos.tolist() == [4, 7]
    assert first_truth(["A" * 16, "A" * 17, "A" * 16]).tolist() == [0, 1, 0]
    assert first_truth([]).size == 0 and dedup_truth([])[0].size == 0
