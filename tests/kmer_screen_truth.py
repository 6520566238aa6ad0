"""The definition of k-mer screening (Fastq.kmer_hits / screen, Fasta.kmer_hits) in plain numpy: per sequence the counted codes
of kmer_truth, looked up in a set of codes with np.isin; the screen's predicate in Python ints.  It imports kmer_truth only."""
import numpy as np

from kmer_truth import counted_codes


def hits_of_codes(per_seq, set_codes):
    """per_seq: the counted codes of every sequence (a list of int64 arrays) -> (n_windows, n_hits), int64, one row each."""
    set_codes = np.asarray(set_codes, dtype=np.int64)
    nw = np.array([c.size for c in per_seq], dtype=np.int64)
    flat = np.concatenate(per_seq) if len(per_seq) else np.zeros(0, dtype=np.int64)
    upto = np.concatenate(([0], np.cumsum(np.isin(flat, set_codes))))       # hits among the first j codes of all sequences
    off = np.concatenate(([0], np.cumsum(nw)))
    return nw, (upto[off[1:]] - upto[off[:-1]]).astype(np.int64)


def hits_truth(seqs, k, set_codes, canonical=False):
    """-> (n_windows, n_hits), int64, one row per sequence: its valid windows and how many of them are in set_codes (a window
    that occurs twice counts twice)."""
    return hits_of_codes([counted_codes(s, k, canonical) for s in seqs], set_codes)


def passes(n_windows, n_hits, min_hits=1, num=0, den=0, invert=False):
    """The predicate of the screen for one query, in Python ints; den = 0: the ratio is not asked."""
    w, h = int(n_windows), int(n_hits)
    ok = h >= int(min_hits) and (den == 0 or h * int(den) >= int(num) * w)
    return ok != bool(invert)


def screen_truth(n_windows, n_hits, min_hits=1, num=0, den=0, invert=False):
    """The ascending positions of the queries that pass -> int64."""
    return np.array([q for q, (w, h) in enumerate(zip(n_windows, n_hits)) if passes(w, h, min_hits, num, den, invert)], dtype=np.int64)


def self_check():
    nw, nh = hits_truth(["ACGTA", "ACNGT", "AC", "acgt", "ACGACG"], 3, [0b000110, 0b011011])      # ACG, CGT
    assert nw.tolist() == [3, 0, 0, 2, 4] and nh.tolist() == [2, 0, 0, 2, 2]
    nw, nh = hits_truth(["ACGTA"], 3, [0b000110], canonical=True)                                   # ACG = CGT reversed: both windows fold onto it
    assert nw.tolist() == [3] and nh.tolist() == [2]
    assert passes(4, 2, 1, 1, 2) and not passes(4, 1, 1, 1, 2) and passes(0, 0, 0, 1, 2) and not passes(0, 0, 1, 1, 2)
    assert passes(4, 1, 1, 1, 2, invert=True) and passes(3, 0, 0) and not passes(3, 0, 1)
    assert screen_truth([4, 4, 0], [2, 1, 0], 0, 1, 2).tolist() == [0, 2]
