"""The definition of the sparse k-mer tables (Fasta.kmer_table, Fastq.kmer_table) in plain numpy: the codes of kmer_truth that
occur at least once, ascending, with their counts.  It imports kmer_truth only."""
import numpy as np

from kmer_truth import CODE, as_bytes, counted_codes, revcomp_code


def table_of_codes(codes, min_count=1):
    """-> (codes int64 ascending, counts int64) of the entries whose count is at least min_count."""
    codes = np.asarray(codes, dtype=np.int64)
    u, c = np.unique(codes, return_counts=True)
    keep = c >= min_count
    return u[keep].astype(np.int64), c[keep].astype(np.int64)


def table_truth(seqs, k, canonical=False, min_count=1):
    """The table of all the sequences together (a sequence listed twice counts twice)."""
    codes = [counted_codes(s, k, canonical) for s in seqs]
    return table_of_codes(np.concatenate(codes) if codes else np.zeros(0, dtype=np.int64), min_count)


def flat_codes(flat, rec_start, k, canonical=False):
    """The counted codes of records laid back to back in `flat` (record r begins at rec_start[r], ascending): rolling codes;
    the k - 1 windows in front of every later record start would cross into it and are left out."""
    c = CODE[as_bytes(flat)].astype(np.uint8)
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    code = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        w = c[j:j + n]
        bad |= w > 3
        code *= 4
        code += w & 3
    for s in np.asarray(rec_start, dtype=np.int64):
        if s > 0:
            bad[max(s - k + 1, 0):min(s, n)] = True
    code = code[~bad]
    return np.minimum(code, revcomp_code(code, k)) if canonical else code


def self_check():
    """k = 31 by hand: 32 letters hold two windows; the first is A * 31 = code 0, the second A * 30 + C = code 1; the reverse
    complement of A * 31 is T * 31 = 4**31 - 1, of A * 30 + C it is G + T * 30 = 2 * 4**30 + (4**30 - 1)."""
    s = "A" * 31 + "C"
    u, c = table_truth([s], 31)
    assert u.tolist() == [0, 1] and c.tolist() == [1, 1] and u.dtype == np.int64
    assert int(revcomp_code(np.int64(0), 31)) == 4 ** 31 - 1 and int(revcomp_code(np.int64(1), 31)) == 3 * 4 ** 30 - 1
    t = "T" * 31
    u, c = table_truth([s, t, "acgtn" * 20], 31, canonical=True)
    assert u.tolist() == [0, 1] and c.tolist() == [2, 1]                  # T * 31 folds onto A * 31; no window of 31 without an n
    u, c = table_truth([s, t], 31)
    assert u.tolist() == [0, 1, 4 ** 31 - 1] and u[-1] == (1 << 62) - 1 and c.tolist() == [1, 1, 1]
    u, c = table_truth([s, s, t], 31, min_count=2)
    assert u.tolist() == [0, 1] and c.tolist() == [2, 2]
    assert np.array_equal(flat_codes(s + t, [0, 32], 31), np.array([0, 1, 4 ** 31 - 1]))
    assert table_truth([], 5)[0].size == 0 and table_truth(["ACG"], 4)[0].size == 0
