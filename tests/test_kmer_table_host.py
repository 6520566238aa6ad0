"""-m "not gpu": the argument rules of kmer_table, the KmerTable object on hand-built arrays and the self-check of the
definition (tests/kmer_table_truth.py)."""
import numpy as np
import pytest

import kmer_table_truth
from pyfastx_amd import kmer


def test_truth_self_check():
    kmer_table_truth.self_check()


def test_argument_rules():
    assert kmer.MAX_TABLE_K == 31
    assert kmer.check_table(31) == (31, 1, 0)
    assert kmer.check_table(np.int64(21), np.int32(3), 1 << 20) == (21, 3, 1 << 20)
    assert kmer.check_table(1, max_bytes=None)[2] == 0
    for k in (0, 32, -1, 21.0, True, "21", None):
        with pytest.raises(ValueError):
            kmer.check_table(k)
    for m in (0, -3, 1.0, True, None, "2"):
        with pytest.raises(ValueError):
            kmer.check_table(21, min_count=m)
    for b in (0, 4096, (1 << 20) - 1, 1e9, True, "1G"):
        with pytest.raises(ValueError):
            kmer.check_table(21, max_bytes=b)
    assert kmer.check_k(13) == 13                              # the dense bound is where it was
    with pytest.raises(ValueError):
        kmer.check_k(14)


def test_kmer_code():
    assert kmer.kmer_code("ACGT", 4) == 0b00011011 and kmer.kmer_code(b"acgt", 4) == 0b00011011
    assert kmer.kmer_code("T" * 31, 31) == 4 ** 31 - 1
    assert kmer.kmer_string(kmer.kmer_code("GATTACAGATTACAGATTACAGATTACAGAT", 31), 31) == "GATTACAGATTACAGATTACAGATTACAGAT"
    for bad, k in (("ACG", 4), ("ACGTA", 4), ("", 1), ("ACGN", 4), ("AC-T", 4), ("ACGU", 4)):
        with pytest.raises(ValueError):
            kmer.kmer_code(bad, k)


def test_table_plain():
    k = 3
    codes = np.array([kmer.kmer_code(s, k) for s in ("AAA", "ACG", "CGT", "TTT")], dtype=np.int64)
    t = kmer.KmerTable(k, False, codes, np.array([5, 1, 1, 2], dtype=np.int64), n_windows=9, n_parts=1)
    assert len(t) == 4 and t.k == 3 and not t.canonical and t.n_windows == 9 and t.n_parts == 1
    assert t.codes.dtype == np.int64 and t.counts.dtype == np.int64
    assert t.count("AAA") == 5 and t.count("aaa") == 5 and t.count("TTT") == 2 and t.count("GGG") == 0 and t.count("TTG") == 0
    assert t.count(int(codes[1])) == 1 and isinstance(t.count("ACG"), int)
    got = t.count(np.array([0, 1, 63, 62, int(codes[2])]))
    assert got.dtype == np.int64 and got.tolist() == [5, 0, 2, 0, 1]
    assert t.count(np.zeros(0, dtype=np.int64)).shape == (0,)
    assert t.spectrum().tolist() == [0, 2, 1, 0, 0, 1] and t.spectrum().dtype == np.int64
    assert t.strings() == ["AAA", "ACG", "CGT", "TTT"] and t.strings(1, 3) == ["ACG", "CGT"] and t.strings(3) == ["TTT"]
    for bad in ("AA", "AAAA", "AAN"):
        with pytest.raises(ValueError):
            t.count(bad)


def test_table_canonical_and_empty():
    k = 3
    # canonical codes only: AAA (= TTT), ACG (= CGT)
    codes = np.array([kmer.kmer_code("AAA", k), kmer.kmer_code("ACG", k)], dtype=np.int64)
    t = kmer.KmerTable(k, True, codes, np.array([7, 2], dtype=np.int64))
    assert t.n_windows == 9
    assert t.count("TTT") == 7 and t.count("AAA") == 7 and t.count("CGT") == 2 and t.count("ACG") == 2 and t.count("CCC") == 0
    assert t.count(np.array([63, 0, kmer.kmer_code("CGT", k), kmer.kmer_code("GGG", k)])).tolist() == [7, 7, 2, 0]
    e = kmer.KmerTable(31, False, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0, 0)
    assert len(e) == 0 and e.count("A" * 31) == 0 and e.count(np.array([0, 5])).tolist() == [0, 0]
    assert e.spectrum().tolist() == [0] and e.strings() == []
    big = kmer.KmerTable(31, True, np.array([0], dtype=np.int64), np.array([3], dtype=np.int64))
    assert big.count("T" * 31) == 3 and big.count(4 ** 31 - 1) == 3
