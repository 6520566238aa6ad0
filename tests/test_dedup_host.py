"""-m "not gpu": the argument rules of Fastq.duplicates / Fastq.dedup (pyfastx_amd/dedup.py), FastQC's duplication levels on
hand-made counts, the definition tests/dedup_truth.py on hand-worked cases, and the two C entries on null pointers and without
a device."""
import ctypes as C
import os

import numpy as np
import pytest

import dedup_truth
from conftest import ROOT
from pyfastx_amd import dedup


def test_truth_self_check():
    dedup_truth.self_check()


def test_truth_hand_worked():
    t = dedup_truth
    # case, N, a first or last byte and the length all tell keys apart
    keys = ["ACGT", "acgt", "ACGN", "TCGT", "ACGA", "ACG", "ACGT"]
    assert t.first_truth(keys).tolist() == [0, 1, 2, 3, 4, 5, 0]
    # a palindrome is its own reverse complement; N maps to itself and keeps its place from the other end
    assert t.rc("GAATTC") == b"GAATTC" and t.rc("ANC") == b"GNT"
    keys = ["GAATTC", "GAATTC", "AANC", "GNTT", "GNTA", "aanc", "gntt"]
    assert t.first_truth(keys, True).tolist() == [0, 0, 2, 2, 4, 5, 5]
    assert t.first_truth(keys, False).tolist() == [0, 0, 2, 3, 4, 5, 6]
    p1, p2 = "ACGTACGTACGTACGA", "TTTTCCCCGGGGAAAA"
    assert t.first_truth([p1 + p2, p2 + p1, p1 + p2]).tolist() == [0, 1, 0]
    pos, cp = t.dedup_truth(["A", "C", "A", "A", "G", "C"], min_copies=2)
    assert pos.tolist() == [0, 1] and cp.tolist() == [3, 2]
    pos, cp = t.dedup_truth(["A", "C", "A", "A", "G", "C"], min_copies=2, max_copies=2)
    assert pos.tolist() == [1] and cp.tolist() == [2]


def test_argument_rules():
    assert dedup.check_copies() == (1, -1) and dedup.check_copies(2, None) == (2, -1)
    assert dedup.check_copies(np.int64(3), 3) == (3, 3) and dedup.check_copies(1, 10 ** 12) == (1, 10 ** 12)
    for lo in (0, -1, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            dedup.check_copies(lo)
    for hi in (0, 1, 2.0, "3", False):
        with pytest.raises(ValueError):
            dedup.check_copies(2, hi)
    assert dedup.check_hash_bits() == 0 and dedup.check_hash_bits(64) == 64 and dedup.check_hash_bits(np.int32(3)) == 3
    for b in (-1, 65, 3.0, True, None):
        with pytest.raises(ValueError):
            dedup.check_hash_bits(b)
    assert dedup.check_flag(True, "revcomp") is True and dedup.check_flag(np.bool_(False), "revcomp") is False
    for v in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            dedup.check_flag(v, "revcomp")
    # the queries are checked before any blob is touched: a blob of None will do
    with pytest.raises(IndexError):
        dedup.duplicates_blob(None, 5, ids=[0, 5])
    with pytest.raises(IndexError):
        dedup.dedup_blob(None, 5, ids=[-1])
    for kw in (dict(start=[0] * 5), dict(end=[1] * 5), dict(start=[0] * 4, end=[1] * 4), dict(ids=[1, 2], start=[0] * 5, end=[1] * 5),
               dict(revcomp=1), dict(hash_bits=65)):
        with pytest.raises(ValueError):
            dedup.duplicates_blob(None, 5, **kw)
    for kw in (dict(min_copies=0), dict(min_copies=2, max_copies=1), dict(return_counts="yes"), dict(revcomp=None), dict(start=[0] * 5)):
        with pytest.raises(ValueError):
            dedup.dedup_blob(None, 5, **kw)


def test_duplication_levels():
    lv = dedup.duplication_levels([1, 1, 1, 2, 9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000, 123456])
    assert lv["labels"] == ("1", "2", "3", "4", "5", "6", "7", "8", "9", ">10", ">50", ">100", ">500", ">1k", ">5k", ">10k")
    assert lv["groups"].tolist() == [3, 1, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2]
    assert lv["reads"].tolist() == [3, 2, 0, 0, 0, 0, 0, 0, 9, 59, 149, 599, 1499, 5999, 14999, 133456]
    assert lv["groups"].dtype == np.int64 and lv["reads"].dtype == np.int64
    assert lv["n_groups"] == 19 and lv["n_reads"] == int(lv["reads"].sum()) == 156774
    assert lv["unique_fraction"] == 19 / 156774
    one = dedup.duplication_levels(np.ones(7, dtype=np.int64))
    assert one["groups"].tolist() == [7] + [0] * 15 and one["unique_fraction"] == 1.0
    none = dedup.duplication_levels(np.zeros(0, dtype=np.int64))
    assert none["n_groups"] == none["n_reads"] == 0 and none["groups"].sum() == 0 and none["unique_fraction"] == 1.0
    big = dedup.duplication_levels(np.array([2 ** 53 + 1, 1], dtype=np.int64))
    assert big["reads"].tolist()[-1] == 2 ** 53 + 1 and big["n_reads"] == 2 ** 53 + 2              # exact: no float on the way
    for bad in ([0], [-1, 2], [[1, 2]], [1.5], ["a"]):
        with pytest.raises(ValueError):
            dedup.duplication_levels(bad)
    # from the truth's copies: 20 reads, 3 distinct
    keys = ["A"] * 12 + ["C"] * 7 + ["G"]
    pos, cp = dedup_truth.dedup_truth(keys)
    lv = dedup.duplication_levels(cp)
    assert lv["groups"][0] == 1 and lv["groups"][6] == 1 and lv["groups"][9] == 1 and lv["n_reads"] == 20 and lv["unique_fraction"] == 3 / 20


def test_declared_exported_bound():
    from pyfastx_amd import _lib
    import pyfastx_amd
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    for name, nargs in (("fx_fastq_dup_first", 12), ("fx_fastq_dedup", 15)):
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    assert _lib.FX_DUP_REVCOMP == 1 and "FX_DUP_REVCOMP = 1" in hdr
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_dd_hash", "k_dd_sort", "k_dd_verify", "k_dd_select"):
        assert names.count(k) == 1, k
    for m in ("fastq_dup_first", "fastq_dedup"):
        assert callable(getattr(_lib.Blob, m))
    for m in ("duplicates", "dedup"):
        assert callable(getattr(pyfastx_amd.Fastq, m))


def test_null_arguments():
    """A null handle or output pointer, start without end: FX_EINVAL and nothing touched, with or without a device."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)        # handle-shaped: refused before it is looked at
    one = np.zeros(1, dtype=np.int64)

    def first(h, null=None, start=None, end=None):
        o = [C.c_void_p(7), C.c_int64(-5), C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)]
        refs = [None if i == null else C.byref(x) for i, x in enumerate(o)]
        return L.fx_fastq_dup_first(h, None, 0, start, end, 0, 0, *refs), [x.value for x in o]

    def dd(h, null=None, start=None, end=None):
        o = [C.c_void_p(7), C.c_void_p(7), C.c_int64(-5), C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)]
        refs = [None if i == null else C.byref(x) for i, x in enumerate(o)]
        return L.fx_fastq_dedup(h, None, 0, start, end, 0, 0, 1, -1, *refs), [x.value for x in o]

    assert first(None) == (_lib.FX_EINVAL, [7, -5, -5, -5, -5])
    assert dd(None) == (_lib.FX_EINVAL, [7, 7, -5, -5, -5, -5])
    for i in range(5):
        rc, vals = first(fake, null=i)
        assert rc == _lib.FX_EINVAL and all(v in (7, -5) for v in vals)
    for i in (0, 2, 3, 4, 5):                                    # copies (1) may be null: not wanted
        rc, vals = dd(fake, null=i)
        assert rc == _lib.FX_EINVAL and all(v in (7, -5) for v in vals)
    for call in (first, dd):
        for kw in (dict(start=one.ctypes.data), dict(end=one.ctypes.data)):
            rc, vals = call(fake, **kw)
            assert rc == _lib.FX_EINVAL and all(v in (7, -5) for v in vals)


def test_no_cpu_fallback_without_gpu():
    """Without a device there is no handle to find duplicates on: FX_EDEVICE, as tests/test_cabi.py sees it for the other
    entries.  With a device the entries are the subject of tests/test_gpu_fastq_dedup.py."""
    from pyfastx_amd import _lib
    if _lib.lib().fx_device_count() > 0:
        return
    for call in (lambda b: dedup.duplicates_blob(b, 1), lambda b: dedup.dedup_blob(b, 1, return_counts=True)):
        with pytest.raises(_lib.FxError) as e:
            call(_lib.Blob.from_bytes(b"@r\nACGT\n+\nIIII\n"))
        assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
