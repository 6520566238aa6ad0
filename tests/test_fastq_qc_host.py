"""CPU: the argument rules of Fastq.read_stats / cycle_profile / select (pyfastx_amd/qc.py) and the C entry points behind them."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = {"fx_fastq_read_stats": 14, "fx_fastq_cycle_hist": 5, "fx_fastq_select": 12}


@pytest.mark.parametrize("x,want", [(30, (30, 1)), (0, (0, 1)), (0.05, (1, 20)), (0.1, (1, 10)), (27.5, (55, 2)),
                                    ("1/3", (1, 3)), (Fraction(7, 9), (7, 9)), (1 / 3, (1, 3)), (0.3333, (1, 3)),
                                    (0.12345, (119, 964)), (np.float32(0.25), (1, 4)), (np.int64(20), (20, 1))])
def test_ratio(x, want):
    """Fraction(x) limited to a denominator <= 1000 (0.12345 -> 119/964, the closest such fraction)."""
    from pyfastx_amd import qc
    num, den = qc.as_ratio(x)
    assert (num, den) == want
    assert 1 <= den <= qc.MAX_DENOMINATOR


@pytest.mark.parametrize("x", [-1, -0.001, float("nan"), float("inf"), None, "x"])
def test_ratio_refused(x):
    from pyfastx_amd import qc
    with pytest.raises(ValueError):
        qc.as_ratio(x)


def test_select_args():
    from pyfastx_amd import qc
    assert qc.select_args() == {"low_qual": 20, "min_len": -1, "max_len": -1, "mean_qual": (0, 0), "low_frac": (0, 0), "max_other": -1}
    a = qc.select_args(min_len=50, max_len=50, min_mean_qual=30, max_low_frac=0.05, max_other=0, low_qual=0)
    assert a == {"low_qual": 0, "min_len": 50, "max_len": 50, "mean_qual": (30, 1), "low_frac": (1, 20), "max_other": 0}
    assert qc.select_args(min_mean_qual=0)["mean_qual"] == (0, 1)          # asked for, and passes everything non-negative
    assert qc.select_args(low_qual=255)["low_qual"] == 255


@pytest.mark.parametrize("kw", [
    {"min_len": -1}, {"max_len": -5}, {"max_other": -1}, {"min_mean_qual": -0.5}, {"max_low_frac": -0.1},
    {"min_len": 11, "max_len": 10}, {"low_qual": 256}, {"low_qual": -1}, {"low_qual": 2.5}, {"min_len": 1.5},
])
def test_select_args_refused(kw):
    from pyfastx_amd import qc
    with pytest.raises(ValueError):
        qc.select_args(**kw)


def test_cycles_and_low_qual():
    from pyfastx_amd import qc
    assert qc.check_cycles(1) == 1 and qc.check_cycles(65536) == 65536 and qc.check_cycles(np.int32(150)) == 150
    for bad in (0, 65537, -3, 1.5, None, True):
        with pytest.raises(ValueError):
            qc.check_cycles(bad)
    assert qc.check_low_qual(0) == 0 and qc.check_low_qual(255) == 255
    for bad in (256, -1, 20.0, None):
        with pytest.raises(ValueError):
            qc.check_low_qual(bad)


def test_cycle_profile_views():
    from pyfastx_amd import qc
    qual = np.zeros((3, 256), dtype=np.int64)
    qual[0, 33 + 40] = 3
    qual[0, 33 + 20] = 1
    qual[1, 33 + 2] = 2
    base = np.zeros((3, 5), dtype=np.int64)
    p = qc.CycleProfile(qual, base, np.array([4, 2, 0]), 33)
    assert p.cycles == 3 and p.qual_scores.shape == (3, 94) and p.qual_scores.base is qual
    assert p.qual_scores[0, 40] == 3 and p.qual_scores[1, 2] == 2
    m = p.mean_qual
    assert m[0] == 35.0 and m[1] == 2.0 and np.isnan(m[2])
    assert qc.CycleProfile(qual, base, np.array([4, 2, 0]), 64).qual_scores[0, 73 - 64] == 3


def test_entry_points_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    for m in ("fastq_read_stats", "fastq_cycle_hist", "fastq_select"):
        assert callable(getattr(_lib.Blob, m))


def test_entry_points_refuse_null_arguments():
    """Argument checks come before any device work: a null handle or a null output gives FX_EINVAL and touches nothing."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    cols = [C.c_void_p(7) for _ in range(7)]
    n, bad = C.c_int64(-5), C.c_int64(-5)
    assert L.fx_fastq_read_stats(None, None, 0, 33, 20, *[C.byref(c) for c in cols], C.byref(n), C.byref(bad)) == _lib.FX_EINVAL
    assert (n.value, bad.value) == (-5, -5) and all(c.value == 7 for c in cols)
    a, b, d = C.c_void_p(7), C.c_void_p(7), C.c_void_p(7)
    assert L.fx_fastq_cycle_hist(None, 150, C.byref(a), C.byref(b), C.byref(d)) == _lib.FX_EINVAL
    assert (a.value, b.value, d.value) == (7, 7, 7)
    ids, k = C.c_void_p(7), C.c_int64(-5)
    assert L.fx_fastq_select(None, 33, 20, -1, -1, 0, 0, 0, 0, -1, C.byref(ids), C.byref(k)) == _lib.FX_EINVAL
    assert (ids.value, k.value) == (7, -5)
    # a handle-shaped argument with null outputs: refused before the handle is looked at
    fake = C.create_string_buffer(8)
    assert L.fx_fastq_select(C.cast(fake, C.c_void_p), 33, 20, -1, -1, 0, 0, 0, 0, -1, None, None) == _lib.FX_EINVAL
    assert L.fx_fastq_cycle_hist(C.cast(fake, C.c_void_p), 150, None, None, None) == _lib.FX_EINVAL
    import pyfastx_amd.qc  # noqa: F401  (importable without a GPU)
