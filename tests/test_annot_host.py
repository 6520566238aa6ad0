"""CPU: the truth of the region / window / class-run tests pinned on hand-written literals, the argument rules of
pyfastx_amd/annot.py, RegionStats' derived figures, and the new entries' declarations -- nothing here needs a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import annot_truth as T
from conftest import ROOT


# ------------------------------------------------------------------ the truth, on literals
def test_truth_counts_literal():
    s = "NNacgTNN-Ryn"
    # A: a; C: c; G: g; T: T; N: N N N N n; other: - R y; masked: a c g y n (five lower-case letters)
    assert T.region_counts(s, 0, len(s)) == [1, 1, 1, 1, 5, 3, 5]
    assert sum(T.region_counts(s, 0, len(s))[:6]) == len(s)
    assert T.region_counts(s, 2, 6) == [1, 1, 1, 1, 0, 0, 3]
    assert T.region_counts(s, 5, 5) == [0] * 7
    assert T.region_counts("UuXx*-", 0, 6) == [0, 0, 0, 0, 0, 6, 2]           # U is not T
    assert T.region_counts("A\xe9\xff", 0, 3) == [1, 0, 0, 0, 0, 2, 0]        # bytes >= 128 are other, never masked


def test_truth_runs_literal():
    s = "NNacgTNN-Ryn"
    assert T.class_runs(s, b"Nn", 1) == [(0, 2), (6, 8), (11, 12)]
    assert T.class_runs(s, b"Nn", 2) == [(0, 2), (6, 8)]
    masked = bytes(range(ord("a"), ord("z") + 1))
    assert T.class_runs(s, masked, 1) == [(2, 5), (10, 12)]
    assert T.class_runs(s, masked, 2) == [(2, 5), (10, 12)]
    assert T.class_runs(s, masked, 3) == [(2, 5)]
    assert T.class_runs(s, "RY", 1) == [(9, 10)]                              # as written: y is not in it
    assert T.class_runs("NNNN", b"Nn", 1) == [(0, 4)]
    assert T.class_runs("", b"Nn", 1) == []
    assert T.class_runs("A-]^N", "-]^", 1) == [(1, 4)]                        # letters that mean something to a regex


def test_truth_windows_literal():
    assert T.windows(10, 4, 3, True) == [(0, 4), (3, 7), (6, 10), (9, 10)]
    assert T.windows(10, 4, 3, False) == [(0, 4), (3, 7), (6, 10)]
    assert T.windows(0, 4, 3, True) == []
    assert T.windows(3, 4, 4, True) == [(0, 3)] and T.windows(3, 4, 4, False) == []
    assert T.windows(8, 4, 4, True) == T.windows(8, 4, 4, False) == [(0, 4), (4, 8)]
    assert T.windows(5, 2, 9, True) == [(0, 2)]


# ------------------------------------------------------------------ argument rules
def test_window_rules():
    from pyfastx_amd import annot
    assert annot.check_windows(5) == (5, 5)                                   # step=None tiles
    assert annot.check_windows(5, 2) == (5, 2)
    assert annot.check_windows(np.int64(7), np.int32(3)) == (7, 3)
    for w, s in ((0, None), (-1, 1), (5, 0), (5, -2), (1.5, None), (5, 2.0), ("5", None), (True, None)):
        with pytest.raises(ValueError):
            annot.check_windows(w, s)
    with pytest.raises(ValueError):
        annot.check_windows(5, 5, max_windows=-1)


def test_window_count_matches_truth():
    from pyfastx_amd import annot
    for slen in (0, 1, 3, 4, 5, 9, 10, 11, 60, 61):
        for w, s in ((1, 1), (4, 3), (5, 5), (5, 2), (5, 9), (slen + 3, slen + 3)):
            for partial in (True, False):
                assert int(annot.count_windows([slen], w, s, partial)[0]) == len(T.windows(slen, w, s, partial)), (slen, w, s, partial)


def test_run_rules():
    from pyfastx_amd import annot
    assert annot.check_runs(1, 10) == (1, 10)
    for m in (0, -3, 1.0, "1", None, False):
        with pytest.raises(ValueError):
            annot.check_runs(m)
    with pytest.raises(ValueError):
        annot.check_runs(1, -1)
    for kind in ("", "x", "n", "NN", b"N", None, 5):                           # one distinct letter is read as a kind, and no such kind exists
        with pytest.raises(ValueError):
            annot.class_set(kind)
    with pytest.raises(ValueError):
        annot.class_set(letters="")
    with pytest.raises(ValueError):
        annot.class_set(letters=b"")
    with pytest.raises(ValueError):
        annot.class_set("N", letters="N")
    with pytest.raises(ValueError):
        annot.class_set(letters="Ł")


def _members(bits):
    return {c for c in range(256) if bits[c >> 3] >> (c & 7) & 1}


def test_byte_set_encoding():
    from pyfastx_amd import annot
    b = annot.byte_set(b"A")
    assert len(b) == 32 and b[8] == 0x02 and sum(b) == 2                       # 'A' = 65: bit 1 of byte 8
    assert _members(annot.byte_set("RY")) == {ord("R"), ord("Y")}             # as written: no case folding
    assert _members(annot.byte_set(bytes([0, 255]))) == {0, 255}
    assert _members(annot.class_set("N")) == {ord("N"), ord("n")}
    assert _members(annot.class_set("masked")) == set(range(ord("a"), ord("z") + 1))
    assert _members(annot.class_set("unmasked")) == set(range(ord("A"), ord("Z") + 1))
    assert _members(annot.class_set("RYry")) == {ord(c) for c in "RYry"}
    assert _members(annot.class_set(letters="n")) == {ord("n")}               # one letter goes through letters=
    assert _members(annot.class_set(b"AT")) == {65, 84}


# ------------------------------------------------------------------ RegionStats
def test_region_stats_properties():
    from pyfastx_amd import annot
    counts = np.array([[1, 1, 1, 1, 5, 3, 5],           # the literal above
                       [3, 0, 1, 0, 0, 0, 0],           # AAAG
                       [0, 0, 0, 0, 4, 2, 0],           # no A C G T at all
                       [2, 0, 0, 2, 0, 0, 4],           # no G + C
                       [0, 0, 0, 0, 0, 0, 0]],          # empty
                      dtype=np.int64)
    z = np.zeros(5, dtype=np.int64)
    r = annot.RegionStats(z, z, z, counts)
    assert r.columns == ("A", "C", "G", "T", "N", "other", "masked") and len(r) == 5
    assert r.length.tolist() == [12, 4, 6, 4, 0]
    gc, skew, mf = r.gc_content, r.gc_skew, r.masked_fraction
    assert gc.dtype == np.float64 and skew.dtype == np.float64 and mf.dtype == np.float64
    assert gc[0] == 50.0 and gc[1] == 25.0 and math.isnan(gc[2]) and gc[3] == 0.0 and math.isnan(gc[4])
    assert skew[0] == 0.0 and skew[1] == 1.0 and math.isnan(skew[2]) and math.isnan(skew[3]) and math.isnan(skew[4])
    assert mf[0] == 5 / 12 and mf[1] == 0.0 and mf[2] == 0.0 and mf[3] == 1.0 and math.isnan(mf[4])


def test_class_runs_object(tmp_path):
    from pyfastx_amd import annot
    r = annot.ClassRuns(np.array([0, 0, 2]), np.array([0, 6, 3]), np.array([2, 8, 10]), names=lambda i: "chr%d" % i)
    assert r.lengths.tolist() == [2, 2, 7] and len(r) == 3
    p = str(tmp_path / "runs.bed")
    r.write_bed(p)
    assert open(p).read() == "chr0\t0\t2\nchr0\t6\t8\nchr2\t3\t10\n"


# ------------------------------------------------------------------ the C entries
ENTRIES = {"fx_fasta_rank_build": 1, "fx_fasta_rank_free": 1, "fx_fasta_region_counts": 8, "fx_fasta_window_counts": 12,
           "fx_fasta_class_runs": 11}


def test_entries_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs, name
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_an_rank", "k_an_scan", "k_an_region", "k_an_runs_count", "k_an_runs_scan", "k_an_runs_emit"):
        assert k in names


def test_entries_without_a_device_or_a_handle():
    """Without a device every entry answers FX_EDEVICE before it looks at an argument; with one, a null handle is FX_EINVAL."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    want = _lib.FX_EDEVICE if L.fx_device_count() <= 0 else _lib.FX_EINVAL
    out = [C.c_void_p() for _ in range(4)]
    n, m = C.c_int64(0), C.c_int64(0)
    assert L.fx_fasta_rank_build(None) == want
    assert L.fx_fasta_rank_free(None) == want
    assert L.fx_fasta_region_counts(None, _lib.FX_HOST, 0, None, None, None, None, C.byref(n)) == want
    assert L.fx_fasta_window_counts(None, None, 0, 5, 5, 1, 10, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(out[3]),
                                    C.byref(n)) == want
    bits = (C.c_ubyte * 32)()
    assert L.fx_fasta_class_runs(None, bits, 1, None, 0, 10, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(n), C.byref(m)) == want
