"""CPU: the argument rules of pyfastx_amd/trim.py, the two C entries of the trimming extension (declared, exported, no
CPU fallback), and the plain-Python definition tests/trim_truth.py on hand-written reads whose answers are written out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from trim_truth import record, trim_truth, truth_kwargs


def u8(x):
    return np.frombuffer(x if isinstance(x, bytes) else x.encode("latin-1"), dtype=np.uint8)


# ------------------------------------------------------------------ argument rules
def test_defaults_and_conversions():
    from pyfastx_amd import trim
    a = trim.trim_args()
    assert a == {"clip_front": 0, "clip_tail": 0, "adapter": None, "min_overlap": 1, "err": (0, 1), "window": None,
                 "front_qual": None, "tail_qual": None}
    a = trim.trim_args(adapter="agatn", max_error_rate=0.1)
    assert a["adapter"] == b"AGATN" and a["err"] == (1, 10) and a["min_overlap"] == 3
    assert trim.trim_args(adapter=b"ACGT", min_overlap=4, max_error_rate=0)["err"] == (0, 1)
    assert trim.trim_args(adapter="A" * 64, max_error_rate="1/8")["err"] == (1, 8)
    assert trim.trim_args(window=(4, 20))["window"] == (4, 20, 1)
    assert trim.trim_args(window=(10, 22.5))["window"] == (10, 45, 2)
    assert trim.trim_args(window=(np.int64(7), 0))["window"] == (7, 0, 1)
    a = trim.trim_args(clip_front=5, clip_tail=np.int32(7), front_qual=0, tail_qual=255)
    assert (a["clip_front"], a["clip_tail"], a["front_qual"], a["tail_qual"]) == (5, 7, 0, 255)


@pytest.mark.parametrize("kw", [
    dict(adapter=""), dict(adapter="A" * 65), dict(adapter="ACGU"), dict(adapter="AC-T"), dict(adapter="ACRT"), dict(adapter=5),
    dict(adapter="ACGé"), dict(adapter="ACGT", min_overlap=0), dict(adapter="ACGT", min_overlap=5),
    dict(adapter="ACGT", min_overlap=2.0), dict(adapter="ACGT", max_error_rate=-0.1), dict(adapter="ACGT", max_error_rate=float("nan")),
    dict(window=(0, 20)), dict(window=(-3, 20)), dict(window=(4, -1)), dict(window=4), dict(window=(4, 20, 1)), dict(window=(4.0, 20)),
    dict(window=(True, 20)), dict(front_qual=-1), dict(front_qual=256), dict(front_qual=20.0), dict(tail_qual=-1), dict(tail_qual=256),
    dict(tail_qual=True), dict(clip_front=-1), dict(clip_tail=-1), dict(clip_front=1.5), dict(clip_tail="3")])
def test_value_errors(kw):
    from pyfastx_amd import trim
    with pytest.raises(ValueError):
        trim.trim_args(**kw)


def test_ids_intervals_and_batches():
    from pyfastx_amd import trim
    assert trim.check_ids(None, 5) is None
    assert trim.check_ids([4, 0, 4], 5).tolist() == [4, 0, 4] and trim.check_ids([], 5).size == 0
    for bad in ([5], [-1], [0, 9, 0]):
        with pytest.raises(IndexError, match="index out of range"):
            trim.check_ids(bad, 5)
    with pytest.raises(ValueError):
        trim.check_ids([[0, 1]], 5)
    assert trim.check_intervals(None, None, 3) == (None, None)
    for s, e in ((None, [1, 2, 3]), ([1, 2, 3], None), ([0, 0], [1, 1, 1]), ([0, 0], [1, 1])):
        with pytest.raises(ValueError):
            trim.check_intervals(s, e, 3)
    tab = {"dlen": np.array([3, 3, 3, 3, 3], dtype=np.int32), "rlen": np.array([10, 10, 100, 10, 10], dtype=np.int64)}
    # upper bounds 29 29 209 29 29
    assert list(trim.batches(tab, None, 5, 1 << 30)) == [(0, 5)]
    assert list(trim.batches(tab, None, 5, 60)) == [(0, 2), (2, 3), (3, 5)]          # a read above the bound is a batch of its own
    assert list(trim.batches(tab, None, 5, 1)) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert list(trim.batches(tab, np.array([0, 1, 3, 4, 0]), 5, 87)) == [(0, 3), (3, 5)]
    assert list(trim.batches(tab, np.array([], dtype=np.int64), 5, 87)) == []
    with pytest.raises(ValueError):
        list(trim.batches(tab, None, 5, 0))


# ------------------------------------------------------------------ the C entries
def _declared():
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", hdr))


def test_declared_and_exported():
    from pyfastx_amd import _lib
    L = _lib.lib()
    for name in ("fx_fastq_trim", "fx_fastq_format_alloc"):
        assert name in _declared() and name in _lib.SYMBOLS and hasattr(L, name)
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_fq_trim", "k_fq_format_count", "k_fq_format_scan", "k_fq_format_emit"):
        assert names.count(k) == 1, k


def test_null_arguments():
    """A null handle or output pointer: FX_EINVAL, with or without a device."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    ps, pe, n, kept, bad = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    rc = L.fx_fastq_trim(None, None, 0, 0, 0, 0, None, 0, 0, 0, 1, -1, 0, 0, 1, -1, C.byref(ps), C.byref(pe), C.byref(n), C.byref(bad))
    assert rc == _lib.FX_EINVAL and ps.value is None and pe.value is None
    rc = L.fx_fastq_format_alloc(None, None, 0, None, None, 0, C.byref(ps), C.byref(pe), C.byref(n), C.byref(kept), C.byref(bad))
    assert rc == _lib.FX_EINVAL and ps.value is None and pe.value is None


def test_no_cpu_fallback_without_gpu():
    """Without a device there is no handle to trim on: FX_EDEVICE, as tests/test_cabi.py sees it for the other entries."""
    from pyfastx_amd import _lib
    if _lib.lib().fx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.FxError) as e:
        _lib.Blob.from_bytes(b"@r\nACGT\n+\nIIII\n").fastq_trim()
    assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)


# ------------------------------------------------------------------ the definition, by hand (p = 33: 'I' 40, '5' 20, '+' 10, '#' 2)
AD = b"AGATCGGAAGAGC"
HAND = [
    # the adapter hangs off the end with exactly min_overlap letters; one letter fewer is no match
    ("ACGTACGTAGA", "I" * 11, dict(adapter=b"AGATCGG", min_overlap=3), (0, 8)),
    ("ACGTACGTAGA", "I" * 11, dict(adapter=b"AGATCGG", min_overlap=4), (0, 11)),
    # one mismatch is allowed at 10 letters (1 * 10 <= 1 * 10) and not at 9 (1 * 10 > 1 * 9)
    ("TTTTACGTACGTAG", "I" * 14, dict(adapter=b"ACGTACGTAC", min_overlap=6), (0, 4)),
    ("TTTTACGAACGTA", "I" * 13, dict(adapter=b"ACGTACGTA", min_overlap=6), (0, 13)),
    ("TTTTACGAACGTA", "I" * 13, dict(adapter=b"ACGTACGTA", min_overlap=3), (0, 8)),      # ... but its first 5 letters match exactly further on
    # N in the adapter matches any byte; N in the read matches only an N of the adapter
    ("GGACGGTGG", "I" * 9, dict(adapter=b"ACNNT"), (0, 2)),
    ("GGNCGGTGG", "I" * 9, dict(adapter=b"ACNNT"), (0, 9)),
    ("ggagatcgg", "I" * 9, dict(adapter=b"AGATCGG"), (0, 9)),                            # lower case never matches
    # a window longer than the read is the whole read
    ("ACGTAC", "IIII##", dict(window=(10, 30, 1)), (0, 0)),
    ("ACGTAC", "IIIII#", dict(window=(10, 30, 1)), (0, 6)),
    ("ACGTACGT", "IIII####", dict(window=(4, 20, 1)), (0, 3)),
    ("ACGTACGTAC", "##I#II#I##", dict(front_qual=20, tail_qual=20), (2, 8)),
    # everything trimmed away; the empty read
    ("ACGTA", "#####", dict(front_qual=20), (5, 5)),
    ("ACGTA", "#####", dict(tail_qual=20), (0, 0)),
    ("", "", dict(clip_front=2, clip_tail=2, adapter=AD, front_qual=20, window=(4, 20, 1), tail_qual=20), (0, 0)),
    # the fixed clip
    ("ACGTACGTAC", "I" * 10, dict(clip_front=3, clip_tail=4), (3, 6)),
    ("ACGTACGTAC", "I" * 10, dict(clip_front=12, clip_tail=4), (10, 10)),
    ("ACGTACGTAC", "I" * 10, dict(clip_front=2, clip_tail=20), (2, 2)),
    # the order of the steps: the clip hides the adapter's first letter; adapter, then 5' end, then 3' end
    ("AGAGGGGGGG", "I" * 10, dict(adapter=b"AGA", err=(0, 1)), (0, 0)),
    ("AGAGGGGGGG", "I" * 10, dict(adapter=b"AGA", err=(0, 1), clip_front=1), (1, 10)),
    ("ACGTACGTACAGATCGGAAG", "#IIIIIII+I" + "I" * 10, dict(adapter=AD, front_qual=20, tail_qual=20), (1, 10)),
    ("ACGTACGTACAGATCGGAAG", "#IIIIIII+I" + "I" * 10, dict(adapter=AD, front_qual=20, window=(2, 30, 1), tail_qual=20), (1, 7)),
]


@pytest.mark.parametrize("k", range(len(HAND)))
def test_truth_by_hand(k):
    s, q, kw, want = HAND[k]
    assert trim_truth(u8(s), u8(q), **kw) == want


def test_truth_kwargs_and_record():
    from pyfastx_amd import trim
    kw = truth_kwargs(trim.trim_args(adapter="agatcgg", min_overlap=3, front_qual=20, window=(4, 20), tail_qual=20, clip_front=1))
    assert kw == dict(clip_front=1, clip_tail=0, adapter=b"AGATCGG", min_overlap=3, err=(1, 10), front_qual=20, window=(4, 20, 1), tail_qual=20)
    assert record(b"@r1 d", u8("ACGTAC"), u8("IIII#I"), 1, 4) == b"@r1 d\nCGT\n+\nIII\n"
    assert record(b"@r", u8("AC"), u8("II"), 1, 1) == b"@r\n\n+\n\n"


def test_fast_truth_equals_truth():
    """The vectorised form the GPU tests use on large files, against the definition on random reads and parameters."""
    from trim_truth import trim_truth_fast
    rng = np.random.default_rng(7)
    ads = [None, b"AGATCGGAAGAGC", b"ACN", b"T", b"ACGTNNACGTACGTTTGACA"]
    for k in range(HAND.__len__()):
        s, q, kw, want = HAND[k]
        assert trim_truth_fast(u8(s), u8(q), **kw) == want
    for _ in range(1500):
        L = int(rng.integers(0, 60))
        s = np.frombuffer(b"ACGTNa", dtype=np.uint8)[rng.choice(6, L, p=[.24, .24, .24, .24, .02, .02])]
        q = np.frombuffer(b"I5+#", dtype=np.uint8)[rng.integers(0, 4, L)]
        ad = ads[int(rng.integers(0, len(ads)))]
        if ad is not None and L > 3 and rng.random() < 0.7:
            at = int(rng.integers(0, L)); m = min(len(ad), L - at)
            s = s.copy(); s[at:at + m] = np.frombuffer(ad, dtype=np.uint8)[:m]
        kw = dict(clip_front=int(rng.integers(0, 4)), clip_tail=int(rng.integers(0, 4)), adapter=ad,
                  min_overlap=1 if ad is None else int(rng.integers(1, len(ad) + 1)), err=(int(rng.integers(0, 3)), int(rng.integers(5, 12))),
                  front_qual=None if rng.random() < 0.4 else int(rng.integers(0, 45)),
                  window=None if rng.random() < 0.4 else (int(rng.integers(1, 70)), int(rng.integers(0, 90)), int(rng.integers(1, 4))),
                  tail_qual=None if rng.random() < 0.4 else int(rng.integers(0, 45)))
        assert trim_truth_fast(s, q, **kw) == trim_truth(s, q, **kw), kw
