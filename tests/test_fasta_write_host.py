"""CPU: the plain-Python definition tests/fasta_write_truth.py on hand-written records whose bytes are written out, the
argument rules and host helpers of pyfastx_amd/fasta_out.py, and the C entry of the FASTA writer (declared, exported, its
null checks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import fasta_write_truth as T

SEQS = ["ACGTacgtNN", "", "AaCcGgTtRYKMryBD"]


def one(query, minus=False, width=60, mask=(), mode="none", char="N", upper=False, min_len=0, header="h"):
    buf, offs = T.records(SEQS, [header], [query], [minus], width, mask, mode, char, upper, min_len)
    assert offs == [0, len(buf)]
    return buf


# ------------------------------------------------------------------ the definition, by hand
@pytest.mark.parametrize("kw, want", [
    (dict(query=(0, None, None)), b">h\nACGTacgtNN\n"),
    (dict(query=(0, None, None), width=4), b">h\nACGT\nacgt\nNN\n"),
    (dict(query=(0, None, None), width=5), b">h\nACGTa\ncgtNN\n"),                       # the last line is full: one newline
    (dict(query=(0, None, None), width=0), b">h\nACGTacgtNN\n"),
    (dict(query=(0, 2, 5), width=1), b">h\nG\nT\na\n"),
    (dict(query=(0, None, None), width=11), b">h\nACGTacgtNN\n"),                        # width > L
    (dict(query=(1, None, None), header="empty record"), b">empty record\n"),            # L = 0: no sequence line
    (dict(query=(0, 3, 3), header=""), b">\n"),
    (dict(query=(0, None, None), upper=True), b">h\nACGTACGTNN\n"),
    (dict(query=(0, None, None), mask=[(0, 2, 6)], mode="soft"), b">h\nACgtacgtNN\n"),
    (dict(query=(0, None, None), mask=[(0, 2, 6)], mode="upper"), b">h\nACGTACgtNN\n"),
    (dict(query=(0, None, None), mask=[(0, 2, 6), (0, 9, 10)], mode="hard"), b">h\nACNNNNgtNN\n"),
    (dict(query=(0, None, None), mask=[(0, 2, 6)], mode="hard", char="x", width=3), b">h\nACx\nxxx\ngtN\nN\n"),
    (dict(query=(0, None, None), mask=[(0, 2, 6)], mode="none"), b">h\nACGTacgtNN\n"),
    (dict(query=(0, None, None), mask=[(2, 0, 16)], mode="hard"), b">h\nACGTacgtNN\n"),  # rows of another record
    (dict(query=(0, 1, 5), mask=[(0, 0, 2), (0, 4, 9)], mode="hard"), b">h\nNGTN\n"),    # rows reach past both ends of the interval
    (dict(query=(0, 0, 4), minus=True), b">h\nACGT\n"),                                  # its own reverse complement
    (dict(query=(0, 2, 8), minus=True), b">h\nacgtAC\n"),
    # minus strand with a soft mask: forward GTac, rows [3, 5) turn T into t and leave a -> Gtac; the complement keeps the case
    # -> Catg; reversed -> gtaC
    (dict(query=(0, 2, 6), minus=True, mask=[(0, 3, 5)], mode="soft"), b">h\ngtaC\n"),
    (dict(query=(0, 2, 6), minus=True, mask=[(0, 3, 5)], mode="hard"), b">h\ngNNC\n"),   # hard, then complemented: N stays N
    (dict(query=(0, 2, 6), minus=True, mask=[(0, 3, 5)], mode="hard", char="A"), b">h\ngTTC\n"),
    (dict(query=(2, None, None), minus=True, width=8), b">h\nHVryKMRY\naAcCgGtT\n"),     # IUPAC pairs, case kept
    (dict(query=(2, None, None), upper=True, minus=True, mask=[(2, 0, 2)], mode="soft", width=0), b">h\nHVRYKMRYAACCGGtt\n"),
    (dict(query=(0, 2, 5), min_len=4), b""),                                             # L < min_len: no bytes
    (dict(query=(0, 2, 6), min_len=4), b">h\nGTac\n"),
    (dict(query=(1, None, None), min_len=1), b""),
])
def test_truth_by_hand(kw, want):
    assert one(**kw) == want


def test_truth_offsets_and_order():
    buf, offs = T.records(SEQS, ["a", "b", "c", "d"], [(0, 0, 4), (1, None, None), (0, 0, 2), (2, 14, 16)], [False, False, True, True],
                          3, [], "none", "N", False, 1)
    assert buf == b">a\nACG\nT\n" + b"" + b">c\nGT\n" + b">d\nHV\n"
    assert offs == [0, 9, 9, 15, 21]


def test_writer_and_parser_round_trip():
    recs = [("r1 first", "ACGTACGTAC"), ("r2", ""), ("r3", "acgtn")]
    for eol in (b"\n", b"\r\n"):
        for last in ("full", "unterminated"):
            data = T.write_fasta(recs, 4, eol, last)
            assert T.parse_fasta(data) == [(h.encode(), s.encode()) for h, s in recs]
    assert T.write_fasta(recs, 4) == b">r1 first\nACGT\nACGT\nAC\n>r2\n>r3\nacgt\nn\n"
    assert T.write_fasta(recs, 4, b"\r\n", "unterminated").endswith(b"acgt\r\nn")
    assert T.parse_fasta(b">x y\nAC GT\n\nA\n") == [(b"x y", b"ACGTA")]


# ------------------------------------------------------------------ merge_intervals
def rows(*r):
    a = np.array(r, dtype=np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def merged(*r):
    from pyfastx_amd import fasta_out
    out = fasta_out.merge_intervals(*rows(*r))
    assert all(c.dtype == np.int64 for c in out)
    return list(zip(*(c.tolist() for c in out)))


def test_merge_intervals():
    assert merged() == []
    assert merged((0, 5, 5), (1, 7, 3)) == []                                            # empty rows are dropped
    assert merged((0, 10, 20)) == [(0, 10, 20)]
    assert merged((0, 10, 20), (0, 0, 5)) == [(0, 0, 5), (0, 10, 20)]                    # unsorted
    assert merged((0, 10, 20), (0, 15, 30)) == [(0, 10, 30)]                             # overlapping
    assert merged((0, 10, 20), (0, 20, 30)) == [(0, 10, 30)]                             # touching
    assert merged((0, 10, 20), (0, 21, 30)) == [(0, 10, 20), (0, 21, 30)]
    assert merged((0, 0, 100), (0, 10, 20), (0, 30, 40), (0, 99, 101)) == [(0, 0, 101)]  # a long row reaches over short ones
    assert merged((0, 0, 100), (0, 10, 20), (0, 150, 160)) == [(0, 0, 100), (0, 150, 160)]
    assert merged((2, 5, 9), (0, 5, 9), (2, 0, 5), (1, 0, 50), (0, 50, 60)) == [(0, 5, 9), (0, 50, 60), (1, 0, 50), (2, 0, 9)]
    assert merged((0, 0, 50), (1, 10, 20)) == [(0, 0, 50), (1, 10, 20)]                  # the reach of a record ends with it
    assert merged((3, 1 << 40, (1 << 40) + 5), (3, (1 << 40) + 5, (1 << 40) + 9)) == [(3, 1 << 40, (1 << 40) + 9)]
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 4, 300)
    a = rng.integers(0, 1000, 300)
    b = a + rng.integers(0, 30, 300)
    cover = np.zeros((4, 1040), dtype=bool)
    for r, x, y in zip(ids, a, b):
        cover[r, x:y] = True
    got = merged(*zip(ids.tolist(), a.tolist(), b.tolist()))
    back = np.zeros_like(cover)
    for r, x, y in got:
        assert y > x and not back[r, max(x - 1, 0):y + 1].any()                          # disjoint and not touching
        back[r, x:y] = True
    assert (back == cover).all() and got == sorted(got)
    from pyfastx_amd import fasta_out
    with pytest.raises(ValueError):
        fasta_out.merge_intervals([0, 1], [0], [1])


def test_mask_rows_take_objects_and_tuples():
    from pyfastx_amd import fasta_out

    class Rows:
        ids, starts, stops = np.array([1, 0]), np.array([4, 0]), np.array([9, 3])
    for m in (Rows(), (Rows.ids, Rows.starts, Rows.stops), [[1, 0], [4, 0], [9, 3]]):
        out = fasta_out.mask_rows(m)
        assert [c.tolist() for c in out] == [[0, 1], [0, 4], [3, 9]]
    assert fasta_out.mask_rows(None) is None
    for bad in (5, ([0], [1]), "ab"):
        with pytest.raises(ValueError):
            fasta_out.mask_rows(bad)


# ------------------------------------------------------------------ argument rules, auto headers
def test_argument_rules():
    from pyfastx_amd import fasta_out as fo
    assert [fo.check_width(w) for w in (0, 1, 60, np.int64(80))] == [0, 1, 60, 80]
    for bad in (-1, 1.5, "60", True, None):
        with pytest.raises(ValueError):
            fo.check_width(bad)
    assert [fo.check_mask_mode(m) for m in ("none", "soft", "hard", "upper")] == [0, 1, 2, 3]
    for bad in ("SOFT", "lower", 1, None, b"soft"):
        with pytest.raises(ValueError):
            fo.check_mask_mode(bad)
    assert fo.check_mask_char("N") == 78 and fo.check_mask_char(b"x") == 120 and fo.check_mask_char("\xff") == 255
    for bad in ("", "NN", b"", 78, None, "€"):
        with pytest.raises(ValueError):
            fo.check_mask_char(bad)
    assert fo.strand_flags(None, 3).tolist() == [False] * 3 and fo.strand_flags("-", 2).tolist() == [True, True]
    assert fo.strand_flags("+", 2).tolist() == [False, False]
    assert fo.strand_flags(["+", "-", 1, 0], 4).tolist() == [False, True, True, False]
    assert fo.strand_flags(np.array([0, 1, ord("+"), ord("-")]), 4).tolist() == [False, True, False, True]
    for bad, n in (("x", 1), (["+", "?"], 2), (["+"], 2)):
        with pytest.raises(ValueError):
            fo.strand_flags(bad, n)
    assert fo.check_intervals(None, None, 2) == (None, None)
    for s, e in ((None, [1, 2]), ([1, 2], None), ([0], [1, 1]), ([[0, 0]], [[1, 1]])):
        with pytest.raises(ValueError):
            fo.check_intervals(s, e, 2)


def test_auto_and_custom_headers():
    from pyfastx_amd import fasta_out as fo
    h = fo.auto_headers(["chr1", "chr1", "s 2"], [0, 99, 5], [10, 200, 6], [False, True, False])
    assert h == [b"chr1:1-10", b"chr1:100-200(-)", b"s 2:6-6"]                           # the `pyfastx subseq` form, 1-based inclusive
    buf, offs = fo.pack_headers(h, 3)
    assert buf.tobytes() == b"chr1:1-10chr1:100-200(-)s 2:6-6" and offs.tolist() == [0, 9, 24, 31]
    buf, offs = fo.pack_headers(["", b"ab", "é"], 3)
    assert buf.tobytes() == b"ab\xc3\xa9" and offs.tolist() == [0, 0, 2, 4]
    buf, offs = fo.pack_headers([], 0)
    assert offs.tolist() == [0] and buf.size >= 1
    for bad, n in (("auto2", 1), (["a"], 2), ([5], 1), (b"ab", 2)):
        with pytest.raises(ValueError):
            fo.pack_headers(bad, n)


def test_size_bound_and_batches():
    from pyfastx_amd import fasta_out as fo
    L = np.array([0, 1, 60, 61, 120])
    assert fo.size_bound(3, L, 60).tolist() == [5, 7, 66, 68, 127]
    assert fo.size_bound(np.array([0, 1, 2, 3, 4]), L, 0).tolist() == [2, 5, 65, 67, 127]
    for w in (0, 1, 7, 60):                                                              # the bound IS the size the truth writes
        for n in (0, 1, 6, 7, 8, 59, 60, 61):
            assert fo.size_bound(1, n, w) == len(T.record("h", b"A" * n, w))
    b = np.array([29, 29, 209, 29, 29])
    assert list(fo.batches(b, 1 << 30)) == [(0, 5)]
    assert list(fo.batches(b, 60)) == [(0, 2), (2, 3), (3, 5)]                           # a query above the bound goes alone
    assert list(fo.batches(b, 1)) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert list(fo.batches(np.zeros(0, dtype=np.int64), 10)) == []
    with pytest.raises(ValueError):
        list(fo.batches(b, 0))


# ------------------------------------------------------------------ the C entry
def test_declared_exported_and_null_arguments():
    from pyfastx_amd import _lib, fasta_out
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    for name in ("fx_fasta_format_alloc", "fx_fasta_format_tile"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.PROTOTYPES and hasattr(L, name)
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_fa_format_size", "k_fa_format_scan", "k_fa_format_emit"):
        assert names.count(k) == 1, k
    t = fasta_out.tile()
    assert t >= 4096 and t % 4096 == 0                       # whole 16-byte chunks for every lane of a workgroup
    dst, offs, kept, bases, bad = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    outs = (C.byref(dst), C.byref(offs), C.byref(kept), C.byref(bases), C.byref(bad))
    rc = L.fx_fasta_format_alloc(None, 0, None, None, None, 0, None, 60, None, None, 0, None, None, None, 0, 78, 0, *outs)
    assert rc == _lib.FX_EINVAL and dst.value is None and offs.value is None
    for hole in range(5):                                    # a null output pointer
        o = list(outs)
        o[hole] = None
        rc = L.fx_fasta_format_alloc(None, 0, None, None, None, 0, None, 60, None, None, 0, None, None, None, 0, 78, 0, *o)
        assert rc == _lib.FX_EINVAL
