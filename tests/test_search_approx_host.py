"""CPU: the argument rules of Fasta.search_approx / search_approx_counts (pyfastx_amd/search.py: compile_approx), the C entry
point behind them (fx_fasta_search_approx) and the oracle the GPU tests compare with (search_approx_truth.py) on cases
whose rows are written out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from search_approx_truth import truth


def test_compile_mode_and_budget():
    from pyfastx_amd import _lib, search
    mode, fwd, rev, d, mask = search.compile_approx("garyn", 2, None, "both", degenerate=True)
    assert mode == _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS | _lib.FX_SEARCH_DEGENERATE
    assert (fwd, rev, d, mask) == (b"GARYN", b"NRYTC", 2, 0)
    mode, fwd, rev, d, mask = search.compile_approx(b"GAATTC", 0, None, "+")     # exact, '+' only: no GPU call for the '-' pattern
    assert (mode, fwd, rev, d, mask) == (_lib.FX_SEARCH_PLUS, b"GAATTC", None, 0, 0)
    assert search.compile_approx("N" * 64, 8, None, "-", degenerate=True)[3] == 8
    assert search.compile_approx("AC", np.int64(1), None, "+")[3] == 1
    assert search.ApproxHits._fields == ("ids", "starts", "stops", "strands", "mismatches")


def test_compile_anchor():
    from pyfastx_amd import search
    guide = "ACGTACGTACGTACGTACGTNGG"
    comp = lambda anchor: search.compile_approx(guide, 3, anchor, "both", degenerate=True)[4]
    assert comp(slice(20, 23)) == 0b111 << 20
    assert comp(slice(20, None)) == 0b111 << 20 and comp(slice(-3, None)) == 0b111 << 20
    assert comp([0]) == 1 and comp([22]) == 1 << 22
    assert comp([22, 0, 5, 5]) == (1 << 22) | (1 << 5) | 1
    assert comp(np.array([1, 2])) == 0b110 and comp(range(3)) == 0b111 and comp(()) == 0 and comp(None) == 0
    assert comp(slice(None)) == (1 << 23) - 1
    assert search.compile_approx("A" * 64, 1, [63], "+")[4] == 1 << 63


@pytest.mark.parametrize("pattern,d,kw", [
    ("GAATTC", -1, {}), ("GAATTC", 9, {}), ("ACGTACGTACGT", 9, {}), ("GAATTC", 6, {}), ("A", 1, {}), ("GAATTC", 1.0, {}),
    ("GAATTC", "1", {}), ("GAATTC", None, {}), ("GAATTC", True, {}),
    ("GAATTC", 1, {"anchor": [6]}), ("GAATTC", 1, {"anchor": [-1]}), ("GAATTC", 1, {"anchor": [0, 64]}),
    ("GAATTC", 1, {"anchor": [1.5]}), ("GAATTC", 1, {"anchor": ["1"]}), ("GAATTC", 1, {"anchor": 3}), ("GAATTC", 1, {"anchor": "012"}),
    ("GAATTC", 1, {"strand": "+-"}), ("GAATTC", 1, {"strand": None}),
    ("", 0, {}), ("A" * 65, 1, {}), ("GA TC", 1, {}), ("GA\nTC", 1, {}), ("GAXTC", 1, {"degenerate": True}),
])
def test_value_errors(pattern, d, kw):
    from pyfastx_amd import search
    kw = dict({"strand": "+"}, **kw)
    with pytest.raises(ValueError):
        search.compile_approx(pattern, d, **kw)


def test_budget_limits_accepted():
    from pyfastx_amd import search
    assert search.compile_approx("GAATTC", 5, None, "+")[3] == 5             # L - 1
    assert search.compile_approx("ACGTACGTA", 8, None, "+")[3] == 8          # 8 = L - 1 = the cap
    assert search.compile_approx("ACGTACGTACGT", 8, None, "+")[3] == 8


def test_entry_point_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fx_fasta_search_approx\s*\(", hdr)
    assert "fx_fasta_search_approx" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "fx_fasta_search_approx") and len(L.fx_fasta_search_approx.argtypes) == 16
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    assert "k_asearch_count" in names and "k_asearch_emit" in names


def test_entry_point_refuses_bad_arguments():
    """What the numbers alone decide is refused before the handle is looked at, so each check shows without a device: the
    message says which one spoke."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    n = C.c_int64(-1)
    out = [C.c_void_p() for _ in range(4)]
    pat = b"ACGTACGTAC"

    def call(plen, d, anchor, mode=_lib.FX_SEARCH_PLUS):
        rc = L.fx_fasta_search_approx(None, pat * 7, pat * 7, plen, mode, d, anchor, None, 0, 10, C.byref(out[0]), C.byref(out[1]),
                                      C.byref(out[2]), C.byref(out[3]), C.byref(n), None)
        return rc, L.fx_last_error().decode()

    rc, msg = call(10, 2, 0b11)
    assert rc == _lib.FX_EINVAL and "null argument" in msg                   # all numbers fine: the null handle
    for plen in (0, 65, -3):
        rc, msg = call(plen, 0, 0)
        assert rc == _lib.FX_EINVAL and "pattern length" in msg, plen
    for plen, d in ((10, -1), (10, 9), (10, 10), (4, 4), (1, 1), (64, 9)):
        rc, msg = call(plen, d, 0)
        assert rc == _lib.FX_EINVAL and "max_mismatch" in msg, (plen, d)
    for plen, anchor in ((10, 1 << 10), (10, 1 << 63), (63, 1 << 63), (1, 2)):
        rc, msg = call(plen, 0, anchor)
        assert rc == _lib.FX_EINVAL and "anchor" in msg, (plen, anchor)
    for plen, d, anchor in ((10, 8, (1 << 10) - 1), (64, 8, 1 << 63), (9, 8, 0), (1, 0, 1)):     # the limits themselves pass these checks
        rc, msg = call(plen, d, anchor)
        assert rc == _lib.FX_EINVAL and "null argument" in msg, (plen, d, anchor)
    assert n.value == -1 and not any(o.value for o in out)                 # nothing was touched


def test_truth_exact_by_hand():
    # distances of the windows of record 0 to ACGT, by start: 0 4 4 4 1 4 4 (the 1: ACGA, its mismatch at position 3)
    seqs = ["ACGTACGAAC", "ACG", ""]
    assert truth(seqs, "ACGT", 0, strand="+") == [(0, 0, 4, "+", 0)]
    assert truth(seqs, "ACGT", 1, strand="+") == [(0, 0, 4, "+", 0), (0, 4, 8, "+", 1)]
    assert truth(seqs, "ACGT", 3, strand="+") == [(0, 0, 4, "+", 0), (0, 4, 8, "+", 1)]
    assert truth(seqs, "ACGT", 1, anchor=[3], strand="+") == [(0, 0, 4, "+", 0)]                      # position 3 held: ACGA goes
    assert truth(seqs, "ACGT", 1, anchor=slice(0, 3), strand="+") == [(0, 0, 4, "+", 0), (0, 4, 8, "+", 1)]
    # to AGG: 1 2 3 3 1 2 3 2 in record 0, and 1 in record 1, a record of exactly L letters; record 2 is empty
    assert truth(seqs, "AGG", 1, strand="+") == [(0, 0, 3, "+", 1), (0, 4, 7, "+", 1), (1, 0, 3, "+", 1)]


def test_truth_both_strands_by_hand():
    # the '-' pattern of AAG is CTT.  Distances by start      to AAG: 0 2 3 3 3 3 3 2 1 1   (AAT at 8: position 2, ATG at 9: 1)
    #                                                         to CTT: 3 3 2 0 2 2 1 3 2 2   (CTA at 6: position 2)
    seqs = ["AAGCTTCTAATG"]
    assert truth(seqs, "AAG", 0, rev="CTT") == [(0, 0, 3, "+", 0), (0, 3, 6, "-", 0)]
    assert truth(seqs, "AAG", 1, rev="CTT") == [(0, 0, 3, "+", 0), (0, 3, 6, "-", 0), (0, 6, 9, "-", 1), (0, 8, 11, "+", 1), (0, 9, 12, "+", 1)]
    # the anchor is given for AAG and mirrored for CTT: letter j of AAG is letter 2 - j of CTT
    assert truth(seqs, "AAG", 1, anchor=[0], rev="CTT") == [(0, 0, 3, "+", 0), (0, 3, 6, "-", 0), (0, 8, 11, "+", 1), (0, 9, 12, "+", 1)]
    assert truth(seqs, "AAG", 1, anchor=[1], rev="CTT") == [(0, 0, 3, "+", 0), (0, 3, 6, "-", 0), (0, 6, 9, "-", 1), (0, 8, 11, "+", 1)]
    assert truth(seqs, "AAG", 1, anchor=[2], rev="CTT") == [(0, 0, 3, "+", 0), (0, 3, 6, "-", 0), (0, 6, 9, "-", 1), (0, 9, 12, "+", 1)]
    assert truth(seqs, "AAG", 1, anchor=[2], strand="-", rev="CTT") == [(0, 3, 6, "-", 0), (0, 6, 9, "-", 1)]
    # a palindrome: both strands at one start, '+' first
    assert truth(["GAATTC", "GAATTG"], "GAATTC", 1, rev="GAATTC") == [(0, 0, 6, "+", 0), (0, 0, 6, "-", 0), (1, 0, 6, "+", 1), (1, 0, 6, "-", 1)]


def test_truth_degenerate_by_hand():
    # N takes every IUPAC letter in either case, G takes G / g alone: R (A or G) is no subset of G, n is none, '-' matches
    # nothing, not even N.  Distances to NNGG by start: 0 1 2 1 1 1 0 1 1 1 (at 9, G-GG: the '-' under an N)
    seqs = ["acGGTRGnGG-GG"]
    assert truth(seqs, "NNGG", 0, strand="+", degenerate=True) == [(0, 0, 4, "+", 0), (0, 6, 10, "+", 0)]
    assert truth(seqs, "nngg", 1, strand="+", degenerate=True) == [
        (0, 0, 4, "+", 0), (0, 1, 5, "+", 1), (0, 3, 7, "+", 1), (0, 4, 8, "+", 1), (0, 5, 9, "+", 1), (0, 6, 10, "+", 0), (0, 7, 11, "+", 1),
        (0, 8, 12, "+", 1), (0, 9, 13, "+", 1)]
    # the GG held: the clean sites, and the one whose mismatch lies under an N
    assert truth(seqs, "NNGG", 1, anchor=slice(2, 4), strand="+", degenerate=True) == [(0, 0, 4, "+", 0), (0, 6, 10, "+", 0), (0, 9, 13, "+", 1)]
    # '-' of NNGG is CCNN; lower case and U in the text.  To NNGG: 2 2 2 1 0, to CCNN: 0 1 2 2 1
    assert truth(["ccAAUCgg"], "NNGG", 1, degenerate=True) == [
        (0, 0, 4, "-", 0), (0, 1, 5, "-", 1), (0, 3, 7, "+", 1), (0, 4, 8, "+", 0), (0, 4, 8, "-", 1)]
