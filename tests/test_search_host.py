"""CPU: the pattern rules of Fasta.search_all / search_counts (pyfastx_amd/search.py) and the C entry point behind them."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def test_iupac_sets():
    from pyfastx_amd import search
    want = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
            "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
    for k, v in want.items():
        assert search.iupac_set(k) == frozenset(v) == search.iupac_set(k.lower())
    assert sorted(search.IUPAC) == sorted(want)
    with pytest.raises(KeyError):
        search.iupac_set("X")


@pytest.mark.parametrize("p,rc", [("RGATCY", "RGATCY"), ("GANTC", "GANTC"), ("ACGTRYKM", "KMRYACGT"), ("acgu", "ACGT"),
                                  ("BDHVSWN", "NWSBDHV")])
def test_iupac_revcomp(p, rc):
    from pyfastx_amd import search
    assert search.iupac_revcomp(p) == rc
    # the complement of a set is the set of the complements
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for a, b in zip(p.upper(), reversed(rc)):
        assert {comp[x] for x in search.iupac_set(a)} == set(search.iupac_set(b))


def test_degenerate_compile():
    from pyfastx_amd import _lib, search
    mode, fwd, rev = search.compile_pattern("garyn", "both", degenerate=True)
    assert mode == _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS | _lib.FX_SEARCH_DEGENERATE
    assert (fwd, rev) == (b"GARYN", b"NRYTC")
    mode, fwd, rev = search.compile_pattern("GAATTC", "+", degenerate=True)
    assert mode == _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_DEGENERATE and rev is None
    mode, fwd, rev = search.compile_pattern(b"GAATTC", "+")            # exact, '+' only: no GPU call for the '-' pattern
    assert (mode, fwd, rev) == (_lib.FX_SEARCH_PLUS, b"GAATTC", None)


@pytest.mark.parametrize("pattern,kw", [
    ("", {}), ("A" * 65, {}), ("A" * 65, {"degenerate": True}),
    ("GA TC", {}), ("GA\nTC", {}), ("GA\rTC", {}), ("GA\tTC", {}),
    ("GAXTC", {"degenerate": True}), ("GA-TC", {"degenerate": True}), ("GA1TC", {"degenerate": True}),
    ("GAATTC", {"strand": "+-"}), ("GAATTC", {"strand": 1}), ("GAATTC", {"strand": None}),
])
def test_value_errors(pattern, kw):
    from pyfastx_amd import search
    with pytest.raises(ValueError):
        search.compile_pattern(pattern, **kw)


def test_lengths_accepted():
    from pyfastx_amd import search
    assert search.compile_pattern("A", "+")[1] == b"A"
    assert search.compile_pattern("N" * 64, "both", degenerate=True)[1] == b"N" * 64


def test_entry_point_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fx_fasta_search\s*\(", hdr)
    assert "fx_fasta_search" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "fx_fasta_search") and len(L.fx_fasta_search.argtypes) == 13


def test_entry_point_refuses_bad_arguments():
    """Argument checks come before any device work: a null handle, a length outside 1..64, no strand."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    n = C.c_int64(-1)
    out = [C.c_void_p() for _ in range(3)]
    args = lambda plen, mode: (None, b"ACGT", b"ACGT", plen, mode, None, 0, 10, C.byref(out[0]), C.byref(out[1]),
                               C.byref(out[2]), C.byref(n), None)
    assert L.fx_fasta_search(*args(4, _lib.FX_SEARCH_PLUS)) == _lib.FX_EINVAL
    assert n.value == -1                                   # a null handle: nothing is touched
    import pyfastx_amd.search  # noqa: F401  (importable without a GPU)
