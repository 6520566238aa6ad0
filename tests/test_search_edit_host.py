"""CPU: the oracle the GPU tests of Fasta.search_edit compare with (search_edit_truth.py) against a second, naive definition
on short strings, the properties of report = "best", edits = 0 against a plain overlapping find, the argument rules of
pyfastx_amd/search.py (compile_edit) and the C entry point behind them (fx_fasta_search_edit)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from search_edit_truth import best_filter, strand_rows, truth


def _ed(a, b):
    """Levenshtein distance, the textbook table in plain Python."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def _naive(s, q, k, report):
    """[(start, stop, edits)] from the definition alone: ed over ALL spans that end at e, the shortest span that has the minimum."""
    D = {}
    for e in range(len(s)):
        d, m = min((_ed(q, s[e + 1 - m:e + 1]), m) for m in range(0, e + 2))
        if d <= k:
            D[e] = (d, m)
    ends = {e: d for e, (d, m) in D.items()}
    keep = sorted(D) if report == "all" else sorted(
        e for e in D if (e - 1 not in ends or ends[e - 1] > ends[e]) and (e + 1 not in ends or ends[e + 1] >= ends[e]))
    return [(e + 1 - D[e][1], e + 1, D[e][0]) for e in keep]


def _cases():
    rng = np.random.default_rng(12)
    for _ in range(400):
        al = "AC" if rng.random() < 0.5 else "ACN"
        L = int(rng.integers(1, 7))
        q = "".join(rng.choice(list(al), L))
        s = "".join(rng.choice(list(al), int(rng.integers(0, 13))))
        yield s, q, int(rng.integers(0, min(3, L - 1) + 1))
    yield "ACGTACGT", "ACGT", 0
    yield "AAAAAAAAAAAA", "AAA", 2
    yield "ACGACGT", "ACGT", 1
    yield "", "AC", 1
    yield "A", "ACGT", 3


def test_truth_against_naive_definition():
    n = 0
    for s, q, k in _cases():
        for report in ("all", "best"):
            want = _naive(s, q, k, report)
            assert strand_rows(s, q, k, False, report) == want, (s, q, k, report)
            n += len(want)
            for a, b, d in want:
                assert len(q) - k <= b - a <= len(q) + k and b - a >= 1 and _ed(q, s[a:b]) == d
    assert n > 1000                                            # the cases are not all empty


def test_best_is_subset_and_covers_every_stretch():
    for s, q, k in _cases():
        every, best = strand_rows(s, q, k, False, "all"), strand_rows(s, q, k, False, "best")
        assert set(best) <= set(every)
        stops, kept = [r[1] for r in every], {r[1] for r in best}
        i = 0
        while i < len(stops):                                 # maximal stretches of consecutive ends
            j = i
            while j + 1 < len(stops) and stops[j + 1] == stops[j] + 1:
                j += 1
            assert kept & set(stops[i:j + 1]), (s, q, k, stops[i:j + 1])
            i = j + 1
    assert best_filter({3: 1, 4: 1, 5: 1}) == [3]                          # a plateau keeps its leftmost end
    assert sorted(best_filter({3: 2, 4: 1, 5: 1, 6: 2, 7: 1, 9: 0})) == [4, 7, 9]
    assert sorted(best_filter({1: 0, 2: 1, 3: 0})) == [1, 3]


def test_no_edits_is_overlapping_find():
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGT"), 300)) for _ in range(3)] + ["AAAAAAAA", "", "ACACACACA"]
    for p, rev in (("AC", "GT"), ("A", "T"), ("ACA", "TGT"), ("GATC", "GATC"), ("AAAA", "TTTT")):
        want = []
        for i, s in enumerate(seqs):
            hits = [(a + len(p), k, a) for k, q in enumerate((p, rev)) for a in range(len(s) - len(p) + 1) if s.startswith(q, a)]
            want += [(i, a, b, "+-"[k], 0) for b, k, a in sorted(hits)]
        assert truth(seqs, p, 0, report="all", rev=rev) == want
        assert [r for r in want if r[3] == "+"] == truth(seqs, p, 0, strand="+", report="all")


def test_degenerate_and_strands():
    rows = truth(["TTGANTCTTGAATCTT"], "GANTC", 1, degenerate=True, report="best")
    # GANTC (its own reverse complement) matches GANTC and GAATC: N in the pattern takes any base, N in the text only an N;
    # the ends one letter to either side cost one edit and lose to the dip between them
    assert rows == [(0, 2, 7, "+", 0), (0, 2, 7, "-", 0), (0, 9, 14, "+", 0), (0, 9, 14, "-", 0)]
    # the text's N is no subset of the pattern's A: one edit
    assert truth(["TTGANTCTT"], "GAATC", 1, strand="+", degenerate=True, report="best") == [(0, 2, 7, "+", 1)]


# ------------------------------------------------------------------ the argument rules
def test_compile_edit():
    from pyfastx_amd import _lib, search
    mode, fwd, rev, k, rep = search.compile_edit("garyn", 2, "both", degenerate=True)
    assert mode == _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS | _lib.FX_SEARCH_DEGENERATE
    assert (fwd, rev, k, rep) == (b"GARYN", b"NRYTC", 2, _lib.FX_EDIT_BEST)
    assert search.compile_edit(b"GAATTC", 0, "+", report="all") == (_lib.FX_SEARCH_PLUS, b"GAATTC", None, 0, _lib.FX_EDIT_ALL)
    assert search.compile_edit("N" * 64, 8, "-", degenerate=True)[3] == 8
    assert search.compile_edit("AC", np.int64(1), "+")[3] == 1
    assert search.compile_edit("GAATTC", 5, "+")[3] == 5 and search.compile_edit("ACGTACGTA", 8, "+")[3] == 8
    assert search.EditHits._fields == ("ids", "starts", "stops", "strands", "edits")


@pytest.mark.parametrize("pattern,k,kw,exc", [
    ("GAATTC", -1, {}, ValueError), ("GAATTC", 9, {}, ValueError), ("ACGTACGTACGT", 9, {}, ValueError), ("GAATTC", 6, {}, ValueError),
    ("A", 1, {}, ValueError), ("GAATTC", 1.0, {}, TypeError), ("GAATTC", "1", {}, TypeError), ("GAATTC", None, {}, TypeError),
    ("GAATTC", True, {}, TypeError), ("GAATTC", 1, {"report": "first"}, ValueError), ("GAATTC", 1, {"report": 1}, TypeError),
    ("GAATTC", 1, {"report": None}, TypeError), ("GAATTC", 1, {"strand": "+-"}, ValueError), ("GAATTC", 1, {"strand": None}, ValueError),
    ("", 0, {}, ValueError), ("A" * 65, 1, {}, ValueError), ("GA TC", 1, {}, ValueError), ("GA\nTC", 1, {}, ValueError),
    ("GAXTC", 1, {"degenerate": True}, ValueError),
])
def test_argument_errors_before_the_library(pattern, k, kw, exc, monkeypatch):
    from pyfastx_amd import _lib, search

    def no_library(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "revcomp_bytes", no_library)
    kw = dict({"strand": "both"}, **kw)
    with pytest.raises(exc):
        search.compile_edit(pattern, k, **kw)
    with pytest.raises(exc):
        search.edit_blob(None, pattern, k, **kw)
    with pytest.raises(exc):
        search.edit_count_blob(None, pattern, k, **kw)


def test_entry_point_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fx_fasta_search_edit\s*\(", hdr)
    assert "fx_fasta_search_edit" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "fx_fasta_search_edit") and len(L.fx_fasta_search_edit.argtypes) == 18
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_esearch_count", "k_esearch_emit", "k_esearch_best", "k_esearch_start"):
        assert k in names


def test_entry_point_refuses_bad_arguments():
    """What the numbers alone decide is refused before the handle is looked at, so each check shows without a device: the
    message says which one spoke."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    n, ne = C.c_int64(-1), C.c_int64(-1)
    out = [C.c_void_p() for _ in range(5)]
    pat = b"ACGTACGTAC"
    both = _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS
    for plen, k, report, word in ((0, 0, 0, "pattern length"), (65, 1, 0, "pattern length"), (-3, 0, 1, "pattern length"),
                                  (10, -1, 0, "max_edits"), (10, 9, 1, "max_edits"), (6, 6, 0, "max_edits"), (1, 1, 1, "max_edits"),
                                  (10, 2, 2, "report"), (10, 2, -1, "report"), (10, 2, 0, "null argument"), (64, 8, 1, "null argument")):
        rc = L.fx_fasta_search_edit(None, pat * 7, pat * 7, plen, both, k, report, None, 0, 10, *[C.byref(p) for p in out],
                                    C.byref(n), C.byref(ne), None)
        assert rc == _lib.FX_EINVAL, (plen, k, report)
        assert word in L.fx_last_error().decode(), (plen, k, report, L.fx_last_error())
        assert n.value == 0 and ne.value == 0 and all(p.value is None for p in out)
