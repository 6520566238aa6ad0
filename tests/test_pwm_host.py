"""CPU: the Pwm object (pyfastx_amd/pwm.py) -- quantisation, geometry, the exact score distribution against brute force,
JASPAR text, the argument rules -- the two C entry points behind Fasta.pwm_scan / pwm_best (fx_fasta_pwm_scan,
fx_fasta_pwm_best) as far as they answer without a device, and the oracle of the GPU tests (pwm_truth.py) on rows written
out by hand."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pwm_truth import NO_SCORE, truth


def _pwm():
    from pyfastx_amd import pwm
    return pwm


def _rand_ints(rng, W, lo=-60, hi=60):
    return rng.integers(lo, hi + 1, (W, 4)).astype(np.int32)


# ------------------------------------------------------------------ quantisation and geometry
def test_from_counts_by_hand():
    """Columns of 8 sequences, pseudocount 0.8, uniform background: a count c gives log2(((c + 0.2) / 8.8) / 0.25), that is
    log2(3.7273) = 1.8981 for c = 8, log2(1 / 11) = -3.4594 for c = 0 and log2(1) = 0 for c = 2."""
    Pwm = _pwm().Pwm
    p = Pwm.from_counts([[8, 0, 2], [0, 8, 2], [0, 0, 2], [0, 0, 2]])
    assert p.ints.dtype == np.int32 and p.ints.shape == (3, 4) and len(p) == 3
    assert p.ints.tolist() == [[190, -346, -346, -346], [-346, 190, -346, -346], [0, 0, 0, 0]]
    assert (p.max_score, p.min_score, p.scale) == (380, -692, 100)
    assert Pwm.from_counts([[8, 0, 2], [0, 8, 2], [0, 0, 2], [0, 0, 2]], scale=10).ints[0].tolist() == [19, -35, -35, -35]
    # a skewed background: the same count is worth less where the letter is common.  A: log2((8.4 / 8.8) / 0.5) = 0.9329,
    # C: log2((0.08 / 8.8) / 0.1) = -3.4594 (the pseudocount follows the background), G: the same, T: log2(1 / 11)
    q = Pwm.from_counts([[8], [0], [0], [0]], background=(0.5, 0.1, 0.1, 0.3))
    assert q.ints.tolist() == [[93, -346, -346, -346]]
    assert Pwm.from_log_odds([[1.234, -2.5, 0, 0.004]], scale=100).ints.tolist() == [[123, -250, 0, 0]]
    assert Pwm.from_ints([[1, 2, 3, 4]]).scale == 1
    assert Pwm.from_log_odds([[1.5, 0, 0, 0]]).to_float([150, -75]).tolist() == [1.5, -0.75]


def test_revcomp_and_score_at():
    Pwm = _pwm().Pwm
    rng = np.random.default_rng(1)
    for W in (1, 2, 7, 64):
        p = Pwm.from_ints(_rand_ints(rng, W))
        r = p.revcomp()
        assert (r.ints == p.ints[::-1, ::-1]).all() and (r.revcomp().ints == p.ints).all()
        assert (r.max_score, r.min_score) == (p.max_score, p.min_score)
        assert p.score_at(0.0) == p.min_score and p.score_at(1.0) == p.max_score
        assert p.min_score <= p.score_at(0.7) <= p.max_score
    # GAATTC as a 0/1 matrix is its own reverse complement
    pal = np.zeros((6, 4), dtype=np.int32)
    pal[np.arange(6), ["ACGT".index(c) for c in "GAATTC"]] = 1
    assert (Pwm.from_ints(pal).revcomp().ints == pal).all()
    assert Pwm.from_ints([[0, 10, 0, 0], [-3, 0, 4, 0]]).score_at(0.5) == 6         # ceil(-3 + 0.5 * 17)


# ------------------------------------------------------------------ the score distribution against all 4^W windows
def _brute(ints, bg):
    """{score: probability} and {score: number of windows} over every window of W letters."""
    W = ints.shape[0]
    prob, count = {}, {}
    for w in itertools.product(range(4), repeat=W):
        s = int(sum(int(ints[j, c]) for j, c in enumerate(w)))
        count[s] = count.get(s, 0) + 1
        prob[s] = prob.get(s, 0.0) + float(np.prod([bg[c] for c in w]))
    return prob, count


@pytest.mark.parametrize("W", [1, 3, 6])
def test_distribution_uniform_exact(W):
    Pwm = _pwm().Pwm
    ints = _rand_ints(np.random.default_rng(10 + W), W, -9, 9)
    p = Pwm.from_ints(ints)
    _, count = _brute(ints, [0.25] * 4)
    scores, probs = p.distribution()
    assert scores.tolist() == list(range(p.min_score, p.max_score + 1)) and probs.shape == scores.shape
    total = 4 ** W
    assert [x * total for x in probs.tolist()] == [float(count.get(s, 0)) for s in scores.tolist()]      # multiples of 4^-W: exact
    at_least = lambda t: sum(n for s, n in count.items() if s >= t)
    for t in range(p.min_score - 2, p.max_score + 3):
        assert p.pvalue(t) == at_least(t) / total, t
    # the smallest t whose tail count is <= p * 4^W
    for k in sorted({0, 1, 2, total // 7, total // 2, total - 1, total} | {at_least(t) for t in range(p.min_score, p.max_score + 1)}):
        want = next(t for t in range(p.min_score, p.max_score + 2) if at_least(t) <= k)
        assert p.threshold_for_pvalue(k / total) == want, k
        if k:                                                # just below a tail probability: that score no longer passes
            want = next(t for t in range(p.min_score, p.max_score + 2) if at_least(t) <= k - 0.5)
            assert p.threshold_for_pvalue((k - 0.5) / total) == want, k
    assert p.threshold_for_pvalue(1.0) == p.min_score
    assert p.threshold_for_pvalue(0.5 / total) == p.max_score + 1 and p.threshold_for_pvalue(0.0) == p.max_score + 1


@pytest.mark.parametrize("W", [1, 3, 6])
def test_distribution_skewed(W):
    Pwm = _pwm().Pwm
    bg = (0.4, 0.1, 0.15, 0.35)
    ints = _rand_ints(np.random.default_rng(20 + W), W, -9, 9)
    p = Pwm.from_ints(ints, background=bg)
    prob, _ = _brute(ints, bg)
    scores, probs = p.distribution()
    for s, x in zip(scores.tolist(), probs.tolist()):
        assert math.isclose(x, prob.get(s, 0.0), rel_tol=1e-9, abs_tol=0.0), s
    for t in range(p.min_score, p.max_score + 2):
        assert math.isclose(p.pvalue(t), sum(v for s, v in prob.items() if s >= t), rel_tol=1e-9, abs_tol=0.0), t
    assert p.pvalue(p.min_score - 1) == 1.0 and p.pvalue(p.max_score + 1) == 0.0


# ------------------------------------------------------------------ JASPAR text
JASPAR = """>MA0000.1 hand
A  [ 8  0  2  1 ]
C  [ 0  8  2  1 ]
G  [ 0  0  2  5 ]
T  [ 0  0  2  1 ]
"""
COUNTS = [[8, 0, 2, 1], [0, 8, 2, 1], [0, 0, 2, 5], [0, 0, 2, 1]]


def test_jaspar_text():
    Pwm = _pwm().Pwm
    want = Pwm.from_counts(COUNTS)
    p = Pwm.from_jaspar(JASPAR)
    assert (p.ints == want.ints).all() and p.name == "MA0000.1 hand" and p.scale == 100
    bare = "8 0 2 1\n0 8 2 1\n\n0 0 2 5\n0 0 2 1"
    assert (Pwm.from_jaspar(bare).ints == want.ints).all() and Pwm.from_jaspar(bare).name is None
    assert (Pwm.from_jaspar(JASPAR.replace("[", "").replace("]", "")).ints == want.ints).all()
    assert (Pwm.from_jaspar(JASPAR.encode(), scale=10).ints == Pwm.from_counts(COUNTS, scale=10).ints).all()


@pytest.mark.parametrize("text", [
    "", ">only a header\n", "A [ 1 2 ]\nC [ 1 2 ]\nG [ 1 2 ]\n",                                  # too few rows
    "A [ 1 2 ]\nC [ 1 2 ]\nG [ 1 2 ]\nT [ 1 ]\n",                                                 # ragged
    "A [ 1 2 ]\nG [ 1 2 ]\nC [ 1 2 ]\nT [ 1 2 ]\n",                                               # rows out of order
    "A [ 1 x ]\nC [ 1 2 ]\nG [ 1 2 ]\nT [ 1 2 ]\n", "A [ 1 2\nC [ 1 2 ]\nG [ 1 2 ]\nT [ 1 2 ]\n",  # no number, no closing bracket
    JASPAR + JASPAR, "A []\nC []\nG []\nT []\n", "A [ -1 2 ]\nC [ 1 2 ]\nG [ 1 2 ]\nT [ 1 2 ]\n",
])
def test_jaspar_malformed(text):
    with pytest.raises(ValueError):
        _pwm().Pwm.from_jaspar(text)


# ------------------------------------------------------------------ errors
def test_value_errors():
    pwm = _pwm()
    Pwm = pwm.Pwm
    ok = [[1, 2, 3, 4]] * 3
    for bad in ([[1, 2, 3]] * 4, [1, 2, 3, 4], [[[1, 2, 3, 4]]], np.zeros((0, 4)), np.zeros((65, 4)), "ACGT", [[1, 2, 3, 40000]],
                [[-32768, 0, 0, 0]], [[0.5, 0, 0, 0]]):
        with pytest.raises(ValueError):
            Pwm.from_ints(bad)
    assert len(Pwm.from_ints(np.zeros((64, 4)))) == 64 and Pwm.from_ints([[32767, -32767, 0, 0]]).max_score == 32767
    for bad in (np.zeros((3, 5)), np.zeros((65, 4)), [[float("nan"), 0, 0, 0]], [[400.0, 0, 0, 0]]):    # 400 * 100 > 32767
        with pytest.raises(ValueError):
            Pwm.from_log_odds(bad)
    for bad in (np.ones((3, 4)), np.ones((4, 0)), np.ones((4, 65)), [[1, 2], [1, 2], [1, -2], [1, 2]], np.ones(4)):
        with pytest.raises(ValueError):
            Pwm.from_counts(bad)
    with pytest.raises(ValueError):
        Pwm.from_counts([[5], [0], [0], [0]], pseudocount=0)                      # log2(0)
    with pytest.raises(ValueError):
        Pwm.from_counts([[10 ** 6], [0], [0], [0]], scale=10 ** 4)                # quantised beyond +-32767
    for bg in ((0.25, 0.25, 0.25), (0.5, 0.5, 0.0, 0.0), (0.3, 0.3, 0.3, 0.3), (0.5, 0.5, 0.5, -0.5), "abcd", None):
        with pytest.raises(ValueError):
            Pwm.from_counts(np.ones((4, 3)), background=bg)
        with pytest.raises(ValueError):
            Pwm.from_ints(ok, background=bg)
    p = Pwm.from_ints(ok)
    with pytest.raises(ValueError):
        p.threshold_for_pvalue(1.5)
    for s in ("x", None, "+-"):
        with pytest.raises(ValueError):
            pwm.strand_mode(s)
    with pytest.raises(ValueError):
        pwm.resolve_min_score(np.array(ok), min_score=1)                          # a bare array is no Pwm


def test_exactly_one_threshold():
    pwm = _pwm()
    p = pwm.Pwm.from_log_odds([[1.0, -1.0, 0.5, 0.0]] * 4, scale=100)
    for kw in ({}, {"min_score": 1, "threshold": 1.0}, {"min_score": 1, "pvalue": 0.1}, {"threshold": 1.0, "pvalue": 0.1},
               {"min_score": 1, "threshold": 1.0, "pvalue": 0.1}):
        with pytest.raises(ValueError, match="exactly one"):
            pwm.resolve_min_score(p, **kw)
    for bad in (1.5, "3", True):
        with pytest.raises(ValueError):
            pwm.resolve_min_score(p, min_score=bad)
    assert pwm.resolve_min_score(p, min_score=-7) == -7 and pwm.resolve_min_score(p, min_score=np.int64(12)) == 12
    assert pwm.resolve_min_score(p, min_score=0) == 0                            # 0 is a threshold, not "not given"
    # threshold * scale, rounded up, with 1e-9 of slack for the product's own rounding: 4.2 * 100 = 420.00000000000006
    assert pwm.resolve_min_score(p, threshold=4.2) == 420 and pwm.resolve_min_score(p, threshold=4.201) == 421
    assert pwm.resolve_min_score(p, threshold=-0.005) == 0 and pwm.resolve_min_score(p, threshold=-0.015) == -1
    assert pwm.resolve_min_score(p, pvalue=1.0) == p.min_score == -400
    assert pwm.resolve_min_score(p, pvalue=0.0) == p.max_score + 1 == 401
    assert pwm.resolve_min_score(p, pvalue=1 / 256) == 351                       # one window of 256 scores 400, four score 350
    assert pwm.resolve_min_score(p, min_score=2 ** 40) == 2 ** 31 - 1
    assert pwm.PwmHits._fields == ("ids", "starts", "stops", "strands", "scores") and pwm.PwmBest._fields == ("scores", "starts")


# ------------------------------------------------------------------ ABI
def test_entry_points_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("fx_fasta_pwm_scan", 14), ("fx_fasta_pwm_best", 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    assert {"k_pwm_count", "k_pwm_emit", "k_pwm_best"} <= set(names)


def test_entry_points_refuse_bad_arguments():
    """What the numbers alone decide is refused before the handle is looked at, so each check shows without a device: the
    message says which one spoke."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    both = _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS
    n = C.c_int64(-1)
    out = [C.c_void_p() for _ in range(4)]
    bs, bp = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int64)
    mat = np.ones((65, 4), dtype=np.int32)

    def calls(m, plen, mode):
        p = None if m is None else m.ctypes.data
        rc = L.fx_fasta_pwm_scan(None, p, plen, mode, 0, None, 0, 10, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(out[3]),
                                 C.byref(n), None)
        yield rc, L.fx_last_error().decode()
        rc = L.fx_fasta_pwm_best(None, p, plen, mode, None, 0, bs.ctypes.data, bp.ctypes.data)
        yield rc, L.fx_last_error().decode()

    for plen in (1, 20, 64):                                 # all numbers fine: the null handle
        for rc, msg in calls(mat, plen, both):
            assert rc == _lib.FX_EINVAL and "null" in msg and "matrix" not in msg, plen
    for plen in (0, 65, -1):
        for rc, msg in calls(mat, plen, both):
            assert rc == _lib.FX_EINVAL and "matrix length" in msg, plen
    for rc, msg in calls(None, 8, both):
        assert rc == _lib.FX_EINVAL and "null matrix" in msg
    for v in (40000, -40000, 32768):
        bad = mat.copy()
        bad[5, 2] = v
        for rc, msg in calls(bad, 8, both):
            assert rc == _lib.FX_EINVAL and "matrix entry %d" % v in msg, v
        for rc, msg in calls(bad, 5, both):                  # the entry lies behind the matrix: not looked at
            assert rc == _lib.FX_EINVAL and "null" in msg and "matrix" not in msg
    edge = mat.copy()
    edge[0] = (32767, -32767, 0, 1)
    for rc, msg in calls(edge, 8, _lib.FX_SEARCH_PLUS):
        assert rc == _lib.FX_EINVAL and "null" in msg and "matrix" not in msg
    for rc, msg in calls(mat, 8, 0):
        assert rc == _lib.FX_EINVAL and "no strand" in msg
    for mode in (both | _lib.FX_SEARCH_DEGENERATE, _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_UPPER, 16, both | 64):
        for rc, msg in calls(mat, 8, mode):
            assert rc == _lib.FX_EINVAL and "mode" in msg, mode
    assert not any(o.value for o in out) and bs.tolist() == [7, 7] and bp.tolist() == [7, 7]


# ------------------------------------------------------------------ the oracle, by hand
def test_truth_by_hand():
    # A = 1, C = 2, G = 3, T = 4 at position 0; ten times that at position 1.  '+' of xy = m0[x] + m1[y]; '-' of xy is '+' of
    # comp(y) comp(x)
    ints = [[1, 2, 3, 4], [10, 20, 30, 40]]
    seqs = ["ACgT", "AnCG", "A", "", "uA"]
    rows, bs, bp = truth(seqs, ints, 0)
    assert rows == [(0, 0, 2, "+", 21), (0, 0, 2, "-", 43), (0, 1, 3, "+", 32), (0, 1, 3, "-", 32), (0, 2, 4, "+", 43), (0, 2, 4, "-", 21),
                    (1, 2, 4, "+", 32), (1, 2, 4, "-", 32), (4, 0, 2, "+", 14), (4, 0, 2, "-", 14)]
    assert bs.tolist() == [[43, 43], [32, 32], [NO_SCORE, NO_SCORE], [NO_SCORE, NO_SCORE], [14, 14]]
    assert bp.tolist() == [[2, 0], [2, 2], [-1, -1], [-1, -1], [0, 0]]
    rows, bs, bp = truth(seqs, ints, 33, strand="-", ids=[4, 0])
    assert rows == [(0, 0, 2, "-", 43)]
    assert bs.tolist() == [[NO_SCORE, 14], [NO_SCORE, 43]] and bp.tolist() == [[-1, 0], [-1, 0]]
    # a tie keeps the smallest start
    assert truth(["ACACAC"], ints, 100)[2].tolist() == [[0, 0]]                  # AC at 0, 2, 4: 21 on '+', 43 on '-'; CA: 12 and 34
