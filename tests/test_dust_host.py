"""CPU: the truth of the DUST tests (dust_truth.py) -- the rolling form against the brute-force definition, the pinned facts
of the definition -- the argument rules and derived columns of pyfastx_amd/complexity.py, and the new entries' declarations.
Nothing here needs a device."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import dust_truth as T
from conftest import ROOT

WINDOWS, THRESHOLDS = (4, 5, 8, 16, 33, 64), (5, 10, 20, 40)


def _random_letters(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


# ------------------------------------------------------------------ rolling == brute force
def test_rolling_equals_brute_force():
    rng = random.Random(5)
    seen_w, seen_t, n_rows, n_cases = set(), set(), 0, 360
    for trial in range(n_cases):
        n = rng.randint(0, 200)
        w, t = WINDOWS[trial % len(WINDOWS)], THRESHOLDS[(trial // len(WINDOWS)) % len(THRESHOLDS)]
        s = _random_letters(rng, n, "ACGTacgtN" if trial % 2 else "AC")
        if rng.random() < 0.5 and n > 20:                    # a planted homopolymer
            k = rng.randint(0, n - 10)
            s = s[:k] + rng.choice("ACGTan") * rng.randint(3, 30) + s[k:]
        min_len = rng.choice((1, 1, 7, 50))
        want = T.mask_brute(s, w, t, min_len)
        assert T.mask(s, w, t, min_len) == want, (s, w, t, min_len)
        seen_w.add(w); seen_t.add(t); n_rows += len(want)
    assert n_cases >= 300 and seen_w == set(WINDOWS) and seen_t == set(THRESHOLDS) and n_rows > 200


def test_brute_force_on_a_literal():
    """Counted by hand: in AAAAAAA the window that ends at 6 holds five AAA: n = 5, S = 10, 100 > 20 * 4 is true; the one that
    ends at 5 holds four: n = 4, S = 6, 60 > 60 is false."""
    assert T.triplets("AAAC") == [0, 1] and T.triplets("ANAC") == [-1, -1] and T.triplets("acgt") == [6, 27]
    assert T.qualifies(5, 10, 20) and not T.qualifies(4, 6, 20) and not T.qualifies(1, 0, 1)
    assert T.mask_brute("A" * 6) == [] and T.mask_brute("A" * 7) == [(0, 7)]


# ------------------------------------------------------------------ the pinned facts of the definition
def test_pinned_homopolymers():
    for f in (T.mask, T.mask_brute):
        assert f("A" * 6, 64, 20) == []
        assert f("A" * 7, 64, 20) == [(0, 7)]
        assert f("a" * 7, 64, 20) == [(0, 7)]                # soft-masked letters score like upper case
        assert f("N" * 300, 64, 1) == []                     # a window of only N never qualifies
        assert f("", 64, 20) == f("A", 64, 20) == f("AA", 64, 20) == f("AAA", 64, 20) == []
    assert T.mask("A" * 7, 64, 20, min_len=8) == []


def test_pinned_random_and_planted():
    """Random letters have no row at W = 64, T = 20 and a few at small windows; (AC) x 40 planted at 1000 takes the flanks the
    windowed form gives it: the row begins W - 1 letters in front of the first qualifying end and ends at the last one."""
    rng = random.Random(11)
    g = _random_letters(rng, 300000)
    assert T.mask(g, 64, 20) == []
    n16, n8 = len(T.mask(g, 16, 20)), len(T.mask(g, 8, 20))
    assert n16 <= n8 and n16 < 20 and 0 < n8 < 100, (n16, n8)  # a handful per 3 x 10^5 letters, more at the smaller window
    h = g[:1000] + "AC" * 40 + g[1000:2000]
    (a64, b64), = T.mask(h, 64, 20)
    (a16, b16), = T.mask(h[:1200], 16, 20)
    assert T.mask_brute(h[900:1200], 64, 20) == [(a64 - 900, b64 - 900)] and T.mask_brute(h[900:1200], 16, 20) == [(a16 - 900, b16 - 900)]
    # The plant is [1000, 1080).  At W = 64 a window needs S > 122: j triplets of the repeat, half ACA and half CAC, give
    # j^2 / 4 - j / 2, which passes at j = 24 (26 letters) -- a few fewer where the random flank adds pairs of its own.  So the
    # flanks are 64 - 30 .. 64 - 20 letters; at W = 16 (S > 26: j = 12, 14 of 16 letters) they are 0 .. 6.
    assert 34 <= 1000 - a64 <= 44 and 34 <= b64 - 1080 <= 44, (a64, b64)
    assert 0 <= 1000 - a16 <= 6 and 0 <= b16 - 1080 <= 6, (a16, b16)


def test_issue_figures_reproduced():
    """The figures the definition was checked with: the generator of that check, consumed in its order."""
    rng = random.Random(5)
    for _ in range(300):
        n = rng.randint(0, 200); rng.choice([4, 5, 8, 16, 33, 64]); rng.choice([5, 10, 20, 40])
        s = "".join(rng.choice("ACGTacgtN" if rng.random() < .5 else "AC") for _ in range(n))
        if rng.random() < .5 and n > 20:
            rng.randint(0, n - 10); rng.randint(3, 30)
    g = "".join(rng.choice("ACGT") for _ in range(300000))
    assert (len(T.mask(g)), len(T.mask(g, 16)), len(T.mask(g, 8))) == (0, 3, 12)
    h = g[:1000] + "AC" * 40 + g[1000:2000]
    assert T.mask(h, 64, 20) == [(960, 1121)] and T.mask(h, 16, 20) == [(997, 1083)]


def test_merged_and_multi():
    assert T.merged([(5, 7), (0, 2), (2, 4), (6, 9)]) == [(0, 4), (5, 9)]
    s = "ACGTTGCA" * 5 + "A" * 9 + "CAGTCGATGCTAGCATGCAT" + "AC" * 12 + "GATTACAGATTACA"
    want = T.merged(T.mask(s, 8, 20) + T.mask(s, 64, 20))
    assert T.mask_multi(s, (8, 64), 20) == want and len(want) >= 1
    assert T.mask_multi(s, (8, 64), 20, min_len=10 ** 6) == []


# ------------------------------------------------------------------ the per-read columns
def test_read_columns_literal():
    assert T.read_columns("") == (0, 0, 0, 0) and T.read_columns("A") == (1, 0, 0, 0) and T.read_columns("AC") == (2, 0, 0, 1)
    assert T.read_columns("AAAAA") == (5, 3, 3, 0)           # three AAA: 3 * 2 / 2
    assert T.read_columns("ACACAC") == (6, 4, 2, 5)          # ACA CAC ACA CAC
    assert T.read_columns("AANAAaa") == (7, 2, 1, 3)         # AAa and Aaa fold onto AAA; A/N, N/A and A/a differ as bytes
    n = 70000
    assert T.read_columns("A" * n) == (n, n - 2, (n - 2) * (n - 3) // 2, 0) and (n - 2) * (n - 3) // 2 > 2 ** 31


def test_derived_columns():
    from pyfastx_amd import complexity as X
    d = X.dust_score([0, 0, 1, 3, 10], [0, 1, 2, 3, 5])
    assert d.dtype == np.float64 and d.tolist() == [0.0, 0.0, 10.0, 15.0, 25.0]
    c = X.fastp_complexity([0, 0, 1, 2], [0, 1, 2, 5])
    assert c.dtype == np.float64 and c.tolist() == [0.0, 0.0, 1.0, 0.5]
    for s, n in ((0, 0), (0, 1), (1, 2), (10, 5)):
        assert X.dust_score([s], [n])[0] == T.dust(s, n)
    for d_, n in ((0, 0), (0, 1), (1, 2), (2, 5)):
        assert X.fastp_complexity([d_], [n])[0] == T.complexity(d_, n)
    cols = X.columns(np.array([5]), np.array([3], dtype=np.int32), np.array([3]), np.array([0], dtype=np.int32))
    assert list(cols) == ["length", "n_triplets", "dust_sum", "n_diff", "dust", "complexity"] and cols["dust"][0] == 15.0


# ------------------------------------------------------------------ the argument rules
def test_check_mask():
    from pyfastx_amd import complexity as X
    assert X.check_mask() == ((64,), 20, 1, 10 ** 8)
    assert X.check_mask((8, 16, 64), 1, 5, 0) == ((8, 16, 64), 1, 5, 0)
    assert X.check_mask([4], 1000) == ((4,), 1000, 1, 10 ** 8)
    assert X.check_mask(np.int64(33), np.int32(7)) == ((33,), 7, 1, 10 ** 8)
    for kw in ({"window": 3}, {"window": 65}, {"window": 6.0}, {"window": True}, {"window": "64"}, {"window": ()},
               {"window": (4, 5, 6, 7, 8)}, {"window": (8, 3)}, {"window": (8, 2.5)},
               {"threshold": 0}, {"threshold": 1001}, {"threshold": 2.0}, {"threshold": None},
               {"min_len": 0}, {"min_len": -3}, {"min_len": 1.5}, {"max_rows": -1}, {"max_rows": 1e8}):
        with pytest.raises(ValueError):
            X.check_mask(**kw)


# ------------------------------------------------------------------ the C entries
def test_entries_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, nargs in (("fx_fasta_low_complexity", 12), ("fx_fastq_complexity", 11)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs, name
    assert hasattr(_lib.Blob, "fasta_low_complexity") and hasattr(_lib.Blob, "fastq_complexity")
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_dust_count", "k_dust_scan", "k_dust_emit", "k_fq_complexity"):
        assert k in names


def test_entries_without_a_device_or_a_handle():
    """Without a device both entries answer FX_EDEVICE before they look at an argument; with one, a null handle is FX_EINVAL."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    want = _lib.FX_EDEVICE if L.fx_device_count() <= 0 else _lib.FX_EINVAL
    out = [C.c_void_p() for _ in range(4)]
    n, m = C.c_int64(0), C.c_int64(0)
    assert L.fx_fasta_low_complexity(None, 64, 20, 1, None, 0, 10, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(n), C.byref(m)) == want
    assert L.fx_fasta_low_complexity(None, 0, 0, 0, None, -1, -1, None, None, None, None, None) == want
    assert L.fx_fastq_complexity(None, None, 0, None, None, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(out[3]), C.byref(n), C.byref(m)) == want
    assert L.fx_fastq_complexity(None, None, -1, None, None, None, None, None, None, None, None) == want
