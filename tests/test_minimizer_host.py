"""CPU: the oracle of the minimizer tests (minimizer_truth.py) against a second, independent model (a monotone deque) and
against a port of the device's lane state machine, pyfastx_amd/minimizer.py (mix and its inverse, the argument rules, the
methods of Minimizers), a pinned hand case, the density of random sequence, and fx_fasta_minimizers as far as it answers
without a device."""
import ctypes as C
import os
import re
from collections import deque

import numpy as np
import pytest

from conftest import ROOT
from minimizer_truth import lane_rows, mix_int, record_rows, truth

HAND = "ACGTNACGTACGTTTTTTTTTGCA"
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def _mz():
    from pyfastx_amd import minimizer
    return minimizer


def _rand(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


# ------------------------------------------------------------------ a second model: rolled codes, a monotone deque
def deque_rows(seq, k, w, canonical, order):
    """The codes are rolled letter by letter; the deque holds (position, key) with keys strictly increasing from its head to
    its tail, so the head is the leftmost smallest of the window; an invalid position never enters."""
    val = {"A": 0, "C": 1, "G": 2, "T": 3}
    mask, fw, rc, run = 4 ** k - 1, 0, 0, 0
    dq, rows, last = deque(), [], None
    for i, ch in enumerate(seq):
        c = val.get(ch.upper())
        if c is None:
            run = 0
        else:
            fw = ((fw << 2) | c) & mask
            rc = (rc >> 2) | ((3 - c) << (2 * k - 2))
            run += 1
        p = i - k + 1                                        # the position whose k-mer ends here
        if p < 0:
            continue
        if run >= k:
            code, strand = (rc, "-") if canonical and rc < fw else (fw, "+")
            key = code if order == "lex" else mix_int(code, k)
            while dq and dq[-1][1] > key:                    # an equal key stays: it is further left
                dq.pop()
            dq.append((p, key, strand, code))
        j = p - w + 1                                        # the window that ends at p
        if j < 0:
            continue
        while dq and dq[0][0] < j:
            dq.popleft()
        if dq and dq[0][0] != last:
            last = dq[0][0]
            rows.append((last, dq[0][2], dq[0][3]))
    return rows


@pytest.mark.parametrize("k", [1, 2, 15, 16, 31])
@pytest.mark.parametrize("w", [1, 2, 10, 32])
def test_model_equals_deque_model(k, w):
    rng = np.random.default_rng(1000 * k + w)
    n_rows = 0
    for order in ("hash", "lex"):
        for canonical in (True, False):
            for alphabet, n in (("ACGT", 400), ("ACGTacgtN", 500), ("AC", 200), ("ACGTNnRYu*", 300)):
                s = _rand(rng, n, alphabet)
                a = int(rng.integers(0, n - 100))
                s = s[:a] + "N" * int(rng.integers(1, w + k + 2)) + s[a:]
                got = record_rows(s, k, w, canonical, order)
                assert got == deque_rows(s, k, w, canonical, order), (order, canonical, alphabet)
                n_rows += len(got)
    assert n_rows > 0


@pytest.mark.parametrize("k,w", [(1, 1), (3, 4), (15, 10), (16, 16), (31, 32), (31, 1), (2, 32)])
def test_lane_state_machine_equals_model(k, w):
    """The carry of csrc/fx_minimizer.hpp in Python ints: one lane per run, warmed up on the w + k - 1 letters in front of it
    from the empty state, emits exactly the model's rows -- at runs of 256 letters and at runs shorter than the warm-up."""
    rng = np.random.default_rng(31 * k + w)
    for order in ("hash", "lex"):
        for canonical in (True, False):
            for alphabet in ("ACGT", "ACGTN", "A", "AC"):
                s = _rand(rng, 700, alphabet)
                s = s[:300] + "N" * (w + k - 1) + s[300:]
                want = record_rows(s, k, w, canonical, order)
                for run in (256, 5, 64):
                    assert lane_rows(s, k, w, canonical, order, run) == want, (order, canonical, alphabet, run)


# ------------------------------------------------------------------ mix
@pytest.mark.parametrize("k", [1, 5, 16, 31])
def test_mix_equals_formula_and_unmix_inverts(k):
    mz = _mz()
    rng = np.random.default_rng(k)
    x = rng.integers(0, 4 ** k, 2000, dtype=np.uint64)
    x[:3] = (0, 4 ** k - 1, 4 ** k // 2)
    y = mz.mix(x, k)
    assert y.dtype == np.uint64 and y.tolist() == [mix_int(int(v), k) for v in x]
    assert (y < np.uint64(4 ** k)).all() if k < 32 else True
    assert (mz.unmix(y, k) == x).all() and (mz.mix(mz.unmix(x, k), k) == x).all()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_mix_is_a_bijection(k):
    mz = _mz()
    y = mz.mix(np.arange(4 ** k, dtype=np.uint64), k)
    assert np.array_equal(np.sort(y), np.arange(4 ** k, dtype=np.uint64))
    assert np.array_equal(mz.unmix(y, k), np.arange(4 ** k, dtype=np.uint64))


# ------------------------------------------------------------------ by hand
def test_hand_case():
    """k = 3, w = 4, canonical, hash order.  The N at 4 voids the positions 2, 3 and 4; TTT is AAA on '-'."""
    rows = record_rows(HAND, 3, 4, True, "hash")
    assert rows[:6] == [(0, "+", 6), (1, "-", 6), (5, "+", 6), (7, "+", 44), (11, "-", 1), (12, "-", 0)]
    assert rows[6:] == [(p, "-", 0) for p in range(13, 19)]  # the run of TTT: every window's leftmost has just left
    assert rows == deque_rows(HAND, 3, 4, True, "hash") == lane_rows(HAND, 3, 4, True, "hash", 5)
    all_rows, counts = truth([HAND, "ACG", "", HAND], 3, 4)
    assert [r for r in all_rows if r[0] == 0] == [(0,) + r for r in rows] and [r[1:] for r in all_rows if r[0] == 3] == rows
    assert counts.tolist() == [[3, 9], [0, 0], [0, 0], [3, 9]]
    assert truth([HAND, "ACG", "", HAND], 3, 4, ids=[3, 1, 3])[1].tolist() == [[0, 0], [3, 9]]
    # lex order, forward codes: ACG = 6 is the smallest of the first window
    assert record_rows(HAND, 3, 4, False, "lex")[:3] == [(0, "+", 6), (1, "+", 27), (5, "+", 6)]
    # a record of w + k - 2 letters has no window; one of w + k - 1 has one
    assert record_rows("ACGTAC"[:5], 3, 4) == [] and len(record_rows("ACGTAC", 3, 4)) == 1


# ------------------------------------------------------------------ density
@pytest.mark.parametrize("k,w", [(15, 10), (21, 11), (31, 32), (5, 4)])
def test_density_of_random_sequence(k, w):
    """Random minimizers of random sequence sample 2 / (w + 1) of the positions."""
    for seed in range(5):
        s = "".join(np.random.default_rng(seed).choice(list("ACGT"), 20000))
        rows = record_rows(s, k, w, True, "hash")
        ratio = len(rows) / (len(s) - k + 1) * (w + 1) / 2
        assert 0.95 <= ratio <= 1.05, (seed, ratio)


# ------------------------------------------------------------------ the Python module
def test_argument_rules():
    mz = _mz()
    assert mz.check_args(1, 1) == (1, 1) and mz.check_args(np.int64(31), np.int32(32), "lex") == (31, 32)
    for k, w in ((0, 5), (32, 5), (-1, 5), (5, 0), (5, 33), (5, -2), (5.0, 5), (5, 5.0), ("5", 5), (None, 5), (True, 5), (5, True)):
        with pytest.raises(ValueError):
            mz.check_args(k, w)
    for order in ("Hash", "random", None, 0):
        with pytest.raises(ValueError):
            mz.check_args(5, 5, order)
    with pytest.raises(ValueError):
        mz.mix([16], 2)
    with pytest.raises(ValueError):
        mz.mix([0], 32)
    assert mz.Minimizers._fields == ("ids", "starts", "stops", "strands", "codes")


def test_minimizers_methods(tmp_path):
    mz = _mz()
    seqs = [HAND, "ACG", _rand(np.random.default_rng(3), 200, "ACGTN")]
    k, w = 3, 4
    rows, _ = truth(seqs, k, w)
    cols = list(zip(*rows))
    m = mz.Minimizers(np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.int64), np.array(cols[1], dtype=np.int64) + k,
                      np.array([ord(s) for s in cols[2]], dtype=np.uint8), np.array(cols[3], dtype=np.uint64))
    assert m.k == k and m.hashes().tolist() == [mix_int(c, k) for c in cols[3]]
    want = []
    for r, start, strand, _ in rows:                         # the letters of the code: the reverse complement on '-'
        word = seqs[r][start:start + k].upper()
        want.append(word if strand == "+" else word[::-1].translate(_COMP))
    assert m.kmers() == want
    d = m.density([len(s) for s in seqs])
    assert d.tolist() == [cols[0].count(0) / 22, 0.0, cols[0].count(2) / 198]
    assert m.density([len(s) for s in seqs] + [0, 2]).tolist()[3:] == [0.0, 0.0]
    with pytest.raises(ValueError):
        m.density([24, 3])
    n = m.write_bed(tmp_path / "m.bed", ["hand", "short", "rand"])
    lines = open(tmp_path / "m.bed").read().splitlines()
    assert n == len(rows) == len(lines) and lines[0] == "hand\t0\t3\tACG\t0\t+" and lines[1] == "hand\t1\t4\tACG\t0\t-"
    e = mz._empty()
    assert [a.dtype for a in e] == [np.int64, np.int64, np.int64, np.uint8, np.uint64] and e.k is None
    assert e.kmers() == [] and e.hashes().size == 0 and e.density([5, 6]).tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ ABI
def test_entry_point_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bint\s+fx_fasta_minimizers\s*\(", hdr) and "fx_fasta_minimizers" in _lib.SYMBOLS
    assert hasattr(L, "fx_fasta_minimizers") and len(L.fx_fasta_minimizers.argtypes) == 13
    assert re.search(r"FX_MZ_CANONICAL\s*=\s*1\s*,\s*FX_MZ_LEX\s*=\s*2", hdr) and (_lib.FX_MZ_CANONICAL, _lib.FX_MZ_LEX) == (1, 2)
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    assert {"k_mz_count", "k_mz_emit"} <= set(names)


def test_entry_point_refuses_bad_arguments():
    """What the numbers alone decide is refused before the handle is looked at, so each check shows without a device."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    n = C.c_int64(-1)
    out = [C.c_void_p() for _ in range(4)]

    def call(k, w, flags):
        rc = L.fx_fasta_minimizers(None, k, w, flags, None, 0, 10, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(out[3]), C.byref(n), None)
        return rc, L.fx_last_error().decode()

    for k, w, flags in ((1, 1, 0), (31, 32, 3), (15, 10, 1), (15, 10, 2)):      # all numbers fine: the null handle
        rc, msg = call(k, w, flags)
        assert rc == _lib.FX_EINVAL and "null" in msg, (k, w, flags)
    for k in (0, 32, -1):
        rc, msg = call(k, 10, 1)
        assert rc == _lib.FX_EINVAL and "k = %d" % k in msg
    for w in (0, 33, -1):
        rc, msg = call(15, w, 1)
        assert rc == _lib.FX_EINVAL and "w = %d" % w in msg
    for flags in (4, 7, 8, -1):
        rc, msg = call(15, 10, flags)
        assert rc == _lib.FX_EINVAL and "flag" in msg
    assert not any(o.value for o in out) and n.value == 0
