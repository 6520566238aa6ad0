"""-m gpu: Fasta.pwm_scan / pwm_counts / pwm_best (fx_fasta_pwm_scan, fx_fasta_pwm_best, csrc/fx_pwm.hpp) against the two
search automata, which share no code with the score tables, and against the numpy oracle of pwm_truth.py over fa[i].seq:
every line layout the index accepts, every group count and the boundary between the one-word and the two-word history,
invalid letters around run boundaries, the limits of the per-run count fields, the cut at slen, hit offsets across a scan
chunk, ties of the best window, and the arguments of the object API.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from pwm_truth import NO_SCORE, truth
from test_gpu_search_approx import _layout                   # the layouts of the approximate search, generated the same way

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 8, 31, 32, 33, 63, 64)
_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


@pytest.fixture(scope="module")
def Pwm():
    from pyfastx_amd.pwm import Pwm
    return Pwm


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


def _revcomp(p):
    return p[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def _planted(rng, n, sites, alphabet="ACGT"):
    t = list(_rand(rng, n, alphabet))
    for a, s in sites:
        assert 0 <= a and a + len(s) <= n
        t[a:a + len(s)] = s
    return "".join(t)


def _rand_pwm(Pwm, rng, W, peak=True):
    """Random weights in -50..50; with peak, one letter of every position stands out, so the consensus is the only best window."""
    m = rng.integers(-50, 51, (W, 4)).astype(np.int32)
    if peak:
        m[np.arange(W), rng.integers(0, 4, W)] = 90
    return Pwm.from_ints(m)


def _consensus(pwm):
    return "".join("ACGT"[c] for c in pwm.ints.argmax(axis=1))


def got(h):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], h.scores.tolist()))


def check(fa, seqs, pwm, t, strand="both", ids=None):
    """pwm_scan against the oracle, pwm_counts against the rows, pwm_best against the oracle."""
    h = fa.pwm_scan(pwm, min_score=t, strand=strand, ids=ids)
    assert [a.dtype for a in h] == [np.int64, np.int64, np.int64, np.uint8, np.int32]
    rows, bs, bp = truth(seqs, pwm.ints, t, strand, ids)
    assert got(h) == rows, (len(pwm), t, strand)
    if ids is None:
        c = fa.pwm_counts(pwm, min_score=t, strand=strand)
        assert c.shape == (len(seqs), 2) and c.dtype == np.int64
        bc = np.zeros((len(seqs), 2), dtype=np.int64)
        np.add.at(bc, (h.ids, (h.strands == ord("-")).astype(np.int64)), 1)
        assert (c == bc).all(), (len(pwm), t)
    b = fa.pwm_best(pwm, strand=strand, ids=ids)
    assert b.scores.dtype == np.int32 and b.starts.dtype == np.int64 and b.scores.shape == b.starts.shape == bs.shape
    assert (b.scores == bs).all() and (b.starts == bp).all(), (len(pwm), strand)
    return h, b


@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


# ------------------------------------------------------------------ against the independent automata
def _match_matrix(p, hit, miss):
    m = np.full((len(p), 4), miss, dtype=np.int32)
    for j, c in enumerate(p.upper()):
        for b in _SETS[c]:
            m[j, "ACGT".index(b)] = hit
    return m


def _rows(h):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), h.strands.tolist()))


def _against_automata(fa, Pwm, exact, approx):
    n = 0
    for p in exact:                            # 0/1: a window scores W exactly where every letter lies in its pattern letter's set
        e = fa.search_all(p, degenerate=True)
        h = fa.pwm_scan(Pwm.from_ints(_match_matrix(p, 1, 0)), min_score=len(p))
        assert _rows(h) == _rows(e), p
        assert (h.scores == len(p)).all()
        assert (fa.pwm_counts(Pwm.from_ints(_match_matrix(p, 1, 0)), min_score=len(p)) == fa.search_counts(p, degenerate=True)).all()
        n += h.ids.size
    for p in approx:                           # 0/-1: the score is minus the Hamming distance
        for d in (0, 1, 3):
            if d > len(p) - 1:
                continue
            a = fa.search_approx(p, d, degenerate=True)
            h = fa.pwm_scan(Pwm.from_ints(_match_matrix(p, 0, -1)), min_score=-d)
            assert _rows(h) == _rows(a), (p, d)
            assert (h.scores == -a.mismatches.astype(np.int32)).all(), (p, d)
            for s in "+-":
                a1, h1 = fa.search_approx(p, d, degenerate=True, strand=s), fa.pwm_scan(Pwm.from_ints(_match_matrix(p, 0, -1)), min_score=-d, strand=s)
                assert _rows(h1) == _rows(a1) and (h1.scores == -a1.mismatches.astype(np.int32)).all(), (p, d, s)
            n += h.ids.size
    return n


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_equals_automata_on_fixture(fx, Pwm, fixture_files, fn):
    fa = fx.Fasta(fixture_files[fn])
    s = fa[3].seq
    n = _against_automata(fa, Pwm, ["GAATTC", "GANTC", "RGATCY", "A", "NNNN", s[10:41], s[5:69]],
                          ["GAATTC", "AT", s[55:67], s[10:41], s[20:53], s[5:69], "GARYNNTC"])
    assert n > 1000


def test_equals_automata_on_mixed_case(fx, Pwm, tmp_path):
    rng = np.random.default_rng(5)
    recs = [_rand(rng, int(rng.integers(300, 1500)), "ACGTacgt") for _ in range(6)]
    fa = fx.Fasta(_write(tmp_path / "mixed_case.fa", "".join(">r%d\n%s\n" % (i, "\n".join(s[a:a + 57] for a in range(0, len(s), 57)))
                                                             for i, s in enumerate(recs))))
    s = recs[2]
    n = _against_automata(fa, Pwm, ["GAATTC", "gantc", "WSNNKM", s[40:72], s[100:164]], ["GAATTC", "ryAC", s[40:52], s[40:72], s[7:40], s[100:164]])
    assert n > 200


# ------------------------------------------------------------------ line layouts
@pytest.mark.parametrize("name", ["irregular", "crlf", "odd"])
def test_layouts(fx, Pwm, tmp_path, name):
    """Irregular lines with blank lines; CRLF with spaces and lower case; N runs, bytes that are no letter, empty and short
    records and an unterminated last line."""
    fa = fx.Fasta(_write(tmp_path / (name + ".fa"), _layout(name)))
    seqs = [fa[i].seq for i in range(len(fa))]
    rng = np.random.default_rng(len(name))
    hits = 0
    for W, frac in ((2, 0.7), (4, 0.7), (7, 0.7), (12, 0.7), (33, 0.7), (64, 0.7), (33, 0.5), (64, 0.5)):    # (long ones: rows only lower down)
        pwm = _rand_pwm(Pwm, rng, W, peak=False)
        h, b = check(fa, seqs, pwm, pwm.score_at(frac))
        hits += h.ids.size
    assert hits > 0
    pwm = _rand_pwm(Pwm, rng, 6, peak=False)
    check(fa, seqs, pwm, pwm.score_at(0.5), strand="+")
    check(fa, seqs, pwm, pwm.score_at(0.5), strand="-")


# ------------------------------------------------------------------ widths: every group count, both history forms, run boundaries
@pytest.mark.parametrize("W", WIDTHS)
def test_widths(fx, Pwm, tmp_path, W):
    """The consensus planted on both strands so that it straddles a 256-byte boundary of the stream at every offset from
    -W + 1 (its last letter alone behind the boundary) to 0 (its first letter on it)."""
    rng = np.random.default_rng(100 + W)
    pwm = _rand_pwm(Pwm, rng, W)
    cons = _consensus(pwm)
    hdr, LW = ">widths\n", 61
    n = 256 * (2 * W + 2)
    off = len(hdr) + np.arange(n) + np.arange(n) // LW       # stream offset of letter i
    sites, fwd, rev = [], [], []
    for j, o in enumerate(range(-W + 1, 1)):
        for k, (s, keep) in enumerate(((cons, fwd), (_revcomp(cons), rev))):
            edge = int(np.searchsorted(off, 256 * (2 * j + k + 1)))                 # the first letter at or behind the boundary
            sites.append((edge + o, s))
            keep.append(edge + o)
    text = _planted(rng, n, sites)
    fa = fx.Fasta(_write(tmp_path / ("w%d.fa" % W), hdr + "\n".join(text[i:i + LW] for i in range(0, n, LW)) + "\n"))
    assert fa[0].seq == text
    t = min(pwm.score_at(0.7), pwm.max_score)
    h, b = check(fa, [text], pwm, t)
    rows = set(got(h))
    for a in fwd:
        assert (0, a, a + W, "+", pwm.max_score) in rows, a
    for a in rev:
        assert (0, a, a + W, "-", pwm.max_score) in rows, a
    assert b.scores.tolist() == [[pwm.max_score] * 2]
    if W >= 8:                                               # (shorter ones turn up by chance in front of the first site)
        assert b.starts.tolist() == [[fwd[0], rev[0]]]
    check(fa, [text], pwm, pwm.max_score)


# ------------------------------------------------------------------ invalid letters
@pytest.mark.parametrize("W", [5, 33])
def test_invalid_letters(fx, Pwm, tmp_path, W):
    """N, R and * just in front of a run boundary, just behind one, inside the warm-up region of a run and W letters in front of
    a window's last letter.  At min_score = pwm.min_score every window without one of them is a hit on both strands."""
    rng = np.random.default_rng(W)
    pwm = _rand_pwm(Pwm, rng, W, peak=False)
    hdr, n = ">inv\n", 256 * 9
    off = len(hdr) + np.arange(n)                            # one line: letter i at stream offset 5 + i
    edge = lambda k: int(np.searchsorted(off, 256 * k))
    bad = {edge(1) - 1: "N", edge(2): "R", edge(3) - W + 2: "*", edge(4) - 2: "n", edge(4) + 1: "r", edge(5) - W: "N", edge(6) - W - 1: "*",
           edge(7) + W: "N", edge(7) - 1: "R", 0: "N", n - 1: "*"}
    text = _planted(rng, n, sorted(bad.items()))
    short, only_n = _rand(rng, W - 1), "N" * (3 * W)
    fa = fx.Fasta(_write(tmp_path / "inv.fa", hdr + text + "\n>short\n" + short + "\n>empty\n>onlyN\n" + only_n + "\n>tail\n" + _rand(rng, W) + "N\n"))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert seqs == [text, short, "", only_n, seqs[4]]
    h, b = check(fa, seqs, pwm, pwm.min_score)
    clean = [s for s in range(n - W + 1) if not any(s <= p < s + W for p in bad)]
    assert [(r[1], r[3]) for r in got(h) if r[0] == 0] == [(s, sd) for s in clean for sd in "+-"]
    assert 0 < len(clean) < n - W + 1 - 5 * W
    assert [r[:4] for r in got(h) if r[0] != 0] == [(4, 0, W, "+"), (4, 0, W, "-")]                 # exactly W valid letters, then an N
    assert b.scores[1:4].tolist() == [[NO_SCORE] * 2] * 3 and b.starts[1:4].tolist() == [[-1, -1]] * 3
    assert fa.pwm_counts(pwm, min_score=pwm.min_score)[1:4].tolist() == [[0, 0]] * 3
    assert fa.pwm_scan(pwm, min_score=pwm.min_score, ids=[1, 2, 3]).ids.size == 0
    check(fa, seqs, pwm, pwm.score_at(0.6))


# ------------------------------------------------------------------ the 9-bit count fields, order at one start
def test_field_limits_and_order(fx, Pwm, tmp_path):
    rng = np.random.default_rng(9)
    text = _rand(rng, 3000)
    fa = fx.Fasta(_write(tmp_path / "line.fa", ">line\n" + text + "\n>sites\nTTGAATTCTTGAATTGTTCAATTCTT\n"))
    seqs = [text, fa[1].seq]
    for W in (2, 9):
        pwm = _rand_pwm(Pwm, rng, W, peak=False)
        h, _ = check(fa, seqs, pwm, pwm.min_score)           # every window, on both strands: 256 + 256 hits in every full run
        assert [(r[1], r[3]) for r in got(h) if r[0] == 0] == [(s, sd) for s in range(3000 - W + 1) for sd in "+-"]
        assert fa.pwm_counts(pwm, min_score=pwm.min_score)[0].tolist() == [3000 - W + 1] * 2
    # a palindromic matrix: '+' then '-' at one start, with equal scores
    pal = np.zeros((6, 4), dtype=np.int32)
    pal[np.arange(6), ["ACGT".index(c) for c in "GAATTC"]] = 7
    h, _ = check(fa, seqs, Pwm.from_ints(pal), 35)
    assert [r for r in got(h) if r[0] == 1] == [(1, 2, 8, "+", 42), (1, 2, 8, "-", 42), (1, 10, 16, "+", 35), (1, 10, 16, "-", 35),
                                                (1, 18, 24, "+", 35), (1, 18, 24, "-", 35)]
    allw = got(fa.pwm_scan(Pwm.from_ints(pal), min_score=0, ids=[0]))
    assert len(allw) == 2 * 2995 and all(a[4] == b[4] and (a[3], b[3]) == ("+", "-") and a[1] == b[1] for a, b in zip(allw[::2], allw[1::2]))
    # GAATTG is not its own reverse complement: the scores differ at one start
    m = np.zeros((6, 4), dtype=np.int32)
    m[np.arange(6), ["ACGT".index(c) for c in "GAATTG"]] = 7
    h, _ = check(fa, seqs, Pwm.from_ints(m), 28)
    assert [r for r in got(h) if r[0] == 1] == [(1, 2, 8, "+", 35), (1, 2, 8, "-", 35), (1, 10, 16, "+", 42), (1, 10, 16, "-", 28),
                                                (1, 18, 24, "+", 28), (1, 18, 24, "-", 42)]


# ------------------------------------------------------------------ the cut at slen
def test_cut_at_slen(fx, Pwm, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: the index takes every line for a
    CR LF line, so slen is smaller than the number of kept bytes (by one per later line) and `seq` stops there.  The consensus sits at the very end of the
    kept bytes -- behind the cut where there is one: no hit and no best window may come from there."""
    rng = np.random.default_rng(55)
    W = 12
    pwm = _rand_pwm(Pwm, rng, W)
    cons = _consensus(pwm)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 20, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        lines[-1] = lines[-1][:-W] + (cons if i % 2 == 0 else _revcomp(cons))
        kept.append(60 * n_lines)
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    lens = np.array([len(fa[i]) for i in range(len(fa))])
    assert [len(s) for s in seqs] == lens.tolist()
    cut = [len(s) <= n - W for s, n in zip(seqs, kept)]      # the whole consensus lies behind the cut
    assert sum(cut) >= 3 and not cut[3], "the case is not exercised"
    for t in (pwm.min_score, pwm.score_at(0.6), pwm.max_score):
        h, b = check(fa, seqs, pwm, t)
        assert (h.stops <= lens[h.ids]).all()
        assert (b.starts + W <= lens[:, None]).all()
    for i, c in enumerate(cut):                              # where it is cut off, the maximum is not reached
        assert not c or b.scores[i].max() < pwm.max_score, i
    assert b.scores[3].tolist()[1] == pwm.max_score and b.starts[3].tolist()[1] == 60 - W       # record 3: one line, the reverse strand


# ------------------------------------------------------------------ hit offsets across a chunk of the scans
def test_scan_chunk(fx, Pwm, tmp_path):
    """One record of more than 4096 runs: the offsets of the hits behind run 4096 carry the sum of a whole scan chunk."""
    rng = np.random.default_rng(77)
    n, W = 1_100_000, 12
    pwm = Pwm.from_counts(rng.integers(0, 30, (4, W)))
    cons = _consensus(pwm)
    text = _planted(rng, n, [(n - 40, cons), (n - 12, _revcomp(cons))])
    fa = fx.Fasta(_write(tmp_path / "big.fa", ">big\n" + "\n".join(text[i:i + 80] for i in range(0, n, 80)) + "\n"))
    t = pwm.threshold_for_pvalue(5e-4)
    rows, bs, bp = truth([text], pwm.ints, t)
    assert 200 <= len(rows) <= 3000
    h = fa.pwm_scan(pwm, min_score=t)
    assert got(h) == rows
    assert int((h.starts > 4096 * 256).sum()) >= 2 and (0, n - 40, n - 28, "+", pwm.max_score) in rows and (0, n - 12, n, "-", pwm.max_score) in rows
    assert fa.pwm_counts(pwm, min_score=t).tolist() == [[sum(r[3] == "+" for r in rows), sum(r[3] == "-" for r in rows)]]
    b = fa.pwm_best(pwm)
    assert (b.scores == bs).all() and (b.starts == bp).all() and b.scores.tolist() == [[pwm.max_score] * 2]


# ------------------------------------------------------------------ ties of the best window
def test_best_ties(fx, Pwm, tmp_path):
    rng = np.random.default_rng(13)
    W = 10
    pwm = _rand_pwm(Pwm, rng, W)
    cons, rc = _consensus(pwm), _revcomp(_consensus(pwm))
    assert cons != rc
    # the consensus three times on '+' and three times on '-' in record 0 (many runs apart, and twice inside one run), twice in
    # record 2; record 1 has none
    r0 = _planted(rng, 5000, [(3100, cons), (700, cons), (760, cons), (4100, rc), (333, rc), (350, rc)])
    r1 = _rand(rng, 900)
    r2 = _planted(rng, 2000, [(1500, cons), (1200, cons), (90, rc), (1900, rc)])
    wrap = lambda s: "\n".join(s[a:a + 70] for a in range(0, len(s), 70))
    fa = fx.Fasta(_write(tmp_path / "ties.fa", ">a\n%s\n>b\n%s\n>c\n%s\n" % (wrap(r0), wrap(r1), wrap(r2))))
    seqs = [r0, r1, r2]
    _, b = check(fa, seqs, pwm, pwm.max_score)
    assert b.scores.tolist() == [[pwm.max_score] * 2, b.scores[1].tolist(), [pwm.max_score] * 2] and b.scores[1].max() < pwm.max_score
    assert b.starts[[0, 2]].tolist() == [[700, 333], [1200, 90]]
    _, b = check(fa, seqs, pwm, pwm.max_score, ids=[2, 0])   # the rows of the best in the order asked for
    assert b.starts.tolist() == [[1200, 90], [700, 333]]
    b = fa.pwm_best(pwm, ids=["c", "a", "c"])
    assert b.starts.tolist() == [[1200, 90], [700, 333], [1200, 90]] and b.scores.tolist() == [[pwm.max_score] * 2] * 3


# ------------------------------------------------------------------ counts, ids, limits, arguments
def test_arguments(fx, Pwm, fixture_files, monkeypatch):
    fa = fx.Fasta(fixture_files["test.fa"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    pwm = Pwm.from_counts(np.random.default_rng(3).integers(0, 20, (4, 8)))
    t = pwm.threshold_for_pvalue(2e-3)
    full, best = check(fa, seqs, pwm, t)
    n = full.ids.size
    assert 100 < n < 2000
    # ids
    sel = [5, 0, 17, 5]
    keep = np.isin(full.ids, [0, 5, 17])
    want = got(type(full)(*(a[keep] for a in full)))
    assert len(want) > 3
    assert got(fa.pwm_scan(pwm, min_score=t, ids=sel)) == want                     # unsorted and repeated: as search_all treats them
    assert got(fa.pwm_scan(pwm, min_score=t, ids=[names[i] for i in sel])) == want
    b = fa.pwm_best(pwm, ids=sel)
    assert (b.scores == best.scores[sel]).all() and (b.starts == best.starts[sel]).all()
    check(fa, seqs, pwm, t, ids=[200, 3])
    with pytest.raises(KeyError):
        fa.pwm_scan(pwm, min_score=t, ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.pwm_best(pwm, ids=[len(fa)])
    # one strand: the other column of the counts is zero, of the best (INT32_MIN, -1)
    for col, strand in enumerate("+-"):
        h, b = check(fa, seqs, pwm, t, strand=strand)
        assert set(h.strands.tolist()) == {ord(strand)}
        c = fa.pwm_counts(pwm, min_score=t, strand=strand)
        assert not c[:, 1 - col].any() and c[:, col].sum() == h.ids.size
        assert (b.scores[:, 1 - col] == NO_SCORE).all() and (b.starts[:, 1 - col] == -1).all()
        assert (b.scores[:, col] == best.scores[:, col]).all() and (b.starts[:, col] == best.starts[:, col]).all()
    # max_hits
    assert got(fa.pwm_scan(pwm, min_score=t, max_hits=n)) == got(full)
    with pytest.raises(ValueError, match="%d hits, more than max_hits" % n):
        fa.pwm_scan(pwm, min_score=t, max_hits=n - 1)
    none = fa.pwm_scan(pwm, min_score=pwm.max_score + 1, max_hits=0)
    assert [a.size for a in none] == [0] * 5 and [a.dtype for a in none] == [np.int64, np.int64, np.int64, np.uint8, np.int32]
    # the three ways to say the threshold
    assert got(fa.pwm_scan(pwm, pvalue=2e-3)) == got(full)
    assert got(fa.pwm_scan(pwm, threshold=t / pwm.scale)) == got(full)
    assert got(fa.pwm_scan(pwm, threshold=(t - 0.5) / pwm.scale)) == got(full)
    assert (fa.pwm_counts(pwm, pvalue=2e-3) == fa.pwm_counts(pwm, min_score=t)).all()
    assert (fa.pwm_counts(pwm, threshold=t / pwm.scale, strand="-") == fa.pwm_counts(pwm, min_score=t, strand="-")).all()
    for kw in ({}, {"min_score": t, "pvalue": 0.1}, {"threshold": 1.0, "pvalue": 0.1}, {"min_score": 1.5}, {"min_score": t, "strand": "x"},
               {"min_score": t, "max_hits": -1}):
        with pytest.raises(ValueError):
            fa.pwm_scan(pwm, **kw)
    for bad in (pwm.ints, "GAATTC", None):
        with pytest.raises(ValueError):
            fa.pwm_scan(bad, min_score=0)
        with pytest.raises(ValueError):
            fa.pwm_best(bad)
    with pytest.raises(ValueError):
        fa.pwm_counts(pwm)
    with pytest.raises(ValueError):
        fa.pwm_best(pwm, strand="both ")
    # the same answers from an index reopened from its .fxi (the table installed from the file)
    del fa
    fa2 = fx.Fasta(fixture_files["test.fa"])
    assert got(fa2.pwm_scan(pwm, min_score=t)) == got(full)
    # byte-range shards and windows carry no halo for a window across a cut: refused, as search_all refuses them
    monkeypatch.setattr(type(fa2), "_sharded", property(lambda self: True))
    for call in (lambda: fa2.pwm_scan(pwm, min_score=t), lambda: fa2.pwm_counts(pwm, min_score=t), lambda: fa2.pwm_best(pwm)):
        with pytest.raises(NotImplementedError):
            call()
