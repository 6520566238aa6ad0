"""-m gpu: Fasta.search_approx / search_approx_counts (fx_fasta_search_approx, csrc/fx_search_approx.hpp) against the
sliding-window oracle of search_approx_truth.py over fa[i].seq: d = 0 against search_all, every line layout the index
accepts, both register forms and their boundary, anchors and their mirror, the limits of the per-run count fields, the cut
at slen, hit offsets across a scan chunk, and the arguments of the object API.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from search_approx_truth import degenerate_revcomp, truth

pytestmark = pytest.mark.gpu

LENGTHS = (2, 12, 31, 32, 33, 40, 64)
BUDGETS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


def _revcomp(p):
    return p[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def _mutate(rng, p, m, keep=()):
    """p with m letters replaced by another base (none of the positions in keep)."""
    q = list(p)
    free = [j for j in range(len(p)) if j not in keep]
    for j in rng.choice(free, m, replace=False):
        q[j] = str(rng.choice([b for b in "ACGT" if b != q[j].upper()]))
    return "".join(q)


def got(h):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], h.mismatches.tolist()))


def check(fa, seqs, p, d, anchor=None, strand="both", degenerate=False, seen=None):
    """search_approx against the oracle, search_approx_counts against the rows; seen[d] collects the distances met."""
    h = fa.search_approx(p, d, anchor=anchor, strand=strand, degenerate=degenerate)
    assert h.ids.dtype == np.int64 and h.starts.dtype == np.int64 and h.stops.dtype == np.int64
    assert h.strands.dtype == np.uint8 and h.mismatches.dtype == np.uint8
    want = truth(seqs, p, d, anchor, strand, degenerate)
    assert got(h) == want, (p, d, anchor, strand, degenerate)
    c = fa.search_approx_counts(p, d, anchor=anchor, strand=strand, degenerate=degenerate)
    assert c.shape == (len(seqs), 2) and c.dtype == np.int64
    bc = np.zeros((len(seqs), 2), dtype=np.int64)
    np.add.at(bc, (h.ids, (h.strands == ord("-")).astype(np.int64)), 1)
    assert (c == bc).all(), (p, d)
    if seen is not None:
        seen.setdefault(d, set()).update(h.mismatches.tolist())
    return h


@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


# ------------------------------------------------------------------ d = 0 is search_all
@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
@pytest.mark.parametrize("upper", [False, True])
def test_no_mismatch_equals_search_all(fx, fixture_files, fn, upper):
    fa = fx.Fasta(fixture_files[fn], uppercase=upper)
    s = fa[3].seq
    cases = [(p, False) for p in ("GAATTC", "gaattc", "A", "AT", s[55:67], s[10:41], s[20:60], s[5:69])]
    cases += [(p, True) for p in ("GANTC", "RGATCY", "NNNNNNNNNNNN", "garyn")]
    for p, deg in cases:
        a, e = fa.search_approx(p, 0, degenerate=deg), fa.search_all(p, degenerate=deg)
        assert got(a) == [r + (0,) for r in zip(e.ids.tolist(), e.starts.tolist(), e.stops.tolist(), [chr(c) for c in e.strands.tolist()])], p
        assert (fa.search_approx_counts(p, 0, degenerate=deg) == fa.search_counts(p, degenerate=deg)).all()
    assert fa.search_approx("GAATTC", 0).ids.size > 10
    for strand in "+-":
        a, e = fa.search_approx("GANTC", 0, strand=strand, degenerate=True), fa.search_all("GANTC", strand=strand, degenerate=True)
        assert (a.ids == e.ids).all() and (a.starts == e.starts).all() and (a.strands == e.strands).all() and not a.mismatches.any()


# ------------------------------------------------------------------ line layouts
def _layout(name):
    rng = np.random.default_rng(2027)
    if name == "irregular":                   # irregular line lengths and blank lines inside records; records start mid-block
        recs = []
        for i in range(8):
            s = _rand(rng, int(rng.integers(70, 900)))
            lines, a = [], 0
            while a < len(s):
                k = int(rng.integers(1, 90))
                lines.append(s[a:a + k])
                a += k
                if rng.random() < 0.15:
                    lines.append("")
            recs.append(">irr%d\n" % i + "\n".join(lines) + "\n")
        return "".join(recs)
    if name == "crlf":                        # CRLF, spaces inside sequence lines, soft-masked lower case
        recs = []
        for i in range(6):
            s = _rand(rng, int(rng.integers(100, 700)), "ACGTacgt")
            lines = [s[a:a + 60] for a in range(0, len(s), 60)]
            lines = [ln[:10] + " " + ln[10:] if j % 3 == 1 else ln for j, ln in enumerate(lines)]
            recs.append(">crlf%d desc\r\n" % i + "\r\n".join(lines) + "\r\n")
        return "".join(recs)
    if name == "odd":                         # N runs, bytes that are no IUPAC letter, empty records, a record shorter than every
        #                                       pattern but L = 2, records of exactly L letters, an unterminated last line
        exact = ["".join(_rand(rng, L)) for L in LENGTHS]
        return "".join([">n0\n" + "ACGTN" * 20 + "NNNNNNNNNNNNNNNNNNNN\n" + "GAA-TTC*GAATTC12RYKM\n", ">empty\n", ">short\nGA\n",
                        ">mixed\n" + _rand(rng, 300, "ACGTNRYKM-*.") + "\n", ">empty2\n\n"] +
                       [">exact%d\n%s\n" % (len(s), s) for s in exact] + [">last\nGAATTCAAAAGAATTC"])
    assert name == "long"                     # a record far longer than one lane's run: hits straddle many block edges
    long = _rand(rng, 50_000)
    return "".join([">long\n" + "\n".join(long[a:a + 70] for a in range(0, len(long), 70)) + "\n", ">edge1\nGAATTCACGTACGTACGATTTTGAATTC\n",
                    ">poly\nAAAA\n", ">edge3\n" + "C" * 300 + "\n"])


@pytest.mark.parametrize("name,upper", [("irregular", False), ("crlf", False), ("crlf", True), ("odd", False), ("long", False)])
def test_layouts(fx, tmp_path, name, upper):
    fa = fx.Fasta(_write(tmp_path / (name + ".fa"), _layout(name)), uppercase=upper)
    seqs = [fa[i].seq for i in range(len(fa))]
    rng = np.random.default_rng(len(name))
    seen, turn = {}, {}
    for L in LENGTHS:
        src = [s for s in seqs if len(s) >= L]
        for d in (d for d in BUDGETS if d <= L - 1):
            # two patterns cut from a record: one with d letters changed, one with fewer (0, 1, .. in turn)
            turn[d] = turn.get(d, -1) + 1
            for m in (d, turn[d] % d):
                s = src[int(rng.integers(0, len(src)))]
                a = int(rng.integers(0, len(s) - L + 1))
                h = check(fa, seqs, _mutate(rng, s[a:a + L], m), d, seen=seen)
                assert h.ids.size >= 1
    # records of exactly L letters, searched with themselves: the single window, and both edges of the record
    for i, s in enumerate(seqs):
        if 2 <= len(s) <= 64 and set(s) <= set("ACGT"):
            d = min(2, len(s) - 1)
            h = check(fa, seqs, _mutate(rng, s, d), d, strand="+", seen=seen)
            assert (i, 0, len(s), "+", d) in got(h)
    for p, d in (("GANTC", 1), ("RGATCY", 2), ("ACGTRYKMSWBDHVNU", 5), ("n" * 33, 8)):
        check(fa, seqs, p, d, degenerate=True, seen=seen)
    for d in BUDGETS:                          # a set that only ever meets distance 0 would hide the levels
        assert seen[d] >= set(range(d + 1)), (d, seen[d])


# ------------------------------------------------------------------ the two register forms and their boundary
def _planted(rng, n, sites):
    """A random text of n letters with the given (position, string) sites written over it."""
    t = list(_rand(rng, n))
    for a, s in sites:
        t[a:a + len(s)] = s
    return "".join(t)


def test_form_boundary(fx, tmp_path):
    """L = 32 (bit 31 of the forward half, bit 63 of the shared word) and L = 33 (two words) with the same 32-letter core, both
    strands, d = 4; L = 64 at d = 8 (bit 63 of both words).  Copies with 0..5 (0..9) changed letters, the first and the last
    letter among them, on both strands."""
    rng = np.random.default_rng(31)
    core64 = _rand(rng, 64)
    p32, p33 = core64[:32], core64[:33]
    sites, a = [], 50
    for m in (0, 1, 2, 3, 4, 5):
        for q in (p33, _revcomp(p33)):
            s = _mutate(rng, q, m)
            sites.append((a, s))
            a += 100
    for flip in ((0,), (31,), (32,), (0, 31), (0, 32), (31, 32)):                  # the edge letters of both patterns, on both strands
        s = "".join("ACGT"["ACGT".index(c) ^ 1] if j in flip else c for j, c in enumerate(p33))
        sites += [(a, s), (a + 100, _revcomp(s))]
        a += 200
    for m in (0, 1, 4, 7, 8, 9):
        sites += [(a, _mutate(rng, core64, m)), (a + 150, _revcomp(_mutate(rng, core64, m)))]
        a += 300
    for flip in ((0, 63), (63,), (0,)):
        s = "".join("ACGT"["ACGT".index(c) ^ 1] if j in flip else c for j, c in enumerate(core64))
        sites += [(a, _mutate(rng, s, 6, keep=flip)), (a + 150, _revcomp(_mutate(rng, s, 6, keep=flip)))]
        a += 300
    text = _planted(rng, a + 100, sites)
    fa = fx.Fasta(_write(tmp_path / "forms.fa", ">forms\n" + "\n".join(text[i:i + 61] for i in range(0, len(text), 61)) + "\n"))
    seqs = [fa[0].seq]
    assert seqs[0] == text
    seen = {}
    h32, h33 = check(fa, seqs, p32, 4, seen=seen), check(fa, seqs, p33, 4, seen=seen)
    assert seen[4] == {0, 1, 2, 3, 4}
    for h in (h32, h33):
        assert {"+", "-"} == {r[3] for r in got(h)} and h.ids.size >= 20
    h64 = check(fa, seqs, core64, 8, seen=seen)
    assert seen[8] >= {0, 1, 4, 7, 8} and h64.ids.size >= 14 and {"+", "-"} == {r[3] for r in got(h64)}
    for d in range(9):                                                            # every budget in both forms
        check(fa, seqs, p32, d)
        check(fa, seqs, p33, d)


# ------------------------------------------------------------------ anchors
def test_anchor(fx, tmp_path):
    rng = np.random.default_rng(23)
    guide = _rand(rng, 20)
    good, broken, sites, a = [], [], [], 40
    for m in (0, 1, 2, 3, 4):
        for pam_ok in (True, False):
            for minus in (False, True):
                site = _mutate(rng, guide, m) + str(rng.choice(list("ACGT"))) + ("GG" if pam_ok else str(rng.choice(["GA", "CG", "TT", "AG"])))
                sites.append((a, _revcomp(site) if minus else site))
                (good if pam_ok and m <= 3 else broken).append((0, a, a + 23, "-" if minus else "+"))
                a += 60
    text = _planted(rng, a + 40, sites)
    fa = fx.Fasta(_write(tmp_path / "guides.fa", ">g\n" + "\n".join(text[i:i + 50] for i in range(0, len(text), 50)) + "\n"))
    seqs = [fa[0].seq]
    p = guide + "NGG"
    # the PAM held, three mismatches in the guide, both strands: every planted site with a whole PAM, none with a broken one
    h = check(fa, seqs, p, 3, anchor=slice(20, 23), degenerate=True)
    rows = {r[:4] for r in got(h)}
    assert set(good) <= rows and not (set(broken) & rows)
    assert sorted({r[4] for r in got(h) if r[:4] in set(good)}) == [0, 1, 2, 3]
    free = {r[:4] for r in got(check(fa, seqs, p, 3, degenerate=True))}           # without the anchor some broken PAMs come back
    assert rows < free and set(broken) & free
    # single positions, and the mirror on '-' alone
    for anchor in ([0], [22], [0, 1, 2, 3, 4]):
        for strand in ("both", "+", "-"):
            check(fa, seqs, p, 3, anchor=anchor, strand=strand, degenerate=True)
    q = _mutate(rng, text[405:425], 2, keep=range(0, 10))                          # exact mode, mismatches in the second half
    for anchor in ([0], [19], range(10, 20), range(0, 10), slice(3, 17, 2)):
        for strand in ("both", "-"):
            check(fa, seqs, q, 3, anchor=anchor, strand=strand)
    assert (0, 405, 425, "+", 2) in got(fa.search_approx(q, 2, anchor=range(0, 10)))
    assert (0, 405, 425, "+", 2) not in got(fa.search_approx(q, 2, anchor=range(10, 20)))
    rq = _revcomp(q)                          # searched as its reverse complement the same site is a '-' hit and the anchor mirrors
    assert (0, 405, 425, "-", 2) in got(fa.search_approx(rq, 2, anchor=range(10, 20), strand="-"))
    assert (0, 405, 425, "-", 2) not in got(fa.search_approx(rq, 2, anchor=range(0, 10), strand="-"))
    # everything held: d plays no part
    for pat, deg in ((p, True), (q, False)):
        e = fa.search_all(pat, degenerate=deg)
        a_ = fa.search_approx(pat, 3, anchor=slice(None), degenerate=deg)
        assert (a_.ids == e.ids).all() and (a_.starts == e.starts).all() and (a_.strands == e.strands).all() and not a_.mismatches.any()


# ------------------------------------------------------------------ the 9-bit count fields, order at one start
def test_field_limits(fx, tmp_path):
    fa = fx.Fasta(_write(tmp_path / "poly.fa", ">polyA\n" + "A" * 2000 + "\n>sites\nTTGAATTCTTGAATTGTTCAATTCTT\n"))
    seqs = [fa[i].seq for i in range(len(fa))]
    # AT against AA: one mismatch, on + and on - (AT is its own reverse complement): 256 + 256 hits in every full run
    h = fa.search_approx("AT", 1, ids=[0])
    assert got(h) == [(0, j, j + 2, s, 1) for j in range(1999) for s in "+-"]
    assert fa.search_approx_counts("AT", 1)[0].tolist() == [1999, 1999]
    h = fa.search_approx("AAAA", 1, ids=[0])                                      # TTTT is four letters away
    assert got(h) == [(0, j, j + 4, "+", 0) for j in range(1997)]
    # a palindrome: both strands at every site, '+' first, the same distance
    h = check(fa, seqs, "GAATTC", 1)
    assert [r for r in got(h) if r[0] == 1] == [(1, 2, 8, "+", 0), (1, 2, 8, "-", 0), (1, 10, 16, "+", 1), (1, 10, 16, "-", 1),
                                                (1, 18, 24, "+", 1), (1, 18, 24, "-", 1)]
    # GAATTG / CAATTC: different distances at one start
    h = check(fa, seqs, "GAATTG", 2)
    assert [r for r in got(h) if r[0] == 1] == [(1, 2, 8, "+", 1), (1, 2, 8, "-", 1), (1, 10, 16, "+", 0), (1, 10, 16, "-", 2),
                                                (1, 18, 24, "+", 2), (1, 18, 24, "-", 0)]


# ------------------------------------------------------------------ the cut at slen
def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: the index counts two bytes off every
    line, so slen is smaller than the number of kept bytes and `seq` stops there -- no window may reach past that cut."""
    rng = np.random.default_rng(55)
    recs, kept, tails = [], [], []
    for i, n_lines in enumerate((3, 12, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        tails.append(lines[-1][-12:])
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert [len(s) for s in seqs] == [len(fa[i]) for i in range(len(fa))]
    assert any(len(s) < n for s, n in zip(seqs, kept)), "no record is cut: the case is not exercised"
    pats = [_mutate(rng, t, m) for t, m in zip(tails, (0, 1, 2, 0, 2))]            # the last kept letters: behind the cut where there is one
    pats += [_mutate(rng, seqs[4][-12:], 1), _mutate(rng, seqs[4][-20:-8], 2), seqs[2][-31:], _mutate(rng, seqs[1][-40:], 2)]
    for p in pats:
        h = check(fa, seqs, p, 2)
        assert (h.stops <= np.array([len(s) for s in seqs])[h.ids]).all(), p
    assert fa.search_approx(seqs[4][-12:], 0, strand="+").ids.size >= 1


# ------------------------------------------------------------------ hit offsets across a chunk of the scans
def test_scan_chunk(fx, tmp_path):
    """One record of more than 4096 runs: the offsets of the hits behind run 4096 carry the sum of a whole scan chunk."""
    rng = np.random.default_rng(77)
    n = 1_100_000
    p = _rand(rng, 12)
    text = _planted(rng, n, [(n - 40, p), (n - 12, _revcomp(p))])
    fa = fx.Fasta(_write(tmp_path / "big.fa", ">big\n" + "\n".join(text[i:i + 80] for i in range(0, n, 80)) + "\n"))
    h = fa.search_approx(p, 3)
    want = truth([text], p, 3, rev=_revcomp(p))
    assert 200 <= len(want) <= 3000
    assert got(h) == want
    assert sorted(set(h.mismatches.tolist())) == [0, 1, 2, 3] and int((h.starts > 4096 * 256).sum()) >= 2
    c = fa.search_approx_counts(p, 3)
    assert c.tolist() == [[sum(r[3] == "+" for r in want), sum(r[3] == "-" for r in want)]]


# ------------------------------------------------------------------ counts, ids, limits, arguments
def test_counts_ids_limits(fx, fixture_files, monkeypatch):
    fa = fx.Fasta(fixture_files["test.fa"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    full = check(fa, seqs, "GAATTC", 1)
    sel = [5, 0, 17, 5]
    keep = np.isin(full.ids, [0, 5, 17])
    want = got(type(full)(*(a[keep] for a in full)))
    assert len(want) > 3
    assert got(fa.search_approx("GAATTC", 1, ids=sel)) == want                    # unsorted and repeated: as search_all treats them
    assert got(fa.search_approx("GAATTC", 1, ids=[names[i] for i in sel])) == want
    e = fa.search_all("GAATTC", ids=sel)
    assert [r[:4] for r in got(fa.search_approx("GAATTC", 0, ids=sel))] == list(zip(e.ids.tolist(), e.starts.tolist(), e.stops.tolist(),
                                                                                    [chr(c) for c in e.strands.tolist()]))
    with pytest.raises(KeyError):
        fa.search_approx("GAATTC", 1, ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.search_approx("GAATTC", 1, ids=[len(fa)])
    n = full.ids.size
    assert n > 100
    assert got(fa.search_approx("GAATTC", 1, max_hits=n)) == got(full)
    with pytest.raises(ValueError, match=str(n)):
        fa.search_approx("GAATTC", 1, max_hits=n - 1)
    for p, d, kw in (("GAATTC", -1, {}), ("GAATTC", 9, {}), ("GAATTC", 6, {}), ("A", 1, {}), ("ACGTACGTACGT", 9, {}), ("GAATTC", 1.5, {}),
                     ("GAATTC", 1, {"anchor": [6]}), ("GAATTC", 1, {"anchor": [-1]}), ("GAATTC", 1, {"anchor": [0.5]}),
                     ("GAATTC", 1, {"strand": "x"}), ("", 0, {}), ("A" * 65, 1, {}), ("GA TC", 1, {}), ("GAXTC", 1, {"degenerate": True})):
        with pytest.raises(ValueError):
            fa.search_approx(p, d, **kw)
        with pytest.raises(ValueError):
            fa.search_approx_counts(p, d, **kw)
    # the same answers from an index reopened from its .fxi (the table installed from the file)
    del fa
    fa2 = fx.Fasta(fixture_files["test.fa"])
    assert got(fa2.search_approx("GAATTC", 1)) == got(full)
    assert got(fa2.search_approx("GAATTC", 1, ids=sel)) == want
    # byte-range shards and windows carry no halo for a hit across a cut: refused, as search_all refuses them
    monkeypatch.setattr(type(fa2), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa2.search_approx("GAATTC", 1)
    with pytest.raises(NotImplementedError):
        fa2.search_approx_counts("GAATTC", 1)
