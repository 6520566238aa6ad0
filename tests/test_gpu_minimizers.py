"""-m gpu: Fasta.minimizers / minimizer_counts (fx_fasta_minimizers, csrc/fx_minimizer.hpp) against the brute-force model of
minimizer_truth.py over fa[i].seq: every line layout the index accepts, layout invariance, every phase of a record's first
byte against the 256-byte runs, invalid letters around run boundaries, ties, the limits of the per-run count fields, the
k-mer tables of the existing device code, the cut at slen, row offsets across a scan chunk, and the arguments of the object
API.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from minimizer_truth import keys, truth
from test_gpu_search_approx import _layout                   # the layouts of the approximate search, generated the same way

pytestmark = pytest.mark.gpu

PAIRS = ((1, 1), (2, 32), (15, 10), (16, 16), (17, 2), (31, 32), (31, 1))
FORMS = [(c, o) for o in ("hash", "lex") for c in (True, False)]
DTYPES = [np.int64, np.int64, np.int64, np.uint8, np.uint64]
_TRUTH = {}


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


def _model(seqs, k, w, canonical, order, ids=None):
    """truth(), computed once per text and form (test.fa and test.fa.gz hold the same records)."""
    key = (hash(tuple(seqs)), k, w, canonical, order, None if ids is None else tuple(ids))
    if key not in _TRUTH:
        _TRUTH[key] = truth(seqs, k, w, canonical, order, ids)
    return _TRUTH[key]


def got(m):
    return list(zip(m.ids.tolist(), m.starts.tolist(), [chr(c) for c in m.strands.tolist()], m.codes.tolist()))


def check(fa, seqs, k, w, canonical=True, order="hash", ids=None):
    """minimizers against the model, minimizer_counts against the rows."""
    m = fa.minimizers(k, w, canonical=canonical, order=order, ids=ids)
    assert [a.dtype for a in m] == DTYPES
    rows, counts = _model(seqs, k, w, canonical, order, ids)
    assert got(m) == rows, (k, w, canonical, order)
    assert (m.stops == m.starts + k).all()
    if ids is None:
        c = fa.minimizer_counts(k, w, canonical=canonical, order=order)
        assert c.shape == (len(seqs), 2) and c.dtype == np.int64
        assert (c == counts).all(), (k, w, canonical, order)
    return m


def _seqs(fa):
    return [fa[i].seq for i in range(len(fa))]


# ------------------------------------------------------------------ line layouts
@pytest.mark.parametrize("k,w", PAIRS)
@pytest.mark.parametrize("name", ["irregular", "crlf", "odd", "long", "test.fa", "test.fa.gz"])
def test_layouts(fx, tmp_path, name, k, w):
    """Irregular lines with blank lines; CRLF with spaces and lower case; N runs, bytes that are no letter, empty and short
    records and an unterminated last line; a record of 50 000 letters; the fixture, plain and gzipped."""
    if name.startswith("test.fa"):
        shutil.copy(os.path.join(DATA, name), tmp_path / name)
        fa = fx.Fasta(str(tmp_path / name))
    else:
        fa = fx.Fasta(_write(tmp_path / (name + ".fa"), _layout(name)))
    seqs = _seqs(fa)
    n = 0
    for canonical, order in FORMS:
        n += check(fa, seqs, k, w, canonical, order).ids.size
    assert n > 0


# ------------------------------------------------------------------ layout invariance
def test_layout_invariance(fx, tmp_path):
    rng = np.random.default_rng(41)
    seqs = [_rand(rng, n, a) for n, a in ((70, "ACGT"), (256, "ACGT"), (257, "ACGTacgt"), (900, "ACGT"), (513, "ACGTN"), (33, "ACGT"), (1200, "ACGTacgtNR"),
                                          (41, "AC"))]
    want = {}
    for width in (1, 7, 60, 255, 256, 257, None):
        for eol in ("\n", "\r\n"):
            text = "".join(">s%d%s%s%s" % (i, eol, eol.join(s[a:a + (width or len(s))] for a in range(0, len(s), width or len(s))), eol)
                           for i, s in enumerate(seqs))
            fa = fx.Fasta(_write(tmp_path / ("inv_%s_%d.fa" % (width, len(eol))), text))
            assert _seqs(fa) == seqs
            for k, w, canonical, order in ((15, 10, True, "hash"), (31, 32, True, "lex"), (4, 5, False, "hash")):
                rows = got(fa.minimizers(k, w, canonical=canonical, order=order))
                if (k, w) not in want:
                    want[k, w] = _model(seqs, k, w, canonical, order)[0]
                    assert len(want[k, w]) > 20
                assert rows == want[k, w], (width, eol, k, w)


# ------------------------------------------------------------------ the phase of a record's first byte
@pytest.mark.parametrize("k,w", [(15, 10), (31, 32)])
def test_record_start_phase(fx, tmp_path, k, w):
    """For every d in 0 .. w + k: a record of 700 letters on one line whose first sequence byte sits at offset 256 - d of a
    256-byte block of the stream (the header is padded), so the look-back of its second run crosses the record's first byte
    for small d and the third run's lies in the second; and records of exactly w + k - 2 (no window), w + k - 1 (one) and
    w + k letters at the same phases."""
    rng = np.random.default_rng(k)
    raw, seqs, firsts = b"", [], []
    for d in range(w + k + 1):
        for n in (700, w + k - 2, w + k - 1, w + k):
            name = ">d%d_%d x" % (d, n)
            pad = (256 - d - (len(raw) + len(name) + 1)) % 256
            raw += (name + "x" * pad + "\n").encode()
            firsts.append((len(raw), d))
            seqs.append(_rand(rng, n))
            raw += seqs[-1].encode() + b"\n"
    assert all(off % 256 == (256 - d) % 256 and raw[off - 1:off] == b"\n" for off, d in firsts)
    fa = fx.Fasta(_write(tmp_path / "phase.fa", raw))
    assert _seqs(fa) == seqs
    for canonical, order in ((True, "hash"), (False, "lex")):
        m = check(fa, seqs, k, w, canonical, order)
        per = np.bincount(m.ids, minlength=len(seqs))
        assert (per[1::4] == 0).all() and (per[2::4] == 1).all() and (per[3::4] >= 1).all() and (per[0::4] > 20).all()


# ------------------------------------------------------------------ invalid letters
def test_invalid_letters(fx, tmp_path):
    """(15, 10), one line, letter i at stream offset 5 + i.  A single N at kept index -1, 0 and 1 of a run; stretches of N of
    w + k - 2, w + k - 1 and w + k letters (around the w + k - 1 letters a lane warms up on) that end at a run boundary, in
    front of one and behind one; U and IUPAC letters.  An N voids the k positions whose k-mer holds it, so with k > w every
    one of them makes windows without a selection, and the selection after such a hole is a new row."""
    k, w = 15, 10
    rng = np.random.default_rng(15)
    hdr, n = ">inv\n", 256 * 32
    t = list(_rand(rng, n))
    edge = lambda j: 256 * j - len(hdr)                      # the letter that is kept index 0 of run j
    for j, o in ((1, -1), (2, 0), (3, 1)):
        t[edge(j) + o] = "N"
    j = 5
    for length in (w + k - 2, w + k - 1, w + k):
        for last in (-1, -4, 3):                             # kept index of the stretch's last N
            z = edge(j) + last + 1
            t[z - length:z] = "N" * length
            j += 2
    assert j < 30
    text = "".join(t)
    other = _rand(rng, 900, "ACGTUuRYKMSWBDHVN*-acgt")
    fa = fx.Fasta(_write(tmp_path / "inv.fa", hdr + text + "\n>other\n" + other + "\n>onlyN\n" + "N" * 300 + "\n"))
    seqs = _seqs(fa)
    assert seqs == [text, other, "N" * 300]
    ky = keys(text, k)
    empty = [p for p in range(len(ky) - w + 1) if all(e is None for e in ky[p:p + w])]
    assert len(empty) >= 12 * (k - w + 1)                    # the case is exercised: holes behind all twelve places
    for canonical, order in FORMS:
        m = check(fa, seqs, k, w, canonical, order)
        assert not (m.ids == 2).any()
    assert fa.minimizer_counts(k, w)[2].tolist() == [0, 0]


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("w", [1, 4, 32])
@pytest.mark.parametrize("k", [3, 4])
def test_ties(fx, tmp_path, k, w):
    """Homopolymers and (AC)n of 600 letters: every run is mid-stretch, every window a tie, the leftmost wins.  ACGT repeated:
    at k = 4 the k-mer ACGT is its own reverse complement and its strand is '+'."""
    seqs = ["A" * 600, "T" * 600, "AC" * 300, "ACGT" * 150, "G" * 300 + "C" * 300, "AC" * 150 + "N" + "GT" * 150]
    fa = fx.Fasta(_write(tmp_path / "ties.fa", "".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(seqs))))
    for canonical, order in FORMS:
        m = check(fa, seqs, k, w, canonical, order)
        if canonical:
            assert set(m.strands[m.ids == 0].tolist()) == {ord("+")} and set(m.strands[m.ids == 1].tolist()) == {ord("-")}
        if canonical and k == 4:
            pal = (m.ids == 3) & (m.codes == 27)             # ACGT = 0 1 2 3
            assert (m.strands[pal] == ord("+")).all() and (w > 1 or pal.sum() == 150)
        if w == 1:
            assert (m.ids == 0).sum() == 600 - k + 1


# ------------------------------------------------------------------ the 9-bit count fields
def test_field_limits(fx, tmp_path):
    """w = 1 on one line of valid letters: every position is a row, 256 rows in every full run.  Poly-A and poly-T halves at
    k = 1, canonical: runs that are all '+', runs that are all '-'."""
    rng = np.random.default_rng(8)
    seqs = ["A" * 1000 + "T" * 1000, _rand(rng, 2000), "T" * 700 + "A" * 700]
    fa = fx.Fasta(_write(tmp_path / "line.fa", "".join(">f%d\n%s\n" % (i, s) for i, s in enumerate(seqs))))
    m = check(fa, seqs, 1, 1, True, "hash")
    assert m.starts[m.ids == 0].tolist() == list(range(2000)) and not m.codes[m.ids != 1].any()
    assert m.strands[m.ids == 0].tobytes() == b"+" * 1000 + b"-" * 1000
    assert fa.minimizer_counts(1, 1).tolist()[0] == [1000, 1000]
    for k, canonical, order in ((1, True, "lex"), (1, False, "hash"), (2, True, "hash"), (9, True, "lex")):
        m = check(fa, seqs, k, 1, canonical, order)
        assert m.starts[m.ids == 1].tolist() == list(range(2000 - k + 1))


# ------------------------------------------------------------------ against the k-mer tables of the existing device code
def test_w1_equals_kmer_tables(fx, tmp_path):
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    for canonical in (True, False):
        for k in (13, 31):
            m = fa.minimizers(k, 1, canonical=canonical, order="lex")
            codes, counts = np.unique(m.codes, return_counts=True)
            t = fa.kmer_table(k, canonical=canonical)
            assert codes.size > 1000 and np.array_equal(codes.astype(np.int64), t.codes) and np.array_equal(counts, t.counts), (k, canonical)
            h = fa.minimizers(k, 1, canonical=canonical, order="hash")     # with w = 1 the order chooses nothing
            assert got(h) == got(m)
        m = fa.minimizers(5, 1, canonical=canonical)
        assert np.array_equal(np.bincount(m.codes.astype(np.int64), minlength=4 ** 5), fa.kmer_counts(5, canonical=canonical))


# ------------------------------------------------------------------ the cut at slen
def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: the index takes every line for a CR LF
    line, so slen is smaller than the number of kept bytes (by one per later line) and `seq` stops there.  No row may reach
    behind the cut, and what lies behind it changes nothing in front."""
    rng = np.random.default_rng(55)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 20, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = _seqs(fa)
    lens = np.array([len(fa[i]) for i in range(len(fa))])
    assert [len(s) for s in seqs] == lens.tolist()
    assert sum(n > len(s) for s, n in zip(seqs, kept)) >= 3, "the case is not exercised"
    for k, w in ((15, 10), (5, 1), (31, 32)):
        for canonical, order in ((True, "hash"), (False, "lex")):
            m = check(fa, seqs, k, w, canonical, order)
            assert (m.stops <= lens[m.ids]).all() and m.ids.size > 0


# ------------------------------------------------------------------ row offsets across a chunk of the scans
def test_scan_chunk(fx, tmp_path):
    """One record of more than 4096 runs, all with rows: the offsets of the rows behind run 4096 carry the sum of a scan chunk."""
    rng = np.random.default_rng(77)
    n = 1_100_000
    text = _rand(rng, n)
    fa = fx.Fasta(_write(tmp_path / "big.fa", ">big\n" + "\n".join(text[i:i + 80] for i in range(0, n, 80)) + "\n"))
    m = check(fa, [text], 15, 10)
    assert int((m.starts > 4096 * 256).sum()) > 1000 and (np.diff(m.starts) > 0).all()
    assert 0.95 <= m.density([n])[0] * 11 / 2 <= 1.05


# ------------------------------------------------------------------ ids, limits, arguments
def test_arguments(fx, tmp_path, monkeypatch):
    from pyfastx_amd import _lib, minimizer
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    seqs = _seqs(fa)
    names = list(fa.keys())
    k, w = 15, 10
    full = check(fa, seqs, k, w)
    n = full.ids.size
    assert n > 10000 and [a.dtype for a in full] == DTYPES
    # ids: a subset, reversed, repeated, by name -- np.unique semantics, as search_all
    keep = np.isin(full.ids, [0, 5, 17])
    want = got(type(full)(*(a[keep] for a in full)))
    assert len(want) > 30
    for sel in ([0, 5, 17], [17, 5, 0], [5, 0, 17, 5], [names[i] for i in (17, 0, 5)]):
        assert got(fa.minimizers(k, w, ids=sel)) == want, sel
    check(fa, seqs, k, w, False, "lex", ids=[200, 3])
    with pytest.raises(KeyError):
        fa.minimizers(k, w, ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.minimizers(k, w, ids=[len(fa)])
    # max_hits
    assert got(fa.minimizers(k, w, max_hits=n)) == got(full)
    with pytest.raises(ValueError, match="%d minimizers, more than max_hits" % n):
        fa.minimizers(k, w, max_hits=n - 1)
    with pytest.raises(ValueError):
        fa.minimizers(k, w, max_hits=-1)
    tiny = fx.Fasta(_write(tmp_path / "tiny.fa", ">a\nACGTACGT\n>b\n\n"))
    none = tiny.minimizers(k, w, max_hits=0)                 # no record reaches w + k - 1 letters: no row, and 0 is room enough
    assert [a.size for a in none] == [0] * 5 and [a.dtype for a in none] == DTYPES and tiny.minimizer_counts(k, w).tolist() == [[0, 0]] * 2
    # k, w, order
    for bad in ((0, 10), (32, 10), (15, 0), (15, 33), (15.0, 10), ("15", 10)):
        with pytest.raises(ValueError):
            fa.minimizers(*bad)
        with pytest.raises(ValueError):
            fa.minimizer_counts(*bad)
    with pytest.raises(ValueError):
        fa.minimizers(k, w, order="random")
    # the methods of the rows
    assert full.hashes().dtype == np.uint64 and (full.hashes() == minimizer.mix(full.codes, k)).all()
    comp = str.maketrans("ACGT", "TGCA")
    words = [seqs[i][a:z].upper() for i, a, z in zip(full.ids.tolist(), full.starts.tolist(), full.stops.tolist())]
    assert full.kmers() == [x if s == ord("+") else x[::-1].translate(comp) for x, s in zip(words, full.strands.tolist())]
    assert full.write_bed(tmp_path / "m.bed", names) == n
    d = full.density([len(s) for s in seqs])
    assert d.shape == (len(seqs),) and 0.12 < d[np.array([len(s) for s in seqs]) > 300].mean() < 0.25       # 2 / 11 = 0.18
    # through the library: what the numbers alone decide
    blob = fa._search_blob()
    for bk, bw, bf in ((0, 10, 1), (32, 10, 1), (15, 0, 1), (15, 33, 1), (15, 10, 4)):
        with pytest.raises(_lib.FxError) as e:
            blob.fasta_minimizers(bk, bw, bf, cap=10)
        assert e.value.code == _lib.FX_EINVAL, (bk, bw, bf)
    with pytest.raises(_lib.FxError) as e:
        blob.fasta_minimizers(k, w, 1, cap=5)
    assert e.value.code == _lib.FX_ERANGE and e.value.n_hits == n
    # the same answers from an index reopened from its .fxi (the table installed from the file)
    del fa, blob
    fa2 = fx.Fasta(str(tmp_path / "test.fa"))
    assert got(fa2.minimizers(k, w)) == got(full)
    # byte-range shards and windows carry no halo for a window across a cut: refused, as search_all refuses them
    monkeypatch.setattr(type(fa2), "_sharded", property(lambda self: True))
    for call in (lambda: fa2.minimizers(k, w), lambda: fa2.minimizer_counts(k, w)):
        with pytest.raises(NotImplementedError):
            call()
