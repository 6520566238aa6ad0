"""-m gpu: Fasta.orfs and Fasta.translate_many (fx_fasta_orfs, fx_fasta_translate_alloc, csrc/fx_orf.hpp) against the plain
Python truth of orf_truth.py over fa[i].seq -- on the fixtures, on generated files with every line layout at which the 256-byte
run layout can go wrong and stops, starts and invalid letters planted at its edges, on segments that span hundreds of runs, on
texts where every run closes several rows, and on the error paths.  Every comparison is exact equality of all five columns and
of the row order.

One bullet of the issue reads "lower case and N give X" for translate_many.  Its definitions, which it calls the contract,
fold lower case onto A C G T, so here lower case translates like upper case and only N (and every other letter outside
A C G T) gives X."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import orf_truth as T
from conftest import DATA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _table(k):
    """The genetic codes of the search as the truth takes them, from the standard dictionary and the differences NCBI lists:
    -> (amino acids by codon, stops, the table's own starts)"""
    aa = dict(T.STANDARD)
    if k in (2, 4):
        aa["TGA"] = "W"
    if k == 2:
        aa.update({"ATA": "M", "AGA": "*", "AGG": "*"})
    starts = {1: ("TTG", "CTG", "ATG"), 2: ("ATT", "ATC", "ATA", "ATG", "GTG"), 4: ("TTA", "TTG", "CTG", "ATT", "ATC", "ATA", "ATG", "GTG"),
              11: ("TTG", "CTG", "ATT", "ATC", "ATA", "ATG", "GTG")}[k]
    return aa, tuple(c for c, a in aa.items() if a == "*"), starts


def _rows(r):
    assert r.ids.dtype == np.int64 and r.starts.dtype == np.int64 and r.stops.dtype == np.int64
    assert r.frames.dtype == np.int8 and r.flags.dtype == np.uint8
    assert len({len(r), r.ids.size, r.starts.size, r.stops.size, r.frames.size, r.flags.size}) == 1
    return list(zip(r.ids.tolist(), r.starts.tolist(), r.stops.tolist(), r.frames.tolist(), r.flags.tolist()))


def _truth(seqs, min_len=75, table=1, starts=("ATG",), mode="start", strand="both", ids=None):
    _, stops, own = _table(table)
    starts = own if starts == "table" else tuple(c.upper() for c in starts)
    return [(i,) + row for i in (range(len(seqs)) if ids is None else ids) for row in T.orfs(seqs[i], stops, starts, mode, min_len, strand)]


def _same(got, want, what):
    """equal lists of rows; the message names the first difference instead of printing thousands of rows"""
    if got != want:
        k = next((j for j, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        raise AssertionError("%s: %d rows, %d expected; first difference at row %d: %s, expected %s"
                             % (what, len(got), len(want), k, got[k:k + 3], want[k:k + 3]))


def _open(fx, tmp_path, name, raw):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(raw)
    fa = fx.Fasta(path)
    return fa, [fa[i].seq for i in range(len(fa))]


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _build(records, width, eol="\n", untidy=False):
    """records: [(name, seq)] -> (bytes of the file, [(offset of the record's first body byte, bytes to its end)]).  untidy: a
    space inside every third sequence line and a blank line behind every fourth."""
    out, spans = bytearray(), []
    for name, s in records:
        out += (">" + name + eol).encode()
        start = len(out)
        for j, k in enumerate(range(0, len(s), width)):
            ln = s[k:k + width]
            if untidy and j % 3 == 1 and len(ln) > 4:
                ln = ln[:3] + " " + ln[3:]
            out += (ln + eol).encode("latin-1")
            if untidy and j % 4 == 2:
                out += eol.encode()
        spans.append((start, len(out) - start))
    return bytes(out), spans


def _edges(raw, span):
    """Text coordinates of the first letter of every 256-byte run of the record but the first."""
    start, n = span
    return [sum(1 for c in raw[start:x] if c not in (10, 13, 32)) for x in range((start // 256 + 1) * 256, start + n, 256)]


def _put(t, at, word):
    for j, ch in enumerate(word):
        if 0 <= at + j < len(t):
            t[at + j] = ch


# ------------------------------------------------------------------ a. the fixtures
@pytest.fixture(scope="module")
def fixture_truth():
    return {}


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fixtures(fx, tmp_path, fn, fixture_truth):
    shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
    fa = fx.Fasta(str(tmp_path / fn))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert len(seqs) == 211

    def want(**kw):                                            # one truth per setting, shared by the two files
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in fixture_truth:
            fixture_truth[key] = _truth(seqs, **kw)
        return fixture_truth[key]

    r = fa.orfs()
    _same(_rows(r), want(), "defaults")
    assert len(r) == 653                                       # the counts of the issue's prototype
    stop75 = fa.orfs(mode="stop")
    _same(_rows(stop75), want(mode="stop"), "stop to stop")
    assert len(stop75) == 2076
    dense = fa.orfs(mode="stop", min_len=3)
    _same(_rows(dense), want(mode="stop", min_len=3), "stop to stop, every segment")
    assert len(dense) == 8440
    _same(_rows(fa.orfs(min_len=3)), want(min_len=3), "min_len 3")
    _same(_rows(fa.orfs(starts="table")), want(starts="table"), "the table's starts")
    assert len(fa.orfs(min_len=300, starts=("ATG", "CTG", "TTG"))) == len(want(min_len=300, starts="table")) == 96
    for strand in ("+", "-"):
        one = fa.orfs(strand=strand)
        _same(_rows(one), want(strand=strand), "strand " + strand)
        assert bytes(one.strands) == strand.encode() * len(one)
    for table in (2, 4, 11):
        _same(_rows(fa.orfs(table=table, starts="table")), want(table=table, starts="table"), "table %d" % table)
    _same(_rows(fa.orfs(table=2, min_len=30, mode="stop")), want(table=2, min_len=30, mode="stop"), "table 2, stop to stop")
    # the derived columns and the files
    assert r.lengths.tolist() == [b - a for _, a, b, _, _ in want()] and bool(r.has_start.all())
    assert r.complete.tolist() == [fl & 5 == 5 for *_, fl in want()]
    assert _rows(dense.sorted_by_start()) == sorted(want(mode="stop", min_len=3), key=lambda x: (x[0], x[1], x[2], x[3] < 0))
    names = list(fa.keys())
    bed = str(tmp_path / "orfs.bed")
    r.write_bed(bed)
    back = [ln.rstrip("\n").split("\t") for ln in open(bed)]
    assert [(names.index(n), int(x), int(y), s) for n, x, y, _, _, s in back] == [(i, a, b, "+" if f > 0 else "-") for i, a, b, f, _ in want()]
    assert [(w, int(sc)) for _, _, _, w, sc, _ in back] == [("orf%d" % k, b - a) for k, (_, a, b, _, _) in enumerate(want())]
    # proteins: the rows translated one by one; no stop inside; M first
    buf, offs = r.proteins()
    data = bytes(buf)
    prot = [data[offs[k]:offs[k + 1]].decode() for k in range(len(r))]
    assert prot == [T.translate(seqs[i][a:b], "+" if f > 0 else "-") for i, a, b, f, _ in want()]
    assert all(p.startswith("M") and "*" not in p and "X" not in p for p in prot) and offs[-1] == len(data)
    faa = str(tmp_path / "orfs.faa")
    r.write_faa(faa)
    lines = open(faa).read().splitlines()
    assert lines[0::2] == [">%s:%d-%d(%s)" % (names[i], a, b, "+" if f > 0 else "-") for i, a, b, f, _ in want()] and lines[1::2] == prot
    p2 = fa.orfs(table=2, starts="table", min_len=150)
    buf, offs = p2.proteins()
    aa2 = _table(2)[0]
    got = [bytes(buf[offs[k]:offs[k + 1]]).decode() for k in range(len(p2))]
    assert got == [T.translate(seqs[i][a:b], "+" if f > 0 else "-", aa2) for i, a, b, f, _ in _rows(p2)] and not any("*" in p for p in got)


# ------------------------------------------------------------------ b. generated layouts, codons planted at the run edges
N_LAYOUT = 1400                                                # letters of the long records: five runs at the widest lines
PLANTS = ("TAA", "TTA", "ATG", "CAT", "N", "TAG", "CTA", "TGATGA")  # a stop, a START and an invalid letter on either strand; two adjacent stops


def _layout_records(rng, width, eol, untidy):
    """Eight long records with a plant at every run edge of the file, the plant starting 0, 1 and 2 letters in front of the
    edge in turn (so that its last letter, its middle letter and its first letter open a run); short records around them."""
    recs = [("r%d" % k, _rand(rng, N_LAYOUT + k % 3, "ACGT" if k % 2 == 0 else "ACGTacgtNRY")) for k in range(8)]
    recs += [("n%d" % n, "ATGTA"[:n]) for n in range(6)]       # 0 to 5 letters
    recs += [("stops", "TAA" + "GCA" * 98 + "TGA"), ("rstops", "TTA" + "GCA" * 98 + "CTA"), ("low", "atgaaacccgggtttaagtga" * 9),
             ("iupac", "ATGRAAYCCKGGMTTTAA" * 11), ("m1", _rand(rng, 301)), ("m2", _rand(rng, 302))]
    raw, spans = _build(recs, width, eol, untidy)
    out, n_plants = [], 0
    for k, (name, s) in enumerate(recs):
        if not name.startswith("r"):
            out.append((name, s))
            continue
        t = list(s)
        for e in _edges(raw, spans[k]):
            if 8 <= e < len(t) - 8:
                _put(t, e - n_plants % 3, PLANTS[(n_plants // 3) % len(PLANTS)])
                n_plants += 1
        line = width * max(1, 500 // width)
        _put(t, line - 1, "ATG")                               # a codon split by a line break (every plant is, at the narrow widths)
        _put(t, line + 58, "TAA")
        out.append((name, "".join(t)))
    assert n_plants >= 3 * len(PLANTS)                         # every plant at every offset
    return out


@pytest.mark.parametrize("width", [1, 7, 60, 61, 255, 256, 257])
def test_generated_layouts(fx, tmp_path, width):
    rng = np.random.default_rng(2000 + width)
    for tag, eol, untidy in (("lf", "\n", False), ("crlf", "\r\n", False), ("untidy", "\n", True)):
        recs = _layout_records(rng, width, eol, untidy)
        raw, _ = _build(recs, width, eol, untidy)
        fa, seqs = _open(fx, tmp_path, "w%d%s.fa" % (width, tag), raw)
        assert seqs == [s for _, s in recs]
        for kw in (dict(mode="stop", min_len=3), dict(mode="start", min_len=3), dict(mode="start", min_len=30, starts="table"),
                   dict(mode="stop", min_len=60, strand="-")):
            _same(_rows(fa.orfs(**kw)), _truth(seqs, **kw), "width %d %s %s" % (width, tag, kw))
    # the short records, by hand: nothing below three letters; ATG alone; ATGT and ATGTA in the frames that hold a codon
    got = [row for row in _rows(fa.orfs(mode="stop", min_len=3, strand="+")) if 8 <= row[0] < 14]
    assert got == [(11, 0, 3, 1, 4), (12, 0, 3, 1, 4), (12, 1, 4, 2, 0), (13, 0, 3, 1, 4), (13, 1, 4, 2, 0), (13, 2, 5, 3, 0)]
    both = _rows(fa.orfs(mode="stop", min_len=200))            # a stop as the very first and the very last codon, on either strand
    assert (14, 3, 297, 1, 3) in both and (15, 3, 297, -1, 3) in both and not any(row[1] == 0 for row in both if (row[0], row[3]) in ((14, 1), (15, -1)))


# ------------------------------------------------------------------ c. long segments
def test_long_segments(fx, tmp_path):
    base = ("GCA" * 20001)[:60001]                             # no stop in any of the six frames (GCA CAG AGC / TGC CTG GCT)

    def plant(s, *at_word):
        t = list(s)
        for at, w in at_word:
            _put(t, at, w)
        return "".join(t)

    recs = [("none", base), ("atg_first", plant(base, (30, "ATG"))), ("cat_last", plant(base, (59991, "CAT"))),
            ("middle", plant(base, (30000, "ATG"), (30100, "CAT"), (30201, "ATG"), (30302, "CAT"))), ("stop_far", plant(base, (59982, "TAA"))),
            ("both", plant(base, (31, "ATG"), (59982, "TAA"), (100, "CAT"), (40000, "CAT"), (59985, "TTA")))]
    raw, spans = _build(recs, 60)
    assert all(len(_edges(raw, sp)) > 230 for sp in spans)
    fa, seqs = _open(fx, tmp_path, "long.fa", raw)
    assert seqs == [s for _, s in recs]
    for kw in (dict(mode="start"), dict(mode="stop"), dict(mode="start", min_len=3), dict(mode="stop", min_len=59000), dict(mode="start", strand="-")):
        _same(_rows(fa.orfs(**kw)), _truth(seqs, **kw), str(kw))
    got = _rows(fa.orfs())
    assert [row for row in got if row[0] == 0] == []           # no START at all
    assert [row for row in got if row[0] == 1] == [(1, 30, 60000, 1, 4)]                  # one ATG in the first run
    assert [row for row in got if row[0] == 2] == [(2, 0, 59994, -2, 4)]                  # one CAT in the last run
    whole = [row for row in _rows(fa.orfs(mode="stop")) if row[0] == 0]
    assert sorted(row[1:3] for row in whole) == [(0, 60000), (0, 60000), (1, 60001), (1, 60001), (2, 59999), (2, 59999)]


# ------------------------------------------------------------------ d. dense output
@pytest.mark.parametrize("alphabet", ["ACGT", "ACGTacgtNnRY*-U"])
def test_dense_output(fx, tmp_path, alphabet):
    from pyfastx_amd import _lib, orf
    rng = np.random.default_rng(len(alphabet))
    recs = [("dense", _rand(rng, 20000, alphabet)), ("more", _rand(rng, 3000, alphabet))]
    raw, _ = _build(recs, 70)
    fa, seqs = _open(fx, tmp_path, "dense.fa", raw)
    want = _truth(seqs, mode="stop", min_len=3)
    assert len(want) > 2000                                    # every run closes several rows
    _same(_rows(fa.orfs(mode="stop", min_len=3)), want, alphabet)
    _same(_rows(fa.orfs(mode="start", min_len=3, starts="table")), _truth(seqs, mode="start", min_len=3, starts="table"), alphabet + " start")
    _, stop_mask, start_mask = orf.genetic_code(1)
    with pytest.raises(_lib.FxError) as e:                     # n_total of the C entry
        fa._search_blob().fasta_orfs(stop_mask, start_mask, 0, 3, 3, cap=len(want) - 1)
    assert e.value.code == _lib.FX_ERANGE and e.value.n_rows == len(want)


@pytest.mark.parametrize("min_len", [2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 32 + 3, 2 ** 63 - 1])
def test_min_len_beyond_32_bits(fx, tmp_path, min_len):
    """min_len is an int64 in every pass: cut to 32 bits these are negative, 0 or 3, and the count pass alone would count the
    rows that close inside a run.  max_orfs=0 refuses any count above 0."""
    raw, _ = _build([("dense", _rand(np.random.default_rng(4), 20000))], 70)
    fa, _ = _open(fx, tmp_path, "dense.fa", raw)
    for mode in ("stop", "start"):
        r = fa.orfs(min_len=min_len, mode=mode, max_orfs=0)
        assert len(r) == 0 and _rows(r) == []


# ------------------------------------------------------------------ e. ids, limits, a sharded stream
def _mixed(rng):
    recs = [("a", _rand(rng, 900)), ("empty", ""), ("b", "ATG" + _rand(rng, 600) + "TAA"), ("n", "ATGNNNTAA"), ("c", _rand(rng, 1300, "ACGTn"))]
    return recs, _build(recs, 50)[0]


def test_ids_and_limits(fx, tmp_path):
    recs, raw = _mixed(np.random.default_rng(9))
    fa, seqs = _open(fx, tmp_path, "mixed.fa", raw)
    names = list(fa.keys())
    kw = dict(mode="stop", min_len=9)
    for ids in ([4, 0, 2, 4, 1], [1], [3, 3], [2, 1, 0], []):
        _same(_rows(fa.orfs(ids=ids, **kw)), _truth(seqs, ids=ids, **kw), "ids %s" % ids)
        _same(_rows(fa.orfs(ids=[names[i] for i in ids], **kw)), _truth(seqs, ids=ids, **kw), "names %s" % ids)
    with pytest.raises(KeyError):
        fa.orfs(ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.orfs(ids=[len(fa)])
    for bad in (dict(min_len=-1), dict(max_orfs=-1), dict(mode="both"), dict(strand="*"), dict(starts=("TAA",)), dict(starts=("ATGG",)), dict(table=3),
                dict(table=("F" * 63, "-" * 64))):
        with pytest.raises(ValueError):
            fa.orfs(**bad)
    want = _truth(seqs, **kw)
    n = len(want)
    _same(_rows(fa.orfs(max_orfs=n, **kw)), want, "the limit met")
    for cap in (n - 1, 0):
        with pytest.raises(ValueError, match=str(n)):
            fa.orfs(max_orfs=cap, **kw)
    _same(_rows(fa.orfs(**kw)), want, "after the refusals")
    e = fa.orfs(min_len=10 ** 6, max_orfs=0)                   # nothing found: empty arrays of the right types
    assert len(e) == 0 and _rows(e) == [] and len(e.sorted_by_start()) == 0
    buf, offs = e.proteins()
    assert buf.size == 0 and offs.tolist() == [0]


def test_sharded_raises(fx, tmp_path, monkeypatch):
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa.orfs()
    with pytest.raises(NotImplementedError):
        fa.translate_many([0], [0], [3])


# ------------------------------------------------------------------ f. translate_many
def _proteins(buf, offs):
    data = bytes(buf)
    return [data[offs[k]:offs[k + 1]].decode("latin-1") for k in range(len(offs) - 1)]


def test_translate_fixture(fx, tmp_path):
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    rng = np.random.default_rng(4)
    n = 10 ** 4
    ids = rng.integers(0, len(seqs), n)
    lens = np.array([len(seqs[i]) for i in ids])
    a = (rng.random(n) * (lens + 1)).astype(np.int64)
    b = np.minimum(a + rng.integers(0, 400, n), lens)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    want = [T.translate(seqs[i][x:y], "-" if s else "+") for i, x, y, s in zip(ids.tolist(), a.tolist(), b.tolist(), strand.tolist())]
    buf, offs = fa.translate_many(ids, a, b, strand)
    assert buf.dtype == np.uint8 and offs.dtype == np.int64 and offs.size == n + 1 and offs[-1] == buf.size
    assert _proteins(buf, offs) == want
    sub = slice(0, 500)
    by_name = fa.translate_many([names[i] for i in ids[sub]], a[sub], b[sub], ["-" if s else "+" for s in strand[sub]])
    assert _proteins(*by_name) == want[sub]
    plus = fa.translate_many(ids[sub], a[sub], b[sub])
    assert _proteins(*plus) == [T.translate(seqs[i][x:y]) for i, x, y in zip(ids[sub].tolist(), a[sub].tolist(), b[sub].tolist())]
    aa2 = _table(2)[0]
    two = fa.translate_many(ids[sub], a[sub], b[sub], strand[sub], table=2)
    assert _proteins(*two) == [T.translate(seqs[i][x:y], "-" if s else "+", aa2) for i, x, y, s in zip(ids[sub].tolist(), a[sub].tolist(), b[sub].tolist(), strand[sub].tolist())]
    buf, offs = fa.translate_many([], [], [])
    assert buf.size == 0 and offs.tolist() == [0]
    # the errors of fetch_many, with the first query that is not valid
    L = len(seqs[5])
    for q, exc, k in ((([5, 5, 5], [0, L - 2, 0], [3, L + 1, 3]), ValueError, 1), (([5, len(seqs), -1], [0, 0, 0], [3, 3, 3]), IndexError, 1),
                      (([0, 1], [4, 7], [9, 6]), ValueError, 1), (([0, 1, 2], [0, 0, -1], [3, 3, 3]), ValueError, 2)):
        with pytest.raises(exc) as e:
            fa.translate_many(*q)
        assert e.value.first_bad == k
    with pytest.raises(KeyError):
        fa.translate_many(["no_such_record"], [0], [3])
    with pytest.raises(ValueError):
        fa.translate_many([0, 1], [0, 0], [3, 3], strand=["+"])


def test_translate_around_line_breaks_and_run_edges(fx, tmp_path):
    rng = np.random.default_rng(6)
    recs = [("x", _rand(rng, 50)), ("mix", _rand(rng, 700, "ACGTacgtN")), ("y", "atgAAAtgaNTTcat")]
    raw, spans = _build(recs, 60)
    fa, seqs = _open(fx, tmp_path, "tr.fa", raw)
    assert seqs == [s for _, s in recs]
    edges = _edges(raw, spans[1])
    assert len(edges) >= 2
    q = [(1, x, x + n, s) for c in (60, 120, edges[0], edges[1]) for x in range(c - 9, c + 3) for n in range(8) for s in (0, 1)]
    q += [(2, 0, 15, 0), (2, 0, 15, 1), (2, 1, 15, 1), (0, 50, 50, 0), (0, 48, 50, 1)]
    ids, a, b, s = (np.array(col) for col in zip(*q))
    got = _proteins(*fa.translate_many(ids, a, b, s))
    assert got == [T.translate(seqs[i][x:y], "-" if st else "+") for i, x, y, st in q]
    assert got[-5:] == ["MK*XH", "MXSFH", "MXSF", "", ""]     # lower case folds; N gives X on either strand


# ------------------------------------------------------------------ g. the C entries directly
def test_c_abi(fx):
    from pyfastx_amd import _lib, orf
    L = _lib.lib()
    raw = b">a\nCCATGAAATAGGG\n>b\nATGATGTAA\n>c\nNNNN\n"
    seqs = ["CCATGAAATAGGG", "ATGATGTAA", "NNNN"]
    aa64, stop_mask, _ = orf.genetic_code(1)
    atg = 1 << orf.codon_index("ATG")
    b = _lib.Blob.from_bytes(raw, device=0)

    def call(h, stop=stop_mask, start=atg, mode=1, strands=3, min_len=3, ids=None, n_ids=0, max_rows=100, null_out=None):
        out = [C.c_void_p() for _ in range(5)]
        n, tot = C.c_int64(-1), C.c_int64(-1)
        refs = [C.byref(p) for p in out] + [C.byref(n), C.byref(tot)]
        if null_out is not None:
            refs[null_out] = None
        rc = L.fx_fasta_orfs(h, stop, start, mode, strands, min_len, ids, n_ids, max_rows, *refs)
        cols = None
        if rc == 0:
            assert all(p.value for p in out)                   # never NULL after FX_OK, even for 0 rows
            t = n.value
            cols = [_lib.pinned_array(p.value, max(t, 1), dt)[:t] for p, dt in zip(out, (np.int64, np.int64, np.int64, np.int8, np.uint8))]
        else:
            assert not any(p.value for p in out[:5] if null_out is None)
        return rc, n.value, tot.value, cols

    def tr(h, q, strand=None, aa=aa64, null=None, n=None):
        ids, a, e = ((C.c_int64 * len(q))(*col) for col in zip(*q)) if q else (None, None, None)
        sd = None if strand is None else (C.c_uint8 * len(strand))(*strand)
        dst, off, bad = C.c_void_p(), C.c_void_p(), C.c_int64(-5)
        refs = [C.byref(dst), C.byref(off), C.byref(bad)]
        if null is not None:
            refs[null] = None
        rc = L.fx_fasta_translate_alloc(h, len(q) if n is None else n, ids, a, e, sd, aa, ord("X"), *refs)
        if rc:
            assert null is not None or not (dst.value or off.value)
            return rc, bad.value, None
        assert dst.value and off.value                          # never NULL after FX_OK
        o = _lib.pinned_array(off.value, len(q) + 2, np.int64)[:len(q) + 1]
        return rc, bad.value, _proteins(_lib.pinned_array(dst.value, max(int(o[-1]), 1))[:int(o[-1])], o)

    assert call(b._h)[0] == _lib.FX_ESTATE and tr(b._h, [(0, 0, 3)])[0] == _lib.FX_ESTATE          # no table built
    b.fasta_build()
    want = _truth(seqs, min_len=3)
    rc, n, tot, cols = call(b._h)
    assert rc == 0 and n == tot == len(want) == 3
    assert [c.dtype for c in cols] == [np.int64, np.int64, np.int64, np.int8, np.uint8]
    assert list(zip(*(c.tolist() for c in cols))) == want == [(0, 2, 8, 3, 5), (0, 1, 4, -1, 4), (1, 0, 6, 1, 5)]
    rc, n, tot, cols = call(b._h, mode=0)
    assert rc == 0 and list(zip(*(c.tolist() for c in cols))) == _truth(seqs, min_len=3, mode="stop")
    rc, n, tot, cols = call(b._h, start=atg | stop_mask)       # a codon in both masks is a stop
    assert rc == 0 and list(zip(*(c.tolist() for c in cols))) == want
    rc, n, tot, cols = call(b._h, max_rows=2)
    assert rc == _lib.FX_ERANGE and n == 0 and tot == 3
    rc, n, tot, cols = call(b._h, min_len=100)                 # 0 rows, blocks all the same
    assert rc == 0 and n == tot == 0 and all(c.size == 0 for c in cols)
    ids = (C.c_int64 * 3)(1, 2, 0)
    rc, n, tot, cols = call(b._h, ids=ids, n_ids=3, strands=1)
    assert rc == 0 and list(zip(*(c.tolist() for c in cols))) == _truth(seqs, min_len=3, strand="+", ids=[1, 2, 0])
    assert call(b._h, ids=(C.c_int64 * 1)(3), n_ids=1)[0] == _lib.FX_ERANGE
    einval = [dict(h=None), dict(mode=2), dict(mode=-1), dict(strands=0), dict(strands=4), dict(stop=0), dict(start=0), dict(start=stop_mask),
              dict(min_len=-1), dict(max_rows=-1), dict(n_ids=-1), dict(n_ids=2)]
    einval += [dict(null_out=k) for k in range(7)]
    for kw in einval:
        kw.setdefault("h", b._h)
        assert call(**kw)[0] == _lib.FX_EINVAL, kw
    assert call(b._h, start=0, mode=0)[0] == 0                 # stop to stop needs no START
    # translation
    assert tr(b._h, [(0, 2, 11), (0, 1, 4), (2, 0, 4), (1, 0, 8)], [0, 1, 0, 1]) == (0, -1, ["MK*", "M", "X", "YI"])
    assert tr(b._h, [(0, 2, 11)]) == (0, -1, ["MK*"]) and tr(b._h, []) == (0, -1, [])
    assert tr(b._h, [(0, 0, 3), (1, 0, 10), (7, 0, 3)])[:2] == (_lib.FX_ERANGE, 1)
    assert tr(None, [(0, 0, 3)])[0] == _lib.FX_EINVAL and tr(b._h, [(0, 0, 3)], aa=None)[0] == _lib.FX_EINVAL
    assert tr(b._h, [(0, 0, 3)], n=-1)[0] == _lib.FX_EINVAL
    for k in range(3):
        assert tr(b._h, [(0, 0, 3)], null=k)[0] == _lib.FX_EINVAL
    ids1 = (C.c_int64 * 1)(0)
    dst, off, bad = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    assert L.fx_fasta_translate_alloc(b._h, 1, None, ids1, ids1, None, aa64, 88, C.byref(dst), C.byref(off), C.byref(bad)) == _lib.FX_EINVAL
    # a byte-range shard carries no halo for a codon across its cuts
    cut = raw.index(b">b")
    sh = _lib.Blob.from_bytes(raw[cut:], device=0)
    sh.set_shard(cut, 10, True)
    sh.fasta_build()
    assert call(sh._h)[0] == _lib.FX_EINVAL and tr(sh._h, [(0, 0, 3)])[0] == _lib.FX_EINVAL
    # the entry built the rank index itself; giving it back and asking again builds it again
    b.fasta_rank_free()
    assert call(b._h)[1] == 3
