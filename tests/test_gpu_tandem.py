"""-m gpu: Fasta.tandem_repeats (fx_fasta_tandem_repeats, csrc/fx_tandem.hpp) against the plain Python truth of
tandem_truth.py over fa[i].seq -- on the fixtures, on generated files with every line layout at which the 256-byte run layout
can go wrong and repeats planted at its edges, on stretches that span hundreds of runs, on texts where every run closes
several rows, and on the error paths.  Every comparison is exact equality of all five columns and of the row order."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import tandem_truth as T
from conftest import DATA

pytestmark = pytest.mark.gpu

TWO = (2,) * 8
DEFAULT = (12, 7, 5, 4, 4, 4)
MOTIFS = {1: "A", 2: "AC", 3: "ACG", 4: "AACT", 5: "AATGG", 6: "ACGTTG", 7: "AACCGTG", 8: "ACGTTGCA"}


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _rows(r):
    assert r.ids.dtype == np.int64 and r.starts.dtype == np.int64 and r.stops.dtype == np.int64
    assert r.periods.dtype == np.uint8 and r.motif_codes.dtype == np.uint32
    assert len({len(r), r.ids.size, r.starts.size, r.stops.size, r.periods.size, r.motif_codes.size}) == 1
    return list(zip(r.ids.tolist(), r.starts.tolist(), r.stops.tolist(), r.periods.tolist(), r.motif_codes.tolist()))


def _truth(seqs, min_copies=DEFAULT, min_len=0, ids=None):
    return [(i,) + row for i in (range(len(seqs)) if ids is None else ids) for row in T.repeats(seqs[i], min_copies, min_len)]


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


def _build(records, width, eol="\n", final_newline=True, untidy=False):
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
    if not final_newline:
        while out and out[-1] in (10, 13):
            out.pop()
        spans[-1] = (spans[-1][0], len(out) - spans[-1][0])
    return bytes(out), spans


def _edges(raw, span):
    """Text coordinates of the first letter of every 256-byte run of the record but the first."""
    start, n = span
    return [sum(1 for c in raw[start:x] if c not in (10, 13, 32)) for x in range((start // 256 + 1) * 256, start + n, 256)]


def _put(t, at, word, n):
    """n letters of word written over t from `at` (clipped to t)"""
    at = max(at, 0)
    for j in range(max(0, min(n, len(t) - at))):
        t[at + j] = word[j % len(word)]


# ------------------------------------------------------------------ a. the fixtures
@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fixtures(fx, tmp_path, fn):
    shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
    fa = fx.Fasta(str(tmp_path / fn))
    seqs = [fa[i].seq for i in range(len(fa))]
    r = fa.tandem_repeats()
    _same(_rows(r), _truth(seqs), "defaults")
    dense = fa.tandem_repeats(TWO)
    want = _truth(seqs, TWO)
    _same(_rows(dense), want, "two copies")
    assert len(dense) > 10 * len(seqs)
    # the derived columns, against the letters
    for (i, a, b, p, m), word, canon, copies in list(zip(want, dense.motifs, dense.canonical_motifs.tolist(), dense.copies.tolist()))[:2000]:
        assert word == seqs[i][a:a + p].upper() and copies == (b - a) // p and canon == T.canonical(m, p)
    assert sum(dense.counts_by_motif(canonical=False).values()) == len(dense) == sum(dense.counts_by_motif().values())
    s = dense.sorted_by_start()
    assert _rows(s) == sorted(want, key=lambda x: (x[0], x[1], x[3]))
    names = list(fa.keys())
    bed = str(tmp_path / "ssr.bed")
    r.write_bed(bed)
    back = [ln.rstrip("\n").split("\t") for ln in open(bed)]
    assert [(names.index(n), int(x), int(y)) for n, x, y, _ in back] == [row[:3] for row in _rows(r)]
    assert [w for _, _, _, w in back] == ["(%s)%d" % (m, c) for m, c in zip(r.motifs, r.copies.tolist())]


# ------------------------------------------------------------------ b. generated layouts, repeats planted at the run edges
N_LAYOUT = 1400                                                # letters of the per-period records: five runs at the widest lines


def _layout_records(rng, width, eol, untidy):
    """One record per period with its motif planted at 0, across a run edge, from the last p - 1 letters of a run, up to the
    first letter of a run, across a line break and up to slen; records that are one repeat; an empty and a one-letter one."""
    n = N_LAYOUT
    recs = [("p%d" % p, _rand(rng, n, "ACGT" if p % 2 else "ACGTacgtNR")) for p in range(1, 9)]
    recs += [("whole3", ("CAG" * 100)[:257]), ("e0", ""), ("one", "g"), ("whole8", ("ACGTTGCA" * 70)[:515]), ("whole1", "t" * 300), ("tail", "GATTACA" + "AC" * 6)]
    raw, spans = _build(recs, width, eol, untidy=untidy)
    out = []
    for k, (name, s) in enumerate(recs):
        if not name.startswith("p"):
            out.append((name, s))
            continue
        p, w, t = k + 1, MOTIFS[k + 1], list(s)
        e = [x for x in _edges(raw, spans[k]) if x >= 6 * p + 4]             # (clear of what is planted at 0)
        assert len(e) >= 3 and e[2] + 3 * p < n - 3 * p, (width, eol, name)
        _put(t, 0, w, 3 * p + 1)                               # begins at 0
        _put(t, e[0] - 2 * p - 1, w, 4 * p + 3)                # across a run edge
        _put(t, e[1] - max(p - 1, 1), w, 3 * p)                # starts in the last p - 1 letters of the run in front
        _put(t, e[2] - 3 * p, w, 3 * p)                        # the first letter of a run breaks it
        t[e[2]] = "ACGT"[("ACGT".index(t[e[2] - p].upper()) + 1) % 4]
        line = width * max(1, 400 // width)
        _put(t, line - p - 2, w, 3 * p + 2)                    # across a line break (every plant is, at the narrow widths)
        _put(t, n - 3 * p, w, 3 * p)                           # ends at slen
        out.append((name, "".join(t)))
    return out


@pytest.mark.parametrize("width", [1, 7, 60, 61, 255, 256, 257])
def test_generated_layouts(fx, tmp_path, width):
    rng = np.random.default_rng(1000 + width)
    for tag, eol, final_newline, untidy in (("lf", "\n", True, False), ("crlf", "\r\n", True, False), ("untidy", "\n", True, True),
                                            ("nofinal", "\n", False, False), ("nofinal_crlf", "\r\n", False, False)):
        recs = _layout_records(rng, width, eol, untidy)
        raw, _ = _build(recs, width, eol, final_newline, untidy)
        fa, seqs = _open(fx, tmp_path, "w%d%s.fa" % (width, tag), raw)
        assert seqs[:-1] == [s for _, s in recs][:-1] and len(seqs) == len(recs)
        for mc in (DEFAULT, TWO):
            got = _rows(fa.tandem_repeats(mc))
            _same(got, _truth(seqs, mc), "width %d %s %s" % (width, tag, mc))
        # what was planted is there: at 0 and at slen in every per-period record, and the records that are one repeat
        for p in range(1, 9):
            mine = [row for row in got if row[0] == p - 1 and row[3] == p]
            assert any(row[1] == 0 and row[2] >= 3 * p + 1 for row in mine) and any(row[2] == N_LAYOUT and row[1] <= N_LAYOUT - 3 * p for row in mine), p
        whole = {row[0]: row for row in got if row[0] in (8, 11, 12)}
        assert whole[8][1:4] == (0, 257, 3) and whole[11][1:4] == (0, 515, 8) and whole[12][1:] == (0, 300, 1, 3)
    # the same records on one line each
    recs = [(n, s) for n, s in recs if s]
    raw, _ = _build(recs, 10 ** 6)
    fa, seqs = _open(fx, tmp_path, "w%doneline.fa" % width, raw)
    _same(_rows(fa.tandem_repeats(TWO)), _truth(seqs, TWO), "one line a record")


# ------------------------------------------------------------------ c. long stretches
def test_long_stretches(fx, tmp_path):
    rng = np.random.default_rng(99)
    big = list("AATGG" * 20000)                                # 100 000 letters: hundreds of runs without a break of period 5
    big[50001] = "C" if big[50001] != "C" else "T"             # one substituted letter splits it
    recs = [("ac", "GT" + "AC" * 500 + "TTG"),                 # 1 000 letters of (AC)n: at least three runs
            ("big", "".join(big)),
            ("left", _rand(rng, 300) + "T" + "ACG" * 20),      # two records that end and begin with the same motif
            ("right", "ACG" * 20 + "T" + _rand(rng, 300)),
            ("poly", "c" * 5000)]
    raw, _ = _build(recs, 60)
    fa, seqs = _open(fx, tmp_path, "long.fa", raw)
    assert seqs == [s for _, s in recs]
    for mc in (TWO, DEFAULT):
        got = _rows(fa.tandem_repeats(mc))
        _same(got, _truth(seqs, mc), str(mc))
    assert (0, 2, 1002, 2, 1) in got
    five = [row for row in got if row[0] == 1 and row[3] == 5]
    assert [row[1:3] for row in five] == [(0, 50001), (50002, 100000)]          # (the four letters in front of the new one agree with it, not 5 on)
    assert (2, 301, 361, 3, 6) in got and (3, 0, 60, 3, 6) in got and (4, 0, 5000, 1, 1) in got
    only = _rows(fa.tandem_repeats({5: 4}, min_len=50000))
    assert only == [five[0]]


# ------------------------------------------------------------------ d. dense output
@pytest.mark.parametrize("alphabet", ["AC", "ACGT", "ACGTacgtNnRYKM*-U"])
def test_dense_output(fx, tmp_path, alphabet):
    rng = np.random.default_rng(len(alphabet))
    recs = [("dense", _rand(rng, 20000, alphabet)), ("more", _rand(rng, 3000, alphabet))]
    raw, _ = _build(recs, 70)
    fa, seqs = _open(fx, tmp_path, "dense.fa", raw)
    want = _truth(seqs, TWO)
    assert len(want) > (4000 if len(alphabet) <= 4 else 500)     # every run closes several rows
    _same(_rows(fa.tandem_repeats(TWO)), want, alphabet)
    _same(_rows(fa.tandem_repeats((3, 2, 0, 2, 0, 0, 0, 2), min_len=7)), _truth(seqs, (3, 2, 0, 2, 0, 0, 0, 2), 7), alphabet + " some periods")


# ------------------------------------------------------------------ e. period selection, ids, limits
def _mixed(rng):
    recs = [("at", _rand(rng, 200) + "G" + "AT" * 40 + "G" + _rand(rng, 331) + "G" + "ATAC" * 9 + "G" + _rand(rng, 50) + "A" * 30 + "G"),
            ("none", "ACGGTCATG" + "N" * 40),
            ("aag", "AAG" * 30 + _rand(rng, 400) + "TTTTAGGG" * 6),
            ("short", "ACAC"),
            ("acgt", _rand(rng, 699) + "G" + "acgt" * 12)]
    return recs, _build(recs, 50)[0]


def test_period_selection(fx, tmp_path):
    recs, raw = _mixed(np.random.default_rng(8))
    fa, seqs = _open(fx, tmp_path, "mixed.fa", raw)
    got = _rows(fa.tandem_repeats((0, 0, 0, 5)))               # periods 1 and 2 are not asked for, yet (AT)40 and (A)30 are no rows
    _same(got, _truth(seqs, (0, 0, 0, 5)), "period 4 alone")
    assert [row[:4] for row in got] == [(0, 614, 650, 4), (4, 700, 748, 4)]
    _same(_rows(fa.tandem_repeats({4: 5})), got, "as a dict")
    _same(_rows(fa.tandem_repeats({8: 2, 6: 2})), _truth(seqs, {8: 2, 6: 2}), "periods 6 and 8")
    for min_len in (30, 80, 81, 10 ** 6, 2 ** 40):
        _same(_rows(fa.tandem_repeats(TWO, min_len=min_len)), _truth(seqs, TWO, min_len), "min_len %d" % min_len)
    assert len(fa.tandem_repeats(TWO, min_len=80)) == 2 and len(fa.tandem_repeats(TWO, min_len=10 ** 6)) == 0


def test_ids_and_limits(fx, tmp_path):
    recs, raw = _mixed(np.random.default_rng(9))
    fa, seqs = _open(fx, tmp_path, "mixed.fa", raw)
    names = list(fa.keys())
    for ids in ([4, 0, 2], [3], [2, 2, 0], [1, 3], []):
        _same(_rows(fa.tandem_repeats(TWO, ids=ids)), _truth(seqs, TWO, ids=ids), "ids %s" % ids)
    _same(_rows(fa.tandem_repeats(ids=[names[2], names[0]])), _truth(seqs, ids=[2, 0]), "by name")
    with pytest.raises(KeyError):
        fa.tandem_repeats(ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.tandem_repeats(ids=[len(fa)])
    for kw in (dict(min_copies=(1,)), dict(min_copies=(0, 0)), dict(min_copies=(2,) * 9), dict(min_len=-1), dict(max_repeats=-1)):
        with pytest.raises(ValueError):
            fa.tandem_repeats(**kw)
    want = _truth(seqs, TWO)
    n = len(want)
    _same(_rows(fa.tandem_repeats(TWO, max_repeats=n)), want, "the limit met")
    for cap in (n - 1, 0):
        with pytest.raises(ValueError, match=str(n)):
            fa.tandem_repeats(TWO, max_repeats=cap)
    _same(_rows(fa.tandem_repeats(TWO)), want, "after the refusals")
    # a file without repeats: empty arrays of the right types, whatever the limit
    fb, none = _open(fx, tmp_path, "none.fa", b">x\nACGTCATGCAT\nNNNNNNNN\n>y\n\n>z\nRYRYRYRY\n")
    assert none == ["ACGTCATGCATNNNNNNNN", "", "RYRYRYRY"] and _truth(none, TWO) == []
    for cap in (0, 5):
        e = fb.tandem_repeats(TWO, max_repeats=cap)
        assert len(e) == 0 and _rows(e) == [] and e.motifs == [] and e.canonical_motifs.size == 0 and len(e.sorted_by_start()) == 0


def test_sharded_raises(fx, tmp_path, monkeypatch):
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa.tandem_repeats()


# ------------------------------------------------------------------ f. the C entry directly
def test_c_abi(fx):
    from pyfastx_amd import _lib
    L = _lib.lib()
    raw = b">a\nGGACACACACACTT\nAAAAAAN\n>b\nacgacgacgacg\n"
    seqs = ["GGACACACACACTTAAAAAAN", "acgacgacgacg"]
    want = _truth(seqs, TWO)
    b = _lib.Blob.from_bytes(raw, device=0)

    def call(h, mc, max_period, min_len=0, ids=None, n_ids=0, max_rows=100, null_out=None, keep=False):
        out = [C.c_void_p() for _ in range(5)]
        n, tot = C.c_int64(-1), C.c_int64(-1)
        arr = None if mc is None else (C.c_int32 * len(mc))(*mc)
        refs = [C.byref(p) for p in out] + [C.byref(n), C.byref(tot)]
        if null_out is not None:
            refs[null_out] = None
        rc = L.fx_fasta_tandem_repeats(h, arr, max_period, min_len, ids, n_ids, max_rows, *refs)
        cols = None
        if rc == 0:
            assert all(p.value for p in out)                   # never NULL after FX_OK, even for 0 rows
            t = n.value
            cols = [_lib.pinned_array(p.value, max(t, 1), dt)[:t] for p, dt in zip(out, (np.int64, np.int64, np.int64, np.uint8, np.uint32))]
        else:
            assert not any(p.value for p in out[:5] if null_out is None)
        return rc, n.value, tot.value, cols

    assert call(b._h, TWO, 8)[0] == _lib.FX_ESTATE             # no table built
    b.fasta_build()
    rc, n, tot, cols = call(b._h, TWO, 8)
    assert rc == 0 and n == tot == len(want) == 5             # GG (AC)5 TT (A)6 and (acg)4
    assert [c.dtype for c in cols] == [np.int64, np.int64, np.int64, np.uint8, np.uint32]
    assert list(zip(*(c.tolist() for c in cols))) == want
    rc, n, tot, cols = call(b._h, TWO, 8, max_rows=4)
    assert rc == _lib.FX_ERANGE and n == 0 and tot == 5
    rc, n, tot, cols = call(b._h, (0, 0, 0, 0, 2), 5)          # no repeat of period 5: 0 rows, blocks all the same
    assert rc == 0 and n == tot == 0 and all(c.size == 0 for c in cols)
    ids = (C.c_int64 * 2)(1, 0)
    rc, n, tot, cols = call(b._h, TWO, 8, ids=ids, n_ids=2)
    assert rc == 0 and list(zip(*(c.tolist() for c in cols))) == _truth(seqs, TWO, ids=[1, 0])
    bad_id = (C.c_int64 * 1)(2)
    assert call(b._h, TWO, 8, ids=bad_id, n_ids=1)[0] == _lib.FX_ERANGE
    einval = [dict(h=None, mc=TWO, max_period=8), dict(mc=None, max_period=8), dict(mc=TWO, max_period=0), dict(mc=TWO + (2,), max_period=9),
              dict(mc=(2, 1), max_period=2), dict(mc=(-3,), max_period=1), dict(mc=(0, 0, 0), max_period=3), dict(mc=(0, 2, 5), max_period=1),
              dict(mc=TWO, max_period=8, min_len=-1), dict(mc=TWO, max_period=8, max_rows=-1), dict(mc=TWO, max_period=8, n_ids=-1),
              dict(mc=TWO, max_period=8, n_ids=2)]
    einval += [dict(mc=TWO, max_period=8, null_out=k) for k in range(7)]
    for kw in einval:
        kw.setdefault("h", b._h)
        assert call(**kw)[0] == _lib.FX_EINVAL, kw
    # a byte-range shard carries no halo for repeats across its cuts
    off = raw.index(b">b")
    sh = _lib.Blob.from_bytes(raw[off:], device=0)
    sh.set_shard(off, 10, True)
    sh.fasta_build()
    assert call(sh._h, TWO, 8)[0] == _lib.FX_EINVAL
    # the entry built the rank index itself; giving it back and asking again builds it again
    b.fasta_rank_free()
    assert call(b._h, TWO, 8)[1] == 5
