"""-m gpu: Fasta.region_stats / window_stats / class_runs (fx_fasta_region_counts, fx_fasta_window_counts,
fx_fasta_class_runs, csrc/fx_annot.hpp) against the plain Python truth of annot_truth.py over fa[i].seq -- on the fixtures,
on generated files with every line layout at which the 256-byte run layout can go wrong, on planted stretches, and on a
small synthetic genome against numpy.  Every comparison is exact integer equality unless it says otherwise."""
import glob
import os
import shutil
import sys

import numpy as np
import pytest

import annot_truth as T
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

ALPHABET = "ACGTacgtNnRYKM*-U"
MASKED = bytes(range(ord("a"), ord("z") + 1))
UNMASKED = bytes(range(ord("A"), ord("Z") + 1))


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


def _cum(seq, slen=None):
    """int64[len + 1, 7]: row i = the truth's counts of seq[:i], added up letter by letter.  slen: the record's length in the
    table, which counts a space inside a sequence line as the reference's index does and may exceed len(seq); coordinates
    run up to it, and the rows behind the text repeat the last one, as seq[a:b] clips."""
    c = np.zeros((max(len(seq), slen or 0) + 1, 7), dtype=np.int64)
    for j in range(len(seq)):
        c[j + 1] = T.region_counts(seq, j, j + 1)
    return np.cumsum(c, axis=0)


def _check_regions(fa, cums, ids, a, b):
    ids, a, b = (np.asarray(x, dtype=np.int64) for x in (ids, a, b))
    r = fa.region_stats(ids, a, b)
    assert r.counts.dtype == np.int64 and r.counts.shape == (ids.size, 7)
    assert r.ids.tolist() == ids.tolist() and r.starts.tolist() == a.tolist() and r.stops.tolist() == b.tolist()
    want = np.array([cums[i][y] - cums[i][x] for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())], dtype=np.int64).reshape(-1, 7)
    bad = np.nonzero((r.counts != want).any(axis=1))[0]
    assert bad.size == 0, (int(ids[bad[0]]), int(a[bad[0]]), int(b[bad[0]]), r.counts[bad[0]].tolist(), want[bad[0]].tolist())
    assert (r.length == want[:, :6].sum(axis=1)).all()
    return r


def _check_windows(fa, slens, cums, window, step, partial, ids=None):
    w = fa.window_stats(window, step, ids=ids, partial=partial)
    rows = [(i, x, y) for i in (range(len(slens)) if ids is None else sorted(set(ids))) for x, y in T.windows(slens[i], window, step, partial)]
    assert list(zip(w.ids.tolist(), w.starts.tolist(), w.stops.tolist())) == rows, (window, step, partial)
    want = np.array([cums[i][y] - cums[i][x] for i, x, y in rows], dtype=np.int64).reshape(-1, 7)
    assert w.counts.shape == want.shape and (w.counts == want).all(), (window, step, partial)
    return w


def _runs_truth(seqs, byteset, min_len, ids=None):
    return [(i, x, y) for i in (range(len(seqs)) if ids is None else ids) for x, y in T.class_runs(seqs[i], byteset, min_len)]


def _rows(r):
    return list(zip(r.ids.tolist(), r.starts.tolist(), r.stops.tolist()))


# ------------------------------------------------------------------ a. the fixtures
@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fixture_regions_and_windows(fx, fixture_files, fn):
    fa = fx.Fasta(fixture_files[fn])
    seqs = [fa[i].seq for i in range(len(fa))]
    cums = [_cum(s) for s in seqs]
    rng = np.random.default_rng(41)
    ids, a, b = [], [], []
    for i, s in enumerate(seqs):
        ids.append(i); a.append(0); b.append(len(s))
        for _ in range(200):
            x = int(rng.integers(0, len(s) + 1))
            y = int(rng.integers(x, len(s) + 1))
            ids.append(i); a.append(x); b.append(y)
    r = _check_regions(fa, cums, ids, a, b)
    full = r.counts[::201]
    assert full.shape[0] == len(seqs)
    # by name
    names = list(fa.keys())
    byname = fa.region_stats([names[i] for i in ids[:500]], a[:500], b[:500])
    assert (byname.counts == r.counts[:500]).all() and byname.ids.tolist() == ids[:500]
    # a tiling of every record adds up to its full-range row
    for window in (1000, 97):
        w = fa.window_stats(window)
        sums = np.zeros((len(seqs), 7), dtype=np.int64)
        np.add.at(sums, w.ids, w.counts)
        assert (sums == full).all()
        assert (w.starts % window == 0).all() and (w.stops - w.starts <= window).all()
    # the six base columns against the composition the build counted (no part of the new truth in this one)
    comp = fa.composition
    fold = np.zeros(6, dtype=np.int64)
    for ch, n in comp.items():
        fold["ACGTN".find(ch.upper()) if ch.upper() in "ACGTN" else 5] += n
    assert full[:, :6].sum(axis=0).tolist() == fold.tolist()
    assert int(full[:, 6].sum()) == sum(n for ch, n in comp.items() if "a" <= ch <= "z")


def _reference():
    if not glob.glob(os.path.join(ROOT, "oracle", "_ref", "pyfastx*.so")):
        pytest.skip("oracle/_ref (the compiled reference) is not built")
    p = os.path.join(ROOT, "oracle", "_ref")
    if p not in sys.path:
        sys.path.insert(0, p)
    import pyfastx
    return pyfastx


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fixture_against_reference(fx, tmp_path, fn):
    ref = _reference()
    for d in ("ours", "theirs"):
        os.makedirs(tmp_path / d)
        shutil.copy(os.path.join(DATA, fn), tmp_path / d / fn)
    fa, rf = fx.Fasta(str(tmp_path / "ours" / fn)), ref.Fasta(str(tmp_path / "theirs" / fn))
    names = list(fa.keys())
    rng = np.random.default_rng(43)
    ids = rng.integers(0, len(names), 200)
    slen = np.array([len(fa[int(i)]) for i in range(len(names))], dtype=np.int64)
    a = (rng.random(200) * slen[ids]).astype(np.int64)
    b = a + 1 + (rng.random(200) * (slen[ids] - a)).astype(np.int64)
    b = np.minimum(b, slen[ids])
    keep = b > a
    ids, a, b = ids[keep], a[keep], b[keep]
    r = fa.region_stats(ids, a, b)
    for k in range(ids.size):
        sub = rf[names[int(ids[k])]][int(a[k]):int(b[k])]
        want = np.zeros(7, dtype=np.int64)
        for ch, n in sub.composition.items():
            want["ACGTN".find(ch.upper()) if ch.upper() in "ACGTN" else 5] += n
            if "a" <= ch <= "z":
                want[6] += n
        assert r.counts[k].tolist() == want.tolist(), (int(ids[k]), int(a[k]), int(b[k]))
        if want[:4].sum():
            g = float(sub.gc_content)                   # float32 arithmetic in the reference, 2^-23 per operation
            assert abs(r.gc_content[k] - g) <= 1e-6 * abs(g) + 1e-30, (r.gc_content[k], g)


# ------------------------------------------------------------------ b. generated layouts
def _rand(rng, n, alphabet=ALPHABET):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _build(records, width, eol="\n", final_newline=True, blanks=False, spaces=False, pad_to=None):
    """records: [(name, seq)] -> (bytes of the file, [(offset of the record's first body byte, bytes to its end)]).
    pad_to: {record index: k} -- the header gets a description long enough to put the body's first byte at offset = k mod 256."""
    out, spans = bytearray(), []
    for i, (name, s) in enumerate(records):
        hdr = ">" + name
        if pad_to and i in pad_to:
            fill = (pad_to[i] - (len(out) + len(hdr) + len(eol))) % 256
            if fill:
                hdr += " " + "d" * (fill - 1 if fill > 1 else 256)      # (one byte cannot hold " d": a whole block more)
        out += hdr.encode() + eol.encode()
        start = len(out)
        lines = [s[k:k + width] for k in range(0, len(s), width)]
        for j, ln in enumerate(lines):
            if spaces and j % 3 == 1 and len(ln) > 4:
                ln = ln[:3] + " " + ln[3:]
            out += ln.encode("latin-1") + eol.encode()
            if blanks and j % 4 == 2:
                out += eol.encode()
        spans.append((start, len(out) - start))
    if not final_newline:
        while out and out[-1] in (10, 13):
            out.pop()
        spans[-1] = (spans[-1][0], len(out) - spans[-1][0])
    return bytes(out), spans


def _edges(raw, span, slen):
    """Text coordinates of the record's 256-byte run edges: letters in front of every multiple of 256 inside its bytes."""
    start, n = span
    out = []
    for x in range((start // 256 + 1) * 256, start + n, 256):
        t = sum(1 for c in raw[start:x] if c not in (10, 13, 32))
        out.append(min(t, slen))
    return out


def _grid(slen, edges):
    g = {0, 1, 2, slen - 2, slen - 1, slen, slen // 2}
    for e in edges:
        g.update(range(e - 2, e + 3))
    return sorted(p for p in g if 0 <= p <= slen)


def _layout_cases():
    rng = np.random.default_rng(2027)
    cases = []
    for width in (1, 7, 60, 255, 256, 257, 300):
        for eol in ("\n", "\r\n"):
            recs = [("a", _rand(rng, 777)), ("e0", ""), ("one", "g"), ("b", _rand(rng, 300 + width)), ("c", _rand(rng, 2 * width))]
            cases.append(("w%d%s" % (width, "crlf" if eol != "\n" else ""), _build(recs, width, eol)))
    recs = [("a", _rand(rng, 900)), ("b", _rand(rng, 333)), ("c", _rand(rng, 61))]
    cases.append(("blanks", _build(recs, 60, blanks=True)))
    cases.append(("spaces", _build(recs, 60, "\r\n", spaces=True)))
    cases.append(("blanks_spaces", _build(recs, 7, blanks=True, spaces=True)))
    cases.append(("nofinal", _build(recs, 60, final_newline=False)))
    cases.append(("nofinal_crlf", _build(recs, 256, "\r\n", final_newline=False)))
    cases.append(("oneline", _build([("x", _rand(rng, 1000)), ("y", _rand(rng, 5))], 1000)))
    # first base exactly on a block edge (b), last base exactly in front of one (c: body at 256 k + 6, 250 letters in one line)
    recs = [("a", _rand(rng, 100)), ("b", _rand(rng, 600)), ("c", _rand(rng, 250)), ("d", _rand(rng, 70))]
    raw, spans = _build(recs, 300, pad_to={1: 0, 2: 6})
    assert spans[1][0] % 256 == 0 and (spans[2][0] + 250) % 256 == 0
    cases.append(("edges", (raw, spans)))
    return cases


LAYOUTS = _layout_cases()


@pytest.mark.parametrize("name", [c[0] for c in LAYOUTS])
def test_generated_layouts(fx, tmp_path, name):
    raw, spans = dict(LAYOUTS)[name]
    path = str(tmp_path / (name + ".fa"))
    with open(path, "wb") as f:
        f.write(raw)
    fa = fx.Fasta(path)
    seqs = [fa[i].seq for i in range(len(fa))]
    assert len(seqs) == len(spans)
    slens = [len(fa[i]) for i in range(len(fa))]           # (above len(seq) where a sequence line holds a space)
    assert all(n >= len(s) for n, s in zip(slens, seqs))
    cums = [_cum(s, n) for s, n in zip(seqs, slens)]
    ids, a, b = [], [], []
    for i, s in enumerate(seqs):
        g = sorted(set(_grid(slens[i], _edges(raw, spans[i], slens[i])) + _grid(len(s), [])))
        for x in g:
            for y in g:
                if y >= x:
                    ids.append(i); a.append(x); b.append(y)
    _check_regions(fa, cums, ids, a, b)
    for partial in (True, False):
        for window, step in ((1, 1), (5, 5), (5, 2), (5, 9)):
            _check_windows(fa, slens, cums, window, step, partial)
        for i, n in enumerate(slens):
            _check_windows(fa, slens, cums, n + 3, n + 3, partial, ids=[i])
    # the runs of every class on the same bytes
    for byteset, kw in ((b"Nn", dict(kind="N")), (MASKED, dict(kind="masked")), (UNMASKED, dict(kind="unmasked")), (b"RY", dict(letters="RY"))):
        for min_len in (1, 2, 3):
            assert _rows(fa.class_runs(min_len=min_len, **kw)) == _runs_truth(seqs, byteset, min_len), (kw, min_len)


# ------------------------------------------------------------------ c. class runs on planted stretches
def _blocks(rng, n):
    """n letters in stretches of 1..80 letters, each from one of a few alphabets: soft-masked, unmasked, R/Y, N."""
    out = []
    while sum(map(len, out)) < n:
        out.append(_rand(rng, int(rng.integers(1, 81)), ["ACGT", "acgt", "RY", "ry", "ACGTRY", "Nn", "acgtN"][int(rng.integers(0, 7))]))
    return "".join(out)[:n]


def _plant(s, at, n, ch="N"):
    """s with n letters ch at `at`, and a letter outside every class under test on both sides (so the stretch is maximal)."""
    t = list(s)
    t[at:at + n] = ch * n
    for p in (at - 1, at + n):
        if 0 <= p < len(t):
            t[p] = "*"
    return "".join(t)


def _planted():
    rng = np.random.default_rng(77)
    recs = []
    s = _plant(_plant(_blocks(rng, 1500), 0, 37), 1500 - 41, 41)                        # from base 0; to slen
    recs.append(("ends", s))
    recs.append(("alln1", "N" * 500))                                                  # whole records, adjacent: two rows
    recs.append(("alln2", "n" * 130))
    recs.append(("long", _plant(_blocks(rng, 2000), 611, 700)))                        # more than two runs
    s = _blocks(rng, 3000)
    for k, n in enumerate((1, 2, 9, 10, 11, 299, 300, 301)):                           # min_len - 1, min_len, min_len + 1
        s = _plant(s, 50 + 340 * k, n)
    recs.append(("lens", s))
    s = _plant(_blocks(rng, 900), 100, 20)                                             # ends exactly at a line end (120 = 2 * 60)
    recs.append(("lineend", s))
    recs.append(("tail", "N" * 70))                                                    # the last record ends inside the class
    raw, spans = _build(recs, 60)
    # one more record whose N stretch ends exactly in front of a 256-byte block edge: found from the bytes of the file
    body0 = len(raw) + len(">blockedge\n")
    s = _blocks(rng, 1200)
    end = next(p for p in range(300, 1200) if p % 60 and (body0 + p + p // 60) % 256 == 0)
    recs.append(("blockedge", _plant(s, end - 45, 45)))
    raw, spans = _build(recs, 60)
    assert (spans[-1][0] + end + end // 60) % 256 == 0
    return raw, recs, end


def test_class_runs_planted(fx, tmp_path):
    raw, recs, edge_end = _planted()
    path = str(tmp_path / "planted.fa")
    with open(path, "wb") as f:
        f.write(raw)
    fa = fx.Fasta(path)
    seqs = [fa[i].seq for i in range(len(fa))]
    assert seqs == [s for _, s in recs]
    names = list(fa.keys())
    for min_len in (1, 10, 300):
        got = _rows(fa.class_runs("N", min_len=min_len))
        assert got == _runs_truth(seqs, b"Nn", min_len), min_len
        planted = [(4, 50 + 340 * k, 50 + 340 * k + n) for k, n in enumerate((1, 2, 9, 10, 11, 299, 300, 301)) if n >= min_len]
        assert [r for r in got if r[0] == 4 and r in planted] == planted               # the lengths around min_len, by hand
    got = _rows(fa.class_runs("N"))
    assert (0, 0, 37) in got and (0, 1500 - 41, 1500) in got
    assert (1, 0, 500) in got and (2, 0, 130) in got and (3, 611, 1311) in got and (5, 100, 120) in got and (6, 0, 70) in got
    assert (7, edge_end - 45, edge_end) in got
    for byteset, kw in ((MASKED, dict(kind="masked")), (UNMASKED, dict(kind="unmasked")), (b"RY", dict(letters="RY")), (b"RYry", dict(kind="RYry"))):
        for min_len in (1, 10, 300):
            assert _rows(fa.class_runs(min_len=min_len, **kw)) == _runs_truth(seqs, byteset, min_len), (kw, min_len)
    # a selection: unsorted and with a repeat = the sorted distinct one; by name too
    want = _runs_truth(seqs, b"Nn", 1, ids=[1, 3, 6])
    assert _rows(fa.class_runs("N", ids=[6, 1, 3, 1])) == want
    assert _rows(fa.class_runs("N", ids=[names[6], names[1], names[3]])) == want
    # BED rows with the names of the index
    r = fa.class_runs("N", min_len=10)
    bed = str(tmp_path / "n.bed")
    r.write_bed(bed)
    back = [ln.rstrip("\n").split("\t") for ln in open(bed)]
    assert [(names.index(n), int(x), int(y)) for n, x, y in back] == _rows(r)
    assert (r.lengths == r.stops - r.starts).all() and (r.lengths >= 10).all()
    # the limit carries the true count
    n = len(got)
    assert _rows(fa.class_runs("N", max_runs=n)) == got
    with pytest.raises(ValueError, match=str(n)):
        fa.class_runs("N", max_runs=n - 1)


# ------------------------------------------------------------------ d. error paths
def test_errors(fx, fixture_files):
    from pyfastx_amd import _lib
    fa = fx.Fasta(fixture_files["test.fa"])
    n0 = len(fa[0])
    with pytest.raises(KeyError):
        fa.region_stats(["no_such_record"], [0], [1])
    for bad in (len(fa), -1):
        with pytest.raises(IndexError):
            fa.region_stats([0, bad], [0, 0], [1, 1])
    for a, b in ((-1, 5), (7, 5), (0, n0 + 1)):
        with pytest.raises(ValueError, match="interval outside the sequence"):
            fa.region_stats([0, 0], [0, a], [n0, b])
    assert fa.region_stats([0, 0], [0, 5], [n0, 5]).counts[1].tolist() == [0] * 7     # an empty interval is valid
    assert len(fa.region_stats([], [], [])) == 0
    # the first bad query is the one reported
    blob = fa._search_blob()
    ids, a, b = np.zeros(2000, dtype=np.int64), np.zeros(2000, dtype=np.int64), np.full(2000, 3, dtype=np.int64)
    b[1234] = n0 + 1; a[1500] = -1; ids[1999] = len(fa)
    with pytest.raises(_lib.FxError) as e:
        blob.fasta_region_counts(ids, a, b)
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 1234
    for args in ((0,), (5, 0), (-3, 1)):
        with pytest.raises(ValueError):
            fa.window_stats(*args)
    total = int(sum((len(fa[i]) + 99) // 100 for i in range(len(fa))))
    assert len(fa.window_stats(100, max_windows=total)) == total
    with pytest.raises(ValueError, match=str(total)):
        fa.window_stats(100, max_windows=total - 1)
    with pytest.raises(IndexError):
        fa.window_stats(100, ids=[len(fa)])
    with pytest.raises(KeyError):
        fa.class_runs("N", ids=["no_such_record"])
    for kw in (dict(kind="x"), dict(kind="N", min_len=0), dict(letters="")):
        with pytest.raises(ValueError):
            fa.class_runs(**kw)


def test_sharded_raises(fx, fixture_files, monkeypatch):
    """A region or a run can straddle the cut of a byte-range shard or a window: refused, as the search is."""
    fa = fx.Fasta(fixture_files["test.fa"])
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa.region_stats([0], [0], [1])
    with pytest.raises(NotImplementedError):
        fa.window_stats(100)
    with pytest.raises(NotImplementedError):
        fa.class_runs("N")


# ------------------------------------------------------------------ e. a small genome
def _genome(total_bp):
    """A synthetic genome resident on the device with its table built -> (blob, flat letters, flat_start, slen, keep-alive)."""
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=total_bp)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fasta_build().n_seq == len(plan["slen"])
    flat = flat_t.cpu().numpy()
    del flat_t
    return b, flat, flat_start, plan["slen"], blob_t


def _np_runs(flat, flat_start, slen, member, min_len):
    """(record, start, stop) of the maximal stretches of `member` letters: np.diff on the mask, split at the records' first letters."""
    first, last = np.zeros(flat.size, dtype=bool), np.zeros(flat.size, dtype=bool)
    first[flat_start[slen > 0]] = True
    last[(flat_start + slen - 1)[slen > 0]] = True
    d = np.diff(member.astype(np.int8), prepend=0, append=0)
    x = np.nonzero((d[:-1] == 1) | (member & first))[0]
    y = np.nonzero((d[1:] == -1) | (member & last))[0] + 1
    assert x.size == y.size
    rec = np.searchsorted(flat_start, x, side="right") - 1
    keep = y - x >= min_len
    return rec[keep], (x - flat_start[rec])[keep], (y - flat_start[rec])[keep]


def _check_np_runs(b, flat, flat_start, slen, kind, member, min_len):
    from pyfastx_amd import annot
    got = annot.runs_blob(b, kind, min_len)
    rec, x, y = _np_runs(flat, flat_start, slen, member, min_len)
    assert got.ids.size == rec.size, (kind, got.ids.size, rec.size)
    assert (got.ids == rec).all() and (got.starts == x).all() and (got.stops == y).all(), kind
    return got


def test_synthetic_genome_60mbp(fx):
    from pyfastx_amd import annot
    b, flat, flat_start, slen, keep = _genome(60_000_000)
    nrec = len(slen)
    rng = np.random.default_rng(60)
    n = 100_000
    ids = rng.integers(0, nrec, n)
    ln = np.minimum(np.exp(rng.uniform(0, np.log(1e5), n)).astype(np.int64), slen[ids])
    a = (rng.random(n) * (slen[ids] - ln + 1)).astype(np.int64)
    e = a + ln
    assert ln.min() == 1 and ln.max() > 90_000
    all_ids, zeros = np.arange(nrec, dtype=np.int64), np.zeros(nrec, dtype=np.int64)
    r = annot.region_blob(b, ids, a, e)
    full = annot.region_blob(b, all_ids, zeros, slen)
    # numpy: one cumulative sum per column over the flat letters
    col = np.full(256, 5, dtype=np.uint8)
    for k, ch in enumerate("ACGTN"):
        col[ord(ch)] = col[ord(ch.lower())] = k
    cls = col[flat]
    for k in range(7):
        hit = (cls == k) if k < 6 else ((flat >= ord("a")) & (flat <= ord("z")))
        cum = np.zeros(flat.size + 1, dtype=np.int32)               # (6 * 10^7 letters: the sums fit)
        np.cumsum(hit, out=cum[1:], dtype=np.int32)
        assert (r.counts[:, k] == cum[flat_start[ids] + e] - cum[flat_start[ids] + a]).all(), k
        assert (full.counts[:, k] == cum[flat_start + slen] - cum[flat_start]).all(), k
        del hit, cum
    # the index is kept: the same rows again; and rebuilt after it was given back
    assert (annot.region_blob(b, ids, a, e).counts == r.counts).all()
    b.fasta_rank_free()
    assert (annot.region_blob(b, ids, a, e).counts == r.counts).all()
    # tiling 1 kb windows add up to the full-record rows
    w = annot.window_blob(b, slen, 1000)
    assert len(w) == int(((slen + 999) // 1000).sum())
    sums = np.zeros((nrec, 7), dtype=np.int64)
    np.add.at(sums, w.ids, w.counts)
    assert (sums == full.counts).all()
    assert (np.diff(w.ids) >= 0).all() and (w.stops - w.starts <= 1000).all()
    _check_np_runs(b, flat, flat_start, slen, "N", (flat == ord("N")) | (flat == ord("n")), 1)
    m = _check_np_runs(b, flat, flat_start, slen, "masked", (flat >= ord("a")) & (flat <= ord("z")), 1000)
    assert len(m) > 500 and m.lengths.min() >= 1000
    del b, keep


def test_synthetic_genome_gaps(fx):
    """synth plants telomere and centromere N runs only in chromosomes above 4 Mbp, which a 60 Mbp plan does not have: at
    70 Mbp the two largest carry them -- stretches that span thousands of runs, begin at base 0 and end at slen, in
    neighbouring records."""
    b, flat, flat_start, slen, keep = _genome(70_000_000)
    assert (slen > 4_000_000).sum() == 2
    g = _check_np_runs(b, flat, flat_start, slen, "N", (flat == ord("N")) | (flat == ord("n")), 1)
    assert _rows(g)[0] == (0, 0, 10_000) and (0, int(slen[0]) - 10_000, int(slen[0])) in _rows(g) and (1, 0, 10_000) in _rows(g)
    assert len(g) >= 4 and g.lengths.max() >= 1_000_000
    _check_np_runs(b, flat, flat_start, slen, "masked", (flat >= ord("a")) & (flat <= ord("z")), 1000)
    del b, keep
