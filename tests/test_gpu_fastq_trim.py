"""-m gpu: Fastq.trim / records / write (fx_fastq_trim, fx_fastq_format_alloc, csrc/fx_fastq_trim.hpp) against the plain-Python
definition tests/trim_truth.py over fq[i].seq / fq[i].qual of the same file -- every comparison exact -- on the fixtures, on
every input of tests/golden/fastq_edge.json, on a generated file of irregular reads with the adapter planted, and against
torch on a synthetic stream of 2 M reads."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA, load_golden
from trim_truth import record, trim_truth, trim_truth_fast, truth_kwargs

pytestmark = pytest.mark.gpu

EDGE = load_golden("fastq_edge")
AD = "AGATCGGAAGAGC"


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _lat(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def truth_of(fq):
    """The definitions, from the object API: per-read rows of (seq bytes, qual bytes) and the offset p."""
    p = fq.phred or 33
    rows = []
    for i in range(len(fq)):
        r = fq[i]
        s, q = np.frombuffer(_lat(r.seq), dtype=np.uint8), np.frombuffer(_lat(r.qual), dtype=np.uint8)
        assert len(s) == len(q)
        rows.append((s, q))
    return p, rows


def want_of(p, rows, kw, ids=None, fn=trim_truth):
    from pyfastx_amd import trim
    tk = truth_kwargs(trim.trim_args(**kw))
    sel = range(len(rows)) if ids is None else ids
    ab = [fn(rows[int(i)][0], rows[int(i)][1], p, **tk) for i in sel]
    return (np.array([x[0] for x in ab], dtype=np.int64), np.array([x[1] for x in ab], dtype=np.int64))


def check_trim(fq, p, rows, kw, ids=None, fn=trim_truth):
    got = fq.trim(ids=ids, **kw)
    a, b = want_of(p, rows, kw, ids, fn)
    assert sorted(got) == ["end", "start"] and got["start"].dtype == got["end"].dtype == np.int64
    assert np.array_equal(got["start"], a), kw
    assert np.array_equal(got["end"], b), kw
    return a, b


CASES = [dict(front_qual=20), dict(tail_qual=20), dict(window=(4, 20)), dict(window=(10, 30)),
         dict(front_qual=30, window=(4, 25), tail_qual=30), dict(adapter=AD), dict(clip_front=5, clip_tail=7)]
# on tests/data/test.fq (800 reads of 150), by the definition on the CPU: reads changed, reads left empty
FIXTURE_COUNTS = [(34, None), (65, None), (113, 1), (288, 17), (396, 5), (9, None), (800, None)]
ALL = dict(clip_front=2, clip_tail=1, adapter=AD, min_overlap=3, max_error_rate=0.1, front_qual=20, window=(4, 20), tail_qual=20)


def check_everything(fq, rng, counts=None):
    """trim: every step alone, all together, odd parameters, gathered ids; records: the bytes and the offsets."""
    p, rows = truth_of(fq)
    n = len(rows)
    L = np.array([len(s) for s, _ in rows], dtype=np.int64)
    for k, kw in enumerate(CASES):
        a, b = want_of(p, rows, kw)
        if counts is not None:                                # a truth that trims nothing cannot pass silently
            changed, empty = counts[k]
            assert int(((a != 0) | (b != L)).sum()) == changed, kw
            assert empty is None or int((b == a).sum()) == empty, kw
        check_trim(fq, p, rows, kw)
    check_trim(fq, p, rows, ALL)
    for kw in (dict(), dict(clip_front=1000), dict(clip_tail=1000), dict(front_qual=0, tail_qual=0), dict(front_qual=255), dict(tail_qual=255),
               dict(window=(1, 20)), dict(window=(16, 30)), dict(window=(17, "61/2")), dict(window=(33, 30)), dict(window=(100000, 35)),
               dict(window=(3, 0)), dict(window=(7, 250)), dict(adapter="A", min_overlap=1, max_error_rate=0), dict(adapter="ACGTN", min_overlap=2),
               dict(adapter="N" * 20, min_overlap=20), dict(adapter=AD, min_overlap=1, max_error_rate=0.34),
               dict(adapter=AD + "ACACGTCTGAACTCCAGTCAC", min_overlap=5, max_error_rate=0.2),
               dict(adapter="GATCGGAAGAGCACACGTCTGAACTCCAGTCACNNNNNNATCTCGTATGCCGTCTTCTGCTTG", max_error_rate=0.25, clip_front=3, tail_qual=10)):
        check_trim(fq, p, rows, kw)
    if n:
        ids = rng.integers(0, n, 3 * n + 5)
        a, b = check_trim(fq, p, rows, ALL, ids)
    empty = fq.trim(ids=[], **ALL)
    assert len(empty["start"]) == 0 and len(empty["end"]) == 0
    for bad in ([n], [-1], [0, n + 7, 0]):
        with pytest.raises(IndexError, match="index out of range"):
            fq.trim(ids=bad, front_qual=20)
        with pytest.raises(IndexError, match="index out of range"):
            fq.records(ids=bad)
    # records: whole reads, trimmed reads with a minimum length, gathered
    hdr = [_lat(fq[i].description) for i in range(n)]
    buf, offs = fq.records()
    assert buf.dtype == np.uint8 and offs.dtype == np.int64 and len(offs) == n + 1 and offs[0] == 0
    assert buf.tobytes() == b"".join(record(hdr[i], rows[i][0], rows[i][1], 0, len(rows[i][0])) for i in range(n))
    if n:
        t = fq.trim(ids=ids, **ALL)
        min_len = int(np.median(t["end"] - t["start"])) + 1
        buf, offs = fq.records(ids, t["start"], t["end"], min_len=min_len)
        parts = [record(hdr[int(i)], rows[int(i)][0], rows[int(i)][1], int(x), int(y)) if y - x >= min_len else b""
                 for i, x, y in zip(ids, a, b)]
        assert np.array_equal(np.diff(offs), [len(x) for x in parts]) and buf.tobytes() == b"".join(parts)
        assert any(len(x) == 0 for x in parts)
        bad_end = t["end"].copy()
        bad_end[len(ids) // 2] = L[ids[len(ids) // 2]] + 1
        with pytest.raises(ValueError):
            fq.records(ids, t["start"], bad_end)
        with pytest.raises(ValueError):
            fq.records(ids, t["start"][1:], t["end"][1:])
    buf, offs = fq.records(ids=[])
    assert len(buf) == 0 and offs.tolist() == [0]
    return p, rows, hdr


def check_write(fx, fq, rows, hdr, tmp_path, kw, min_len, ids=None, batches=5):
    """write in one batch and in several: the same file, the counts, and the file re-opened."""
    n = len(rows)
    sel = np.arange(n) if ids is None else np.asarray(ids)
    t = fq.trim(ids=ids, **kw)
    a, b = t["start"], t["end"]
    keep = (b - a) >= min_len
    want = b"".join(record(hdr[int(i)], rows[int(i)][0], rows[int(i)][1], int(x), int(y)) for i, x, y, k in zip(sel, a, b, keep) if k)
    tag = "w%d" % len(os.listdir(tmp_path))                   # a fresh pair of names per call: an index file belongs to its file
    one, many = str(tmp_path / (tag + "_one.fq")), str(tmp_path / (tag + "_many.fq"))
    r1 = fq.write(one, ids, a, b, min_len=min_len)
    ub = int((fq._tab_host["dlen"][sel].astype(np.int64) + 2 * fq._tab_host["rlen"][sel] + 6).sum())
    from pyfastx_amd import trim
    small = ub // batches - 1
    assert len(list(trim.batches(fq._tab_host, None if ids is None else sel, n, small))) >= batches
    r2 = fq.write(many, ids, a, b, min_len=min_len, batch_bytes=small)
    assert r1 == r2 == {"reads": int(keep.sum()), "bases": int((b - a)[keep].sum()), "dropped": int((~keep).sum())}
    assert open(one, "rb").read() == want and open(many, "rb").read() == want
    back = fx.Fastq(one)
    kept = np.nonzero(keep)[0]
    assert len(back) == r1["reads"] == len(kept) and len(kept) > 0
    for j, k in enumerate(kept):
        i = int(sel[k])
        r = back[j]
        assert _lat(r.seq) == rows[i][0][a[k]:b[k]].tobytes() and _lat(r.qual) == rows[i][1][a[k]:b[k]].tobytes()
        assert r.name == fq[i].name
    assert np.array_equal(back.read_stats()["length"], (b - a)[kept])
    return r1


@pytest.mark.parametrize("fn", ["test.fq", "test.fq.gz"])
def test_fixtures(fx, tmp_path, fn):
    shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
    fq = fx.Fastq(str(tmp_path / fn))
    assert len(fq) == 800
    p, rows, hdr = check_everything(fq, np.random.default_rng(3), FIXTURE_COUNTS)
    r = check_write(fx, fq, rows, hdr, tmp_path, dict(front_qual=30, window=(4, 25), tail_qual=30), min_len=100)
    assert 0 < r["dropped"] < 800
    ids = np.random.default_rng(4).permutation(800)[:500]     # no repeats: the written file is opened again, names are its keys
    check_write(fx, fq, rows, hdr, tmp_path, ALL, min_len=1, ids=ids)
    # a well-formed '\n'-terminated file whose third lines are a bare '+' (test.fq; the lines of test.fq.gz end in "\r\n"):
    # whole records are the raw records
    for q in (np.arange(800), ids) if fn == "test.fq" else ():
        rb, ro = fq.records(q)
        wb, wo = fq.raw_many(q)
        assert np.array_equal(ro, wo) and rb.tobytes() == wb.tobytes()


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_inputs(fx, tmp_path, name):
    """Every input of fastq_edge.json, opened as a file; quirks (CRLF, a '\\r' inside a quality line, a truncated tail) come
    out as fq[i].seq / fq[i].qual / fq[i].description show them."""
    path = tmp_path / (name + ".fq")
    path.write_bytes(EDGE[name]["text"].encode("latin-1"))
    fq = fx.Fastq(str(path))
    assert len(fq) == EDGE[name]["count"]
    check_everything(fq, np.random.default_rng(5))


def _irregular_fastq(n, seed, empty_at=None):
    """n reads of 1..400 bases; qualities from a skewed four-value distribution; lower-case and IUPAC letters sprinkled in."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 401, n)
    if empty_at is not None:
        lens[empty_at] = 0
    tot = int(lens.sum())
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, tot)].copy()
    odd = np.frombuffer(b"acgtnNRYKMSWryBDHV", dtype=np.uint8)
    w = rng.random(tot) < 0.03
    seq[w] = odd[rng.integers(0, len(odd), int(w.sum()))]
    qual = np.frombuffer(b"F:,#", dtype=np.uint8)[rng.choice(4, tot, p=[0.80, 0.12, 0.06, 0.02])]
    offs = np.concatenate(([0], np.cumsum(lens)))
    parts = []
    for i in range(n):
        a, b = int(offs[i]), int(offs[i + 1])
        parts.append(b"@r%d len=%d\n" % (i, b - a) + seq[a:b].tobytes() + b"\n+\n" + qual[a:b].tobytes() + b"\n")
    return b"".join(parts), lens


def _planted_fastq(n, seed):
    """The generator above, then: the adapter planted in every third read at a random position -- whole, or cut by the
    read's end down to 1 letter -- with 0, 1 or 2 substitutions, and qualities that decay towards the 3' end."""
    raw, lens = _irregular_fastq(n, seed)
    rng = np.random.default_rng(seed + 1)
    lines = raw.split(b"\n")
    A = np.frombuffer(AD.encode(), dtype=np.uint8)
    decay = np.frombuffer(b"F:,#", dtype=np.uint8)
    for i in range(n):
        L = int(lens[i])
        q = np.frombuffer(lines[4 * i + 3], dtype=np.uint8).copy()
        # from a random point on, each quality drops one class with probability rising to the end
        cut = int(rng.integers(0, L + 1))
        drop = rng.random(L - cut) < np.linspace(0.2, 0.9, L - cut) if L > cut else np.zeros(0, dtype=bool)
        cls = np.searchsorted(np.array([35, 44, 58, 70]), q[cut:])          # '#' ',' ':' 'F' -> 0..3
        q[cut:] = decay[::-1][np.maximum(cls - drop, 0)]
        lines[4 * i + 3] = q.tobytes()
        if i % 3 == 0:
            s = np.frombuffer(lines[4 * i + 1], dtype=np.uint8).copy()
            at = int(rng.integers(0, L))
            m = min(len(A), L - at)
            piece = A[:m].copy()
            for _ in range(int(rng.integers(0, 3))):
                piece[int(rng.integers(0, m))] = b"ACGT"[int(rng.integers(0, 4))]
            s[at:at + m] = piece
            lines[4 * i + 1] = s.tobytes()
    return b"\n".join(lines), lens


@pytest.fixture(scope="module")
def planted(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_planted")
    raw, lens = _planted_fastq(200_000, 11)
    p = d / "planted.fq"
    p.write_bytes(raw)
    return fx.Fastq(str(p)), raw, lens


def test_generated_planted_adapter(fx, planted, tmp_path):
    """2 x 10^5 reads of 1..400 bases: lane groups of 25 lanes, the adapter at every offset and overlap, qualities that
    decay.  The truth is taken from the file's own lines; a sample of reads pins that against fq[i]."""
    from pyfastx_amd import trim
    fq, raw, lens = planted
    lines = raw.split(b"\n")
    n = len(lens)
    assert len(fq) == n and int(fq.maxlen) == 400
    rows = [(np.frombuffer(lines[4 * i + 1], dtype=np.uint8), np.frombuffer(lines[4 * i + 3], dtype=np.uint8)) for i in range(n)]
    rng = np.random.default_rng(17)
    for i in rng.integers(0, n, 200):
        r = fq[int(i)]
        assert _lat(r.seq) == rows[i][0].tobytes() and _lat(r.qual) == rows[i][1].tobytes()
    p = fq.phred or 33
    assert p == 33
    fast = trim_truth_fast                                    # the definition, vectorised per read (held to trim_truth on the CPU)
    a, b = want_of(p, rows, dict(adapter=AD), fn=fast)
    for i in rng.integers(0, n, 300):
        assert trim_truth(rows[i][0], rows[i][1], p, **truth_kwargs(trim.trim_args(adapter=AD))) == (a[i], b[i])
    frac = float((b < lens).mean())
    assert 0.20 <= frac <= 0.45, frac
    for kw in (dict(adapter=AD), dict(adapter=AD, min_overlap=1, max_error_rate=0.2), dict(front_qual=11, tail_qual=25), dict(window=(4, 20)),
               dict(window=(20, 30)), ALL):
        wa, wb = check_trim(fq, p, rows, kw, fn=fast)
        changed = int(((wa != 0) | (wb != lens)).sum())       # some reads and not all -- but a fixed clip changes every read
        assert changed == n if "clip_front" in kw else 0 < changed < n, kw
    ids = rng.permutation(n)[:50_000]                         # (repeats: test_fixtures; this file is written and opened again)
    check_trim(fq, p, rows, ALL, ids, fn=fast)
    t = fq.trim(ids=ids, **ALL)
    hdr = {int(i): lines[4 * int(i)] for i in ids}
    buf, offs = fq.records(ids, t["start"], t["end"], min_len=30)
    parts = [record(hdr[int(i)], rows[int(i)][0], rows[int(i)][1], int(x), int(y)) if y - x >= 30 else b""
             for i, x, y in zip(ids, t["start"], t["end"])]
    assert np.array_equal(np.diff(offs), [len(x) for x in parts]) and buf.tobytes() == b"".join(parts)
    out = str(tmp_path / "out.fq")
    r = fq.write(out, ids, t["start"], t["end"], min_len=30, batch_bytes=1 << 20)
    keep = (t["end"] - t["start"]) >= 30
    assert r == {"reads": int(keep.sum()), "bases": int((t["end"] - t["start"])[keep].sum()), "dropped": int((~keep).sum())}
    assert 0 < r["dropped"] < len(ids) and open(out, "rb").read() == b"".join(parts)
    back = fx.Fastq(out)
    assert len(back) == r["reads"] and np.array_equal(back.read_stats()["length"], (t["end"] - t["start"])[keep])


def test_empty_sequence_line(fx, tmp_path):
    """One read with an empty sequence (and quality) line among others: whatever fq[i] gives."""
    raw, lens = _irregular_fastq(40, 23, empty_at=17)
    p = tmp_path / "empty.fq"
    p.write_bytes(raw)
    fq = fx.Fastq(str(p))
    assert len(fq) == 40 and fq[17].seq == "" and fq[17].qual == ""
    check_everything(fq, np.random.default_rng(29))


def test_long_reads(fx, tmp_path):
    """Reads beyond 1024 bases do not fit a lane group: they are walked by one lane, with the same rules."""
    rng = np.random.default_rng(31)
    parts = []
    for i, L in enumerate([1500, 40, 1024, 1025, 3000, 7, 2047]):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()
        q = np.frombuffer(b"F:,#", dtype=np.uint8)[rng.choice(4, L, p=[0.7, 0.15, 0.1, 0.05])]
        if L > 30:
            at = int(rng.integers(L // 2, L - 5))
            m = min(len(AD), L - at)
            s[at:at + m] = np.frombuffer(AD.encode(), dtype=np.uint8)[:m]
        parts.append(b"@long%d\n" % i + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
    p = tmp_path / "long.fq"
    p.write_bytes(b"".join(parts))
    fq = fx.Fastq(str(p))
    assert len(fq) == 7 and int(fq.maxlen) == 3000
    check_everything(fq, np.random.default_rng(37))


def test_sharded_raises(fx, tmp_path, monkeypatch):
    """A stream in several windows is refused by all three methods, as the quality-control methods refuse it."""
    import torch
    from pyfastx_amd import synth
    n = 400_000                                               # ~140 MB
    blob, cols = synth.fastq_generate(n, torch.device("cuda", 0))
    raw = blob[:cols["n_bytes"]].cpu().numpy()
    del blob
    torch.cuda.empty_cache()
    p = str(tmp_path / "big.fq")
    raw.tofile(p)
    monkeypatch.setenv("FX_HBM_BUDGET", "64M")
    fq = fx.Fastq(p)
    assert fq._st.md is not None and fq._st.md.windows > 1 and fq._sharded and len(fq) == n
    for call in (lambda: fq.trim(front_qual=20), lambda: fq.trim(ids=[0, 1]), lambda: fq.records(), lambda: fq.records(ids=[0]),
                 lambda: fq.write(str(tmp_path / "x.fq")), lambda: fq.write(str(tmp_path / "x.fq"), ids=[0])):
        with pytest.raises(NotImplementedError):
            call()


def test_argument_errors(fx, tmp_path):
    shutil.copy(os.path.join(DATA, "test.fq"), tmp_path / "test.fq")
    fq = fx.Fastq(str(tmp_path / "test.fq"))
    for call in (lambda: fq.trim(adapter="ACGU"), lambda: fq.trim(adapter="ACGT", min_overlap=5), lambda: fq.trim(window=(0, 20)),
                 lambda: fq.trim(front_qual=256), lambda: fq.trim(tail_qual=-1), lambda: fq.trim(clip_front=-1),
                 lambda: fq.trim(adapter="ACGT", max_error_rate=-1), lambda: fq.records(min_len=-1), lambda: fq.records(start=[0] * 800),
                 lambda: fq.write(str(tmp_path / "x.fq"), batch_bytes=0)):
        with pytest.raises(ValueError):
            call()


def test_c_level_states(fx):
    """Before fx_fastq_build: FX_ESTATE from both; a byte-range shard: FX_EINVAL; bad arguments: FX_EINVAL; a bad interval:
    FX_ERANGE with its position."""
    from pyfastx_amd import _lib
    raw = open(os.path.join(DATA, "test.fq"), "rb").read()
    b = _lib.Blob.from_bytes(raw, device=0)
    for call in (lambda: b.fastq_trim(), lambda: b.fastq_format_alloc()):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_ESTATE
    b.fastq_build()
    s, e_ = b.fastq_trim()
    assert s.tolist() == [0] * 800 and e_.tolist() == [150] * 800
    for call in (lambda: b.fastq_trim(adapter=b"acgt", min_overlap=1), lambda: b.fastq_trim(adapter=b"ACGT", min_overlap=5),
                 lambda: b.fastq_trim(adapter=b"A" * 65, min_overlap=1), lambda: b.fastq_trim(front_qual=256), lambda: b.fastq_trim(clip_front=-1),
                 lambda: b.fastq_trim(window=(4, 20, 0)), lambda: b.fastq_trim(window=(-1, 20, 1)), lambda: b.fastq_format_alloc(min_len=-1),
                 lambda: b.fastq_format_alloc(start=[0] * 800)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    for ids, s, e_, where in (([3, 900], None, None, 1), ([1, 2, 3], [0, 0, 5], [150, 151, 4], 1), ([1, 2, 3], [0, 0, -1], [150, 150, 4], 2)):
        for call in ((lambda: b.fastq_trim(ids),) if s is None else ()) + (lambda: b.fastq_format_alloc(ids, s, e_),):
            with pytest.raises(_lib.FxError) as e:
                call()
            assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == where
    buf, offs, kept = b.fastq_format_alloc([5, 5], [0, 10], [150, 10], min_len=1)
    assert kept == 1 and offs[1] == offs[2] == len(buf)
    off = [i for i, c in enumerate(raw[:4096]) if c == 10][3] + 1          # where the second record begins
    b = _lib.Blob.from_bytes(raw[off:], device=0)
    b.set_shard(off, 10, True)
    assert b.fastq_build().n_reads > 0
    for call in (lambda: b.fastq_trim(), lambda: b.fastq_format_alloc()):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL


def test_scale_against_torch(fx):
    """2 M reads of 150 bases generated in HBM (synth.fastq_generate); the quality steps and the record sizes by torch over the
    (n_reads, rec) view, the adapter step on a slice of 50 000 reads against the definition."""
    import torch
    from pyfastx_amd import _lib, synth, trim
    dev = torch.device("cuda", 0)
    n, rlen = 2_000_000, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    rec, hl = int(cols["rec"]), int(cols["soff"][0])
    view = blob_t[:n * rec].view(n, rec)
    s, q = view[:, hl:hl + rlen], view[:, hl + rlen + 3:hl + 2 * rlen + 3]
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(cols["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    p, fq_, tq, w, wn, wd = 33, 12, 9, 6, 31, 2              # the scores are uniform on 2..37
    d = q.to(torch.int64) - p
    j = torch.arange(rlen, device=dev, dtype=torch.int64)
    ge = d >= fq_
    a = torch.where(ge.any(1), ge.to(torch.int8).argmax(1), torch.full((n,), rlen, device=dev))          # 3: first base at or above
    cs = torch.cat([torch.zeros((n, 1), dtype=torch.int64, device=dev), d.cumsum(1)], 1)
    Lw = rlen - a                                             # 4: windows of we = min(w, b - a) inside [a, rlen)
    we = torch.clamp(Lw, max=w)
    end_idx = torch.clamp(j[None, :] + we[:, None], max=rlen)
    ws = cs.gather(1, end_idx) - cs[:, :rlen]
    fail = (ws * wd < wn * we[:, None]) & (j[None, :] >= a[:, None]) & (j[None, :] + we[:, None] <= rlen) & (Lw[:, None] > 0)
    bb = torch.where(fail.any(1), fail.to(torch.int8).argmax(1), torch.full((n,), rlen, device=dev))
    okt = (d >= tq) & (j[None, :] >= a[:, None]) & (j[None, :] < bb[:, None])                            # 5: last base at or above
    last = rlen - 1 - okt.flip(1).to(torch.int8).argmax(1)
    bb = torch.where(okt.any(1), last + 1, a)
    st, en = b.fastq_trim(phred=p, front_qual=fq_, window=(w, wn, wd), tail_qual=tq)
    wa, wb = a.cpu().numpy(), bb.cpu().numpy()
    assert np.array_equal(st, wa) and np.array_equal(en, wb)
    assert 0 < int(((wa != 0) | (wb != rlen)).sum()) and int((wb - wa == rlen).sum()) > 0
    # record sizes and a sample of the bytes
    min_len = 60
    k = wb - wa
    hlen = hl - 1                                             # the header line without its '\n'
    size = np.where(k >= min_len, hlen + 2 * k + 5, 0)
    buf, offs, kept = b.fastq_format_alloc(None, st, en, min_len)
    assert np.array_equal(np.diff(offs), size) and kept == int((k >= min_len).sum()) and 0 < kept < n
    host = view[:2000].cpu().numpy()
    for i in range(2000):
        want = b"" if k[i] < min_len else record(host[i, :hlen].tobytes(), host[i, hl:hl + rlen], host[i, hl + rlen + 3:hl + 2 * rlen + 3], int(wa[i]), int(wb[i]))
        assert buf[offs[i]:offs[i + 1]].tobytes() == want
    # the adapter step on a slice, with letters of the adapter written into the reads first
    m = 50_000
    ids = np.arange(0, n, n // m, dtype=np.int64)[:m]
    A = torch.tensor(list(AD.encode()), dtype=torch.uint8, device=dev)
    g = torch.Generator(device="cpu").manual_seed(5)
    at = torch.randint(0, rlen, (m,), generator=g)
    for r, x in zip(ids[::3].tolist(), at[::3].tolist()):
        mm = min(len(AD), rlen - x)
        s[r, x:x + mm] = A[:mm]
    torch.cuda.synchronize(dev)
    hs, hq = s[torch.from_numpy(ids).to(dev)].cpu().numpy(), q[torch.from_numpy(ids).to(dev)].cpu().numpy()
    kw = dict(adapter=AD, min_overlap=3, max_error_rate=0.1, front_qual=fq_, tail_qual=tq)
    tk = truth_kwargs(trim.trim_args(**kw))
    want = [trim_truth(hs[i], hq[i], p, **tk) for i in range(m)]
    st, en = b.fastq_trim(ids, phred=p, **{**trim.trim_args(**kw)})
    assert st.tolist() == [x[0] for x in want] and en.tolist() == [x[1] for x in want]
    assert sum(1 for i in range(0, m, 3) if want[i][1] <= int(at[i])) > m // 4
