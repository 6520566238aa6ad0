"""-m gpu: Fastq.read_stats / cycle_profile / select (fx_fastq_read_stats, fx_fastq_cycle_hist, fx_fastq_select,
csrc/fx_fastq_qc.hpp) against plain numpy over fq[i].seq / fq[i].qual of the same file -- every comparison exact -- on the
fixtures, on every input of tests/golden/fastq_edge.json, on a generated file of irregular reads, and against torch on a
synthetic stream of 2 M reads."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA, load_golden

pytestmark = pytest.mark.gpu

EDGE = load_golden("fastq_edge")
# inputs of fastq_edge.json that Fastq(path) itself refuses: name -> the exception.  (None: every input opens.)
EDGE_REFUSED = {}


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


def stats_truth(p, rows, low_qual=20, ids=None):
    sel = range(len(rows)) if ids is None else ids
    out = {k: [] for k in ("length", "qsum", "qmin", "qmax", "n_low", "n_gc", "n_other")}
    for i in sel:
        s, q = rows[int(i)]
        d = q.astype(np.int64) - p
        out["length"].append(len(s))
        out["qsum"].append(int(d.sum()))
        out["qmin"].append(int(d.min()) if len(d) else 0)
        out["qmax"].append(int(d.max()) if len(d) else 0)
        out["n_low"].append(int((d < low_qual).sum()))
        out["n_gc"].append(int(((s == ord("G")) | (s == ord("C"))).sum()))
        out["n_other"].append(int((~np.isin(s, np.frombuffer(b"ACGT", dtype=np.uint8))).sum()))
    dt = {"length": np.int64, "qsum": np.int64, "qmin": np.int16, "qmax": np.int16, "n_low": np.int32, "n_gc": np.int32, "n_other": np.int32}
    return {k: np.array(v, dtype=dt[k]) for k, v in out.items()}


def cycle_truth(rows, cycles):
    qual = np.zeros((cycles, 256), dtype=np.int64)
    base = np.zeros((cycles, 5), dtype=np.int64)
    depth = np.zeros(cycles, dtype=np.int64)
    cls = np.full(256, 4, dtype=np.int64)
    for k, c in enumerate(b"ACGT"):
        cls[c] = k
    for s, q in rows:
        m = min(len(s), cycles)
        j = np.arange(m)
        np.add.at(qual, (j, q[:m]), 1)
        np.add.at(base, (j, cls[s[:m]]), 1)
        depth[:m] += 1
    return qual, base, depth


def check_stats(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), k


def check_profile(prof, rows, cycles):
    qual, base, depth = cycle_truth(rows, cycles)
    assert prof.qual.shape == (cycles, 256) and prof.base.shape == (cycles, 5) and prof.depth.shape == (cycles,)
    assert prof.qual.dtype == prof.base.dtype == prof.depth.dtype == np.int64
    assert np.array_equal(prof.qual, qual)
    assert np.array_equal(prof.base, base)
    assert np.array_equal(prof.depth, depth)


def mask_of(st, min_len=None, max_len=None, mean_qual=None, low_frac=None, max_other=None):
    """The integer inequalities of select over read_stats columns; the ratios as (num, den)."""
    L, qs, nl, no = (st[k].astype(np.int64) for k in ("length", "qsum", "n_low", "n_other"))
    m = np.ones(len(L), dtype=bool)
    if min_len is not None:
        m &= L >= min_len
    if max_len is not None:
        m &= L <= max_len
    if mean_qual is not None:
        m &= qs * mean_qual[1] >= mean_qual[0] * L
    if low_frac is not None:
        m &= nl * low_frac[1] <= low_frac[0] * L
    if max_other is not None:
        m &= no <= max_other
    return np.nonzero(m)[0].astype(np.int64)


def check_everything(fq, rng, well_formed):
    """read_stats (all, gathered, other thresholds), cycle_profile (default, shorter, longer), select, on one object."""
    p, rows = truth_of(fq)
    n = len(rows)
    st = fq.read_stats()
    check_stats(st, stats_truth(p, rows))
    for lq in (0, 2, 41, 255):
        check_stats(fq.read_stats(low_qual=lq), stats_truth(p, rows, lq))
    ids = rng.integers(0, n, 3 * n + 5)
    check_stats(fq.read_stats(ids=ids, low_qual=30), stats_truth(p, rows, 30, ids))
    check_stats(fq.read_stats(ids=[]), stats_truth(p, rows, 20, []))
    for bad in ([n], [-1], [0, n + 7, 0]):
        with pytest.raises(IndexError, match="index out of range"):
            fq.read_stats(ids=bad)
    maxlen = max((len(s) for s, _ in rows), default=0)
    prof = fq.cycle_profile()
    assert prof.cycles == max(int(fq.maxlen), 1) and prof.phred == p
    check_profile(prof, rows, prof.cycles)
    if maxlen > 1:
        check_profile(fq.cycle_profile(cycles=maxlen // 2), rows, maxlen // 2)
    big = fq.cycle_profile(cycles=maxlen + 70)
    check_profile(big, rows, maxlen + 70)
    assert not big.qual[maxlen:].any() and not big.base[maxlen:].any() and not big.depth[maxlen:].any()
    check_profile(fq.cycle_profile(cycles=1), rows, 1)
    if well_formed:
        comp = fq.composition
        assert big.base.sum(0).tolist() == [comp[k] for k in "ACGT"] + [comp["N"]]
        assert big.depth[0] == len(fq)
        assert np.array_equal(big.qual.sum(1), big.depth)
        qs = big.qual_scores
        assert int(st["qsum"].sum()) == int((qs * np.arange(qs.shape[1], dtype=np.int64)).sum())
    # select: each criterion alone, all together, everything, nothing
    from pyfastx_amd import qc
    Ls = sorted(len(s) for s, _ in rows)
    midL = Ls[len(Ls) // 2]
    mq = max(float(np.median(st["qsum"] / np.maximum(st["length"], 1))), 0.0)
    cases = [dict(min_len=midL), dict(max_len=midL), dict(min_mean_qual=mq), dict(min_mean_qual=int(mq)), dict(max_low_frac=0.05),
             dict(max_low_frac=0.5, low_qual=38), dict(max_other=0), dict(max_other=1),
             dict(min_len=max(midL - 3, 0), max_len=midL + 40, min_mean_qual=max(mq - 2, 0), max_low_frac=0.4, max_other=2, low_qual=30),
             dict(), dict(min_len=0, min_mean_qual=0, max_low_frac=1, max_other=10**6), dict(min_len=maxlen + 1),
             dict(min_mean_qual=250), dict(min_mean_qual=30, max_other=0)]
    for kw in cases:
        lq = kw.get("low_qual", 20)
        stq = st if lq == 20 else fq.read_stats(low_qual=lq)
        want = mask_of(stq, kw.get("min_len"), kw.get("max_len"),
                       None if "min_mean_qual" not in kw else qc.as_ratio(kw["min_mean_qual"]),
                       None if "max_low_frac" not in kw else qc.as_ratio(kw["max_low_frac"]), kw.get("max_other"))
        got = fq.select(**kw)
        assert got.dtype == np.int64 and np.array_equal(got, want), kw
    assert len(fq.select()) == n and len(fq.select(min_len=maxlen + 1)) == 0
    # the loop closed: the selected reads, fetched
    ids = fq.select(min_mean_qual=30, max_other=0)
    r = fq.fetch_many(ids, want=("seq", "qual"))
    assert len(r["offsets"]) == len(ids) + 1
    for k, i in enumerate(ids):
        a, b = int(r["offsets"][k]), int(r["offsets"][k + 1])
        assert r["seq"][a:b].tobytes() == rows[int(i)][0].tobytes() and r["qual"][a:b].tobytes() == rows[int(i)][1].tobytes()
        assert np.isin(rows[int(i)][0], np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    return st


@pytest.mark.parametrize("fn", ["test.fq", "test.fq.gz"])
def test_fixtures(fx, tmp_path, fn):
    shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
    fq = fx.Fastq(str(tmp_path / fn))
    st = check_everything(fq, np.random.default_rng(3), well_formed=True)
    assert len(st["length"]) == 800


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_inputs(fx, tmp_path, name):
    """Every input of fastq_edge.json, opened as a file; quirks (a '\\r' inside a quality line, a truncated tail) come out
    as fq[i].seq / fq[i].qual show them."""
    path = tmp_path / (name + ".fq")
    path.write_bytes(EDGE[name]["text"].encode("latin-1"))
    assert name not in EDGE_REFUSED
    fq = fx.Fastq(str(path))
    assert len(fq) == EDGE[name]["count"]
    check_everything(fq, np.random.default_rng(5), well_formed=False)


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


@pytest.fixture(scope="module")
def irregular(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("qc_irregular")
    raw, lens = _irregular_fastq(200_000, 11)
    p = d / "irregular.fq"
    p.write_bytes(raw)
    return fx.Fastq(str(p)), raw, lens


def test_generated_irregular_reads(fx, irregular):
    """2 x 10^5 reads of 1..400 bases: several 16-byte pieces and lane groups per read, seven tiles of 64 cycles, four
    quality values (every lane of a cycle hits the same few counters), lower-case and IUPAC letters.  The truth is taken
    from the file's own bytes, line by line; a sample of reads pins that against fq[i]."""
    fq, raw, lens = irregular
    lines = raw.split(b"\n")
    n = len(lens)
    assert len(fq) == n
    rows = [(np.frombuffer(lines[4 * i + 1], dtype=np.uint8), np.frombuffer(lines[4 * i + 3], dtype=np.uint8)) for i in range(n)]
    rng = np.random.default_rng(17)
    for i in rng.integers(0, n, 200):
        r = fq[int(i)]
        assert _lat(r.seq) == rows[i][0].tobytes() and _lat(r.qual) == rows[i][1].tobytes()
    p = fq.phred or 33
    assert p == 33
    want = stats_truth(p, rows)
    st = fq.read_stats()
    check_stats(st, want)
    ids = rng.integers(0, n, 50_000)
    got = fq.read_stats(ids=ids, low_qual=12)
    w12 = stats_truth(p, rows, 12)
    check_stats(got, {k: v[ids] for k, v in w12.items()})
    with pytest.raises(IndexError, match="index out of range"):
        fq.read_stats(ids=[0, n])
    assert int(fq.maxlen) == 400
    for cycles in (None, 64, 65, 150, 470):
        prof = fq.cycle_profile(cycles=cycles)
        check_profile(prof, rows, 400 if cycles is None else cycles)
    big = fq.cycle_profile(cycles=470)
    comp = fq.composition
    assert big.base.sum(0).tolist() == [comp[k] for k in "ACGT"] + [comp["N"]]
    assert big.depth[0] == n and np.array_equal(big.qual.sum(1), big.depth) and not big.depth[400:].any()
    qs = big.qual_scores
    assert int(st["qsum"].sum()) == int((qs * np.arange(qs.shape[1], dtype=np.int64)).sum())
    from pyfastx_amd import qc
    for kw in (dict(min_len=100), dict(max_len=250), dict(min_mean_qual=30), dict(min_mean_qual=31.37), dict(max_low_frac=0.1),
               dict(max_low_frac="1/7", low_qual=12), dict(max_other=0), dict(max_other=3),
               dict(min_len=50, max_len=350, min_mean_qual=29.5, max_low_frac=0.25, max_other=5), dict(), dict(min_len=401),
               dict(min_mean_qual=38), dict(min_mean_qual=0, max_low_frac=1)):
        stq = st if kw.get("low_qual", 20) == 20 else w12
        wantm = mask_of(stq, kw.get("min_len"), kw.get("max_len"),
                        None if "min_mean_qual" not in kw else qc.as_ratio(kw["min_mean_qual"]),
                        None if "max_low_frac" not in kw else qc.as_ratio(kw["max_low_frac"]), kw.get("max_other"))
        assert np.array_equal(fq.select(**kw), wantm), kw
    assert len(fq.select(min_len=401)) == 0 and len(fq.select()) == n
    ids = fq.select(min_mean_qual=30, max_other=0)
    assert 0 < len(ids) < n
    r = fq.fetch_many(ids, want=("seq", "qual"))
    assert np.array_equal(np.diff(r["offsets"]), lens[ids])
    for k in rng.integers(0, len(ids), 300):
        a, b = int(r["offsets"][k]), int(r["offsets"][k + 1])
        assert r["seq"][a:b].tobytes() == rows[int(ids[k])][0].tobytes() and r["qual"][a:b].tobytes() == rows[int(ids[k])][1].tobytes()


def test_empty_sequence_line(fx, tmp_path):
    """One read with an empty sequence (and quality) line among others (the index accepts it): whatever fq[i] gives."""
    raw, lens = _irregular_fastq(40, 23, empty_at=17)
    p = tmp_path / "empty.fq"
    p.write_bytes(raw)
    fq = fx.Fastq(str(p))
    assert len(fq) == 40 and fq[17].seq == "" and fq[17].qual == ""
    check_everything(fq, np.random.default_rng(29), well_formed=False)


def test_sharded_raises(fx, tmp_path, monkeypatch):
    """A stream in several windows (larger than the HBM it may use, as tests/test_gpu_windows.py makes one) is refused by all
    three methods, as Fasta.search_all refuses it; what the object already answers keeps working."""
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
    for call in (lambda: fq.read_stats(), lambda: fq.read_stats(ids=[0, 1]), lambda: fq.cycle_profile(),
                 lambda: fq.cycle_profile(cycles=10), lambda: fq.select(min_len=1), lambda: fq.select()):
        with pytest.raises(NotImplementedError):
            call()
    r = fq.fetch_many([0, n - 1], want=("seq",))
    assert np.diff(r["offsets"]).tolist() == [150, 150]


def test_argument_errors(fx, tmp_path):
    shutil.copy(os.path.join(DATA, "test.fq"), tmp_path / "test.fq")
    fq = fx.Fastq(str(tmp_path / "test.fq"))
    for call in (lambda: fq.read_stats(low_qual=256), lambda: fq.read_stats(low_qual=-1), lambda: fq.cycle_profile(cycles=0),
                 lambda: fq.cycle_profile(cycles=65537), lambda: fq.select(min_len=10, max_len=9), lambda: fq.select(min_mean_qual=-1),
                 lambda: fq.select(max_low_frac=-0.5), lambda: fq.select(max_other=-1), lambda: fq.select(low_qual=256)):
        with pytest.raises(ValueError):
            call()
    assert fq.cycle_profile(cycles=65536).qual.shape == (65536, 256)


def test_c_level_states(fx):
    """Before fx_fastq_build: FX_ESTATE from all three; a byte-range shard: FX_EINVAL."""
    from pyfastx_amd import _lib
    raw = open(os.path.join(DATA, "test.fq"), "rb").read()
    b = _lib.Blob.from_bytes(raw, device=0)
    for call in (lambda: b.fastq_read_stats(), lambda: b.fastq_cycle_hist(10), lambda: b.fastq_select()):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_ESTATE
    b.fastq_build()
    assert len(b.fastq_select()) == 800
    off = [i for i, c in enumerate(raw[:4096]) if c == 10][3] + 1          # where the second record begins
    b = _lib.Blob.from_bytes(raw[off:], device=0)
    b.set_shard(off, 10, True)                                # the stream from its second record on, as a shard at `off`
    assert b.fastq_build().n_reads > 0                       # (which reads a shard owns is the sharded build's business)
    for call in (lambda: b.fastq_read_stats(), lambda: b.fastq_cycle_hist(10), lambda: b.fastq_select()):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL


def test_scale_against_torch(fx):
    """2 M reads of 150 bases generated in HBM (synth.fastq_generate); the truth by torch over the (n_reads, rec) view."""
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda", 0)
    n, rlen = 2_000_000, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)                               # the generator's last writes, before the library's own stream reads the blob
    rec, hl = int(cols["rec"]), int(cols["soff"][0])
    view = blob_t[:n * rec].view(n, rec)
    s, q = view[:, hl:hl + rlen], view[:, hl + rlen + 3:hl + 2 * rlen + 3]
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(cols["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    p, lq = 33, 20
    d = q.to(torch.int64) - p
    acgt = (s == 65) | (s == 67) | (s == 71) | (s == 84)
    want = {"length": torch.full((n,), rlen, dtype=torch.int64), "qsum": d.sum(1), "qmin": d.min(1).values.to(torch.int16),
            "qmax": d.max(1).values.to(torch.int16), "n_low": (d < lq).sum(1).to(torch.int32),
            "n_gc": ((s == 67) | (s == 71)).sum(1).to(torch.int32), "n_other": (~acgt).sum(1).to(torch.int32)}
    st = b.fastq_read_stats(phred=p, low_qual=lq)
    for k, v in want.items():
        assert np.array_equal(st[k], v.cpu().numpy()), k
    qual, base, depth = b.fastq_cycle_hist(rlen)
    j = torch.arange(rlen, device=dev, dtype=torch.int64)
    wq = torch.bincount((j[None, :] * 256 + q.to(torch.int64)).view(-1), minlength=rlen * 256).view(rlen, 256)
    cls = torch.full((256,), 4, dtype=torch.int64, device=dev)
    for k, c in enumerate(b"ACGT"):
        cls[c] = k
    wb = torch.bincount((j[None, :] * 5 + cls[s.to(torch.int64)]).view(-1), minlength=rlen * 5).view(rlen, 5)
    assert np.array_equal(qual, wq.cpu().numpy()) and np.array_equal(base, wb.cpu().numpy())
    assert np.array_equal(depth, np.full(rlen, n, dtype=np.int64))
    # mean score >= 19.5 (the scores are uniform on 2..37), at most one non-ACGT byte, at most 2 % of the scores below 3
    d3 = (d < 3).sum(1)
    m = (want["qsum"] * 2 >= 39 * rlen) & (want["n_other"].to(torch.int64) <= 1) & (d3 * 50 <= rlen)
    ids = b.fastq_select(phred=p, low_qual=3, mean_qual=(39, 2), low_frac=(1, 50), max_other=1)
    assert np.array_equal(ids, torch.nonzero(m).view(-1).cpu().numpy())
    assert 0 < len(ids) < n
