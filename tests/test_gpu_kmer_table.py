"""-m gpu: Fasta.kmer_table and Fastq.kmer_table (fx_fasta_kmer_table, fx_fastq_kmer_table, csrc/fx_kmer_table.hpp) against the
definition tests/kmer_table_truth.py, computed from fa[i].seq / fq[i].seq, from the strings a file was written from or from
a generator's flat bases -- never from the library's own k-mer path.  Every comparison is exact."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from kmer_table_truth import flat_codes, table_of_codes, table_truth
from kmer_truth import revcomp_code

pytestmark = pytest.mark.gpu

KS = (1, 7, 14, 21, 31)
MIB = 1 << 20


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def same(t, want, k=None, canonical=None):
    """A KmerTable against (codes, counts) of the truth."""
    codes, counts = want
    assert t.codes.dtype == np.int64 and t.counts.dtype == np.int64 and t.codes.shape == t.counts.shape == (len(t),)
    if k is not None:
        assert t.k == k and t.canonical == bool(canonical)
    return np.array_equal(t.codes, codes) and np.array_equal(t.counts, counts)


def check(obj, seqs, ks=KS, **kw):
    for k in ks:
        for canonical in (False, True):
            t = obj.kmer_table(k, canonical=canonical, **kw)
            assert same(t, table_truth(seqs, k, canonical), k, canonical), (k, canonical)
            assert t.counts.sum() == t.n_windows
            if canonical:
                assert (t.codes <= revcomp_code(t.codes, k)).all()


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, letters="ACGT"):
    return "".join(np.array(list(letters))[rng.integers(0, len(letters), n)]) if n else ""


def _fasta(seqs, width=60):
    out = []
    for i, s in enumerate(seqs):
        body = s + "\n" if width == 0 else "".join(s[a:a + width] + "\n" for a in range(0, len(s), width))
        out.append(">r%d\n%s" % (i, body))
    return "".join(out)


def _fastq(seqs):
    return "".join("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


# ------------------------------------------------------------------ 1, 2: the fixture files, the dense form
@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz", "test.fq", "test.fq.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz", "test.fq", "test.fq.gz"])
def test_fixture(fx, fixture_files, fn):
    obj = (fx.Fasta if ".fa" in fn else fx.Fastq)(fixture_files[fn])
    seqs = [obj[i].seq for i in range(len(obj))]
    check(obj, seqs)


@pytest.mark.parametrize("fn", ["test.fa", "test.fq"])
def test_agrees_with_dense(fx, fixture_files, fn):
    obj = (fx.Fasta if ".fa" in fn else fx.Fastq)(fixture_files[fn])
    for k in (6, 7, 13):
        for canonical in (False, True):
            dense = np.asarray(obj.kmer_counts(k, canonical=canonical))
            nz = np.nonzero(dense)[0].astype(np.int64)
            t = obj.kmer_table(k, canonical=canonical)
            assert same(t, (nz, dense[nz])), (k, canonical)
            assert t.n_windows == dense.sum()


# ------------------------------------------------------------------ 3: the warm-up over k - 1 <= 30 kept bytes
@pytest.mark.parametrize("width", [0, 61, 255, 256, 17, 7])
def test_long_warmup(fx, tmp_path, width):
    """A run begins at every 256-byte block of the stream; at width 7 a window of 31 covers five lines, and the records of 1,
    30 and 31 bases in front make record starts fall inside the reach of a later run."""
    rng = np.random.default_rng(300 + width)
    seqs = [_rand(rng, n) for n in (1, 30, 31, 3000, 30, 1, 31, 700)]
    fa = fx.Fasta(_write(tmp_path / "w.fa", _fasta(seqs, width)))
    assert [fa[i].seq for i in range(len(fa))] == seqs
    check(fa, seqs, ks=(14, 17, 31))


# ------------------------------------------------------------------ 4: lengths around k
def test_lengths_around_k(fx, tmp_path):
    rng = np.random.default_rng(4)
    k = 31
    seqs = [_rand(rng, n) for n in (k - 1, k, k + 1)]
    fa = fx.Fasta(_write(tmp_path / "l.fa", _fasta(seqs)))
    check(fa, seqs, ks=(k,))
    assert [fa.kmer_table(k, ids=[i]).n_windows for i in range(3)] == [0, 1, 2]
    lens = (15, 16, 17, 30, 31, 32, 33, 47, 48, 49, 400)
    reads = [_rand(rng, n) for n in lens]
    fq = fx.Fastq(_write(tmp_path / "l.fq", _fastq(reads)))
    check(fq, reads, ks=(k, 16, 17))
    assert [fq.kmer_table(k, ids=[i]).n_windows for i in range(len(lens))] == [max(n - k + 1, 0) for n in lens]
    # intervals shorter than k, equal to k, the whole read, and one that begins inside a 16-byte piece
    ids = [10, 10, 10, 10, 7, 5]
    start = [5, 100, 0, 37, 16, 1]
    end = [35, 131, 400, 390, 47, 32]
    cut = [reads[i][a:b] for i, a, b in zip(ids, start, end)]
    for canonical in (False, True):
        t = fq.kmer_table(k, canonical=canonical, ids=ids, start=start, end=end)
        assert same(t, table_truth(cut, k, canonical)), canonical
        assert t.n_windows == 0 + 1 + 370 + 323 + 1 + 1


# ------------------------------------------------------------------ 5: invalid bytes
def test_invalid_bytes(fx, tmp_path):
    rng = np.random.default_rng(5)
    s = list(_rand(rng, 4000))
    s[::40] = "N" * len(s[::40])                               # 31 of every 40 windows of 31 hold an N
    s = "".join(s)
    mixed = _rand(rng, 900)
    seqs = [s, mixed, mixed.lower(), "N" * 500]
    fa = fx.Fasta(_write(tmp_path / "n.fa", _fasta(seqs)))
    check(fa, seqs, ks=(31, 14))
    assert fa.kmer_table(31, ids=[0]).n_windows == 100 * 9
    assert same(fa.kmer_table(31, ids=[1]), (fa.kmer_table(31, ids=[2]).codes, fa.kmer_table(31, ids=[2]).counts))
    only_n = fx.Fasta(_write(tmp_path / "nn.fa", _fasta(["N" * 3000, "n" * 70])))
    for k in (1, 21, 31):
        t = only_n.kmer_table(k, canonical=True)
        assert len(t) == 0 and t.codes.shape == (0,) and t.counts.shape == (0,) and t.n_windows == 0 and t.n_parts == 0
    fq = fx.Fastq(_write(tmp_path / "n.fq", _fastq([s, mixed.lower(), "N" * 100])))
    check(fq, [s, mixed.lower(), "N" * 100], ks=(31,))


# ------------------------------------------------------------------ 6: the cut at slen
def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: slen is smaller than the number of kept
    bytes and `seq` stops there -- no window may reach past that cut."""
    rng = np.random.default_rng(55)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 12, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert any(len(s) < n for s, n in zip(seqs, kept)), "no record is cut: the case is not exercised"
    check(fa, seqs, ks=(14, 31))
    assert same(fa.kmer_table(31, ids=[4, 1, 4]), table_truth([seqs[4], seqs[1], seqs[4]], 31))


# ------------------------------------------------------------------ 7: canonical
def test_canonical(fx, tmp_path):
    rng = np.random.default_rng(7)
    h7, h15 = _rand(rng, 7), _rand(rng, 15)
    pal14, pal30 = h7 + _rc(h7), h15 + _rc(h15)
    body = _rand(rng, 500) + pal14 + _rand(rng, 300) + pal30 + _rand(rng, 200) + pal30 + "N" + pal14
    seqs = [body, _rc(body)]
    fa = fx.Fasta(_write(tmp_path / "c.fa", _fasta(seqs)))
    check(fa, seqs, ks=(14, 30, 31, 21))
    from pyfastx_amd import kmer
    for k, pal, times in ((14, pal14, 2), (30, pal30, 2)):
        code = kmer.kmer_code(pal, k)
        assert int(revcomp_code(np.int64(code), k)) == code
        assert fa.kmer_table(k, canonical=True, ids=[0]).count(pal) == times      # its own reverse complement: once per occurrence
        assert fa.kmer_table(k, canonical=True).count(pal) == 2 * times
    for k in (14, 30, 31):
        a, b = fa.kmer_table(k, canonical=True, ids=[0]), fa.kmer_table(k, canonical=True, ids=[1])
        assert same(a, (b.codes, b.counts)) and len(a) > 0


# ------------------------------------------------------------------ 8, 9: runs of equal keys, key counts around the tile
def test_equal_keys_across_tiles(fx, tmp_path):
    rng = np.random.default_rng(8)
    seqs = ["A" * 5000, "AC" * 3000, "ACG" * 2000, "ACGT" * 2000, _rand(rng, 2000)]
    fa = fx.Fasta(_write(tmp_path / "lc.fa", _fasta(seqs, 80)))
    t = fa.kmer_table(31, ids=[0])
    assert t.codes.tolist() == [0] and t.counts.tolist() == [4970] and t.n_windows == 4970
    t = fa.kmer_table(31, canonical=True, ids=[0, 0])
    assert t.codes.tolist() == [0] and t.counts.tolist() == [9940]
    for i, distinct in ((1, 2), (2, 3), (3, 4)):
        assert len(fa.kmer_table(31, ids=[i])) == distinct
    check(fa, seqs, ks=(31, 21, 13))                           # all-equal digits (skipped passes) and mixed ones in one sort
    fq = fx.Fastq(_write(tmp_path / "lc.fq", _fastq(seqs)))
    check(fq, seqs, ks=(31,))


def test_key_counts_around_the_tile(fx, tmp_path):
    rng = np.random.default_rng(9)
    k = 31
    ns = (1, 2047, 2048, 2049)
    seqs = [_rand(rng, k + n - 1) for n in ns]
    fa = fx.Fasta(_write(tmp_path / "t.fa", _fasta(seqs, 70)))
    fq = fx.Fastq(_write(tmp_path / "t.fq", _fastq(seqs)))
    for obj in (fa, fq):
        for i, n in enumerate(ns):
            for canonical in (False, True):
                t = obj.kmer_table(k, canonical=canonical, ids=[i])
                assert t.n_windows == n and same(t, table_truth([seqs[i]], k, canonical)), (i, canonical)


# ------------------------------------------------------------------ 10, 11: budgets
def test_small_budget_many_partitions(fx, tmp_path):
    rng = np.random.default_rng(10)
    base = open(os.path.join(DATA, "test.fa")).read()
    big = _rand(rng, 600_000)
    fa = fx.Fasta(_write(tmp_path / "b.fa", base + _fasta([big], 80).replace(">r0", ">big")))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert seqs[-1] == big
    for k in (21, 31):
        for canonical in (False, True):
            want = table_truth(seqs, k, canonical)
            t = fa.kmer_table(k, canonical=canonical, max_bytes=MIB)
            d = fa.kmer_table(k, canonical=canonical)
            assert same(t, want) and same(d, want), (k, canonical)
            assert t.n_parts >= 3 and d.n_parts == 1 and t.n_windows == d.n_windows == want[1].sum()
            assert (np.diff(t.codes) > 0).all()


def test_bin_above_the_cap_and_min_count_after_the_fold(fx, tmp_path):
    """Poly-A and (AC)n put 3 x 10^5 windows into one code range each, more than 1 MiB holds: those ranges are taken in
    position sub-chunks and folded.  A motif planted twice, 250 000 bases apart, has count 2 only after the fold."""
    from pyfastx_amd import kmer
    rng = np.random.default_rng(11)
    k = 21
    motif = _rand(rng, 40, "CGT")
    poly = "A" * 300_000
    planted = "A" * 20_000 + "C" + motif + "C" + "A" * (250_000 - 42) + "C" + motif + "C" + "A" * 29_000
    seqs = [poly, "AC" * 150_000, _rand(rng, 5000), planted]
    fa = fx.Fasta(_write(tmp_path / "f.fa", _fasta(seqs, 80)))
    t = fa.kmer_table(k, ids=[0, 1, 2], max_bytes=MIB)
    assert same(t, table_truth(seqs[:3], k)) and t.count("A" * k) == 299_980 and t.n_parts >= 3
    sel = [3, 1, 2]
    picked = [seqs[i] for i in sel]
    windows = table_truth(picked, k)[1].sum()
    shared = "A" * 10 + "C" + motif[:10]                       # begins inside the poly-A stretch: the code range of the poly-A code
    for canonical in (False, True):
        for m in (1, 2, 3):
            t = fa.kmer_table(k, canonical=canonical, ids=sel, min_count=m, max_bytes=MIB)
            assert same(t, table_truth(picked, k, canonical, m)), (canonical, m)
            assert t.n_windows == windows and (t.counts >= m).all()
            assert t.count(shared) == (2 if m <= 2 else 0) and t.count(motif[3:3 + k]) == (2 if m <= 2 else 0)
            d = fa.kmer_table(k, canonical=canonical, ids=sel, min_count=m)
            assert same(d, (t.codes, t.counts)) and d.n_parts == 1
    assert kmer.kmer_code(shared, k) >> 30 == 0
    fq = fx.Fastq(_write(tmp_path / "f.fq", _fastq(seqs)))      # one read of 3 x 10^5 windows does not fit a key buffer of 1 MiB
    from pyfastx_amd import _lib
    with pytest.raises(_lib.FxError) as e:
        fq.kmer_table(k, max_bytes=MIB)
    assert e.value.code == _lib.FX_ENOMEM and "max_bytes" in str(e.value)
    assert same(fq.kmer_table(k, min_count=2, max_bytes=64 * MIB), table_truth(seqs, k, False, 2))


# ------------------------------------------------------------------ 12, 13: selections, states
def test_selections(fx, fixture_files):
    from pyfastx_amd import _lib
    fa = fx.Fasta(fixture_files["test.fa"])
    fq = fx.Fastq(fixture_files["test.fq"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    t = fa.kmer_table(21, ids=[2, 0, 2])
    assert same(t, table_truth([seqs[2], seqs[0], seqs[2]], 21))
    assert same(fa.kmer_table(21, ids=[names[2], names[0], names[2]]), (t.codes, t.counts))
    reads = [fq[i].seq for i in (5, 3, 5)]
    assert same(fq.kmer_table(25, canonical=True, ids=[5, 3, 5], min_count=2), table_truth(reads, 25, True, 2))
    for obj in (fa, fq):
        e = obj.kmer_table(21, ids=[])
        assert len(e) == 0 and e.n_windows == 0 and e.codes.dtype == np.int64
        with pytest.raises(IndexError):
            obj.kmer_table(21, ids=[0, len(obj)])
        for bad in (dict(k=0), dict(k=32), dict(k=21, min_count=0), dict(k=21, max_bytes=4096), dict(k=21.0), dict(k=21, min_count=True)):
            with pytest.raises(ValueError):
                obj.kmer_table(**bad)
    with pytest.raises(ValueError, match="query 1"):
        fq.kmer_table(21, ids=[1, 2, 3], start=[0, 0, 0], end=[150, 151, 4])
    b = fa._search_blob()
    with pytest.raises(_lib.FxError) as e:
        b.fasta_kmer_table(21, ids=[0, 1, len(fa)])
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2


def test_c_level_states(fx):
    from pyfastx_amd import _lib
    L = _lib.lib()
    raw = open(os.path.join(DATA, "test.fa"), "rb").read()
    b = _lib.Blob.from_bytes(raw, device=0)
    with pytest.raises(_lib.FxError) as e:
        b.fasta_kmer_table(21)
    assert e.value.code == _lib.FX_ESTATE
    b.fasta_build()
    codes, counts, nw, parts = b.fasta_kmer_table(21)
    assert counts.sum() == nw > 0 and parts == 1
    for call in (lambda: b.fasta_kmer_table(0), lambda: b.fasta_kmer_table(32), lambda: b.fasta_kmer_table(21, min_count=0),
                 lambda: b.fasta_kmer_table(21, max_bytes=4096), lambda: b.fasta_kmer_table(21, max_bytes=-1)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL

    def raw_fasta(flags=0, null=None):
        out = [C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)]
        refs = [None if i == null else C.byref(o) for i, o in enumerate(out)]
        return L.fx_fasta_kmer_table(b._h, 21, flags, None, 0, 1, 0, *refs), out

    assert raw_fasta()[0] == _lib.FX_OK
    assert raw_fasta(flags=2)[0] == _lib.FX_EINVAL and raw_fasta(flags=_lib.FX_KMER_CANONICAL | 4)[0] == _lib.FX_EINVAL
    for i in range(6):
        assert raw_fasta(null=i)[0] == _lib.FX_EINVAL, i
    out = [C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)]
    assert L.fx_fasta_kmer_table(None, 21, 0, None, 0, 1, 0, *[C.byref(o) for o in out]) == _lib.FX_EINVAL
    rawq = open(os.path.join(DATA, "test.fq"), "rb").read()
    q = _lib.Blob.from_bytes(rawq, device=0)
    with pytest.raises(_lib.FxError) as e:
        q.fastq_kmer_table(21)
    assert e.value.code == _lib.FX_ESTATE
    q.fastq_build()
    assert 0 < q.fastq_kmer_table(21)[2] <= 800 * 130
    for call in (lambda: q.fastq_kmer_table(0), lambda: q.fastq_kmer_table(32), lambda: q.fastq_kmer_table(21, start=[0] * 800),
                 lambda: q.fastq_kmer_table(21, min_count=0), lambda: q.fastq_kmer_table(21, max_bytes=4096)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    for ids, s, e_, where in (([3, 900], None, None, 1), ([1, 2, 3], [0, 0, 5], [150, 151, 4], 1), ([1, 2, 3], [0, 0, -1], [150, 150, 4], 2)):
        with pytest.raises(_lib.FxError) as e:
            q.fastq_kmer_table(21, ids=ids, start=s, end=e_)
        assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == where
    off = [i for i, c in enumerate(rawq[:4096]) if c == 10][3] + 1         # where the second record begins
    q = _lib.Blob.from_bytes(rawq[off:], device=0)
    q.set_shard(off, 10, True)
    assert q.fastq_build().n_reads > 0
    with pytest.raises(_lib.FxError) as e:
        q.fastq_kmer_table(21)
    assert e.value.code == _lib.FX_EINVAL


def test_sharded_raises(fx, fixture_files, monkeypatch):
    fa = fx.Fasta(fixture_files["test.fa"])
    fq = fx.Fastq(fixture_files["test.fq"])
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    monkeypatch.setattr(type(fq), "_sharded", property(lambda self: True))
    for call in (lambda: fa.kmer_table(21), lambda: fq.kmer_table(21), lambda: fa.kmer_table(21, ids=[0])):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------ 14: one mid-size leg each
def test_synthetic_genome_20mbp(fx):
    import torch
    from pyfastx_amd import _lib, kmer, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=20_000_000)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fasta_build().n_seq == len(plan["slen"])
    flat = flat_t.cpu().numpy()
    del flat_t
    want = table_of_codes(flat_codes(flat, flat_start, 21, True))
    assert want[1].sum() > 15_000_000
    t = kmer.fasta_table_blob(b, 21, canonical=True)
    assert same(t, want, 21, True) and t.n_windows == want[1].sum() and t.n_parts == 1
    keep = want[1] >= 2
    assert same(kmer.fasta_table_blob(b, 21, canonical=True, min_count=2, max_bytes=64 * MIB), (want[0][keep], want[1][keep]))
    del b, blob_t


def test_synthetic_reads_200k(fx):
    import torch
    from pyfastx_amd import _lib, kmer, synth
    dev = torch.device("cuda", 0)
    n, rlen = 200_000, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    rec, hl = int(cols["rec"]), int(cols["soff"][0])
    bases = blob_t[:n * rec].view(n, rec)[:, hl:hl + rlen].cpu().numpy()
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(cols["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    flat = np.ascontiguousarray(bases).reshape(-1)
    want = table_of_codes(flat_codes(flat, np.arange(n, dtype=np.int64) * rlen, 25))
    t = kmer.fastq_table_blob(b, n, 25)
    assert same(t, want, 25, False) and t.n_windows == want[1].sum()
    small = kmer.fastq_table_blob(b, n, 25, max_bytes=32 * MIB)
    assert same(small, want) and small.n_parts > 1
    del b, blob_t
