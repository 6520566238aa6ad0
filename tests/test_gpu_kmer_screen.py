"""-m gpu: the device k-mer set (fx_kmer_set_*), Fastq.kmer_hits / screen and Fasta.kmer_hits (csrc/fx_kmer_screen.hpp) against
the definition tests/kmer_screen_truth.py, computed from the strings a file was written from or from fa[i].seq / fq[i].seq --
never from the library's own k-mer path.  Every comparison is exact."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from kmer_screen_truth import hits_of_codes, hits_truth, screen_truth
from kmer_table_truth import flat_codes, table_truth
from kmer_truth import counted_codes, revcomp_code

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


@pytest.fixture(scope="module")
def blob(fx):
    """A handle on device 0 to create sets through."""
    from pyfastx_amd import _lib
    b = _lib.Blob.from_bytes(b">a\nACGT\n", device=0)
    yield b
    b.close()


def truth_table(seqs, k, canonical=False):
    """A KmerTable whose codes come from the numpy definition, not from the package."""
    from pyfastx_amd import kmer
    codes, counts = table_truth(seqs, k, canonical)
    return kmer.KmerTable(k, canonical, codes, counts)


def table_of(codes, k, canonical=False):
    from pyfastx_amd import kmer
    codes = np.unique(np.asarray(codes, dtype=np.int64))
    return kmer.KmerTable(k, canonical, codes, np.ones(codes.size, dtype=np.int64))


def same_hits(got, want, dtype):
    nw, nh = got
    assert nw.dtype == dtype and nh.dtype == dtype and nw.shape == nh.shape == want[0].shape
    return np.array_equal(nw, want[0]) and np.array_equal(nh, want[1])


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


# ------------------------------------------------------------------ 1: set membership
def _distinct(rng, n, k):
    """n distinct codes of [0, 4^k), and as many that are not among them (at k = 1 there are four codes: two and two)."""
    if k == 1:
        p = rng.permutation(4).astype(np.int64)
        m = min(n, 2)
        return p[:m], p[2:2 + m]
    c = np.unique(rng.integers(0, 4 ** k, 2 * n + 64, dtype=np.int64))
    assert c.size >= 2 * n
    c = rng.permutation(c)
    return c[:n], c[n:2 * n]


def _membership(blob, rng, n, k):
    from pyfastx_amd import _lib
    present, absent = _distinct(rng, n, k)
    given = present if k > 1 or n <= 2 else np.concatenate([present, rng.choice(present, n - 2)])     # k = 1: n codes of the two, repeated
    s = _lib.KmerSet(blob, k, False, given)
    near = [present ^ (np.int64(1) << b) for b in (0, 31, 32, 2 * k - 1) if b < 2 * k]
    q = np.concatenate([present, absent] + near)
    want = np.isin(q, present).astype(np.uint8)
    got = s.contains(q)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (n, k)
    assert present.size == 0 or (got[:present.size] == 1).all()
    assert (got[present.size:present.size + absent.size] == 0).all()
    twice = _lib.KmerSet(blob, k, False, rng.permutation(np.repeat(given, 2)))
    assert np.array_equal(twice.contains(q), want), (n, k)
    s.close()
    twice.close()


@pytest.mark.parametrize("k", [1, 16, 31])
def test_set_membership(fx, blob, k):
    from pyfastx_amd import kmer
    rng = np.random.default_rng(100 + k)
    for n in (0, 1, 2, 31, 32, 33, kmer.SCREEN_LDS_KEYS, kmer.SCREEN_LDS_KEYS + 1, 100_000):
        _membership(blob, rng, n, k)


@pytest.mark.parametrize("k", [16, 31])
def test_set_chains_wrap_at_load_half(fx, blob, k):
    """32 codes in the smallest table (64 slots), 200 seeds: chains that begin near the end wrap to slot 0."""
    for seed in range(200):
        _membership(blob, np.random.default_rng(seed), 32, k)


def test_set_rejects_bad_codes(fx, blob):
    from pyfastx_amd import _lib
    ok = np.arange(0, 5000, dtype=np.int64)
    for k, canonical, bad in ((3, True, 63), (3, False, 64), (3, False, -1), (31, False, 4 ** 31), (31, True, 4 ** 31 - 1), (16, True, 4 ** 16 - 1)):
        codes = ok[:20].copy() if k == 3 else ok.copy()
        if canonical:
            codes = np.unique(np.minimum(codes, revcomp_code(codes, k)))
        _lib.KmerSet(blob, k, canonical, codes).close()                       # the rest is fine
        codes[codes.size // 2] = bad
        with pytest.raises(_lib.FxError) as e:
            _lib.KmerSet(blob, k, canonical, codes)
        assert e.value.code == _lib.FX_EINVAL, (k, canonical, bad)
    for k in (0, 32):
        with pytest.raises(_lib.FxError) as e:
            _lib.KmerSet(blob, k, False, ok)
        assert e.value.code == _lib.FX_EINVAL
    s = C.c_void_p()
    assert _lib.lib().fx_kmer_set_create(blob._h, 21, 2, None, 0, C.byref(s)) == _lib.FX_EINVAL and not s.value
    e = _lib.KmerSet(blob, 21, True, np.zeros(0, dtype=np.int64))              # a valid empty set
    assert e.contains([0, 1, 2]).tolist() == [0, 0, 0]
    e.close()
    with pytest.raises(_lib.FxError):
        e.contains([0])


# ------------------------------------------------------------------ 2: the fixture files
@pytest.fixture(scope="module")
def fixture_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ks")
    out = {}
    for fn in ("test.fa", "test.fq", "test.fq.gz"):
        shutil.copy(os.path.join(DATA, fn), d / fn)
        out[fn] = str(d / fn)
    return out


def test_fixtures(fx, fixture_files):
    fa = fx.Fasta(fixture_files["test.fa"])
    recs = [fa[i].seq for i in range(len(fa))]
    fq = fx.Fastq(fixture_files["test.fq"])
    gz = fx.Fastq(fixture_files["test.fq.gz"])
    reads = [fq[i].seq for i in range(len(fq))]
    for canonical in (False, True):
        t = fa.kmer_table(21, canonical=canonical)
        assert len(t) > 4096
        want = hits_truth(reads, 21, t.codes, canonical)
        assert same_hits(fq.kmer_hits(t), want, np.int32), canonical
        assert same_hits(gz.kmer_hits(t), want, np.int32), canonical
        nw, nh = fa.kmer_hits(t)
        assert same_hits((nw, nh), hits_truth(recs, 21, t.codes, canonical), np.int64)
        assert np.array_equal(nw, nh) and nw.sum() == t.n_windows
        # against a table of their own windows, reads hit with every one
        own = truth_table(reads[:50], 21, canonical)
        nw, nh = fq.kmer_hits(own, ids=list(range(50)))
        assert np.array_equal(nw, nh) and nw.sum() > 0
        t.release()
        assert not t._sets


# ------------------------------------------------------------------ 3: lengths around k and around pieces
LENS = (15, 16, 17, 30, 31, 32, 33, 47, 48, 49, 400, 1025, 2100)


@pytest.fixture(scope="module")
def length_reads(fx, tmp_path_factory):
    rng = np.random.default_rng(3)
    pool = _rand(rng, 2600)                                    # the reads are slices of one pool: they share k-mers
    reads = []
    for n in LENS:
        a = int(rng.integers(0, len(pool) - n + 1))
        reads.append(pool[a:a + n])
    fq = fx.Fastq(_write(tmp_path_factory.mktemp("len") / "l.fq", _fastq(reads)))
    assert len(fq) == len(LENS)
    half = sorted(rng.permutation(len(LENS))[:len(LENS) // 2].tolist())
    return fq, reads, [reads[i] for i in half]


@pytest.mark.parametrize("k", [16, 17, 31])
def test_lengths_around_k(fx, length_reads, k):
    fq, reads, source = length_reads
    for canonical in (False, True):
        t = truth_table(source, k, canonical)
        want = hits_truth(reads, k, t.codes, canonical)
        assert want[0].tolist() == [max(n - k + 1, 0) for n in LENS] and 0 < want[1].sum() < want[0].sum()
        assert same_hits(fq.kmer_hits(t), want, np.int32), (k, canonical)
        # intervals shorter than k, equal to k, the whole read, and ones that begin inside a 16-byte piece
        ids = [10, 10, 10, 10, 7, 5, 12, 11]
        start = [5, 100, 0, 37, 16, 1, 1033, 1]
        end = [35, 131, 400, 390, 47, 32, 2099, 1025]
        cut = [reads[i][a:b] for i, a, b in zip(ids, start, end)]
        assert same_hits(fq.kmer_hits(t, ids=ids, start=start, end=end), hits_truth(cut, k, t.codes, canonical), np.int32), (k, canonical)


# ------------------------------------------------------------------ 4: invalid bytes
def test_invalid_bytes(fx, tmp_path):
    rng = np.random.default_rng(4)
    src = _rand(rng, 3000)
    odd = "NRYKMSWBDHVnacgt\x80\xff-*"
    seqs = []
    for j in range(40):
        s = list(src[j * 50:j * 50 + 600])
        for p in rng.integers(0, len(s), 12):
            s[p] = odd[int(rng.integers(0, len(odd)))]
        seqs.append("".join(s))
    seqs += [src[:300].lower(), "N" * 100, src[100:160] + "N" + src[161:230]]
    fq = fx.Fastq(_write(tmp_path / "n.fq", _fastq(seqs)))
    fa = fx.Fasta(_write(tmp_path / "n.fa", _fasta(seqs, 70)))
    assert len(fq) == len(fa) == len(seqs)
    for k in (14, 31):
        for canonical in (False, True):
            t = truth_table([src], k, canonical)
            want = hits_truth(seqs, k, t.codes, canonical)
            clean = np.array([max(len(s) - k + 1, 0) for s in seqs])
            assert (want[0][:40] < clean[:40]).all() and want[0][-2] == 0 and want[1][-3] == want[0][-3] == 300 - k + 1
            assert same_hits(fq.kmer_hits(t), want, np.int32), (k, canonical)
            assert same_hits(fa.kmer_hits(t), want, np.int64), (k, canonical)


# ------------------------------------------------------------------ 5: strands
def test_strands(fx, tmp_path):
    rng = np.random.default_rng(5)
    src = _rand(rng, 900)
    reads = [src[a:a + 120] for a in range(0, 700, 90)] + [_rc(src[a:a + 120]) for a in range(10, 700, 90)] + [_rand(rng, 120)]
    fq = fx.Fastq(_write(tmp_path / "s.fq", _fastq(reads)))
    fa = fx.Fasta(_write(tmp_path / "s.fa", _fasta(reads)))
    for k in (21, 31):
        canon = truth_table([src], k, True)
        nw, nh = fq.kmer_hits(canon)
        assert same_hits((nw, nh), hits_truth(reads, k, canon.codes, True), np.int32)
        assert np.array_equal(nw[:-1], nh[:-1]) and nh[-1] == 0 and (nw == 120 - k + 1).all()
        plain = truth_table([src], k, False)
        want = hits_truth(reads, k, plain.codes, False)
        assert (want[1][:8] == want[0][:8]).all() and want[1][8:].sum() == 0
        assert same_hits(fq.kmer_hits(plain), want, np.int32) and same_hits(fa.kmer_hits(plain), want, np.int64)
        assert same_hits(fa.kmer_hits(canon), hits_truth(reads, k, canon.codes, True), np.int64)


# ------------------------------------------------------------------ 6: the table in LDS and in global memory
def test_both_table_forms(fx, tmp_path):
    from pyfastx_amd import kmer
    rng = np.random.default_rng(6)
    k, n = 21, 20_000
    src = _rand(rng, 6000)
    lens = rng.integers(100, 152, n).tolist()
    noise = _rand(rng, 152 * n // 2)
    at = rng.integers(0, len(src) - 151, n).tolist()
    reads = [noise[152 * (i // 2):152 * (i // 2) + m] if i % 2 else src[a:a + m] for i, (m, a) in enumerate(zip(lens, at))]      # every other read is cut from the source
    fq = fx.Fastq(_write(tmp_path / "f.fq", _fastq(reads)))
    assert len(fq) == n
    starts = np.concatenate(([0], np.cumsum(lens)))
    per = np.split(flat_codes("".join(reads), starts[:-1], k), np.cumsum(np.asarray(lens) - k + 1)[:-1])        # the codes of every read
    assert len(per) == n and np.array_equal(per[7], counted_codes(reads[7], k)) and np.array_equal(per[-1], counted_codes(reads[-1], k))
    codes = table_truth([src], k)[0]
    small = rng.permutation(codes)[:kmer.SCREEN_LDS_KEYS]
    assert small.size == kmer.SCREEN_LDS_KEYS
    extra = np.int64(0)                                        # poly-A: in no read
    assert not np.isin(np.concatenate(per), [extra]).any() and extra not in small
    want = hits_of_codes(per, small)
    assert 0 < want[1].sum() < want[0].sum()
    in_lds = fq.kmer_hits(table_of(small, k))
    in_global = fq.kmer_hits(table_of(np.append(small, extra), k))
    assert same_hits(in_lds, want, np.int32) and same_hits(in_global, want, np.int32)
    assert np.array_equal(in_lds[0], in_global[0]) and np.array_equal(in_lds[1], in_global[1])
    # a set of 1000 codes: a smaller image in LDS
    few = small[:1000]
    assert same_hits(fq.kmer_hits(table_of(few, k)), hits_of_codes(per, few), np.int32)
    keep = fq.screen(table_of(small, k), min_hits=3)
    assert np.array_equal(keep, screen_truth(want[0], want[1], 3)) and 0 < keep.size < n


# ------------------------------------------------------------------ 7: empty cases
def test_empty_cases(fx, tmp_path):
    rng = np.random.default_rng(7)
    reads = [_rand(rng, 80), "", _rand(rng, 40)]
    fq = fx.Fastq(_write(tmp_path / "e.fq", _fastq(reads)))
    fa = fx.Fasta(_write(tmp_path / "e.fa", _fasta([reads[0], reads[2]])))
    assert len(fq) == 3
    k = 21
    t = truth_table(reads, k)
    assert same_hits(fq.kmer_hits(t), (np.array([60, 0, 20]), np.array([60, 0, 20])), np.int32)
    empty = table_of([], k)
    assert same_hits(fq.kmer_hits(empty), (np.array([60, 0, 20]), np.zeros(3, dtype=np.int64)), np.int32)
    assert same_hits(fa.kmer_hits(empty), (np.array([60, 20]), np.zeros(2, dtype=np.int64)), np.int64)
    assert fq.screen(empty).size == 0 and fq.screen(empty, invert=True).tolist() == [0, 1, 2]
    for obj, dt in ((fq, np.int32), (fa, np.int64)):
        nw, nh = obj.kmer_hits(t, ids=[])
        assert nw.shape == nh.shape == (0,) and nw.dtype == nh.dtype == dt
    p = fq.screen(t, ids=[])
    assert p.shape == (0,) and p.dtype == np.int64
    one = fx.Fastq(_write(tmp_path / "one.fq", _fastq([reads[0]])))
    assert same_hits(one.kmer_hits(t), (np.array([60]), np.array([60])), np.int32) and one.screen(t).tolist() == [0]
    assert same_hits(one.kmer_hits(truth_table([reads[2]], k)), (np.array([60]), np.array([0])), np.int32)


# ------------------------------------------------------------------ 8: ids
def test_ids_rules(fx, fixture_files):
    from pyfastx_amd import _lib
    fq = fx.Fastq(fixture_files["test.fq"])
    fa = fx.Fasta(fixture_files["test.fa"])
    reads = [fq[i].seq for i in range(len(fq))]
    t = truth_table(reads[::3], 25, True)
    ids = [700, 3, 3, 0, 799, 3, 6]
    assert same_hits(fq.kmer_hits(t, ids=ids), hits_truth([reads[i] for i in ids], 25, t.codes, True), np.int32)
    recs = [fa[i].seq for i in (5, 0, 5, 210)]
    ft = truth_table(recs[:2], 25)
    want = hits_truth(recs, 25, ft.codes)
    assert same_hits(fa.kmer_hits(ft, ids=[5, 0, 5, 210]), want, np.int64) and want[0][0] == want[0][2] == want[1][2]
    names = list(fa.keys())
    assert same_hits(fa.kmer_hits(ft, ids=[names[5], names[0], names[5], names[210]]), want, np.int64)
    for call in (lambda: fq.kmer_hits(t, ids=[0, len(fq)]), lambda: fq.screen(t, ids=[0, -1]), lambda: fa.kmer_hits(ft, ids=[0, len(fa)])):
        with pytest.raises(IndexError):
            call()
    for call in (lambda: fq.kmer_hits(t, ids=[1, 2, 3], start=[0, 0, 0], end=[150, 151, 4]),
                 lambda: fq.screen(t, ids=[1, 2, 3], start=[0, 0, 0], end=[150, 151, 4])):
        with pytest.raises(ValueError, match="query 1"):
            call()
    for call in (lambda: fq.kmer_hits(t.codes), lambda: fq.screen(None), lambda: fa.kmer_hits([1, 2])):
        with pytest.raises(TypeError):
            call()
    for kw in (dict(min_hits=-1), dict(min_hits=True), dict(min_hits=1.0), dict(min_frac=1.5), dict(min_frac=-0.5)):
        with pytest.raises(ValueError):
            fq.screen(t, **kw)
    b = fq._qc_blob()
    s = b.kmer_set(25, True, t.codes)
    with pytest.raises(_lib.FxError) as e:
        b.fastq_kmer_hits(s, ids=[0, 1, 900])
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    with pytest.raises(_lib.FxError) as e:
        b.fastq_kmer_screen(s, ids=[1, 2, 3], start=[0, 0, -1], end=[150, 150, 4])
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    for kw in (dict(min_hits=-1), dict(frac=(1, 10 ** 9 + 1)), dict(frac=(-1, 2))):
        with pytest.raises(_lib.FxError) as e:
            b.fastq_kmer_screen(s, **kw)
        assert e.value.code == _lib.FX_EINVAL
    s.close()


def test_states_and_sharded(fx, fixture_files, blob, monkeypatch):
    from pyfastx_amd import _lib
    s = blob.kmer_set(21, False, np.arange(10, dtype=np.int64))
    rawq = open(os.path.join(DATA, "test.fq"), "rb").read()
    q = _lib.Blob.from_bytes(rawq, device=0)
    with pytest.raises(_lib.FxError) as e:
        q.fastq_kmer_hits(s)
    assert e.value.code == _lib.FX_ESTATE
    q.fastq_build()
    nw, nh = q.fastq_kmer_hits(s)                              # a set made through another handle of the device
    assert nw.shape == (800,) and nh.sum() == 0
    off = [i for i, c in enumerate(rawq[:4096]) if c == 10][3] + 1
    sh = _lib.Blob.from_bytes(rawq[off:], device=0)
    sh.set_shard(off, 10, True)
    assert sh.fastq_build().n_reads > 0
    for call in (lambda: sh.fastq_kmer_hits(s), lambda: sh.fastq_kmer_screen(s)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    a = _lib.Blob.from_bytes(open(os.path.join(DATA, "test.fa"), "rb").read(), device=0)
    with pytest.raises(_lib.FxError) as e:
        a.fasta_kmer_hits(s)
    assert e.value.code == _lib.FX_ESTATE
    s.close()
    fa = fx.Fasta(fixture_files["test.fa"])
    fq = fx.Fastq(fixture_files["test.fq"])
    t = table_of([1, 2, 3], 21)
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    monkeypatch.setattr(type(fq), "_sharded", property(lambda self: True))
    for call in (lambda: fa.kmer_hits(t), lambda: fq.kmer_hits(t), lambda: fq.screen(t)):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------ 9: the screen
def test_screen(fx, tmp_path):
    from pyfastx_amd import qc
    rng = np.random.default_rng(9)
    k = 16
    src = _rand(rng, 400)
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]        # a letter that does not continue the source
    reads = [src[0:17] + 2 * other(src[17]), src[0:16] + other(src[16]) + "AT", src[50:60], src[100:180], _rand(rng, 90), src[200:230] + _rand(rng, 30),
             _rc(src[300:380]), src[20:36]]
    reads += [src[a:a + 40] + _rand(rng, int(rng.integers(0, 60))) for a in rng.integers(0, 360, 40).tolist()]
    fq = fx.Fastq(_write(tmp_path / "s.fq", _fastq(reads)))
    t = truth_table([src], k)
    nw, nh = hits_truth(reads, k, t.codes)
    assert (nw[0], nh[0]) == (4, 2) and (nw[1], nh[1]) == (4, 1) and nw[2] == 0 and (nw[7], nh[7]) == (1, 1)
    assert same_hits(fq.kmer_hits(t), (nw, nh), np.int32)
    for min_hits in (0, 1, 5):
        for frac in (None, 0.5, 0.25, 1, 0, 1 / 3, 0.999):
            num, den = (0, 0) if frac is None else qc.as_ratio(frac)
            for invert in (False, True):
                got = fq.screen(t, min_hits=min_hits, min_frac=frac, invert=invert)
                assert got.dtype == np.int64 and np.array_equal(got, screen_truth(nw, nh, min_hits, num, den, invert)), (min_hits, frac, invert)
    half = fq.screen(t, min_hits=0, min_frac=0.5).tolist()
    assert 0 in half and 1 not in half and 2 in half           # 2 of 4 is a half, 1 of 4 is not, no windows pass the ratio
    assert 2 not in fq.screen(t, min_hits=1, min_frac=0.5).tolist()
    # with what trim returned: positions among the queries
    ids = np.array(list(range(len(reads) - 1, -1, -2)), dtype=np.int64)
    iv = fq.trim(ids=ids, clip_front=3, clip_tail=2)
    cut = [reads[int(i)][int(a):int(b)] for i, a, b in zip(ids, iv["start"], iv["end"])]
    cw, ch = hits_truth(cut, k, t.codes)
    assert same_hits(fq.kmer_hits(t, ids=ids, start=iv["start"], end=iv["end"]), (cw, ch), np.int32)
    pos = fq.screen(t, min_hits=2, min_frac=0.4, ids=ids, start=iv["start"], end=iv["end"])
    assert np.array_equal(pos, screen_truth(cw, ch, 2, 2, 5)) and 0 < pos.size < ids.size
    # the positions of a whole-file screen are read ids: write takes them
    keep = fq.screen(t, min_hits=5, invert=True)
    assert np.array_equal(keep, screen_truth(nw, nh, 5, invert=True)) and 0 < keep.size < len(reads)
    out = tmp_path / "kept.fq"
    info = fq.write(str(out), ids=keep)
    assert info["reads"] == keep.size
    assert open(out, "rb").read() == "".join("@q%d\n%s\n+\n%s\n" % (i, reads[i], "I" * len(reads[i])) for i in keep.tolist()).encode()
    sel = ids[pos]
    info = fq.write(str(out), ids=sel, start=np.asarray(iv["start"])[pos], end=np.asarray(iv["end"])[pos])
    assert info["reads"] == pos.size
    assert open(out, "rb").read() == "".join("@q%d\n%s\n+\n%s\n" % (int(i), cut[int(p)], "I" * len(cut[int(p)])) for i, p in zip(sel, pos)).encode()


# ------------------------------------------------------------------ 10: FASTA layouts
@pytest.mark.parametrize("width", [0, 61, 255, 256, 17, 7])
def test_fasta_layouts(fx, tmp_path, width):
    rng = np.random.default_rng(1000 + width)
    pool = _rand(rng, 3200)
    seqs = []
    for n in (1, 30, 31, 3000, 30, 1, 31, 700):
        a = int(rng.integers(0, len(pool) - n + 1))
        seqs.append(pool[a:a + n])
    fa = fx.Fasta(_write(tmp_path / "w.fa", _fasta(seqs, width)))
    assert [fa[i].seq for i in range(len(fa))] == seqs
    for k in (14, 17, 31):
        for canonical in (False, True):
            t = truth_table([seqs[7], seqs[2], seqs[1]], k, canonical)
            want = hits_truth(seqs, k, t.codes, canonical)
            assert 0 < want[1][3] < want[0][3] and want[1][7] == want[0][7]
            assert same_hits(fa.kmer_hits(t), want, np.int64), (k, canonical)
            ids = [3, 0, 3, 7, 6]
            assert same_hits(fa.kmer_hits(t, ids=ids), (want[0][ids], want[1][ids]), np.int64), (k, canonical)


def test_fasta_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: slen is smaller than the number of kept
    bytes and `seq` stops there -- no window behind that cut counts or hits, though the set holds its code."""
    rng = np.random.default_rng(55)
    recs, kept, whole = [], [], []
    for i, n_lines in enumerate((3, 12, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        whole.append("".join(lines))
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert any(len(s) < n for s, n in zip(seqs, kept)), "no record is cut: the case is not exercised"
    assert all(w.startswith(s) for w, s in zip(whole, seqs))
    for k in (14, 31):
        t = truth_table(whole, k)                              # the codes behind the cuts are in the set
        want = hits_truth(seqs, k, t.codes)
        assert np.array_equal(want[0], want[1])
        assert same_hits(fa.kmer_hits(t), want, np.int64), k
        assert same_hits(fa.kmer_hits(t, ids=[4, 1, 4]), (want[0][[4, 1, 4]], want[1][[4, 1, 4]]), np.int64)
