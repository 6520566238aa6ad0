"""-m gpu: FastqPair.overlap / trim / merge / write / write_merged (fx_fastq_pair_overlap, fx_fastq_pair_merge_alloc,
csrc/fx_fastq_pair.hpp) against the plain-Python definition tests/pair_truth.py over fq[i].seq / fq[i].qual of the same files --
every comparison exact -- on a sweep of every diagonal, on overlaps planted across the 16-byte pieces, on random pairs, on reads
that fill and that exceed a lane group, and synth.fastq_pair_generate against its own ground truth."""
import numpy as np
import pytest

from pair_truth import NONE, insert_of, merged_truth, overlap_truth, revcomp

pytestmark = pytest.mark.gpu

COLS = ("diag", "overlap", "mismatches", "end1", "end2", "insert")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _lat(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def letters(rng, n):
    return bytes(ACGT[rng.integers(0, 4, n)])


def mates(rng, F, L1, L2):
    """The mates of a random fragment of F letters: its first L1, the first L2 of its reverse complement; random letters (the
    adapter) fill what the fragment does not."""
    frag = letters(rng, F)
    return (frag + letters(rng, L1))[:L1], (revcomp(frag) + letters(rng, L2))[:L2]


def plant(s, pos, c=None):
    b = bytearray(s)
    b[pos] = c if c is not None else b"CATG"[b"ACGT".index(b[pos])]
    return bytes(b)


def substitute(rng, s, rate):
    b = bytearray(s)
    for p in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[p] = b"CATG"[b"ACGT".index(b[p])] if rng.random() < 0.5 else b"GTAC"[b"ACGT".index(b[p])]
    return bytes(b)


# ------------------------------------------------------------------ the pairs of every file
def sweep_pairs(rng):
    """One pair per fragment length, so that every diagonal of every shape is the answer once."""
    out = []
    for L1, L2 in ((40, 40), (33, 47), (16, 16), (17, 15), (1, 1), (0, 20)):
        for F in range(1, max(L1 + L2, 2)):
            out.append(mates(rng, F, L1, L2))
    return out


PIECE_LENGTHS = (15, 16, 17, 31, 32, 33, 150, 151, 250)
PIECE_KW = dict(min_overlap=8, max_diff=2, max_error_rate=0.2)


def piece_pairs(rng):
    """Every combination of the lengths, with the overlap beginning / ending next to a piece boundary (bytes 15 | 16 and 31 | 32)
    of either mate, and mismatches, N and lower case planted at the first, the last and a middle letter of it."""
    out = []
    v = 0
    for L1 in PIECE_LENGTHS:
        for L2 in PIECE_LENGTHS:
            for d in (15, 16, 31, 32, L1 - 16, L1 - 17, -15, -16, -(L2 - 16), -(L2 - 17), 0):
                if not -(L2 - 1) <= d <= L1 - 1:
                    continue
                lo, hi = max(0, d), min(L1, d + L2)
                if hi - lo < 8:
                    continue
                s1, s2 = mates(rng, d + L2, L1, L2)
                spots = [lo, hi - 1, (lo + hi) // 2]
                kind = v % 7
                v += 1
                if kind in (1, 2):                            # max_diff, max_diff + 1 mismatches in read 1
                    for p in spots[:kind + 1]:
                        s1 = plant(s1, p)
                elif kind in (3, 4):                          # the same in read 2
                    for p in spots[:kind - 1]:
                        s2 = plant(s2, L2 - 1 - (p - d))
                elif kind == 5:                               # N in one mate, lower case in the other
                    s1 = plant(s1, spots[0], ord("N"))
                    s2 = plant(s2, L2 - 1 - (spots[1] - d), s2[L2 - 1 - (spots[1] - d)] | 0x20)
                elif kind == 6:
                    s1 = plant(s1, spots[1], s1[spots[1]] | 0x20)
                    s2 = plant(s2, L2 - 1 - (spots[0] - d), ord("N"))
                out.append((s1, s2))
    # read 2 inside read 1: the overlap is exactly bytes [15 or 16, 31 .. 33] of read 1
    for L1 in (33, 150, 250):
        for L2 in (15, 16, 17, 18):
            for d in (15, 16):
                if d + L2 > L1:
                    continue
                s1 = letters(rng, L1)
                out.append((s1, revcomp(s1[d:d + L2])))
                out.append((plant(plant(s1, d), d + L2 - 1), revcomp(s1[d:d + L2])))
                out.append((plant(plant(plant(s1, d), d + L2 - 1), d + 7), revcomp(s1[d:d + L2])))
    return out


def random_pairs(rng, n=2000, rlen=150, rate=0.01):
    """-> (pairs, true inserts): inserts uniform on 20..400, one pair in twelve of exactly the read length (d = 0)."""
    out, ins = [], []
    for _ in range(n):
        F = rlen if rng.random() < 1 / 12 else int(rng.integers(20, 401))
        s1, s2 = mates(rng, F, rlen, rlen)
        out.append((substitute(rng, s1, rate), substitute(rng, s2, rate)))
        ins.append(F)
    return out, np.array(ins, dtype=np.int64)


def long_pairs(rng, L):
    return [mates(rng, F, L, L) for F in (L + L // 2, L, L - L // 3)]


SEEDS = {"sweep": 1, "pieces": 2, "random": 3, "long1024": 4, "long1100": 5}


def make_pairs(name, rng):
    """-> (pairs, the true inserts or None)"""
    if name == "random":
        return random_pairs(rng)
    return {"sweep": sweep_pairs, "pieces": piece_pairs, "long1024": lambda r: long_pairs(r, 1024), "long1100": lambda r: long_pairs(r, 1100)}[name](rng), None


class Corpus:
    """A pair of files written from (s1, s2) pairs, the FastqPair over them, and the rows the truth reads: what fq[i].seq /
    .qual / .description show.  The truth of an argument set is computed once and shared."""

    def __init__(self, fx, tmp, name, pairs, rng):
        self.n = len(pairs)
        p1, p2 = str(tmp / (name + "_R1.fq")), str(tmp / (name + "_R2.fq"))
        for path, k in ((p1, 0), (p2, 1)):
            with open(path, "wb") as f:
                for i, pr in enumerate(pairs):
                    q = bytes(rng.integers(33, 74, len(pr[k]), dtype=np.uint8))
                    f.write(b"@%s%d/%d len=%d\n%s\n+\n%s\n" % (name.encode(), i, k + 1, len(pr[k]), pr[k], q))
        self.fq1, self.fq2 = fx.Fastq(p1), fx.Fastq(p2)
        self.pair = fx.FastqPair(self.fq1, self.fq2)
        assert len(self.pair) == self.n
        self.rows = []
        for i in range(self.n):
            a, b = self.fq1[i], self.fq2[i]
            self.rows.append((_lat(a.seq), _lat(a.qual), _lat(b.seq), _lat(b.qual), _lat(a.description)))
            assert self.rows[-1][0] == pairs[i][0] and self.rows[-1][2] == pairs[i][1]
        self._truth = {}

    def truth(self, **kw):
        from pyfastx_amd import pair
        args = pair.overlap_args(**kw)
        key = (args["min_overlap"], args["max_diff"], args["err"])
        if key not in self._truth:
            rows = [overlap_truth(r[0], r[2], **args) for r in self.rows]
            self._truth[key] = {c: np.array([r[c] for r in rows], dtype=np.int64) for c in COLS}
        return self._truth[key]

    def check_overlap(self, ids=None, **kw):
        got = self.pair.overlap(ids=ids, **kw)
        want = self.truth(**kw)
        assert sorted(got) == sorted(COLS)
        assert got["diag"].dtype == got["overlap"].dtype == got["mismatches"].dtype == np.int32
        assert got["end1"].dtype == got["end2"].dtype == got["insert"].dtype == np.int64
        sel = slice(None) if ids is None else ids
        for c in COLS:
            w = want[c][sel]
            assert got[c].shape == w.shape, (c, kw)
            bad = np.nonzero(got[c] != w)[0]
            assert bad.size == 0, (c, kw, int(bad[0]), int(got[c][bad[0]]), int(w[bad[0]]), len(self.rows[int(np.arange(self.n)[sel][bad[0]])][0]))
        return want

    def merged(self, i, d, min_len=0):
        r = self.rows[int(i)]
        return merged_truth(r[4], r[0], r[1], r[2], r[3], int(d), min_len)

    def check_merge(self, diag, ids=None, min_len=0):
        buf, offs = self.pair.merge(ids=ids, diag=diag, min_len=min_len)
        sel = np.arange(self.n) if ids is None else ids
        parts = [self.merged(i, d, min_len) for i, d in zip(sel, diag)]
        assert buf.dtype == np.uint8 and offs.dtype == np.int64 and len(offs) == len(sel) + 1 and offs[0] == 0
        assert np.array_equal(np.diff(offs), [len(x) for x in parts])
        for k, x in enumerate(parts):
            assert buf[offs[k]:offs[k + 1]].tobytes() == x, (k, int(sel[k]), int(diag[k]))
        return parts


@pytest.fixture(scope="module")
def corpora(fx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pairs")
    made = {}

    def get(name):
        if name not in made:
            rng = np.random.default_rng([20261018, SEEDS[name]])      # a stream of its own: a file does not depend on which tests ran before
            pairs, ins = make_pairs(name, rng)
            made[name] = Corpus(fx, tmp, name, pairs, rng)
            made[name].inserts = ins
        return made[name]
    return get


# ------------------------------------------------------------------ overlap
@pytest.mark.parametrize("min_overlap", [1, 8, 30])
def test_diagonal_sweep(corpora, min_overlap):
    c = corpora("sweep")
    assert c.n == 79 + 79 + 31 + 31 + 1 + 19
    strict = c.check_overlap(min_overlap=min_overlap, max_diff=0, max_error_rate=0)
    if min_overlap == 8:                                     # every diagonal of the (40, 40) pairs with 8 letters or more is its pair's answer
        assert strict["diag"][7:72].tolist() == list(range(-32, 33)) and (strict["insert"][7:72] == np.arange(8, 73)).all()
    assert (strict["diag"][-19:] == NONE).all()               # an empty read 1 overlaps nothing
    c.check_overlap(min_overlap=min_overlap)
    c.check_overlap(min_overlap=min_overlap, max_diff=3, max_error_rate="1/3")


def test_piece_boundaries(corpora):
    c = corpora("pieces")
    want = c.check_overlap(**PIECE_KW)
    # by the truth: both outcomes occur, and overlaps that begin and end on either side of a piece boundary are found
    found = want["diag"] != NONE
    assert found.sum() > 300 and (~found).sum() > 50
    L1 = np.array([len(r[0]) for r in c.rows])
    lo, hi = np.maximum(want["diag"], 0)[found], np.maximum(want["diag"], 0)[found] + want["overlap"][found]
    assert {15, 16, 31, 32} <= set(lo.tolist()) and {16, 17, 32, 33} <= set(hi.tolist())
    assert {0, 2} <= set(want["mismatches"][found].tolist()) and int(L1.max()) == 250
    c.check_overlap()
    c.check_overlap(min_overlap=15, max_diff=3, max_error_rate=0.1)


def test_random_pairs(corpora):
    c = corpora("random")
    want = c.truth()
    d = want["diag"]
    # by the truth, before any comparison: every class has its members, and the truth recovers the inserts it can
    classes = {"fwd": int(((d > 0) & (d != NONE)).sum()), "zero": int((d == 0).sum()), "back": int(((d < 0) & (d != NONE)).sum()), "none": int((d == NONE).sum())}
    assert min(classes.values()) >= 100, classes
    inside = (c.inserts >= 30) & (c.inserts <= 270)
    hit = int((want["insert"][inside] == c.inserts[inside]).sum())
    assert hit >= 0.95 * int(inside.sum()), (hit, int(inside.sum()))
    c.check_overlap()
    c.check_overlap(ids=np.arange(0, c.n, 7), min_overlap=12, max_diff=8, max_error_rate=0.15)
    h = c.pair.insert_histogram(want["insert"])
    assert h.sum() == int((d != NONE).sum()) and h[150] >= 100


@pytest.mark.parametrize("name,L", [("long1024", 1024), ("long1100", 1100)])
def test_long_reads(corpora, name, L):
    c = corpora(name)                                         # 1024: a lane group of 64 lanes; 1100: one lane walks the pair
    assert c.n == 3 and c.fq1.maxlen == L
    want = c.check_overlap()
    assert want["insert"].tolist() == [L + L // 2, L, L - L // 3]
    c.check_overlap(min_overlap=600)
    c.check_merge(want["diag"].astype(np.int32))


def test_gathered_ids(corpora):
    c = corpora("sweep")
    rng = np.random.default_rng(3)
    ids = rng.integers(0, c.n, 3 * c.n + 5)
    c.check_overlap(ids=ids, min_overlap=8)
    c.check_overlap(ids=ids[:1], min_overlap=8)
    empty = c.pair.overlap(ids=np.zeros(0, dtype=np.int64))
    assert all(empty[k].size == 0 for k in COLS)
    for bad in ([0, c.n], [-1], [2**40]):
        with pytest.raises(IndexError):
            c.pair.overlap(ids=bad)
        with pytest.raises(IndexError):
            c.pair.merge(ids=bad, diag=np.zeros(len(bad), dtype=np.int32))


def test_id_outside_the_table_at_the_abi(corpora):
    """Below the Python checks: FX_ERANGE with *first_bad, nothing allocated."""
    from pyfastx_amd import _lib
    c = corpora("sweep")
    b1, b2, n = c.pair._blobs()
    for call in (lambda ids: b1.fastq_pair_overlap(b2, ids), lambda ids: b1.fastq_pair_merge_alloc(b2, np.zeros(3, dtype=np.int32), ids)):
        with pytest.raises(_lib.FxError) as e:
            call(np.array([0, 1, n], dtype=np.int64))
        assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    for kw in (dict(min_overlap=0), dict(max_diff=-1), dict(err=(1, 0)), dict(err=(-1, 5)), dict(err=(10**9 + 1, 1))):
        with pytest.raises(_lib.FxError) as e:
            b1.fastq_pair_overlap(b2, None, **kw)
        assert e.value.code == _lib.FX_EINVAL


# ------------------------------------------------------------------ merge
@pytest.mark.parametrize("name", ["sweep", "pieces", "random"])
def test_merge(corpora, name):
    c = corpora(name)
    kw = PIECE_KW if name == "pieces" else dict(min_overlap=8) if name == "sweep" else {}
    want = c.truth(**kw)
    diag = want["diag"].astype(np.int32)
    parts = c.check_merge(diag)
    assert sum(1 for x in parts if x) == int((diag != NONE).sum()) > 0
    # min_len drops records
    med = int(np.median(want["insert"][diag != NONE]))
    parts = c.check_merge(diag, min_len=med + 1)
    assert 0 < sum(1 for x in parts if x) < int((diag != NONE).sum())
    # any diagonal of the pair's range merges by the same rule, whether its letters agree or not: every geometry, the tie rule
    rng = np.random.default_rng(8)
    ids = rng.integers(0, c.n, min(c.n, 400))
    L1, L2 = np.array([len(c.rows[i][0]) for i in ids]), np.array([len(c.rows[i][2]) for i in ids])
    ok = L1 + L2 - 1 > 0
    ids, L1, L2 = ids[ok], L1[ok], L2[ok]
    any_d = (-(L2 - 1) + (rng.random(ids.size) * (L1 + L2 - 1)).astype(np.int64)).astype(np.int32)
    assert (any_d >= -(L2 - 1)).all() and (any_d <= L1 - 1).all()
    c.check_merge(any_d, ids=ids)
    c.check_merge(np.concatenate([L1[:50] - 1, -(L2[50:100] - 1)]).astype(np.int32), ids=ids[:100])      # the two ends of the range
    if name == "random":
        buf, offs = c.pair.merge()                            # diag = None: overlap with its defaults
        got = c.pair.merge(diag=diag)
        assert buf.tobytes() == got[0].tobytes() and np.array_equal(offs, got[1])


def test_merge_refuses_a_diagonal_outside_its_pair(corpora):
    c = corpora("sweep")                                      # the first 79 pairs are (40, 40)
    diag = np.zeros(c.n, dtype=np.int32)
    diag[:] = NONE
    for k, d in ((5, 40), (5, -40), (3, 2**31 - 1), (7, NONE + 1)):
        bad = diag.copy()
        bad[k] = d
        bad[60] = 1000
        with pytest.raises(ValueError, match="query %d " % k):
            c.pair.merge(diag=bad)
    ok = diag.copy()
    ok[5], ok[6] = 39, -39
    buf, offs = c.pair.merge(diag=ok)
    assert np.diff(offs).nonzero()[0].tolist() == [5, 6]
    with pytest.raises(ValueError):
        c.pair.merge(diag=diag[:-1])
    with pytest.raises(ValueError):
        c.pair.merge(diag=diag, min_len=-1)


# ------------------------------------------------------------------ files
def test_write_and_write_merged(fx, corpora, tmp_path):
    c = corpora("random")
    want = c.truth()
    diag = want["diag"].astype(np.int32)
    out = str(tmp_path / "merged.fq")
    r = c.pair.write_merged(out, min_len=40, batch_bytes=100_000)                   # several batches
    keep = (diag != NONE) & (want["insert"] >= 40)
    assert r["merged"] == int(keep.sum()) and r["bases"] == int(want["insert"][keep].sum())
    assert np.array_equal(r["unmerged"], np.nonzero(~keep)[0]) and r["merged"] + r["unmerged"].size == c.n
    assert open(out, "rb").read() == b"".join(c.merged(i, diag[i], 40) for i in range(c.n))
    m = fx.Fastq(out)
    assert len(m) == r["merged"]
    for k, i in list(enumerate(np.nonzero(keep)[0]))[::97]:
        rec = c.merged(i, diag[i]).split(b"\n")
        assert _lat(m[k].description) == rec[0] and _lat(m[k].seq) == rec[1] and _lat(m[k].qual) == rec[3]
    # what did not merge stays paired: trimmed, filtered together, the two files in step
    t = c.pair.trim(ids=r["unmerged"], front_qual=5, tail_qual=5)
    p1, p2 = str(tmp_path / "u_R1.fq"), str(tmp_path / "u_R2.fq")
    w = c.pair.write(p1, p2, ids=r["unmerged"], start1=t["start1"], end1=t["end1"], start2=t["start2"], end2=t["end2"], min_len=150, batch_bytes=50_000)
    k1, k2 = t["end1"] - t["start1"] >= 150, t["end2"] - t["start2"] >= 150
    both = k1 & k2
    assert 0 < int(both.sum()) < int(k1.sum()) and int(both.sum()) < int(k2.sum())       # each mate alone drops reads the other keeps
    assert w == {"pairs": int(both.sum()), "bases1": int((t["end1"] - t["start1"])[both].sum()), "bases2": int((t["end2"] - t["start2"])[both].sum()),
                 "dropped": int((~both).sum())}
    u1, u2 = fx.Fastq(p1), fx.Fastq(p2)
    assert len(u1) == len(u2) == w["pairs"]
    fx.FastqPair(u1, u2).check_names(n=w["pairs"])
    kept = r["unmerged"][both]
    for k in range(0, w["pairs"], 53):
        i = int(kept[k])
        assert u1[k].name == c.fq1[i].name and u2[k].name == c.fq2[i].name
        a, b = int(t["start2"][both][k]), int(t["end2"][both][k])
        assert _lat(u2[k].seq) == c.rows[i][2][a:b] and _lat(u2[k].qual) == c.rows[i][3][a:b]
    # merged plus unmerged is the run
    c.pair.check_names()


def test_trim_with_the_overlap(corpora):
    c = corpora("random")
    want = c.truth()
    t = c.pair.trim(clip_front=3)
    s1, s2 = c.fq1.trim(clip_front=3), c.fq2.trim(clip_front=3)
    assert np.array_equal(t["diag"], want["diag"]) and t["diag"].dtype == np.int32
    assert np.array_equal(t["end1"], np.minimum(s1["end"], want["end1"])) and np.array_equal(t["end2"], np.minimum(s2["end"], want["end2"]))
    assert np.array_equal(t["start1"], np.minimum(s1["start"], t["end1"])) and (t["start1"] <= t["end1"]).all() and (t["start2"] <= t["end2"]).all()
    back = (want["diag"] < 0) & (want["diag"] != NONE)
    assert (t["end1"][back] == want["insert"][back]).all() and (t["end1"][~back] == 150).all()     # read-through is cut, nothing else
    loose = c.pair.trim(overlap=dict(min_overlap=12, max_diff=8, max_error_rate=0.15), ids=np.arange(0, c.n, 7))
    assert np.array_equal(loose["diag"], c.truth(min_overlap=12, max_diff=8, max_error_rate=0.15)["diag"][::7])


def test_error_states(fx, corpora, tmp_path):
    from pyfastx_amd import _lib
    a, b = corpora("long1024"), corpora("sweep")
    with pytest.raises(ValueError, match="numbers of reads"):
        fx.FastqPair(a.fq1, b.fq2)
    with pytest.raises(TypeError):
        fx.FastqPair(a.fq1, str(tmp_path / "x.fq"))
    # the same at the ABI: different numbers of reads, a handle without its table
    b1 = a.pair._blobs()[0]
    b2 = b.pair._blobs()[1]
    with pytest.raises(_lib.FxError) as e:
        b1.fastq_pair_overlap(b2)
    assert e.value.code == _lib.FX_EINVAL
    raw = _lib.Blob.from_bytes(b"@r\nACGT\n+\nIIII\n", device=0)
    with pytest.raises(_lib.FxError) as e:
        b1.fastq_pair_overlap(raw)
    assert e.value.code == _lib.FX_ESTATE
    with pytest.raises(_lib.FxError) as e:
        raw.fastq_pair_merge_alloc(b1, np.zeros(1, dtype=np.int32))
    assert e.value.code == _lib.FX_ESTATE
    # a pair of a file with itself is a pair like any other
    same = fx.FastqPair(a.fq1, a.fq1).overlap()
    assert same["diag"].shape == (3,)


def test_synthetic_pairs_against_their_truth(fx):
    """2 x 10^5 pairs generated in HBM (synth.fastq_pair_generate): the insert of overlap against the generator's."""
    import torch
    from pyfastx_amd import _lib, pair, synth
    dev = torch.device("cuda", 0)
    n, rlen = 200_000, 150
    t1, c1, t2, c2, ins = synth.fastq_pair_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    assert ins.shape == (n,) and ins.dtype == np.int64 and 20 <= ins.min() < rlen < ins.max() <= 2 * rlen + 100
    b1 = _lib.Blob.from_device(t1.data_ptr(), int(c1["n_bytes"]), device=0, keepalive=t1)
    b2 = _lib.Blob.from_device(t2.data_ptr(), int(c2["n_bytes"]), device=0, keepalive=t2)
    assert b1.fastq_build().n_reads == n and b2.fastq_build().n_reads == n
    cols = pair.overlap_blob(b1, b2, n, None, pair.overlap_args())
    got = pair.insert_of(cols["diag"], rlen, rlen)
    inside = (ins >= 30) & (ins <= 270)
    hit = int((got[inside] == ins[inside]).sum())
    assert int(inside.sum()) > 0.7 * n and hit >= 0.95 * int(inside.sum()), (hit, int(inside.sum()))
    short = ins < rlen                                        # read-through: both ends cut to the insert where it was found
    found = short & (got == ins)
    assert found.sum() > 1000 and (cols["end1"][found] == ins[found]).all() and (cols["end2"][found] == ins[found]).all()
    assert (cols["end1"][~short] == rlen).sum() >= 0.99 * int((~short).sum())
    # the records of a slice against the definition
    ids = np.arange(0, n, n // 200, dtype=np.int64)[:200]
    buf, offs, merged = b1.fastq_pair_merge_alloc(b2, cols["diag"][ids], ids)
    h1, h2 = t1.cpu().numpy(), t2.cpu().numpy()
    rec, hl = int(c1["rec"]), int(c1["soff"][0])
    for k, i in enumerate(ids):
        r1, r2 = h1[i * rec:(i + 1) * rec], h2[i * rec:(i + 1) * rec]
        want = merged_truth(r1[:hl - 1].tobytes(), r1[hl:hl + rlen], r1[hl + rlen + 3:hl + 2 * rlen + 3], r2[hl:hl + rlen], r2[hl + rlen + 3:hl + 2 * rlen + 3],
                            int(cols["diag"][i]))
        assert buf[offs[k]:offs[k + 1]].tobytes() == want
        assert insert_of(int(cols["diag"][i]), rlen, rlen) == got[i]
    assert merged == int((cols["diag"][ids] != NONE).sum())
