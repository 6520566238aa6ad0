"""-m gpu: Fastq.duplicates / Fastq.dedup and the two C entries behind them (csrc/fx_fastq_dedup.hpp) against the definition
tests/dedup_truth.py, computed from the strings a file was written from -- never from the library.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA
from dedup_truth import dedup_truth, first_truth, rc

pytestmark = pytest.mark.gpu


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


def _rand(rng, n, letters="ACGT"):
    return "".join(np.array(list(letters))[rng.integers(0, len(letters), n)]) if n else ""


def _fastq(seqs, eol="\n", quals="I"):
    """Names differ from read to read, and so do the quality letters: neither may play a part."""
    return "".join("@q%d some/%d%s%s%s+%s%s%s" % (i, i % 7, eol, s, eol, eol, quals[i % len(quals)] * len(s), eol) for i, s in enumerate(seqs))


def _rcs(s):
    return rc(s).decode("latin-1")


def check_all(fq, keys, revcomp=False, hash_bits=0, min_rounds=1, max_rounds=1, **q):
    """duplicates, dedup and copies of the queries q against the truth of `keys`; -> n_rounds"""
    blob = fq._qc_blob()
    want = first_truth(keys, revcomp)
    wpos, wcp = dedup_truth(keys, revcomp)
    first, groups, rounds = blob.fastq_dup_first(revcomp=revcomp, hash_bits=hash_bits, **q)
    assert first.dtype == np.int64 and np.array_equal(first, want), (revcomp, hash_bits)
    assert groups == wpos.size and min_rounds <= rounds <= max_rounds, (groups, rounds)
    pos, cp, groups2, rounds2 = blob.fastq_dedup(revcomp=revcomp, hash_bits=hash_bits, want_copies=True, **q)
    assert pos.dtype == np.int64 and cp.dtype == np.int64
    assert np.array_equal(pos, wpos) and np.array_equal(cp, wcp) and (groups2, rounds2) == (groups, rounds), (revcomp, hash_bits)
    if hash_bits == 0:                                         # the object API: the same answers
        assert np.array_equal(fq.duplicates(revcomp=revcomp, **q), want)
        assert np.array_equal(fq.dedup(revcomp=revcomp, **q), wpos)
        p2, c2 = fq.dedup(revcomp=revcomp, return_counts=True, **q)
        assert np.array_equal(p2, wpos) and np.array_equal(c2, wcp)
    return rounds


# ------------------------------------------------------------------ 1: lengths and near-equal reads
def _near_equal_reads(rng):
    kinds = []
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 150, 151, 255, 256, 257):
        kinds.append(_rand(rng, n))
    long_read = _rand(rng, 5000)
    kinds.append(long_read)
    base = _rand(rng, 150)
    kinds += [base,
              ("C" if base[0] != "C" else "G") + base[1:],                   # the first byte only
              base[:-1] + ("C" if base[-1] != "C" else "G"),                 # the last byte only
              base.lower(), base[:70] + base[70].lower() + base[71:],       # case, everywhere and in one place
              base[:40] + "N" + base[41:], base[:149] + "N",                 # an N in the middle, at the end
              base[:149], base[:16], base[:17],                              # proper prefixes
              "A" * 16, "A" * 17, "A" * 15, "A" * 32, "A" * 33,
              long_read[:-1], long_read[:4999] + ("C" if long_read[4999] != "C" else "G"), long_read[1:]]
    p1, p2 = _rand(rng, 16), _rand(rng, 16)
    kinds += [p1 + p2, p2 + p1, p1 + p1, p2 + p2, p1, p2, p1 + p2 + p1, p1 + p1 + p2]
    kinds += [_rand(rng, 150) for _ in range(20)]
    reps = [kinds[i] for i in rng.permutation(np.repeat(np.arange(len(kinds)), 5)).tolist()]         # every kind five times, interleaved
    return reps


def test_lengths_and_near_equal_reads(fx, tmp_path):
    """One file, every kind several times.  n_rounds == 1 at 64 bits is a condition: a fingerprint that ignored the length,
    the order of the pieces or a byte of a partial piece would give two different keys one fingerprint and cost a second round
    (a true 64-bit collision among 300 reads has a chance of about n^2 / 2^65 = 2e-15)."""
    rng = np.random.default_rng(41)
    reads = _near_equal_reads(rng)
    assert 280 <= len(reads) <= 400 and len(set(reads)) * 5 == len(reads)
    fq = fx.Fastq(_write(tmp_path / "near.fq", _fastq(reads, quals="I5#F")))
    assert [fq[i].seq for i in (0, 7, len(reads) - 1)] == [reads[i] for i in (0, 7, len(reads) - 1)]
    for revcomp in (False, True):
        assert check_all(fq, reads, revcomp) == 1
    assert first_truth(reads).tolist().count(reads.index("")) == 5      # all empty keys are one group
    # min_copies / max_copies select among the groups
    blob = fq._qc_blob()
    for lo, hi in ((5, None), (6, None), (1, 4), (5, 5), (2, 10)):
        pos, cp, groups, rounds = blob.fastq_dedup(min_copies=lo, max_copies=-1 if hi is None else hi, want_copies=True)
        wp, wc = dedup_truth(reads, False, lo, hi)
        assert np.array_equal(pos, wp) and np.array_equal(cp, wc) and groups == len(set(reads)) and rounds == 1
        assert np.array_equal(fq.dedup(min_copies=lo, max_copies=hi), wp)
    pos, cp, _, _ = blob.fastq_dedup(want_copies=False)
    assert cp is None and pos.size == len(set(reads))


# ------------------------------------------------------------------ 2: alignment independence
@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_alignment_independence(fx, tmp_path, eol):
    """prefix_j + core with start = j: the key does not depend on where it lies in memory, nor on the cut at its tail."""
    rng = np.random.default_rng(42)
    core = _rand(rng, 180)
    reads, start, end, cut = [], [], [], []
    for j in range(18):
        for c in range(18):
            reads.append(_rand(rng, j) + core)
            start.append(j)
            end.append(j + len(core) - c)
            cut.append(c)
    order = rng.permutation(len(reads)).tolist()
    reads, start, end, cut = ([x[i] for i in order] for x in (reads, start, end, cut))
    fq = fx.Fastq(_write(tmp_path / "align.fq", _fastq(reads, eol=eol)))
    keys = [r[a:b] for r, a, b in zip(reads, start, end)]
    assert len(set(keys)) == 18
    for revcomp in (False, True):
        assert check_all(fq, keys, revcomp, start=start, end=end) == 1
    first = fq.duplicates(start=start, end=end)
    for c in range(18):                                        # all queries with the same cut of the core: one group
        members = [q for q in range(len(reads)) if cut[q] == c]
        assert set(first[members].tolist()) == {members[0]}
    # the cut at the front instead: suffixes of the core, at every alignment of the key's last byte
    s2 = [a + c for a, c in zip(start, cut)]
    e2 = [len(r) for r in reads]
    keys2 = [r[a:b] for r, a, b in zip(reads, s2, e2)]
    for revcomp in (False, True):
        assert check_all(fq, keys2, revcomp, start=s2, end=e2) == 1


# ------------------------------------------------------------------ 3: ids
def test_ids(fx, tmp_path):
    rng = np.random.default_rng(43)
    pool = [_rand(rng, int(n)) for n in rng.integers(20, 200, 30)]
    reads = [pool[i] for i in rng.integers(0, 30, 120).tolist()]
    fq = fx.Fastq(_write(tmp_path / "ids.fq", _fastq(reads)))
    ids = rng.permutation(120)[:70].tolist()
    ids = ids + ids[10:30] + [ids[0]]                          # a permuted subset with repeats
    keys = [reads[i] for i in ids]
    check_all(fq, keys, ids=ids)
    check_all(fq, keys, True, ids=ids)
    first = fq.duplicates(ids=ids)
    assert first[-1] == 0 and first[70] <= 10                  # positions refer to queries, not to reads
    lone = [i for i in range(120) if reads.count(reads[i]) == 1][:1] or [0]
    pos, cp = fq.dedup(ids=lone * 2, return_counts=True)       # a read listed twice forms a group of two
    assert pos.tolist() == [0] and cp.tolist() == [2]
    assert fq.duplicates(ids=[]).size == 0 and fq.dedup(ids=[]).size == 0
    assert fq._qc_blob().fastq_dup_first(ids=[])[1:] == (0, 0)
    # intervals with ids: row q belongs to query q
    a = [int(rng.integers(0, 10)) for _ in ids]
    b = [len(reads[i]) - int(rng.integers(0, 10)) for i in ids]
    check_all(fq, [reads[i][x:y] for i, x, y in zip(ids, a, b)], ids=ids, start=a, end=b)


# ------------------------------------------------------------------ 4: reverse complement
def test_reverse_complement(fx, tmp_path):
    rng = np.random.default_rng(44)
    reads = []
    for n in (1, 15, 16, 17, 33, 150):
        s = _rand(rng, n)
        while _rcs(s) == s:
            s = _rand(rng, n)
        changed = _rcs(s)
        at = n // 2
        changed = changed[:at] + ("A" if changed[at] != "A" else "C") + changed[at + 1:]
        reads += [s, _rcs(s), changed]
    half = _rand(rng, 40)
    reads += [half + _rcs(half), half + _rcs(half), "GAATTC", "AT", "ACGT"]             # palindromes
    mixed = "ACGTNacgtnRYACGTTTGACAnnNN" + _rand(rng, 20)
    reads += [mixed, _rcs(mixed), mixed.upper(), _rcs(mixed.upper()), "N" * 20, "N" * 20, "aacc", "ggtt", "GGTT", "AACC", "aaCC", "GGtt"]
    reads = [reads[i] for i in rng.permutation(len(reads)).tolist()]
    fq = fx.Fastq(_write(tmp_path / "rc.fq", _fastq(reads)))
    assert check_all(fq, reads, True) == 1
    assert check_all(fq, reads, False) == 1
    with_rc, without = first_truth(reads, True), first_truth(reads, False)
    assert len(set(with_rc.tolist())) < len(set(without.tolist()))
    for s in reads:                                            # with the flag s and rc(s) are one group, without it they stay apart
        if _rcs(s) != s and _rcs(s) in reads:
            i, j = reads.index(s), reads.index(_rcs(s))
            assert with_rc[i] == with_rc[j] and without[i] != without[j]
    # over intervals: the key's reverse complement, not the read's
    a = [min(2, len(s)) for s in reads]
    b = [max(len(s) - 1, x) for s, x in zip(reads, a)]
    check_all(fq, [s[x:y] for s, x, y in zip(reads, a, b)], True, start=a, end=b)


# ------------------------------------------------------------------ 5: the collision path
@pytest.mark.parametrize("revcomp", [False, True])
def test_collision_path(fx, tmp_path, revcomp):
    """Three fingerprint bits: a round resolves at most 2^3 groups, 40 distinct sequences need five rounds or more, and the
    answer is the truth's all the same."""
    rng = np.random.default_rng(45)
    pool = [_rand(rng, int(n)) for n in rng.integers(20, 120, 36)] + ["A" * 16, "A" * 17, "ACGT" * 8, "CGTA" * 8]
    assert len(set(pool)) == 40 and len({min(s, _rcs(s)) for s in pool}) == 40
    picks = np.concatenate([np.arange(40), rng.integers(0, 40, 260)])
    reads = [pool[i] if rng.random() < 0.7 else _rcs(pool[i]) for i in rng.permutation(picks).tolist()]
    fq = fx.Fastq(_write(tmp_path / "coll.fq", _fastq(reads)))
    rounds = check_all(fq, reads, revcomp, hash_bits=3, min_rounds=5, max_rounds=40)
    assert rounds >= 5
    assert check_all(fq, reads, revcomp, hash_bits=1, min_rounds=20, max_rounds=80) >= 20
    assert check_all(fq, reads, revcomp, hash_bits=64) == 1


# ------------------------------------------------------------------ 6: one contended group
def test_contended_group(fx, tmp_path):
    rng = np.random.default_rng(46)
    s, other = _rand(rng, 100), _rand(rng, 100)
    for at in (20000, 0, 7777):
        reads = [s] * 20000
        reads.insert(at, other)
        fq = fx.Fastq(_write(tmp_path / ("same%d.fq" % at), _fastq(reads)))
        pos, cp = fq.dedup(return_counts=True)
        want = [(0, 20000), (20000, 1)] if at == 20000 else [(0, 1), (1, 20000)] if at == 0 else [(0, 20000), (7777, 1)]
        assert list(zip(pos.tolist(), cp.tolist())) == want
        first = fq.duplicates()
        assert np.array_equal(first, first_truth(reads))
        assert fq.dedup(min_copies=2).tolist() == [want[0][0] if want[0][1] > 1 else want[1][0]]


# ------------------------------------------------------------------ 7: several tiles and scan chunks
def test_many_tiles(fx, tmp_path):
    """200 000 reads of about 30 bases from a pool of 50 000, and two groups of 10 000 and 5 000 members: their runs of equal
    fingerprints are longer than a sort tile (2048) and a scan chunk (4096), so they straddle both."""
    rng = np.random.default_rng(47)
    text = _rand(rng, 4000 * 30)
    pool = np.array([text[i * 30:i * 30 + int(n)] for i, n in enumerate(rng.integers(24, 31, 4000))], dtype=object)
    pool = np.array([pool[i % 4000] + "ACGT"[(i // 4000) % 4] + "ACGT"[(i // 16000) % 4] for i in range(50000)], dtype=object)
    picks = rng.integers(0, 50000, 185000)
    reads = pool[picks].tolist() + [pool[0] + "TT"] * 10000 + [pool[1] + "GG"] * 5000
    reads = [reads[i] for i in rng.permutation(len(reads)).tolist()]
    assert len(reads) == 200000
    fq = fx.Fastq(_write(tmp_path / "many.fq", _fastq(reads)))
    blob = fq._qc_blob()
    want = first_truth(reads)
    wpos, wcp = dedup_truth(reads)
    first, groups, rounds = blob.fastq_dup_first()
    assert np.array_equal(first, want) and groups == wpos.size and rounds == 1
    pos, cp, groups, rounds = blob.fastq_dedup(want_copies=True)
    assert np.array_equal(pos, wpos) and np.array_equal(cp, wcp) and groups == wpos.size and rounds == 1
    assert sorted(cp.tolist())[-2:] == [5000, 10000]
    pos, cp, _, _ = blob.fastq_dedup(min_copies=5000, want_copies=True)
    assert np.array_equal(pos, dedup_truth(reads, False, 5000)[0]) and sorted(cp.tolist()) == [5000, 10000]
    # the collision path over several tiles: 12 bits leave many runs with more than one key
    first, groups, rounds = blob.fastq_dup_first(hash_bits=12)
    assert np.array_equal(first, want) and groups == wpos.size and rounds > 1
    pos, cp, _, r2 = blob.fastq_dedup(hash_bits=12, want_copies=True, revcomp=True)
    wp, wc = dedup_truth(reads, True)
    assert np.array_equal(pos, wp) and np.array_equal(cp, wc) and r2 > 1
    from pyfastx_amd import dedup
    lv = dedup.duplication_levels(wcp)
    assert lv["n_reads"] == 200000 and lv["groups"][-1] == 1 and lv["groups"][-2] == 1


# ------------------------------------------------------------------ 8: composition
def test_composition(fx, tmp_path):
    rng = np.random.default_rng(48)
    pool = [_rand(rng, int(n)) for n in rng.integers(30, 160, 25)]
    reads = [pool[i] for i in rng.integers(0, 25, 90).tolist()] + [_rand(rng, 80) for _ in range(3)]       # three of them occur once
    quals = ["".join(chr(int(c)) for c in rng.integers(65, 75, len(s))) for s in reads]
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(reads, quals)))
    fq = fx.Fastq(_write(tmp_path / "comp.fq", text))
    keep = fq.dedup()
    out = tmp_path / "dedup.fq"
    info = fq.write(str(out), ids=keep)
    wpos, _ = dedup_truth(reads)
    assert info["reads"] == wpos.size == len(set(reads))
    assert open(out, "rb").read() == "".join("@r%d\n%s\n+\n%s\n" % (i, reads[i], quals[i]) for i in wpos.tolist()).encode()
    # over what trim returned: reads that differ only in what is clipped fall together
    ids = np.arange(len(reads) - 1, -1, -1, dtype=np.int64)
    iv = fq.trim(ids=ids, clip_front=4, clip_tail=3)
    cut = [reads[int(i)][int(a):int(b)] for i, a, b in zip(ids, iv["start"], iv["end"])]
    pos, cp = fq.dedup(ids=ids, start=iv["start"], end=iv["end"], min_copies=2, return_counts=True)
    wp, wc = dedup_truth(cut, False, 2)
    assert np.array_equal(pos, wp) and np.array_equal(cp, wc) and 0 < pos.size < len(set(cut))
    sel = ids[pos]
    info = fq.write(str(out), ids=sel, start=np.asarray(iv["start"])[pos], end=np.asarray(iv["end"])[pos])
    assert info["reads"] == pos.size
    want = "".join("@r%d\n%s\n+\n%s\n" % (int(i), cut[int(p)], quals[int(i)][4:len(reads[int(i)]) - 3]) for i, p in zip(sel, pos))
    assert open(out, "rb").read() == want.encode()
    # the fixture file, plain and gzip: the same stream, the same answer
    plain, gz = fx.Fastq(os.path.join(DATA, "test.fq")), fx.Fastq(os.path.join(DATA, "test.fq.gz"))
    seqs = [plain[i].seq for i in range(len(plain))]
    assert np.array_equal(plain.duplicates(), first_truth(seqs)) and np.array_equal(gz.duplicates(revcomp=True), first_truth(seqs, True))


# ------------------------------------------------------------------ 9: errors
def test_errors(fx, tmp_path, monkeypatch):
    from pyfastx_amd import _lib
    L = _lib.lib()
    rawq = open(os.path.join(DATA, "test.fq"), "rb").read()
    q = _lib.Blob.from_bytes(rawq, device=0)
    for call in (lambda: q.fastq_dup_first(), lambda: q.fastq_dedup()):          # before fx_fastq_build
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_ESTATE
    q.fastq_build()
    assert q.fastq_dup_first()[0].shape == (800,)
    for call in (lambda: q.fastq_dup_first(hash_bits=65), lambda: q.fastq_dup_first(hash_bits=-1), lambda: q.fastq_dedup(hash_bits=65),
                 lambda: q.fastq_dedup(min_copies=0), lambda: q.fastq_dedup(min_copies=-3)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    # unknown flag bits, more than 2^31 queries (refused before an id is read), start without end: through the raw entries
    p, pc, n, g, r, bad = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    one = np.zeros(1, dtype=np.int64)
    tail_first = (C.byref(p), C.byref(n), C.byref(g), C.byref(r), C.byref(bad))
    tail_dedup = (C.byref(p), C.byref(pc), C.byref(n), C.byref(g), C.byref(r), C.byref(bad))
    assert L.fx_fastq_dup_first(q._h, None, 0, None, None, 2, 0, *tail_first) == _lib.FX_EINVAL
    assert L.fx_fastq_dedup(q._h, None, 0, None, None, 3, 0, 1, -1, *tail_dedup) == _lib.FX_EINVAL
    assert L.fx_fastq_dup_first(q._h, one.ctypes.data, 2 ** 31 + 1, None, None, 0, 0, *tail_first) == _lib.FX_EINVAL
    assert L.fx_fastq_dedup(q._h, one.ctypes.data, 2 ** 31 + 1, None, None, 0, 0, 1, -1, *tail_dedup) == _lib.FX_EINVAL
    assert L.fx_fastq_dup_first(q._h, one.ctypes.data, -1, None, None, 0, 0, *tail_first) == _lib.FX_EINVAL
    assert L.fx_fastq_dup_first(q._h, None, 0, one.ctypes.data, None, 0, 0, *tail_first) == _lib.FX_EINVAL
    assert L.fx_fastq_dedup(q._h, None, 0, None, one.ctypes.data, 0, 0, 1, -1, *tail_dedup) == _lib.FX_EINVAL
    assert p.value is None and pc.value is None
    # a bad id, a bad interval: FX_ERANGE with its position, nothing allocated
    for call in (lambda: q.fastq_dup_first(ids=[0, 1, 800]), lambda: q.fastq_dedup(ids=[0, 1, -1])):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    for call in (lambda: q.fastq_dup_first(ids=[1, 2, 3], start=[0, 151, 0], end=[150, 151, 4]),
                 lambda: q.fastq_dedup(ids=[1, 2, 3], start=[0, 5, 0], end=[150, 4, 4]),
                 lambda: q.fastq_dedup(ids=[1, 2, 3], start=[0, -1, 0], end=[150, 4, 4])):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 1
    assert q.fastq_dup_first(ids=[1, 2, 3], start=[0, 150, 0], end=[150, 150, 0])[0].tolist() == [0, 1, 1]      # empty keys are equal
    # a byte-range shard
    off = [i for i, c in enumerate(rawq[:4096]) if c == 10][3] + 1
    sh = _lib.Blob.from_bytes(rawq[off:], device=0)
    sh.set_shard(off, 10, True)
    assert sh.fastq_build().n_reads > 0
    for call in (lambda: sh.fastq_dup_first(), lambda: sh.fastq_dedup()):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    # the three Python exception types
    fq = fx.Fastq(os.path.join(DATA, "test.fq"))
    for call in (lambda: fq.duplicates(ids=[0, len(fq)]), lambda: fq.dedup(ids=[-1])):
        with pytest.raises(IndexError):
            call()
    for call in (lambda: fq.duplicates(start=[0] * len(fq)), lambda: fq.duplicates(revcomp=1), lambda: fq.dedup(min_copies=0),
                 lambda: fq.dedup(min_copies=3, max_copies=2), lambda: fq.dedup(return_counts=1), lambda: fq.dedup(max_copies=1.5),
                 lambda: fq.duplicates(ids=[1, 2], start=[0, 0], end=[150, 151])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="query 1"):
        fq.dedup(ids=[1, 2], start=[0, 9], end=[150, 8])
    monkeypatch.setattr(type(fq), "_sharded", property(lambda self: True))
    for call in (lambda: fq.duplicates(), lambda: fq.dedup()):
        with pytest.raises(NotImplementedError):
            call()
