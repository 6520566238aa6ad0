"""-m gpu: Fasta.sketch / Fastq.sketch / sketch.Sketch (fx_fasta_sketch, fx_fastq_sketch, fx_sketch_*, csrc/fx_sketch.hpp) against
the brute-force model of sketch_truth.py over fa[i].seq and the read strings: every line layout the index accepts, layout
invariance, every phase of a record's first byte against the 256-byte runs, invalid letters around run boundaries, the cut at
slen, row offsets across a scan chunk, the limits of the per-run count field, duplicates, the k-mer tables of the existing device
code, the retry rounds, many sets, the comparison kernel against the merge of two lists, and the round trips of the object.
Every comparison is exact."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from sketch_truth import compare_model, cut, key_set, key_set_np, keys_np
from test_gpu_search_approx import _layout                   # the layouts of the approximate search, generated the same way

pytestmark = pytest.mark.gpu

KS = (1, 4, 15, 21, 31)
KEEP = ((1, None), (3, None), (50, None), (None, 1), (None, 16), (7, 5), (None, 10 ** 6))     # (scaled, size)
_SETS = {}


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


def _seqs(fa):
    return [fa[i].seq for i in range(len(fa))]


def _fastq(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads))


def _full(seqs, k, canonical):
    """The key set of every text, computed once per (texts, k, canonical): the integer form for small texts, the numpy form
    (pinned against it in test_sketch_host) for large ones."""
    key = (hash(tuple(seqs)), k, canonical)
    if key not in _SETS:
        small = sum(len(s) for s in seqs) <= 6000
        _SETS[key] = [key_set(s, k, canonical) if small else set(key_set_np(s, k, canonical).tolist()) for s in seqs]
    return _SETS[key]


def want_sets(seqs, k, canonical, scaled, size, ids=None, pooled=False):
    from pyfastx_amd import sketch
    full = _full(seqs, k, canonical)
    sel = range(len(seqs)) if ids is None else sorted(set(int(i) for i in ids))
    per = [full[i] for i in sel]
    if pooled:
        per = [set().union(*per)]
    return [cut(s, sketch.max_key_of(k, scaled), size or 0) for s in per]


def same(sk, sets):
    """The sketch holds exactly these sets: offsets and keys at once."""
    off, keys = sk._arrays()
    assert off.dtype == np.int64 and keys.dtype == np.uint64 and sk.n_sets == len(sets)
    assert off.tolist() == np.concatenate(([0], np.cumsum([len(s) for s in sets], dtype=np.int64))).tolist()
    assert keys.tolist() == [x for s in sets for x in s]
    return True


def check(fa, seqs, k, canonical=True, scaled=None, size=None, ids=None, pooled=False, **kw):
    sk = fa.sketch(k, scaled=scaled, size=size, canonical=canonical, ids=ids, pooled=pooled, **kw)
    assert same(sk, want_sets(seqs, k, canonical, scaled, size, ids, pooled)), (k, canonical, scaled, size, pooled)
    return sk


# ------------------------------------------------------------------ line layouts
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["irregular", "crlf", "odd", "long", "test.fa", "test.fa.gz"])
def test_layouts(fx, tmp_path, name, k):
    if name.startswith("test.fa"):
        shutil.copy(os.path.join(DATA, name), tmp_path / name)
        fa = fx.Fasta(str(tmp_path / name))
    else:
        fa = fx.Fasta(_write(tmp_path / (name + ".fa"), _layout(name)))
    seqs = _seqs(fa)
    n = 0
    for canonical in (True, False):
        for scaled, size in KEEP:
            for pooled in (False, True):
                sk = check(fa, seqs, k, canonical, scaled, size, pooled=pooled)
                n += int(sk.sizes.sum())
                assert (sk.k, sk.canonical, sk.scaled, sk.size, len(sk.names)) == (k, canonical, scaled, size or 0, 1 if pooled else len(seqs))
    assert n > 0


# ------------------------------------------------------------------ layout invariance
def test_layout_invariance(fx, tmp_path):
    rng = np.random.default_rng(41)
    seqs = [_rand(rng, n, a) for n, a in ((70, "ACGT"), (256, "ACGT"), (257, "ACGTacgt"), (900, "ACGT"), (513, "ACGTN"), (33, "ACGT"), (1200, "ACGTacgtNR"),
                                          (41, "AC"))]
    for width in (1, 7, 60, 255, 256, 257, None):
        for eol in ("\n", "\r\n"):
            text = "".join(">s%d%s%s%s" % (i, eol, eol.join(s[a:a + (width or len(s))] for a in range(0, len(s), width or len(s))), eol)
                           for i, s in enumerate(seqs))
            fa = fx.Fasta(_write(tmp_path / ("inv_%s_%d.fa" % (width, len(eol))), text))
            assert _seqs(fa) == seqs
            for k, canonical, scaled, size, pooled in ((15, True, 2, None, False), (31, True, None, 20, False), (4, False, 1, None, True), (21, True, 3, 40, True)):
                check(fa, seqs, k, canonical, scaled, size, pooled=pooled)


# ------------------------------------------------------------------ the phase of a record's first byte
@pytest.mark.parametrize("k", [4, 21, 31])
def test_record_start_phase(fx, tmp_path, k):
    """For every d in 0 .. k the first sequence byte of a record sits at offset 256 - d of a 256-byte block (the header is
    padded): records of k - 1 letters (no window), k letters (one window) and 700 letters."""
    rng = np.random.default_rng(k)
    raw, seqs, firsts = b"", [], []
    for d in range(k + 1):
        for n in (700, k - 1, k):
            name = ">d%d_%d x" % (d, n)
            pad = (256 - d - (len(raw) + len(name) + 1)) % 256
            raw += (name + "x" * pad + "\n").encode()
            firsts.append((len(raw), d))
            seqs.append(_rand(rng, n))
            raw += seqs[-1].encode() + b"\n"
    assert all(off % 256 == (256 - d) % 256 and raw[off - 1:off] == b"\n" for off, d in firsts)
    fa = fx.Fasta(_write(tmp_path / "phase.fa", raw))
    assert _seqs(fa) == seqs
    for canonical in (True, False):
        sk = check(fa, seqs, k, canonical, 1, None)
        per = sk.sizes
        assert (per[1::3] == 0).all() and (per[2::3] == 1).all() and (per[0::3] > 100 if k > 4 else per[0::3] > 20).all()
        check(fa, seqs, k, canonical, 3, 50)
        check(fa, seqs, k, canonical, None, 30, pooled=True)


# ------------------------------------------------------------------ invalid letters
def test_invalid_letters(fx, tmp_path):
    """k = 15, one line, letter i at stream offset 5 + i.  A single N at kept index -1, 0 and 1 of a run; stretches of N of k - 1
    and k letters that end at a run boundary, in front of one and behind one; U and IUPAC letters."""
    k = 15
    rng = np.random.default_rng(15)
    hdr, n = ">inv\n", 256 * 24
    t = list(_rand(rng, n))
    edge = lambda j: 256 * j - len(hdr)                      # the letter that is kept index 0 of run j
    for j, o in ((1, -1), (2, 0), (3, 1)):
        t[edge(j) + o] = "N"
    j = 5
    for length in (k - 1, k):
        for last in (-1, -4, 3):                             # kept index of the stretch's last N
            z = edge(j) + last + 1
            t[z - length:z] = "N" * length
            j += 2
    assert j < 22
    text = "".join(t)
    other = _rand(rng, 900, "ACGTUuRYKMSWBDHVN*-acgt")
    fa = fx.Fasta(_write(tmp_path / "inv.fa", hdr + text + "\n>other\n" + other + "\n>onlyN\n" + "N" * 300 + "\n"))
    seqs = _seqs(fa)
    assert seqs == [text, other, "N" * 300]
    assert len(_full(seqs, k, True)[0]) < n - k + 1 - 200     # the Ns void windows
    for canonical in (True, False):
        sk = check(fa, seqs, k, canonical, 1, None)
        assert sk.sizes[2] == 0
        check(fa, seqs, k, canonical, 3, None, pooled=True)
        check(fa, seqs, 4, canonical, 1, None)
        check(fa, seqs, k, canonical, None, 100)


# ------------------------------------------------------------------ the cut at slen
def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: slen is smaller than the number of kept
    bytes and `seq` stops there.  No key may come from behind the cut."""
    rng = np.random.default_rng(55)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 20, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = _seqs(fa)
    assert sum(n > len(s) for s, n in zip(seqs, kept)) >= 3, "the case is not exercised"
    for k in (15, 5, 31):
        for canonical in (True, False):
            check(fa, seqs, k, canonical, 1, None)
            check(fa, seqs, k, canonical, 2, 300, pooled=True)
            check(fa, seqs, k, canonical, None, 200, oversample=1)


# ------------------------------------------------------------------ row offsets across a chunk of the scans
def test_scan_chunk(fx, tmp_path):
    """One record of more than 4096 runs, all with rows: the offsets of the rows behind run 4096 carry the sum of a scan chunk."""
    rng = np.random.default_rng(77)
    n = 1_100_000
    text = _rand(rng, n)
    fa = fx.Fasta(_write(tmp_path / "big.fa", ">big\n" + "\n".join(text[i:i + 80] for i in range(0, n, 80)) + "\n"))
    want = key_set_np(text, 15, True)
    sk = fa.sketch(15, scaled=1)
    assert sk.sizes.tolist() == [want.size] and np.array_equal(sk.hashes(0), want)
    half = fa.sketch(15, scaled=2, pooled=True)
    assert np.array_equal(half.hashes(0), want[want < np.uint64(4 ** 15 // 2)]) and 0.45 < half.sizes[0] / want.size < 0.55
    bottom = fa.sketch(15, size=1000)
    assert np.array_equal(bottom.hashes(0), want[:1000])


# ------------------------------------------------------------------ the 9-bit count field
def test_field_limits(fx, tmp_path):
    """k = 1 with scaled = 1 on one line of valid letters: every byte of a full run is a row, 256 of them."""
    rng = np.random.default_rng(8)
    seqs = ["A" * 1000 + "T" * 1000, _rand(rng, 2000), "C" * 700]
    fa = fx.Fasta(_write(tmp_path / "line.fa", "".join(">f%d\n%s\n" % (i, s) for i, s in enumerate(seqs))))
    for canonical in (True, False):
        sk = check(fa, seqs, 1, canonical, 1, None)
        assert sk.sizes.tolist() == ([1, 2, 1] if canonical else [2, 4, 1])
        check(fa, seqs, 1, canonical, 1, None, pooled=True)
        check(fa, seqs, 2, canonical, 1, None)


# ------------------------------------------------------------------ duplicates
def test_duplicates(fx, tmp_path):
    rng = np.random.default_rng(3)
    block = _rand(rng, 300)
    base = _rand(rng, 3000)
    seqs = [block * 10] + [base[:1500] + _rand(rng, 20) + base[1500:] for _ in range(6)]
    fa = fx.Fasta(_write(tmp_path / "dup.fa", "".join(">u%d\n%s\n" % (i, "\n".join(s[a:a + 70] for a in range(0, len(s), 70))) for i, s in enumerate(seqs))))
    for k in (15, 21):
        sk = check(fa, seqs, k, True, 1, None)
        assert sk.sizes[0] == 300                            # ten copies of a block: every k-mer of the circle once
        pooled = check(fa, seqs, k, True, 1, None, ids=[1, 2, 3, 4, 5, 6], pooled=True)
        assert pooled.sizes[0] < 1.2 * sk.sizes[1]
        check(fa, seqs, k, False, 4, 100, pooled=True)


# ------------------------------------------------------------------ against the k-mer tables of the existing device code
def test_against_kmer_tables(fx, tmp_path):
    from pyfastx_amd import minimizer
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    shutil.copy(os.path.join(DATA, "test.fq"), tmp_path / "test.fq")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    fq = fx.Fastq(str(tmp_path / "test.fq"))
    for k in (4, 21, 31):
        for canonical in (True, False):
            for ids in (None, [200, 3, 17, 3]):
                sk = fa.sketch(k, scaled=1, canonical=canonical, ids=ids, pooled=True)
                t = fa.kmer_table(k, canonical=canonical, ids=None if ids is None else sorted(set(ids)))
                assert sk.n_sets == 1 and np.array_equal(np.sort(minimizer.unmix(sk.hashes(0), k)).astype(np.int64), t.codes), (k, canonical, ids)
            sq = fq.sketch(k, scaled=1, canonical=canonical)
            assert np.array_equal(np.sort(minimizer.unmix(sq.hashes(0), k)).astype(np.int64), fq.kmer_table(k, canonical=canonical).codes)
    rng = np.random.default_rng(12)
    reads = [_rand(rng, int(rng.integers(30, 200)), "ACGTN" if i % 7 == 0 else "ACGT") for i in range(2000)]
    fq2 = fx.Fastq(_write(tmp_path / "syn.fq", _fastq(reads)))
    ids = rng.integers(0, 2000, 1500)
    lens = np.array([len(reads[i]) for i in ids])
    start = (rng.random(1500) * lens).astype(np.int64)
    end = start + (rng.random(1500) * (lens - start + 1)).astype(np.int64)
    for k in (4, 21, 31):
        sq = fq2.sketch(k, scaled=1, canonical=True, ids=ids, start=start, end=end)
        t = fq2.kmer_table(k, canonical=True, ids=ids, start=start, end=end)
        assert np.array_equal(np.sort(minimizer.unmix(sq.hashes(0), k)).astype(np.int64), t.codes) and t.codes.size > 100
    # and against the model, with a size and a scaled
    pool = set()
    for q, i in enumerate(ids.tolist()):
        pool |= key_set(reads[i][start[q]:end[q]], 21, False)
    assert fq2.sketch(21, scaled=5, size=300, canonical=False, ids=ids, start=start, end=end).hashes(0).tolist() == cut(pool, -(-4 ** 21 // 5), 300)
    assert fq2.sketch(21, size=64, canonical=False, ids=ids, start=start, end=end, oversample=1).hashes(0).tolist() == cut(pool, 4 ** 21, 64)
    with pytest.raises(ValueError):
        fq2.sketch(21, scaled=5, ids=[0, 1, 2], start=[0, 0, 5], end=[10, 10, 4])


# ------------------------------------------------------------------ retry rounds
def test_retry_rounds(fx, tmp_path):
    rng = np.random.default_rng(21)
    fa = fx.Fasta(_write(tmp_path / "acac.fa", ">acac\n" + "AC" * 2500 + "\n"))
    for canonical in (True, False):
        sk = check(fa, ["AC" * 2500], 21, canonical, None, 16)
        assert sk.sizes[0] in (1, 2) and sk.n_rounds > 1
    seqs = [_rand(rng, 2000) for _ in range(200)]
    fb = fx.Fasta(_write(tmp_path / "r200.fa", "".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))))
    got = {o: fb.sketch(21, size=64, oversample=o) for o in (1, 4, 64)}
    assert same(got[4], want_sets(seqs, 21, True, None, 64))
    for o in (1, 64):
        assert np.array_equal(got[o]._arrays()[0], got[4]._arrays()[0]) and np.array_equal(got[o]._arrays()[1], got[4]._arrays()[1])
    assert got[1].n_rounds > 1 and got[64].n_rounds == 1
    assert same(fb.sketch(21, scaled=3, size=64, oversample=1, pooled=True), want_sets(seqs, 21, True, 3, 64, pooled=True))


# ------------------------------------------------------------------ many sets
def test_many_sets(fx, tmp_path):
    """70 000 records of 20 to 40 letters at k = 15, scaled = 2: the slot needs a third radix digit.  Records shorter than k and
    records of N only give empty sets."""
    rng = np.random.default_rng(70)
    n, k = 70_000, 15
    lens = rng.integers(20, 41, n)
    lens[::997] = rng.integers(0, k, lens[::997].size)       # shorter than k
    only_n = np.zeros(n, dtype=bool)
    only_n[5::1013] = True
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum()))]
    starts = np.concatenate(([0], np.cumsum(lens)))
    recs = []
    for i in range(n):
        s = letters[starts[i]:starts[i + 1]].tobytes()
        recs.append(b"N" * len(s) if only_n[i] else s)
    fa = fx.Fasta(_write(tmp_path / "many.fa", b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(recs))))
    assert len(fa) == n
    # the model in one piece: the records joined by N, every valid window to its record
    joined = b"N".join(recs)
    first = np.concatenate(([0], np.cumsum([len(s) + 1 for s in recs])))[:-1]
    ok, key = keys_np(joined, k, True)
    pos = np.nonzero(ok)[0]
    rec = (np.searchsorted(first, pos, side="right") - 1).astype(np.uint64)
    pairs = np.unique((rec << np.uint64(30)) | key[pos])     # (record, key) in one word: keys lie below 4^15 = 2^30
    r_all, k_all = (pairs >> np.uint64(30)).astype(np.int64), pairs & np.uint64(2 ** 30 - 1)
    below = k_all < np.uint64(4 ** k // 2)
    sk = fa.sketch(k, scaled=2)
    off, keys = sk._arrays()
    assert sk.n_sets == n and np.array_equal(keys, k_all[below])
    assert np.array_equal(np.diff(off), np.bincount(r_all[below], minlength=n))
    assert (sk.sizes[::997] == 0).all() and (sk.sizes[5::1013] == 0).all() and sk.sizes.max() > 5 and sk.names[69_999] == "s69999"
    # a bottom-4 sketch of the same records: most sets need a second round at oversample = 1
    b4 = fa.sketch(k, size=4, oversample=1)
    rank = np.arange(r_all.size) - np.searchsorted(r_all, r_all, side="left")
    assert np.array_equal(b4._arrays()[1], k_all[rank < 4]) and np.array_equal(b4.sizes, np.bincount(r_all[rank < 4], minlength=n)) and b4.n_rounds > 1
    assert fa.sketch(k, scaled=2, ids=[]).n_sets == 0 and fa.sketch(k, scaled=2, ids=[], pooled=True).sizes.tolist() == [0]
    part = fa.sketch(k, scaled=2, ids=[69_999, 3, 3, 40_000])
    assert part.names == ["s3", "s40000", "s69999"] and [part.hashes(i).tolist() for i in range(3)] == [sk.hashes(i).tolist() for i in (3, 40_000, 69_999)]


# ------------------------------------------------------------------ the comparison kernel
def test_compare_against_model(fx):
    from pyfastx_amd.sketch import Sketch
    rng = np.random.default_rng(64)
    k, top = 21, 4 ** 21
    draw = lambda n: np.unique(rng.integers(0, top, 2 * n + 8, dtype=np.uint64))[:n] if n else np.zeros(0, dtype=np.uint64)
    A = [draw(n) for n in (0, 1, 63, 64, 65, 1000, 5000)]
    big = A[6]
    B = [big.copy(),                                         # identical to A[6]
         np.setdiff1d(draw(1000), big),                      # disjoint from it (and from nearly everything)
         np.sort(np.concatenate([big[::2], np.setdiff1d(draw(2500), big)])),      # interleaved: every other key of A[6] among strangers
         big[:640].copy(), big[:64].copy(),                  # prefixes
         A[5][3:].copy(), np.zeros(0, dtype=np.uint64), A[2].copy(), np.array([big[4999]], dtype=np.uint64)]
    a = Sketch.from_hashes(A, k, scaled=1)
    b = Sketch.from_hashes(B, k, scaled=1, names=["b%d" % i for i in range(len(B))])
    La, Lb = [x.tolist() for x in A], [x.tolist() for x in B]
    cutk = int(big[2500])                                    # cuts both sides of most pairs
    for limit, max_key in ((0, None), (1, None), (64, None), (1000, None), (10 ** 9, None), (0, cutk), (100, cutk), (0, 1)):
        shared, total = a.compare(b, limit=limit, max_key=max_key)
        assert shared.shape == total.shape == (len(A), len(B)) and shared.dtype == total.dtype == np.int64
        for i in range(len(A)):
            for j in range(len(B)):
                assert (int(shared[i, j]), int(total[i, j])) == compare_model(La[i], Lb[j], limit, max_key or 0), (limit, max_key, i, j)
    ia, ib = [6, 0, 5, 5, 2], [8, 2, 0]
    shared, total = a.compare(b, limit=700, ia=ia, ib=ib)
    assert [[compare_model(La[i], Lb[j], 700) for j in ib] for i in ia] == [list(zip(r, t)) for r, t in zip(shared.tolist(), total.tolist())]
    assert a.compare(b, ia=[], ib=[1])[0].shape == (0, 1)
    both = Sketch.concat([a, b])
    shared, total = both.compare()
    assert np.array_equal(shared, shared.T) and np.array_equal(total, total.T) and np.array_equal(np.diag(shared), both.sizes)
    assert np.array_equal(np.diag(total), both.sizes)
    # what follows from the counts
    j = a.jaccard(b)
    assert j[6, 0] == 1.0 and j[6, 1] == 0.0 and j[0, 6] == 0.0 and j[6, 3] == 640 / 5000
    c = b.containment(a)
    assert c[3, 6] == 1.0 and c[2, 6] == 2500 / len(B[2]) and c[6, 0] == 0.0
    assert b.ani(a)[3, 6] == 1.0
    with pytest.raises(ValueError):
        a.mash_distance(b)                                   # no size
    s1 = Sketch.from_hashes([big[:1000], A[5]], k, size=1000)
    s2 = Sketch.from_hashes([big[:500]], k, size=500)
    d = s1.mash_distance(s2)
    jj = compare_model(La[5], big[:500].tolist(), 500)[0] / 500
    assert d.shape == (2, 1) and d[0, 0] == 0.0 and d[1, 0] == pytest.approx(min(1.0, -np.log(2 * jj / (1 + jj)) / k) if jj else 1.0)
    # sketches that differ in max_key compare below the smaller one
    lo = Sketch.from_hashes([big[big < np.uint64(top // 4)]], k, scaled=4)
    sh, tot = a.compare(lo)
    assert (int(sh[6, 0]), int(tot[6, 0])) == compare_model(La[6], lo.hashes(0).tolist(), 0, lo.max_key) and sh[6, 0] == tot[6, 0] == lo.sizes[0]
    assert a.containment(lo)[6, 0] == 1.0


# ------------------------------------------------------------------ round trips, rejections, states
def test_round_trips_and_rejections(fx, tmp_path):
    from pyfastx_amd import _lib
    from pyfastx_amd.sketch import Sketch
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    fa = fx.Fasta(str(tmp_path / "test.fa"))
    names = list(fa.keys())
    sk = fa.sketch(21, scaled=10, size=50)
    assert sk.names == names and same(sk, want_sets(_seqs(fa), 21, True, 10, 50)) and sk.sizes.max() <= 50 < fa.sketch(21, scaled=10).sizes.max()
    sk.save(str(tmp_path / "s.npz"))
    back = Sketch.load(str(tmp_path / "s.npz"))
    assert (back.k, back.canonical, back.scaled, back.size, back.max_key, back.names) == (21, True, 10, 50, sk.max_key, names)
    assert np.array_equal(back._arrays()[0], sk._arrays()[0]) and np.array_equal(back._arrays()[1], sk._arrays()[1])
    sub = sk.select([5, 0, 5])
    assert sub.names == [names[5], names[0], names[5]] and [sub.hashes(i).tolist() for i in range(3)] == [sk.hashes(i).tolist() for i in (5, 0, 5)]
    joined = Sketch.concat([sub, back])
    assert joined.n_sets == 3 + len(fa) and joined.hashes(3).tolist() == sk.hashes(0).tolist() and joined.names[:3] == sub.names
    assert np.array_equal(np.diag(sk.compare(back)[0]), sk.sizes)
    words = sk.kmers(7)
    seq7, comp = fa[7].seq.upper(), str.maketrans("ACGT", "TGCA")
    assert len(words) == sk.sizes[7] > 0 and all(w in seq7 or w[::-1].translate(comp) in seq7 for w in words)
    assert sk.cardinality().shape == (len(fa),) and sk.hashes(0).dtype == np.uint64 and (np.diff(sk.hashes(0).astype(np.int64)) > 0).all()
    with pytest.raises(ValueError):
        Sketch.concat([sk, fa.sketch(21, scaled=10)])
    with pytest.raises(ValueError):
        sk.compare(fa.sketch(15, scaled=10))
    with pytest.raises(ValueError):
        sk.compare(fa.sketch(21, scaled=10, canonical=False))
    with pytest.raises(ValueError, match="%d pairs" % (len(fa) ** 2)):
        sk.compare(max_pairs=len(fa) ** 2 - 1)
    for bad in (lambda: fa.sketch(21), lambda: fa.sketch(0, scaled=1), lambda: fa.sketch(32, scaled=1), lambda: fa.sketch(21, scaled=0),
                lambda: fa.sketch(21, size=-1)):
        with pytest.raises(ValueError):
            bad()
    # what from_hashes refuses
    ok = np.array([1, 5, 9], dtype=np.uint64)
    assert Sketch.from_hashes([ok, []], 4, scaled=1).sizes.tolist() == [3, 0]
    for arrays, kw in (([[5, 1, 9]], dict(scaled=1)), ([[1, 5, 5]], dict(scaled=1)), ([ok, [7, 7]], dict(scaled=1)), ([[1, 5, 256]], dict(scaled=1)),
                       ([[1, 5, 64]], dict(scaled=4)), ([[1, 2, 3, 4]], dict(size=3)), ([ok, [9, 8]], dict(size=3))):
        with pytest.raises(ValueError):
            Sketch.from_hashes(arrays, 4, **kw)
    # through the library
    L = _lib.lib()
    off_bad = np.array([0, 2, 1, 3], dtype=np.int64)
    s = C.c_void_p()
    assert L.fx_sketch_from_host(0, 4, 1, 256, 0, 3, off_bad.ctypes.data, ok.ctypes.data, C.byref(s)) == _lib.FX_EINVAL and s.value is None
    raw = open(os.path.join(DATA, "test.fa"), "rb").read()
    b = _lib.Blob.from_bytes(raw, device=0)
    with pytest.raises(_lib.FxError) as e:
        b.fasta_sketch(21, 1, max_key=4 ** 21)
    assert e.value.code == _lib.FX_ESTATE
    b.fasta_build()
    o21, rounds = b.fasta_sketch(21, 1, max_key=sk.max_key, size=50)
    assert rounds >= 1 and np.array_equal(o21.read()[1], sk._arrays()[1])
    o15, _ = b.fasta_sketch(15, 1, max_key=4 ** 15)
    with pytest.raises(_lib.FxError) as e:
        o21.compare(o15)
    assert e.value.code == _lib.FX_EINVAL
    with pytest.raises(_lib.FxError) as e:
        o21.compare(o21, max_pairs=10)
    assert e.value.code == _lib.FX_ERANGE and "211 x 211" in str(e.value)
    with pytest.raises(_lib.FxError) as e:
        b.fasta_sketch(21, 1, ids=[0, 211], max_key=4 ** 21)
    assert e.value.code == _lib.FX_ERANGE
    second = raw.index(b"\n>", 1) + 1
    r = _lib.Blob.from_file_range(str(tmp_path / "test.fa"), second, len(raw) - second, 0)
    r.fasta_build()
    with pytest.raises(_lib.FxError) as e:
        r.fasta_sketch(21, 1, max_key=4 ** 21)
    assert e.value.code == _lib.FX_EINVAL
    rawq = open(os.path.join(DATA, "test.fq"), "rb").read()
    q = _lib.Blob.from_bytes(rawq, device=0)
    with pytest.raises(_lib.FxError) as e:
        q.fastq_sketch(21, 1, max_key=4 ** 21)
    assert e.value.code == _lib.FX_ESTATE
    q.fastq_build()
    oq, _ = q.fastq_sketch(21, 1, max_key=4 ** 21 // 10)
    assert oq.n_sets == 1 and oq.flags == _lib.FX_SK_CANONICAL | _lib.FX_SK_POOLED and oq.compare(o21)[0].shape == (1, 211)
    sk.release()
    with pytest.raises(_lib.FxError):
        sk.compare()


def test_sharded_raises(fx, tmp_path, monkeypatch):
    shutil.copy(os.path.join(DATA, "test.fa"), tmp_path / "test.fa")
    shutil.copy(os.path.join(DATA, "test.fq"), tmp_path / "test.fq")
    fa, fq = fx.Fasta(str(tmp_path / "test.fa")), fx.Fastq(str(tmp_path / "test.fq"))
    assert fa.sketch(21, scaled=100, pooled=True).names == ["test.fa"] and fq.sketch(21, scaled=100).names == ["test.fq"]
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    monkeypatch.setattr(type(fq), "_sharded", property(lambda self: True))
    for call in (lambda: fa.sketch(21, scaled=100), lambda: fq.sketch(21, scaled=100)):
        with pytest.raises(NotImplementedError):
            call()
