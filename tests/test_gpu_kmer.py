"""-m gpu: Fasta.kmer_counts / kmer_profile and Fastq.kmer_counts (fx_fasta_kmers, fx_fastq_kmers, csrc/fx_kmer.hpp) against
the definition tests/kmer_truth.py, computed from fa[i].seq / fq[i].seq or from a generator's flat bases -- never from the
library's own k-mer path.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from kmer_truth import CODE, flat_counts, kmer_counts_truth, kmer_profile_truth, revcomp_code

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 6, 7, 8, 9, 11, 13)             # 6 | 7 is the border between the table in LDS and the table in global memory
SMALL_KS = (1, 2, 3, 4, 5, 6)


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def same(got, want):
    assert got.dtype == np.int64 and got.shape == want.shape
    return np.array_equal(got, want)


def fold(counts, k):
    """canonical counts from plain ones (kmer_truth.fold_canonical, by bincount: exact below 2^53)."""
    idx = np.arange(4 ** k, dtype=np.int64)
    return np.bincount(np.minimum(idx, revcomp_code(idx, k)), weights=counts, minlength=4 ** k).astype(np.int64)


def check_fasta(fa, seqs, ks=KS):
    for k in ks:
        plain = kmer_counts_truth(seqs, k)
        assert same(fa.kmer_counts(k), plain), k
        assert same(fa.kmer_counts(k, canonical=True), kmer_counts_truth(seqs, k, True)), k
        assert plain.sum() == sum(max(len(s) - k + 1, 0) for s in seqs) - _invalid_windows(seqs, k)
    for k in (1, 2, 5, 6):
        for canonical in (False, True):
            p = fa.kmer_profile(k, canonical=canonical)
            assert same(p, kmer_profile_truth(seqs, k, canonical)), (k, canonical)


def _invalid_windows(seqs, k):
    n = 0
    for s in seqs:
        bad = CODE[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)] > 3
        if bad.size >= k:
            c = np.concatenate([[0], np.cumsum(bad)])
            n += int(((c[k:] - c[:-k]) > 0).sum())
    return n


# ------------------------------------------------------------------ fixtures
@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz", "test.fq", "test.fq.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fasta_fixture(fx, fixture_files, fn):
    fa = fx.Fasta(fixture_files[fn])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    check_fasta(fa, seqs)
    # k = 1 against the composition
    comp = fa.composition
    c1 = fa.kmer_counts(1)
    up = "".join(seqs).upper()
    assert c1.tolist() == [up.count(c) for c in "ACGT"]
    if not any(c.islower() for s in seqs for c in s):
        assert c1.tolist() == [comp.get(c, 0) for c in "ACGT"]
    # ids: as ids, as names, with a repeat, empty
    sel = [5, 0, 17, 5]
    for k in (3, 6, 7, 11):
        want = kmer_counts_truth([seqs[i] for i in sel], k)
        assert same(fa.kmer_counts(k, ids=sel), want)
        assert same(fa.kmer_counts(k, ids=[names[i] for i in sel]), want)
        assert same(fa.kmer_counts(k, canonical=True, ids=np.array(sel)), kmer_counts_truth([seqs[i] for i in sel], k, True))
        z = fa.kmer_counts(k, ids=[])
        assert z.shape == (4 ** k,) and z.dtype == np.int64 and not z.any()
    p = fa.kmer_profile(4, ids=sel)
    assert same(p, kmer_profile_truth([seqs[i] for i in sel], 4)) and same(p[0], p[3])
    assert fa.kmer_profile(4, ids=[]).shape == (0, 256)
    assert same(fa.kmer_profile(3, ids=[names[2]]), kmer_profile_truth([seqs[2]], 3))
    # rows equal the single-record spectra, their sum the whole
    p = fa.kmer_profile(6, canonical=True)
    assert same(p.sum(axis=0), fa.kmer_counts(6, canonical=True))
    for i in (0, 7, len(fa) - 1):
        assert same(p[i], fa.kmer_counts(6, canonical=True, ids=[i]))
    with pytest.raises(KeyError):
        fa.kmer_counts(4, ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.kmer_counts(4, ids=[len(fa)])
    with pytest.raises(IndexError):
        fa.kmer_profile(4, ids=[-1])
    for bad in (0, 14, 4.0, True, "4"):
        with pytest.raises(ValueError):
            fa.kmer_counts(bad)
    for bad in (0, 7, 4.0, True):
        with pytest.raises(ValueError):
            fa.kmer_profile(bad)
    with pytest.raises(ValueError, match=str(len(fa) * 4096 * 8)):
        fa.kmer_profile(6, max_bytes=len(fa) * 4096 * 8 - 1)
    # the same answers from an index reopened from its .fxi (the table installed from the file)
    del fa
    fa2 = fx.Fasta(fixture_files[fn], uppercase=True)                      # uppercase= plays no part
    for k in (2, 6, 9):
        assert same(fa2.kmer_counts(k), kmer_counts_truth(seqs, k))
        assert same(fa2.kmer_counts(k, canonical=True, ids=sel), kmer_counts_truth([seqs[i] for i in sel], k, True))
    assert same(fa2.kmer_profile(3), kmer_profile_truth(seqs, 3))


# ------------------------------------------------------------------ generated layouts
def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def _layouts(tmp_path):
    rng = np.random.default_rng(4242)
    files = {}
    recs = []                                                 # irregular line lengths and blank lines inside records
    for i in range(8):
        s = _rand(rng, int(rng.integers(50, 1500)))
        lines, a = [], 0
        while a < len(s):
            n = int(rng.integers(1, 90))
            lines.append(s[a:a + n])
            a += n
            if rng.random() < 0.15:
                lines.append("")
            if rng.random() < 0.05:
                lines += ["", "", ""]
        recs.append(">irr%d\n" % i + "\n".join(lines) + "\n")
    files["irregular"] = _write(tmp_path / "irregular.fa", "".join(recs))
    recs = []                                                 # CRLF, spaces inside sequence lines, soft-masked lower case
    for i in range(6):
        s = _rand(rng, int(rng.integers(100, 900)), "ACGTacgt")
        lines = [s[a:a + 60] for a in range(0, len(s), 60)]
        lines = [ln[:10] + " " + ln[10:] if j % 3 == 1 else ln for j, ln in enumerate(lines)]
        recs.append(">crlf%d desc\r\n" % i + "\r\n".join(lines) + "\r\n")
    files["crlf"] = _write(tmp_path / "crlf.fa", "".join(recs))
    # N runs, bytes that are no IUPAC letter, empty records, a record shorter than k, an unterminated last line
    recs = [">n0\n" + "ACGTN" * 20 + "NNNNNNNNNNNNNNNNNNNN\n" + "GAA-TTC*GAATTC12RYKM\n", ">empty\n", ">short\nGA\n",
            ">mixed\n" + _rand(rng, 600, "ACGTACGTACGTNRYKM-*.") + "\n", ">empty2\n\n", ">u\nACGUACGU\n", ">last\nGAATTCAAAAGAATTC"]
    files["odd"] = _write(tmp_path / "odd.fa", "".join(recs))
    long = _rand(rng, 50_000)                                 # a record far longer than one lane's run; junctions
    recs = [">long\n" + "\n".join(long[a:a + 70] for a in range(0, len(long), 70)) + "\n",
            ">edge1\nGAATTCACGTACGTACGATTTTGAATTC\n", ">edge2\nTTCGGGAAAAAAAAACCCGA\n", ">poly\nAAAA\n", ">edge3\n" + "C" * 300 + "\n"]
    files["long"] = _write(tmp_path / "long.fa", "".join(recs))
    return files


def test_generated_layouts(fx, tmp_path):
    for name, path in _layouts(tmp_path).items():
        fa = fx.Fasta(path)
        seqs = [fa[i].seq for i in range(len(fa))]
        check_fasta(fa, seqs, ks=(1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13))
        assert same(fa.kmer_counts(7, ids=[len(fa) - 1, 0]), kmer_counts_truth([seqs[-1], seqs[0]], 7))


def test_junction(fx, tmp_path):
    """The k-mer made of the tail of one record and the head of the next -- a newline and a header apart in the stream -- is
    not counted."""
    fa = fx.Fasta(_write(tmp_path / "j.fa", ">a\nAAAAAAAC\n>b\nGGGGGGGG\n>c\nTTTT"))
    for k in (2, 4, 7, 8):
        c = fa.kmer_counts(k)
        assert c.sum() == 2 * (8 - k + 1) + max(4 - k + 1, 0)
        for cut in range(1, k):
            junction = ("AAAAAAAC"[-cut:] + "GGGGGGGG"[:k - cut])
            code = sum("ACGT".index(ch) * 4 ** (k - 1 - j) for j, ch in enumerate(junction))
            assert c[code] == 0, (k, junction)
    assert same(fa.kmer_profile(4), kmer_profile_truth(["AAAAAAAC", "GGGGGGGG", "TTTT"], 4))


@pytest.mark.parametrize("width", [0, 61, 255, 256, 17])
def test_run_boundaries(fx, tmp_path, width):
    """Records whose every 256-byte block boundary falls inside a window (no invalid byte anywhere); with lines of 255 or 256
    columns a newline sits at or next to every boundary, with 17 columns the 16 bytes in front of a run hold one."""
    rng = np.random.default_rng(77 + width)
    recs, seqs = [], []
    for i, n in enumerate((3000, 255, 256, 257, 511, 513, 1, 12, 13, 5000)):
        s = _rand(rng, n)
        seqs.append(s)
        body = s if width == 0 else "\n".join(s[a:a + width] for a in range(0, n, width))
        recs.append(">r%d%s\n%s\n" % (i, "x" * int(rng.integers(0, 40)), body))
    fa = fx.Fasta(_write(tmp_path / "b.fa", "".join(recs)))
    assert [fa[i].seq for i in range(len(fa))] == seqs
    for k in (1, 2, 6, 7, 12, 13):
        assert same(fa.kmer_counts(k), kmer_counts_truth(seqs, k)), k
        assert same(fa.kmer_counts(k, canonical=True), kmer_counts_truth(seqs, k, True)), k
    for k in (1, 3, 6):
        assert same(fa.kmer_profile(k, canonical=True), kmer_profile_truth(seqs, k, True)), k


def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: the index counts two bytes off every
    line, so slen is smaller than the number of kept bytes and `seq` stops there -- no window may reach past that cut."""
    rng = np.random.default_rng(55)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 12, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append(60 * n_lines)
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert [len(s) for s in seqs] == [len(fa[i]) for i in range(len(fa))]
    assert any(len(s) < n for s, n in zip(seqs, kept)), "no record is cut: the case is not exercised"
    check_fasta(fa, seqs, ks=(1, 2, 5, 6, 7, 13))
    assert same(fa.kmer_counts(8, ids=[4, 1, 4]), kmer_counts_truth([seqs[4], seqs[1], seqs[4]], 8))
    assert same(fa.kmer_profile(5, ids=[4, 1, 4]), kmer_profile_truth([seqs[4], seqs[1], seqs[4]], 5))


def test_low_complexity(fx, tmp_path):
    """Single-letter and dinucleotide runs: all lanes of a wave add to one or two counters."""
    seqs = ["A" * 1_000_000, "AC" * 500_000, "N" * 100_000, "ACG" * 100_000, "ACGT" * 50_000, "T" * 300 + "n" * 5 + "GGGG" * 400]
    text = "".join(">lc%d\n%s\n" % (i, "\n".join(s[a:a + 80] for a in range(0, len(s), 80))) for i, s in enumerate(seqs))
    fa = fx.Fasta(_write(tmp_path / "lc.fa", text))
    assert len(fa) == len(seqs) and [len(fa[i]) for i in range(len(fa))] == [len(s) for s in seqs]
    for k in range(1, 14):
        for canonical in (False, True):
            assert same(fa.kmer_counts(k, canonical=canonical), kmer_counts_truth(seqs, k, canonical)), (k, canonical)
    for k in SMALL_KS:
        assert same(fa.kmer_profile(k), kmer_profile_truth(seqs, k)), k
    c = fa.kmer_counts(13, ids=[0])
    assert c[0] == 1_000_000 - 12 and c.sum() == c[0]
    assert not fa.kmer_counts(9, ids=[2]).any()


def test_many_short_records(fx, tmp_path):
    """10^5 records of 20-300 bases: workgroups that span many records (kmer_profile adds to the rows directly)."""
    rng = np.random.default_rng(99)
    n = 100_000
    lens = rng.integers(20, 301, n).astype(np.int64)
    lens[::977] = 0                                            # some empty records
    lens[5::1013] = 3
    flat = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, int(lens.sum()), p=[.2475, .2475, .2475, .2475, .01])]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    parts = []
    for i in range(n):
        parts.append(b">s%d\n" % i)
        if lens[i]:
            parts.append(flat[starts[i]:starts[i] + lens[i]].tobytes())
            parts.append(b"\n")
    fa = fx.Fasta(_write(tmp_path / "short.fa", b"".join(parts)))
    assert len(fa) == n
    for k in (1, 4, 6, 7, 11):
        for canonical in (False, True):
            assert same(fa.kmer_counts(k, canonical=canonical), flat_counts(flat, starts, lens, k, canonical)), (k, canonical)
    for k in (2, 4):
        # rows by numpy: (record, code) of every valid window that lies inside its record
        m = flat.size - k + 1
        c = CODE[flat]
        code, bad = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=bool)
        for j in range(k):
            bad |= c[j:j + m] > 3
            code = code * 4 + (c[j:j + m] & 3)
        pos = np.arange(m, dtype=np.int64)
        rec = np.searchsorted(starts, pos, side="right") - 1
        ok = ~bad & (pos + k <= starts[rec] + lens[rec])
        want = np.bincount(rec[ok] * 4 ** k + code[ok], minlength=n * 4 ** k).reshape(n, 4 ** k)
        got = fa.kmer_profile(k)
        assert same(got, want), k
        assert same(got.sum(axis=0), fa.kmer_counts(k))
    sel = rng.integers(0, n, 5000)
    want = kmer_profile_truth([flat[starts[i]:starts[i] + lens[i]] for i in sel], 3)
    assert same(fa.kmer_profile(3, ids=sel), want)
    assert same(fa.kmer_counts(8, ids=sel), flat_counts(np.concatenate([flat[starts[i]:starts[i] + lens[i]] for i in sel]),
                                                        np.concatenate([[0], np.cumsum(lens[sel])[:-1]]), lens[sel], 8))


# ------------------------------------------------------------------ FASTQ
def check_fastq(fq, seqs, ks=KS):
    for k in ks:
        assert same(fq.kmer_counts(k), kmer_counts_truth(seqs, k)), k
        assert same(fq.kmer_counts(k, canonical=True), kmer_counts_truth(seqs, k, True)), k


@pytest.mark.parametrize("fn", ["test.fq", "test.fq.gz"])
def test_fastq_fixture(fx, fixture_files, fn):
    fq = fx.Fastq(fixture_files[fn])
    seqs = [fq[i].seq for i in range(len(fq))]
    check_fastq(fq, seqs)
    sel = [7, 0, 799, 7]
    for k in (2, 6, 7, 11):
        assert same(fq.kmer_counts(k, ids=sel), kmer_counts_truth([seqs[i] for i in sel], k))
        assert not fq.kmer_counts(k, ids=[]).any()
    # the intervals of trim, the ids of select
    keep = fq.select(min_mean_qual=20, max_other=0)
    assert 0 < keep.size <= len(fq)
    iv = fq.trim(ids=keep, clip_front=3, front_qual=25, window=(4, 28), tail_qual=25)
    cut = [seqs[i][a:b] for i, a, b in zip(keep.tolist(), iv["start"].tolist(), iv["end"].tolist())]
    assert any(len(c) < 150 for c in cut)
    for k in (1, 4, 6, 7, 11, 13):
        for canonical in (False, True):
            got = fq.kmer_counts(k, canonical=canonical, ids=keep, start=iv["start"], end=iv["end"])
            assert same(got, kmer_counts_truth(cut, k, canonical)), (k, canonical)
    iv = fq.trim(front_qual=30, tail_qual=30)
    cut = [s[a:b] for s, a, b in zip(seqs, iv["start"].tolist(), iv["end"].tolist())]
    assert same(fq.kmer_counts(5, start=iv["start"], end=iv["end"]), kmer_counts_truth(cut, 5))
    # a bad interval or id: what records raises
    n = len(fq)
    for s, e in (([0] * (n - 1) + [5], [150] * (n - 1) + [4]), ([0] * n, [151] + [150] * (n - 1)), ([-1] + [0] * (n - 1), [150] * n)):
        with pytest.raises(ValueError, match="lies outside its read"):
            fq.records(start=s, end=e)
        with pytest.raises(ValueError, match="lies outside its read"):
            fq.kmer_counts(4, start=s, end=e)
    with pytest.raises(ValueError):
        fq.kmer_counts(4, start=[0] * n)
    with pytest.raises(ValueError):
        fq.kmer_counts(4, ids=[1, 2], start=[0], end=[1])
    with pytest.raises(IndexError):
        fq.kmer_counts(4, ids=[n])
    for bad in (0, 14, 4.0, True):
        with pytest.raises(ValueError):
            fq.kmer_counts(bad)


def test_fastq_read_lengths(fx, tmp_path):
    """Reads of length 0, below k, exactly k, around the 16-byte pieces, and beyond 1024 bases; N and lower case inside."""
    rng = np.random.default_rng(123)
    lens = [0, 1, 5, 6, 7, 12, 13, 14, 15, 16, 17, 31, 32, 33, 150, 151, 1023, 1024, 1025, 3000, 40, 0, 2047, 13, 160]
    parts, seqs = [], []
    for i, L in enumerate(lens):
        s = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.choice(9, L, p=[.22, .22, .22, .22, .02, .025, .025, .025, .025])]
        seqs.append(s.tobytes().decode())
        parts.append(b"@r%d\n" % i + s.tobytes() + b"\n+\n" + b"I" * L + b"\n")
    p = tmp_path / "lens.fq"
    p.write_bytes(b"".join(parts))
    fq = fx.Fastq(str(p))
    assert len(fq) == len(lens) and [fq[i].seq for i in range(len(fq))] == seqs
    check_fastq(fq, seqs, ks=(1, 2, 6, 7, 12, 13))
    # intervals that begin and end anywhere, including empty ones and ones shorter than k
    for rep in range(4):
        a = np.array([int(rng.integers(0, L + 1)) for L in lens], dtype=np.int64)
        b = np.array([int(rng.integers(x, L + 1)) for x, L in zip(a, lens)], dtype=np.int64)
        cut = [s[x:y] for s, x, y in zip(seqs, a, b)]
        for k in (1, 3, 6, 7, 13):
            assert same(fq.kmer_counts(k, start=a, end=b), kmer_counts_truth(cut, k)), (rep, k)
            assert same(fq.kmer_counts(k, canonical=True, start=a, end=b), kmer_counts_truth(cut, k, True)), (rep, k)
    ids = np.array([19, 19, 3, 22, 0], dtype=np.int64)
    a = np.array([5, 2990, 0, 17, 0], dtype=np.int64)
    b = np.array([2999, 3000, 6, 2047, 0], dtype=np.int64)
    cut = [seqs[i][x:y] for i, x, y in zip(ids, a, b)]
    for k in (4, 11):
        assert same(fq.kmer_counts(k, ids=ids, start=a, end=b), kmer_counts_truth(cut, k))


def test_c_level_states(fx):
    """Before the build: FX_ESTATE; k out of range and unknown flags: FX_EINVAL; a bad id or interval: FX_ERANGE with its
    position; a byte-range shard: FX_EINVAL."""
    from pyfastx_amd import _lib
    raw = open(os.path.join(DATA, "test.fa"), "rb").read()
    b = _lib.Blob.from_bytes(raw, device=0)
    with pytest.raises(_lib.FxError) as e:
        b.fasta_kmers(4)
    assert e.value.code == _lib.FX_ESTATE
    n = b.fasta_build().n_seq
    assert b.fasta_kmers(2).sum() > 0 and b.fasta_kmers(2, per_record=True).shape == (n, 16)
    for call in (lambda: b.fasta_kmers(0), lambda: b.fasta_kmers(14), lambda: b.fasta_kmers(7, per_record=True)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    with pytest.raises(_lib.FxError) as e:
        b.fasta_kmers(4, ids=[0, 1, n])
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    rawq = open(os.path.join(DATA, "test.fq"), "rb").read()
    q = _lib.Blob.from_bytes(rawq, device=0)
    with pytest.raises(_lib.FxError) as e:
        q.fastq_kmers(4)
    assert e.value.code == _lib.FX_ESTATE
    q.fastq_build()
    assert q.fastq_kmers(1).sum() > 0
    for call in (lambda: q.fastq_kmers(0), lambda: q.fastq_kmers(14), lambda: q.fastq_kmers(4, start=[0] * 800)):
        with pytest.raises(_lib.FxError) as e:
            call()
        assert e.value.code == _lib.FX_EINVAL
    for ids, s, e_, where in (([3, 900], None, None, 1), ([1, 2, 3], [0, 0, 5], [150, 151, 4], 1), ([1, 2, 3], [0, 0, -1], [150, 150, 4], 2)):
        with pytest.raises(_lib.FxError) as e:
            q.fastq_kmers(4, ids=ids, start=s, end=e_)
        assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == where
    off = [i for i, c in enumerate(rawq[:4096]) if c == 10][3] + 1         # where the second record begins
    q = _lib.Blob.from_bytes(rawq[off:], device=0)
    q.set_shard(off, 10, True)
    assert q.fastq_build().n_reads > 0
    with pytest.raises(_lib.FxError) as e:
        q.fastq_kmers(4)
    assert e.value.code == _lib.FX_EINVAL


def test_sharded_raises(fx, fixture_files, monkeypatch):
    """Byte-range shards and windows carry no halo for a window across a cut: refused by all three methods.  The objects are
    made to report themselves sharded, as a multi-device or windowed one does."""
    fa = fx.Fasta(fixture_files["test.fa"])
    fq = fx.Fastq(fixture_files["test.fq"])
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    monkeypatch.setattr(type(fq), "_sharded", property(lambda self: True))
    for call in (lambda: fa.kmer_counts(4), lambda: fa.kmer_profile(4), lambda: fq.kmer_counts(4), lambda: fa.kmer_counts(4, ids=[0])):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------ scale
def test_synthetic_genome_200mbp(fx):
    import torch
    from pyfastx_amd import _lib, kmer, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=200_000_000)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
    s = b.fasta_build()
    assert s.n_seq == len(plan["slen"])
    flat = flat_t.cpu().numpy()
    del flat_t
    for k in (4, 11, 13):
        want = flat_counts(flat, flat_start, plan["slen"], k)
        assert want.sum() > 150_000_000
        assert same(kmer.fasta_counts_blob(b, k), want), k
        assert same(kmer.fasta_counts_blob(b, k, canonical=True), fold(want, k)), k
    sel = np.array([3, 0, 3], dtype=np.int64)
    rows = kmer.fasta_profile_blob(b, 4, False, sel, s.n_seq, 1 << 30)
    for j, r in enumerate(sel):
        a = int(flat_start[r])
        n = int(plan["slen"][r])
        assert same(rows[j], flat_counts(flat[a:a + n], [0], [n], 4)), j
    del b, blob_t


def test_synthetic_reads_2m(fx):
    import torch
    from pyfastx_amd import _lib, kmer, synth
    dev = torch.device("cuda", 0)
    n, rlen = 2_000_000, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    rec, hl = int(cols["rec"]), int(cols["soff"][0])
    bases = blob_t[:n * rec].view(n, rec)[:, hl:hl + rlen].cpu().numpy()
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(cols["n_bytes"]), device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    flat = np.ascontiguousarray(bases).reshape(-1)
    starts = np.arange(n, dtype=np.int64) * rlen
    lens = np.full(n, rlen, dtype=np.int64)
    for k in (4, 11):
        want = flat_counts(flat, starts, lens, k)
        assert same(kmer.fastq_counts_blob(b, n, k), want), k
        assert same(kmer.fastq_counts_blob(b, n, k, canonical=True), fold(want, k)), k
    # a gather with intervals
    rng = np.random.default_rng(3)
    ids = rng.integers(0, n, 300_000).astype(np.int64)
    a = rng.integers(0, 60, ids.size).astype(np.int64)
    e = a + rng.integers(0, 91, ids.size)
    cutlen = e - a
    idx = np.repeat(ids * rlen + a - np.concatenate([[0], np.cumsum(cutlen)[:-1]]), cutlen) + np.arange(int(cutlen.sum()))
    want = flat_counts(flat[idx], np.concatenate([[0], np.cumsum(cutlen)[:-1]]), cutlen, 11)
    assert same(kmer.fastq_counts_blob(b, n, 11, ids=ids, start=a, end=e), want)
    del b, blob_t
