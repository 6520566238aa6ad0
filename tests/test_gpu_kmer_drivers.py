"""-m gpu: the host choreography of the k-mer family on the resident streams, in the manner of test_gpu_fastq_drivers.py: the
spectra (fx_fasta_kmers), the sketches (fx_fasta_sketch, fx_fastq_sketch) and what all seven FASTA entries that walk the runs
of the selected records (fx_fasta_search, _pwm_scan, _minimizers, _kmers, _kmer_table, _kmer_hits, _sketch) and the seven FASTQ
entries of the family share and no result test looks at: which kernels a call launches and under which timing id (prof_read),
the exits -- a table that was never built, a byte-range shard, an id outside the table, an empty selection, a selection of
empty records -- with the code, the message and first_bad they leave, and which of two failing checks answers.

The launch counts are read off the host code: a scan that writes its offsets out is three launches under its id (chunk sums,
top, apply), one whose offsets the next kernel applies itself is two.  A spectrum is the run plan and the kept-byte scan under
k_kmer_scan (6), one count pass, one fix.  A sketch that keeps every key (size = 0) is one round: the letters, the thresholds,
two scans and the fix under k_sk_scan (9; the FASTQ form has the first two alone), one count, one emit, one sort, and under
k_sk_reduce the head scan (2), its compaction, the bounds, the decision, the take scan (2), its compaction and the offsets
(3): 11.  The FASTA form plans its runs under k_search_scan (3); FASTQ intervals are checked once under k_kmer_scan."""
import ctypes as C

import numpy as np
import pytest

from kmer_screen_truth import hits_truth
from kmer_table_truth import table_truth
from kmer_truth import kmer_counts_truth, kmer_profile_truth
from sketch_truth import fasta_sets, fastq_set

pytestmark = pytest.mark.gpu

N = 48
LONG = 20                                                                # the read above 1024 bases
EMPTY = 2                                                                # the record with no bases
LDS_K = 6                                                                # KMER_LDS_K: above it the spectrum is counted in global memory
SK_K = 5
SK_TOP = 4 ** SK_K                                                       # max_key that keeps every key
KMER = {"k_kmer_scan": 6, "k_kmer_fasta": 1, "k_kmer_fix": 1}
SK_REST = {"k_sk_count": 1, "k_sk_emit": 1, "k_sk_sort": 1, "k_sk_reduce": 11}


def _fasta_seqs():
    rng = np.random.default_rng(31)
    big = "".join(rng.choice(list("ACGT"), 700))
    return [big, "ACGTACGTAC", "", "ACGGTCATTGACCANGTTACGGATCCAT"]


def _fasta():
    big, ten, none, with_n = _fasta_seqs()
    return (">big\n" + "".join(big[k:k + 60] + "\n" for k in range(0, 700, 60)) + ">ten\n" + ten + "\n>none\n>with_n\n" + with_n + "\n").encode()


def _reads():
    rng = np.random.default_rng(49)
    L = [1, 2, 5, 6, 31, 32, 33, 64, 65, 150] + [int(x) for x in rng.integers(20, 201, N - 10)]
    L[LONG] = 1100
    return ["".join(rng.choice(list("ACGT"), n)) for n in L]


def _fastq():
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(_reads())).encode()


@pytest.fixture(scope="module")
def lib():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def fasta(lib):
    b = lib.Blob.from_bytes(_fasta(), device=0)
    assert b.fasta_build().n_seq == 4
    b.prof_enable(1)
    return b


@pytest.fixture(scope="module")
def fastq(lib):
    b = lib.Blob.from_bytes(_fastq(), device=0)
    assert b.fastq_build().n_reads == N
    b.prof_enable(1)
    return b


@pytest.fixture(scope="module")
def unbuilt(lib):
    """(a FASTA stream, a FASTQ stream) whose tables were never built"""
    a, q = lib.Blob.from_bytes(_fasta(), device=0), lib.Blob.from_bytes(_fastq(), device=0)
    a.prof_enable(1)
    q.prof_enable(1)
    return a, q


@pytest.fixture(scope="module")
def shard(lib):
    raw = _fasta()
    off = raw.index(b">ten")
    b = lib.Blob.from_bytes(raw[off:], device=0)
    b.set_shard(off, 10, True)
    assert b.fasta_build().n_seq == 3
    b.prof_enable(1)
    return b


@pytest.fixture(scope="module")
def kset(lib, fasta):
    return lib.KmerSet(fasta, 8, False, table_truth(["ACGTACGTAC"], 8)[0])


def _launches(b, call):
    b.prof_reset()
    out = call()
    return out, {k: n for k, (_, n) in b.prof_read().items()}


def _fails(lib, b, call):
    """-> (the FxError of the call, its launches); str(e) is what fx_last_error() holds"""
    b.prof_reset()
    with pytest.raises(lib.FxError) as e:
        call()
    assert str(e.value) == lib.lib().fx_last_error().decode()
    return e.value, {k: n for k, (_, n) in b.prof_read().items()}


def _sets(obj):
    off, keys = obj.read()
    return [keys[off[i]:off[i + 1]].tolist() for i in range(obj.n_sets)]


MAT = np.full((6, 4), -10, dtype=np.int32)


def _fasta_entries(lib, b, kset, ids=None, k=4):
    """The seven entries on blob b: (name, the call, the noun of its shard message, whether it reports first_bad)."""
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    return (("search", lambda: b.fasta_search(b"ACGT", b"ACGT", both, ids=ids, cap=10000), "hits", False),
            ("pwm", lambda: b.fasta_pwm_scan(MAT, both, -60, ids=ids, cap=10000), "hits", False),
            ("minimizers", lambda: b.fasta_minimizers(k, 4, lib.FX_MZ_CANONICAL, ids=ids, cap=10000), "windows", False),
            ("kmers", lambda: b.fasta_kmers(k, ids=ids), "windows", True),
            ("kmer_table", lambda: b.fasta_kmer_table(k, ids=ids), "windows", True),
            ("kmer_hits", lambda: b.fasta_kmer_hits(kset, ids=ids), "windows", True),
            ("sketch", lambda: b.fasta_sketch(k if k else 0, lib.FX_SK_CANONICAL, ids=ids, max_key=4 ** max(k, 1)), "windows", False))


def _fastq_entries(lib, b, kset, k=4, **q):
    """The seven entries on blob b (kset: a set of the same device)."""
    return (("kmers", lambda: b.fastq_kmers(k, **q)),
            ("kmer_table", lambda: b.fastq_kmer_table(k, **q)),
            ("kmer_hits", lambda: b.fastq_kmer_hits(kset, **q)),
            ("kmer_screen", lambda: b.fastq_kmer_screen(kset, **q)),
            ("sketch", lambda: b.fastq_sketch(k, lib.FX_SK_CANONICAL, max_key=4 ** max(k, 1), **q)),
            ("dup_first", lambda: b.fastq_dup_first(**q)),
            ("dedup", lambda: b.fastq_dedup(**q)))


def test_text_is_what_the_cases_need():
    raw, seqs = _fasta(), _fasta_seqs()
    assert [len(s) for s in seqs] == [700, 10, 0, 28] and "N" in seqs[3] and not set("".join(seqs[:2])) - set("ACGT")
    lines = raw.split(b"\n>")[0].split(b"\n")[1:]
    assert [len(x) for x in lines] == [60] * 11 + [40] and b">none\n>with_n\n" in raw and raw.count(b">") == 4
    assert (raw.index(b">ten") - 1) // 256 - (raw.index(b"\n") + 1) // 256 + 1 >= 3       # the 256-byte runs of the first record
    reads = _reads()
    L = [len(s) for s in reads]
    assert len(reads) == N and L[0] == 1 and L[LONG] > 1024 and max(L[:LONG] + L[LONG + 1:]) <= 200 and not set("".join(reads)) - set("ACGT")
    assert _fastq().count(b"\n") == 4 * N


# ------------------------------------------------------------------ the launches of every call, and what they compute
def test_fasta_spectra(fasta):
    seqs = _fasta_seqs()
    for k in (4, LDS_K + 1):
        got, n = _launches(fasta, lambda: fasta.fasta_kmers(k))
        assert n == KMER and got.dtype == np.int64 and np.array_equal(got, kmer_counts_truth(seqs, k))
    got, n = _launches(fasta, lambda: fasta.fasta_kmers(4, canonical=True, ids=[3, 0, 3]))
    assert n == KMER and np.array_equal(got, kmer_counts_truth([seqs[3], seqs[0], seqs[3]], 4, True))
    got, n = _launches(fasta, lambda: fasta.fasta_kmers(3, per_record=True))
    assert n == KMER and got.dtype == np.int64 and got.shape == (4, 64) and np.array_equal(got, kmer_profile_truth(seqs, 3))
    assert got[EMPTY].sum() == 0 and got[1].sum() == 8


def test_fasta_sketches(lib, fasta):
    seqs = _fasta_seqs()
    want = dict(SK_REST, k_search_scan=3, k_sk_scan=9)
    (o, rounds), n = _launches(fasta, lambda: fasta.fasta_sketch(SK_K, lib.FX_SK_CANONICAL, max_key=SK_TOP))
    assert n == want and rounds == 1 and o.n_sets == 4 and o.flags == lib.FX_SK_CANONICAL
    assert _sets(o) == fasta_sets(seqs, SK_K, True, SK_TOP) and _sets(o)[EMPTY] == [] and len(_sets(o)[0]) > 100
    (o, rounds), n = _launches(fasta, lambda: fasta.fasta_sketch(SK_K, lib.FX_SK_POOLED, ids=[0, 3], max_key=SK_TOP))
    assert n == want and rounds == 1 and o.n_sets == 1 and o.flags == lib.FX_SK_POOLED
    assert _sets(o) == fasta_sets(seqs, SK_K, False, SK_TOP, ids=[0, 3], pooled=True)


def test_fastq_sketches(lib, fastq):
    reads = _reads()
    want = dict(SK_REST, k_sk_scan=2)
    (o, rounds), n = _launches(fastq, lambda: fastq.fastq_sketch(SK_K, lib.FX_SK_CANONICAL, max_key=SK_TOP))
    assert n == want and rounds == 1 and o.n_sets == 1 and o.flags == lib.FX_SK_CANONICAL | lib.FX_SK_POOLED
    assert _sets(o) == [fastq_set(reads, SK_K, True, SK_TOP)] and o.n_keys > 100
    ids = np.array([LONG, 0, 9, 7], dtype=np.int64)
    start, end = np.array([1000, 0, 3, 64]), np.array([1100, 1, 150, 64])
    (o, rounds), n = _launches(fastq, lambda: fastq.fastq_sketch(SK_K, 0, ids=ids, start=start, end=end, max_key=SK_TOP))
    assert n == dict(want, k_kmer_scan=1) and rounds == 1
    assert _sets(o) == [fastq_set(reads, SK_K, False, SK_TOP, ids=ids, start=start, end=end)] and o.n_keys > 50


# ------------------------------------------------------------------ the exits of the FASTA entries
def test_fasta_table_never_built(lib, unbuilt, kset):
    for name, call, _, has_bad in _fasta_entries(lib, unbuilt[0], kset):
        e, n = _fails(lib, unbuilt[0], call)
        assert (e.code, str(e), n) == (lib.FX_ESTATE, "fx_fasta_build has not run", {}), name
        assert not has_bad or e.first_bad == -1, name


def test_fasta_byte_range_shard(lib, shard, kset):
    for name, call, noun, has_bad in _fasta_entries(lib, shard, kset):
        e, n = _fails(lib, shard, call)
        assert (e.code, str(e), n) == (lib.FX_EINVAL, "a byte-range shard carries no halo for %s across its cuts" % noun, {}), name
        assert not has_bad or e.first_bad == -1, name


def test_fasta_id_outside_the_table(lib, fasta, kset):
    for name, call, _, has_bad in _fasta_entries(lib, fasta, kset, ids=[0, 1, 4, -1]):
        e, n = _fails(lib, fasta, call)
        assert (e.code, str(e), n) == (lib.FX_ERANGE, "record id 4 outside the table", {}), name
        assert not has_bad or e.first_bad == 2, name


def _fasta_zero(lib, fasta, kset, ids, rows, launches):
    """what the seven entries give where no record has a base: `rows` rows of nothing"""
    e = dict((name, call) for name, call, _, _ in _fasta_entries(lib, fasta, kset, ids=np.array(ids, dtype=np.int64)))
    for name in ("search", "pwm", "minimizers"):
        out, n = _launches(fasta, e[name])
        assert out == (0, None, None) and n == launches(name), name
    got, n = _launches(fasta, e["kmers"])
    assert n == launches("kmers") and got.dtype == np.int64 and got.tolist() == [0] * 256
    (c, cnt, nw, parts), n = _launches(fasta, e["kmer_table"])
    assert n == launches("kmer_table") and c.dtype == cnt.dtype == np.int64 and c.size == cnt.size == 0 and (nw, parts) == (0, 0)
    (w, h), n = _launches(fasta, e["kmer_hits"])
    assert n == launches("kmer_hits") and w.dtype == h.dtype == np.int64 and w.tolist() == h.tolist() == [0] * rows
    (o, rounds), n = _launches(fasta, e["sketch"])
    assert n == launches("sketch") and (o.n_sets, o.n_keys, rounds) == (rows, 0, 0) and o.read()[0].tolist() == [0] * (rows + 1)
    got, n = _launches(fasta, lambda: fasta.fasta_kmers(3, ids=np.array(ids, dtype=np.int64), per_record=True))
    assert n == launches("kmers") and got.dtype == np.int64 and got.shape == (rows, 64) and not got.any()


def test_fasta_empty_selection(lib, fasta, kset):
    _fasta_zero(lib, fasta, kset, [], 0, lambda name: {})


def test_fasta_selection_of_empty_records(lib, fasta, kset):
    """the run plan alone, under the entry's scan id; fx_fasta_kmer_hits still splits its zeroed accumulators"""
    def launches(name):
        if name in ("search", "pwm", "minimizers", "sketch"):
            return {"k_search_scan": 3}
        return {"k_kmer_scan": 3, "k_ks_fasta": 1} if name == "kmer_hits" else {"k_kmer_scan": 3}
    _fasta_zero(lib, fasta, kset, [EMPTY], 1, launches)


# ------------------------------------------------------------------ which of two failing checks answers
def test_fasta_precedence(lib, fasta, shard, unbuilt, kset):
    a = unbuilt[0]
    # the numbers of an entry against the state of the handle: the spectra and the table look at the handle first
    for b, code, text in ((a, lib.FX_ESTATE, "fx_fasta_build has not run"),
                          (shard, lib.FX_EINVAL, "a byte-range shard carries no halo for windows across its cuts")):
        for call in (lambda: b.fasta_kmers(0), lambda: b.fasta_kmers(LDS_K + 1, per_record=True), lambda: b.fasta_kmer_table(0),
                     lambda: b.fasta_kmer_table(32), lambda: b.fasta_kmer_table(8, min_count=0)):
            e, n = _fails(lib, b, call)
            assert (e.code, str(e), e.first_bad, n) == (code, text, -1, {})
    # ... the minimizers, the sketch, the search and the matrix at their numbers
    for call, text in ((lambda: a.fasta_minimizers(0, 4, 0, cap=10), "k = 0 outside 1..31"), (lambda: a.fasta_minimizers(5, 0, 0, cap=10), "w = 0 outside 1..32"),
                       (lambda: a.fasta_sketch(0, 0, max_key=1), "k = 0 outside 1..31"), (lambda: a.fasta_sketch(4, 0, max_key=257), "max_key 257 outside 1..4^4"),
                       (lambda: a.fasta_sketch(4, 0, max_key=256, oversample=-1), None),
                       (lambda: a.fasta_search(b"A" * 65, None, lib.FX_SEARCH_PLUS, cap=10), "pattern length 65 outside 1..64"),
                       (lambda: a.fasta_pwm_scan(np.zeros((65, 4), dtype=np.int32), lib.FX_SEARCH_PLUS, 0, cap=10), "matrix length 65 outside 1..64")):
        e, n = _fails(lib, a, call)
        assert e.code == lib.FX_EINVAL and n == {} and (text is None or str(e) == text)
    # on a built table the numbers answer before the ids do, and a letter that is no IUPAC code before the ids
    bad = [0, 9]
    for call, text in ((lambda: fasta.fasta_kmers(0, ids=bad), "k 0 outside 1..13"), (lambda: fasta.fasta_kmer_table(32, ids=bad), "k 32 outside 1..31"),
                       (lambda: fasta.fasta_kmers(LDS_K + 1, ids=bad, per_record=True), "k 7 outside 1..6"),
                       (lambda: fasta.fasta_search(b"AC!T", None, lib.FX_SEARCH_PLUS | lib.FX_SEARCH_DEGENERATE, ids=bad, cap=10), "a pattern letter is not an IUPAC code")):
        e, n = _fails(lib, fasta, call)
        assert (e.code, str(e), n) == (lib.FX_EINVAL, text, {})
        assert getattr(e, "first_bad", -1) == -1


def test_fastq_precedence(lib, fastq, unbuilt, kset):
    q = unbuilt[1]
    half = np.zeros(N, dtype=np.int64)
    # start without end answers before the handle is looked at, in all seven
    for b in (q, fastq):
        for name, call in _fastq_entries(lib, b, kset, start=half) + _fastq_entries(lib, b, kset, end=half):
            e, n = _fails(lib, b, call)
            assert (e.code, str(e), e.first_bad, n) == (lib.FX_EINVAL, "start and end come together", -1, {}), name
    for name, call in _fastq_entries(lib, q, kset):
        e, n = _fails(lib, q, call)
        assert (e.code, str(e), e.first_bad, n) == (lib.FX_ESTATE, "fx_fastq_build has not run", -1, {}), name
    # the numbers of an entry on a table that was never built: the handle answers, except where the numbers are looked at first
    for call in (lambda: q.fastq_kmers(0), lambda: q.fastq_kmers(14), lambda: q.fastq_kmer_table(0), lambda: q.fastq_kmer_table(8, min_count=0),
                 lambda: q.fastq_dup_first(hash_bits=65), lambda: q.fastq_dedup(hash_bits=-1), lambda: q.fastq_dedup(min_copies=0)):
        e, n = _fails(lib, q, call)
        assert (e.code, str(e), e.first_bad, n) == (lib.FX_ESTATE, "fx_fastq_build has not run", -1, {})
    for call, text in ((lambda: q.fastq_sketch(0, 0, max_key=1), "k = 0 outside 1..31"), (lambda: q.fastq_sketch(4, 4, max_key=1), "unknown flag bits 4"),
                       (lambda: q.fastq_sketch(4, 0, max_key=257), "max_key 257 outside 1..4^4"),
                       (lambda: q.fastq_kmer_screen(kset, min_hits=-1), "min_hits -1 below 0"),
                       (lambda: q.fastq_kmer_screen(kset, frac=(-1, 2)), "a ratio outside 0..10^9")):
        e, n = _fails(lib, q, call)
        assert (e.code, str(e), e.first_bad, n) == (lib.FX_EINVAL, text, -1, {})
    # the numbers of the sketch and of the screen even before start without end is refused
    for call, text in ((lambda: q.fastq_sketch(0, 0, start=half, max_key=1), "k = 0 outside 1..31"),
                       (lambda: q.fastq_kmer_screen(kset, start=half, min_hits=-1), "start and end come together")):
        e, n = _fails(lib, q, call)
        assert (e.code, str(e), n) == (lib.FX_EINVAL, text, {})
    # on a built table the numbers answer before the ids do
    bad = [0, N]
    for call, text in ((lambda: fastq.fastq_kmers(14, ids=bad), "k 14 outside 1..13"), (lambda: fastq.fastq_kmer_table(32, ids=bad), "k 32 outside 1..31"),
                       (lambda: fastq.fastq_dup_first(ids=bad, hash_bits=65), "hash_bits 65 outside 0..64"),
                       (lambda: fastq.fastq_dedup(ids=bad, min_copies=0), "min_copies 0 below 1")):
        e, n = _fails(lib, fastq, call)
        assert (e.code, str(e), e.first_bad, n) == (lib.FX_EINVAL, text, -1, {})


def test_fastq_id_counts(lib, fastq, unbuilt):
    """An id array with a negative count, and a count without an array: fx_fastq_sketch calls both a null id array, on an
    unbuilt handle too; the spectrum refuses the first and takes the second for every read."""
    L = lib.lib()
    ids = np.zeros(4, dtype=np.int64)
    for b in (fastq, unbuilt[1]):
        for p, n_ids in ((ids.ctypes.data, -1), (None, 3), (None, -1)):
            s, nr, bad = C.c_void_p(), C.c_int(0), C.c_int64(7)
            b.prof_reset()
            rc = L.fx_fastq_sketch(b._h, SK_K, 0, p, n_ids, None, None, SK_TOP, 0, 0, C.byref(s), C.byref(nr), C.byref(bad))
            assert (rc, L.fx_last_error().decode(), s.value, bad.value, b.prof_read()) == (lib.FX_EINVAL, "null id array", None, -1, {})
        p, bad = C.c_void_p(), C.c_int64(7)
        b.prof_reset()
        rc = L.fx_fastq_kmers(b._h, 4, 0, ids.ctypes.data, -1, None, None, C.byref(p), C.byref(bad))
        assert (rc, L.fx_last_error().decode(), p.value, bad.value, b.prof_read()) == (lib.FX_EINVAL, "negative id count", None, -1, {})
    p, bad = C.c_void_p(), C.c_int64(7)
    assert L.fx_fastq_kmers(fastq._h, 2, 0, None, 3, None, None, C.byref(p), C.byref(bad)) == 0
    assert np.array_equal(lib.pinned_array(p.value, 16, np.int64), kmer_counts_truth(_reads(), 2))


def test_fastq_sketch_exits(lib, fastq):
    e, n = _fails(lib, fastq, lambda: fastq.fastq_sketch(SK_K, 0, ids=[0, 1, N, -1], max_key=SK_TOP))
    assert (e.code, str(e), e.first_bad, n) == (lib.FX_ERANGE, "read id %d out of range" % N, 2, {})
    ids = np.arange(N - 1, -1, -1)
    L = np.array([len(s) for s in _reads()], dtype=np.int64)
    start, end = np.zeros(N, dtype=np.int64), L[ids].copy()
    end[3] += 1
    e, n = _fails(lib, fastq, lambda: fastq.fastq_sketch(SK_K, 0, ids=ids, start=start, end=end, max_key=SK_TOP))
    assert (e.code, str(e), e.first_bad, n) == (lib.FX_ERANGE, "the interval of query 3 lies outside its read", 3, {"k_kmer_scan": 1})
    (o, rounds), n = _launches(fastq, lambda: fastq.fastq_sketch(SK_K, 0, ids=np.zeros(0, dtype=np.int64), max_key=SK_TOP))
    assert n == {} and (o.n_sets, o.n_keys, rounds) == (1, 0, 0) and o.read()[0].tolist() == [0, 0]
