"""-m gpu: the host choreography of the entries on the resident FASTQ stream -- the per-read columns (fx_fastq_read_stats,
fx_fastq_trim, fx_fastq_pair_overlap, fx_fastq_demux), the passes that turn flags into ascending positions (fx_fastq_select,
fx_fastq_kmer_screen, fx_fastq_dedup), the variable-length records (fx_fastq_format_alloc, fx_fastq_pair_merge_alloc) and the
query batches with intervals (fx_fastq_kmers, fx_fastq_kmer_table, fx_fastq_kmer_hits, fx_fastq_dup_first) -- and of the two
FASTA entries that scan the kept bytes of the runs (fx_fasta_kmer_table, fx_fasta_kmer_hits).  What is pinned here is what the
entries share and no result test looks at: which kernels a call launches and under which timing id (prof_read), and the exits
-- an empty selection, an id outside the table, an interval or a diagonal outside its read, start without end -- with the
code, the message and first_bad they leave.  A few results are compared with plain Python on the same reads, so that a
driver which launches the right kernels on the wrong buffers does not pass.

The launch counts are read off the host code: a scan whose offsets the next kernel applies itself is two launches under its
id (chunk sums, top), one that writes its offsets out is three; a round of the duplicate search is six launches under
k_dd_verify (two scans of two, the rank, the verification) and seven where the group sizes are asked for."""
import numpy as np
import pytest

from kmer_screen_truth import hits_truth, screen_truth
from kmer_table_truth import table_truth
from kmer_truth import kmer_counts_truth

pytestmark = pytest.mark.gpu

N = 48
LONG = 20                                                                # the read above 1024 bases
BC = ("ACGTTGCA", "TTGACCAG")
DUPS = ((40, 13), (41, 17), (42, 19))                                    # exact copies: (copy, original)
RC_DUP = (43, 14)                                                        # read 43 is the reverse complement of read 14
NONE = -2**31                                                            # FX_PAIR_NONE


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _reads():
    """-> (mate 1, mate 2): lists of (sequence, quality) strings, N each."""
    rng = np.random.default_rng(48)

    def rand(n):
        return "".join(rng.choice(list("ACGT"), n))

    L = [1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 150, 199, 200, 1100] + [int(x) for x in rng.integers(20, 201, N - 21)]
    s1 = [rand(n) for n in L]
    for i in range(N):
        if L[i] >= 20 and i % 3:
            s1[i] = BC[i & 1] + s1[i][8:]
    s1[5] = s1[5][:3] + "N" + s1[5][4:]
    for c, o in DUPS:
        s1[c] = s1[o]
    s1[RC_DUP[0]] = _rc(s1[RC_DUP[1]])
    s2 = [_rc(s[-min(len(s), 60):]) if i % 2 == 0 else rand(int(rng.integers(1, 151))) for i, s in enumerate(s1)]

    def qual(n):
        return "".join(chr(33 + int(q)) for q in rng.integers(2, 41, n))

    return [(s, qual(len(s))) for s in s1], [(s, qual(len(s))) for s in s2]


def _text(rows, mate):
    return "".join("@r%d/%d\n%s\n+\n%s\n" % (i, mate, s, q) for i, (s, q) in enumerate(rows)).encode()


def _record(rows, i, a=0, b=None):
    s, q = rows[i]
    return ("@r%d/1\n%s\n+\n%s\n" % (i, s[a:b], q[a:b])).encode()


def _first(seqs, revcomp=False):
    seen, out = {}, []
    for i, s in enumerate(seqs):
        out.append(seen.setdefault(min(s, _rc(s)) if revcomp else s, i))
    return out


FASTA_SEQS = ("".join(np.random.default_rng(7).choice(list("ACGT"), 700)), "ACGTACGTAC")


def _fasta():
    big, small = FASTA_SEQS
    return (">big\n" + "".join(big[k:k + 60] + "\n" for k in range(0, 700, 60)) + ">small\n" + small + "\n").encode()


@pytest.fixture(scope="module")
def lib():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def reads():
    return _reads()


@pytest.fixture(scope="module")
def blob(lib, reads):
    b = lib.Blob.from_bytes(_text(reads[0], 1), device=0)
    assert b.fastq_build().n_reads == N
    b.prof_enable(1)
    return b


@pytest.fixture(scope="module")
def mate(lib, reads):
    b = lib.Blob.from_bytes(_text(reads[1], 2), device=0)
    assert b.fastq_build().n_reads == N
    return b


@pytest.fixture(scope="module")
def kset(lib, blob):
    return lib.KmerSet(blob, 8, False, table_truth([BC[0]], 8)[0])


@pytest.fixture(scope="module")
def fasta(lib):
    b = lib.Blob.from_bytes(_fasta(), device=0)
    assert b.fasta_build().n_seq == 2
    b.prof_enable(1)
    return b


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


def _seqs(reads):
    return [s for s, _ in reads[0]]


def _lens(reads):
    return np.array([len(s) for s, _ in reads[0]], dtype=np.int64)


def test_text_is_what_the_cases_need():
    m1, m2 = _reads()
    assert len(m1) == len(m2) == N
    L = [len(s) for s, _ in m1]
    assert L[0] == 1 and L[LONG] > 1024 and max(L[:LONG] + L[LONG + 1:]) <= 200 and {16, 17, 64, 65} <= set(L)
    assert all(len(s) == len(q) for s, q in m1 + m2) and all(33 <= ord(c) < 127 for _, q in m1 + m2 for c in q)
    seqs = [s for s, _ in m1]
    first = _first(seqs)
    assert sorted((i, f) for i, f in enumerate(first) if f != i) == sorted(DUPS)
    assert [(i, f) for i, f in enumerate(_first(seqs, True)) if f != first[i]] == [RC_DUP]
    assert sum(s.startswith(BC[0]) for s in seqs) >= 5 and sum(s.startswith(BC[1]) for s in seqs) >= 5
    assert sum(_rc(b) == a[-len(b):] for (a, _), (b, _) in zip(m1, m2)) >= N // 2
    assert sum(len(s) >= 100 for s in seqs) not in (0, N) and "N" in seqs[5]


# ------------------------------------------------------------------ the launches of every call, and what they compute
def test_column_entries(lib, blob, mate, reads):
    st, k = _launches(blob, lambda: blob.fastq_read_stats(low_qual=20))
    assert k == {"k_fq_read_stats": 1}
    dt = dict(length=np.int64, qsum=np.int64, qmin=np.int16, qmax=np.int16, n_low=np.int32, n_gc=np.int32, n_other=np.int32)
    assert {c: a.dtype for c, a in st.items()} == dt and all(a.size == N for a in st.values())
    for i in (0, 5, LONG):
        s, q = reads[0][i]
        d = [ord(c) - 33 for c in q]
        want = dict(length=len(s), qsum=sum(d), qmin=min(d), qmax=max(d), n_low=sum(x < 20 for x in d), n_gc=s.count("G") + s.count("C"),
                    n_other=len(s) - sum(s.count(c) for c in "ACGT"))
        assert {c: int(a[i]) for c, a in st.items()} == want, i
    (a, z), k = _launches(blob, lambda: blob.fastq_trim(adapter=b"AGATCGGAAGAGC", min_overlap=3, err=(1, 10), tail_qual=10))
    assert k == {"k_fq_trim": 1}
    assert a.dtype == z.dtype == np.int64 and a.size == z.size == N and (0 <= a).all() and (a <= z).all() and (z <= _lens(reads)).all()
    (qual, base, depth), k = _launches(blob, lambda: blob.fastq_cycle_hist(300))
    assert k == {"k_fq_cycle_hist": 1}
    assert depth.tolist() == [int((_lens(reads) > j).sum()) for j in range(300)] and (qual.sum(axis=1) == depth).all() and (base.sum(axis=1) == depth).all()
    ov, k = _launches(blob, lambda: blob.fastq_pair_overlap(mate, min_overlap=8))
    assert k == {"k_fp_overlap": 1}
    assert [ov[c].dtype for c in ("diag", "overlap", "mismatches", "end1", "end2")] == [np.int32] * 3 + [np.int64] * 2
    assert all(a.size == N for a in ov.values()) and (ov["diag"][[12, 16, 18, LONG]] != NONE).all()     # (mate 2 of an even pair overlaps)


def test_demux(lib, blob, reads):
    bc = np.array([list(b.encode()) for b in BC], dtype=np.uint8)
    want = [0 if s.startswith(BC[0]) else 1 if s.startswith(BC[1]) else -1 for s in _seqs(reads)]
    out, k = _launches(blob, lambda: blob.fastq_demux(bc, [0], [0], [8], [0], want_order=False))
    assert k == {"k_fq_demux": 1}
    assert [out[c].dtype for c in ("sample", "dist", "second", "counts")] == [np.int32] * 3 + [np.int64] and out["sample"].tolist() == want
    out, k = _launches(blob, lambda: blob.fastq_demux(bc, [0], [0], [8], [0], want_order=True))
    assert k == {"k_fq_demux": 1, "k_fq_demux_group": 1}
    assert out["sample"].tolist() == want and out["order"].dtype == np.int64 and sorted(out["order"].tolist()) == list(range(N))
    assert int(out["counts"].sum()) == N and out["bin_off"][-1] == N


def test_select(blob, reads):
    ids, k = _launches(blob, lambda: blob.fastq_select(min_len=100))
    assert k == {"k_fq_select": 1, "k_fq_select_scan": 2, "k_fq_select_emit": 1}
    assert ids.dtype == np.int64 and ids.tolist() == np.nonzero(_lens(reads) >= 100)[0].tolist()
    ids, k = _launches(blob, lambda: blob.fastq_select(min_len=5000))
    assert k == {"k_fq_select": 1, "k_fq_select_scan": 2}
    assert ids.dtype == np.int64 and ids.size == 0


def test_records(lib, blob, mate, reads):
    pick = [0, LONG, 13]
    (buf, offs, kept), k = _launches(blob, lambda: blob.fastq_format_alloc(ids=pick))
    assert k == {"k_fq_format_count": 1, "k_fq_format_scan": 3, "k_fq_format_emit": 1}
    want = [_record(reads[0], i) for i in pick]
    assert buf.dtype == np.uint8 and offs.dtype == np.int64 and kept == 3 and buf.tobytes() == b"".join(want)
    assert offs.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
    L = _lens(reads)
    (buf, offs, kept), k = _launches(blob, lambda: blob.fastq_format_alloc(start=L // 2, end=L, min_len=8))
    assert k == {"k_fq_format_count": 1, "k_fq_format_scan": 3, "k_fq_format_emit": 1}
    want = [_record(reads[0], i, int(L[i]) // 2) if L[i] - L[i] // 2 >= 8 else b"" for i in range(N)]
    assert kept == sum(1 for w in want if w) and buf.tobytes() == b"".join(want)
    (buf, offs, kept), k = _launches(blob, lambda: blob.fastq_format_alloc(min_len=5000))
    assert k == {"k_fq_format_count": 1, "k_fq_format_scan": 3}
    assert kept == 0 and buf.size == 0 and offs.tolist() == [0] * (N + 1)
    diag = blob.fastq_pair_overlap(mate, min_overlap=8)["diag"]
    (buf, offs, merged), k = _launches(blob, lambda: blob.fastq_pair_merge_alloc(mate, diag))
    assert k == {"k_fp_merge_count": 1, "k_fp_merge_scan": 3, "k_fp_merge_emit": 1}
    assert merged == int((diag != NONE).sum()) > 0 and offs.size == N + 1 and buf.size == offs[N]
    assert ((np.diff(offs) > 0) == (diag != NONE)).all() and buf[:7].tobytes().startswith(b"@r%d/1\n" % np.nonzero(diag != NONE)[0][0])


def test_query_batches(lib, blob, kset, reads):
    seqs, L, zero = _seqs(reads), _lens(reads), np.zeros(N, dtype=np.int64)
    want = kmer_counts_truth(seqs, 4)
    got, k = _launches(blob, lambda: blob.fastq_kmers(4))
    assert k == {"k_kmer_fastq": 1} and got.dtype == np.int64 and np.array_equal(got, want)
    got, k = _launches(blob, lambda: blob.fastq_kmers(4, start=zero, end=L))
    assert k == {"k_kmer_fastq": 1, "k_kmer_scan": 1} and np.array_equal(got, want)
    codes, counts = table_truth(seqs, 8)
    (c, n, nw, parts), k = _launches(blob, lambda: blob.fastq_kmer_table(8))
    assert "k_kmer_scan" not in k and k["k_kt_hist"] == 1 and k["k_kt_emit"] == parts == 1
    assert c.dtype == n.dtype == np.int64 and np.array_equal(c, codes) and np.array_equal(n, counts) and nw == int(counts.sum())
    (c, n, nw, parts), k2 = _launches(blob, lambda: blob.fastq_kmer_table(8, start=zero, end=L))
    assert k2 == dict(k, k_kmer_scan=1) and np.array_equal(c, codes) and np.array_equal(n, counts)
    want = hits_truth(seqs, 8, table_truth([BC[0]], 8)[0])
    (w, h), k = _launches(blob, lambda: blob.fastq_kmer_hits(kset))
    assert k == {"k_ks_fastq": 1} and w.dtype == h.dtype == np.int32 and np.array_equal(w, want[0]) and np.array_equal(h, want[1])
    (w, h), k = _launches(blob, lambda: blob.fastq_kmer_hits(kset, start=zero, end=L))
    assert k == {"k_ks_fastq": 1, "k_kmer_scan": 1} and np.array_equal(w, want[0]) and np.array_equal(h, want[1])
    pos, k = _launches(blob, lambda: blob.fastq_kmer_screen(kset))
    assert k == {"k_ks_fastq": 1, "k_ks_screen": 4}
    assert pos.dtype == np.int64 and pos.size > 0 and np.array_equal(pos, screen_truth(want[0], want[1], 1))
    pos, k = _launches(blob, lambda: blob.fastq_kmer_screen(kset, min_hits=10**6))
    assert k == {"k_ks_fastq": 1, "k_ks_screen": 3} and pos.dtype == np.int64 and pos.size == 0


def test_duplicates(blob, reads):
    seqs = _seqs(reads)
    first = _first(seqs)
    (f, groups, rounds), k = _launches(blob, lambda: blob.fastq_dup_first(hash_bits=0))
    assert k == {"k_dd_hash": 1, "k_dd_sort": 1, "k_dd_verify": 6}
    assert f.dtype == np.int64 and f.tolist() == first and groups == len(set(first)) and rounds == 1
    both = _first(seqs, True)
    size = np.bincount(both, minlength=N)
    (pos, copies, groups, rounds), k = _launches(blob, lambda: blob.fastq_dedup(revcomp=True, want_copies=True))
    assert k == {"k_dd_hash": 1, "k_dd_sort": 1, "k_dd_verify": 7, "k_dd_select": 5}
    assert pos.dtype == copies.dtype == np.int64 and pos.tolist() == sorted(set(both)) and copies.tolist() == size[pos].tolist()
    assert groups == pos.size and rounds == 1
    (pos, copies, _, _), k = _launches(blob, lambda: blob.fastq_dedup(revcomp=True, min_copies=2))
    assert k == {"k_dd_hash": 1, "k_dd_sort": 1, "k_dd_verify": 7, "k_dd_select": 4}
    assert copies is None and pos.tolist() == np.nonzero(size >= 2)[0].tolist() == [13, 14, 17, 19]
    (pos, copies, _, _), k = _launches(blob, lambda: blob.fastq_dedup(min_copies=100, want_copies=True))
    assert k == {"k_dd_hash": 1, "k_dd_sort": 1, "k_dd_verify": 7, "k_dd_select": 3}
    assert pos.dtype == copies.dtype == np.int64 and pos.size == copies.size == 0


def test_kept_bytes_of_the_fasta_runs(lib, fasta):
    codes, counts = table_truth(FASTA_SEQS, 8)
    (c, n, nw, parts), k = _launches(fasta, lambda: fasta.fasta_kmer_table(8))
    assert k["k_kt_kept"] == 1 and k["k_kmer_scan"] == 6 and k["k_kt_hist"] == 1 and k["k_kt_emit"] == parts == 1
    assert np.array_equal(c, codes) and np.array_equal(n, counts) and nw == int(counts.sum())
    word = table_truth([FASTA_SEQS[1]], 8)[0]
    s = lib.KmerSet(fasta, 8, False, word)
    want = hits_truth(FASTA_SEQS, 8, word)
    (w, h), k = _launches(fasta, lambda: fasta.fasta_kmer_hits(s))
    assert k == {"k_kmer_scan": 6, "k_kt_kept": 1, "k_ks_fasta": 2}
    assert w.dtype == h.dtype == np.int64 and np.array_equal(w, want[0]) and np.array_equal(h, want[1]) and h[1] == 3
    s.close()


# ------------------------------------------------------------------ the exits
def test_empty_selection(lib, blob, mate, kset):
    e = np.zeros(0, dtype=np.int64)
    bc = np.array([list(b.encode()) for b in BC], dtype=np.uint8)
    for call, dtypes in ((lambda: tuple(blob.fastq_read_stats(ids=e).values()), [np.int64] * 2 + [np.int16] * 2 + [np.int32] * 3),
                         (lambda: blob.fastq_trim(ids=e, tail_qual=10), [np.int64] * 2),
                         (lambda: tuple(blob.fastq_pair_overlap(mate, ids=e).values()), [np.int32] * 3 + [np.int64] * 2),
                         (lambda: tuple(blob.fastq_demux(bc, [0], [0], [8], [0], ids=e)[c] for c in ("sample", "dist", "second", "order")), [np.int32] * 3 + [np.int64]),
                         (lambda: blob.fastq_kmer_table(8, ids=e)[:2], [np.int64] * 2),
                         (lambda: blob.fastq_kmer_hits(kset, ids=e), [np.int32] * 2),
                         (lambda: (blob.fastq_kmer_screen(kset, ids=e),), [np.int64]),
                         (lambda: blob.fastq_dup_first(ids=e)[:1], [np.int64]),
                         (lambda: blob.fastq_dedup(ids=e, want_copies=True)[:2], [np.int64] * 2)):
        out, k = _launches(blob, call)
        assert k == {} and [a.dtype for a in out] == dtypes and all(a.size == 0 for a in out)
    for call in (lambda: blob.fastq_format_alloc(ids=e), lambda: blob.fastq_pair_merge_alloc(mate, np.zeros(0, dtype=np.int32), ids=e)):
        (buf, offs, kept), k = _launches(blob, call)
        assert k == {} and buf.dtype == np.uint8 and buf.size == 0 and offs.dtype == np.int64 and offs.tolist() == [0] and kept == 0
    got, k = _launches(blob, lambda: blob.fastq_kmers(3, ids=e))
    assert k == {} and got.dtype == np.int64 and got.tolist() == [0] * 64
    assert blob.fastq_kmer_table(8, ids=e)[2:] == (0, 0) and blob.fastq_dup_first(ids=e)[1:] == (0, 0) and blob.fastq_dedup(ids=e)[2:] == (0, 0)
    assert blob.fastq_demux(bc, [0], [0], [8], [0], ids=e)["counts"].tolist() == [0] * 4


def test_id_outside_the_table(lib, blob, mate, kset):
    ids = [0, 1, N, -1]
    for call in (lambda: blob.fastq_kmers(4, ids=ids), lambda: blob.fastq_dedup(ids=ids), lambda: blob.fastq_kmer_screen(kset, ids=ids),
                 lambda: blob.fastq_format_alloc(ids=ids), lambda: blob.fastq_pair_merge_alloc(mate, np.zeros(4, dtype=np.int32), ids=ids),
                 lambda: blob.fastq_read_stats(ids=ids), lambda: blob.fastq_trim(ids=ids), lambda: blob.fastq_pair_overlap(mate, ids=ids)):
        e, k = _fails(lib, blob, call)
        assert e.code == lib.FX_ERANGE and str(e) == "read id %d out of range" % N and e.first_bad == 2 and k == {}


def test_bad_interval(lib, blob, mate, kset, reads):
    L = _lens(reads)
    ids = np.arange(N - 1, -1, -1)
    start, end = np.zeros(N, dtype=np.int64), L[ids].copy()
    end[3] += 1
    end[7] += 5
    for call in (lambda: blob.fastq_kmers(4, ids=ids, start=start, end=end), lambda: blob.fastq_kmer_table(8, ids=ids, start=start, end=end),
                 lambda: blob.fastq_kmer_hits(kset, ids=ids, start=start, end=end), lambda: blob.fastq_kmer_screen(kset, ids=ids, start=start, end=end),
                 lambda: blob.fastq_dup_first(ids=ids, start=start, end=end), lambda: blob.fastq_dedup(ids=ids, start=start, end=end)):
        e, k = _fails(lib, blob, call)
        assert e.code == lib.FX_ERANGE and str(e) == "the interval of query 3 lies outside its read" and e.first_bad == 3
        assert k == {"k_kmer_scan": 1}
    e, k = _fails(lib, blob, lambda: blob.fastq_format_alloc(ids=ids, start=start, end=end))
    assert e.code == lib.FX_ERANGE and str(e) == "the interval of query 3 lies outside its read" and e.first_bad == 3
    assert k == {"k_fq_format_count": 1, "k_fq_format_scan": 3}
    diag = np.zeros(N, dtype=np.int32)
    diag[3], diag[7] = L[3], 5000
    e, k = _fails(lib, blob, lambda: blob.fastq_pair_merge_alloc(mate, diag))
    assert e.code == lib.FX_ERANGE and str(e) == "the diagonal of query 3 lies outside its pair" and e.first_bad == 3
    assert k == {"k_fp_merge_count": 1, "k_fp_merge_scan": 3}


def test_start_without_end(lib, blob, kset):
    start = np.zeros(N, dtype=np.int64)
    for call in (lambda: blob.fastq_kmers(4, start=start), lambda: blob.fastq_kmer_table(8, start=start), lambda: blob.fastq_kmer_hits(kset, start=start),
                 lambda: blob.fastq_kmer_screen(kset, end=start), lambda: blob.fastq_dup_first(start=start), lambda: blob.fastq_dedup(end=start),
                 lambda: blob.fastq_format_alloc(start=start)):
        e, k = _fails(lib, blob, call)
        assert e.code == lib.FX_EINVAL and str(e) == "start and end come together" and e.first_bad == -1 and k == {}
