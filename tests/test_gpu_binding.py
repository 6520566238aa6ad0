"""-m gpu: every wrapper of _lib.Blob that takes a selection `ids`, through the one call path (_lib._sel, _call, _ragged), on the
smallest inputs: a FASTA of three records (two lines, one line, no base) and a FASTQ of four reads of unequal length.  Three
calls each -- ids=None; the empty selection, as a list and as a slice of an array, which must give the same zero rows; one call
the library refuses with a status (a cap one below the true count, whose .n_hits / .n_rows is that count, or an id equal to the
table size, whose index is .first_bad) -- and of every array that comes back the dtype, the length and that its memory is the
library's pinned pool."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TWO = ("ACGTACGTAAAAAAAAAAAA", "ATGGCTGCTGCTGCTTAACG")             # ACGT twice, 13 A, ATG (GCT)4 TAA
ONE = "ACGTTTTTTTTTTTTACGT"                                           # ACGT twice, 12 T
FASTA = (">two\n%s\n%s\n>one\n%s\n>none\n" % (TWO + (ONE,))).encode()
READS = ["ACGTACGTAC", "ACGTA", "ACGTACGTACGTACGTACGT", "ACGTACGTAC"]  # the last repeats the first
FASTQ = "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(READS)).encode()
EMPTIES = ([], np.arange(4, dtype=np.int64)[2:2])
NONE = -2**31                                                         # FX_PAIR_NONE
SET_A = bytes(2 if i == ord("A") >> 3 else 0 for i in range(32))      # the byte set {A}
STOPS, ATG = (1 << 48) | (1 << 50) | (1 << 56), 1 << 14               # TAA TAG TGA, ATG by codon index
i8, u8, i16, i32, u32, i64, u64 = np.int8, np.uint8, np.int16, np.int32, np.uint32, np.int64, np.uint64


@pytest.fixture(scope="module")
def lib():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def fasta(lib):
    b = lib.Blob.from_bytes(FASTA, device=0)
    assert b.fasta_build().n_seq == 3
    return b


@pytest.fixture(scope="module")
def fastq(lib):
    b, mate = lib.Blob.from_bytes(FASTQ, device=0), lib.Blob.from_bytes(FASTQ, device=0)
    assert b.fastq_build().n_reads == mate.fastq_build().n_reads == 4
    return b, mate


@pytest.fixture(scope="module")
def kset(lib, fasta):
    return lib.KmerSet(fasta, 4, False, np.array([0b00011011], dtype=np.int64))          # ACGT


def _arrays(lib, arrays, dtypes, lengths):
    """dtype, length and pinned memory of every array of an answer"""
    assert len(arrays) == len(dtypes) == len(lengths)
    for a, dt, n in zip(arrays, dtypes, lengths):
        assert isinstance(a, np.ndarray) and a.dtype == dt and (n is None or a.shape[0] == n), (a.dtype, a.shape, dt, n)
        assert lib.lib().fx_pinned_holds(a.ctypes.data, max(a.nbytes, 1)) == 1


def _norm(x):
    if isinstance(x, np.ndarray):
        return str(x.dtype), x.shape, x.tolist()
    if isinstance(x, (tuple, list)):
        return [_norm(v) for v in x]
    if isinstance(x, dict):
        return {k: _norm(v) for k, v in x.items()}
    return ("sketch", x.n_sets, x.n_keys, _norm(x.read())) if hasattr(x, "read") else x


def _empty(call):
    """The answer to the empty selection: the same from a list and from a slice of an array."""
    a, b = (call(e) for e in EMPTIES)
    assert _norm(a) == _norm(b)
    return a


def _refused(lib, call, **attr):
    with pytest.raises(lib.FxError) as e:
        call()
    assert e.value.code == lib.FX_ERANGE and str(e.value) == lib.lib().fx_last_error().decode()
    assert {k: getattr(e.value, k) for k in attr} == attr
    return e.value


def _mat():
    """10 for the letter of ACGT, -10 for every other: 40 is ACGT alone"""
    mat = np.full((4, 4), -10, dtype=np.int32)
    mat[np.arange(4), np.arange(4)] = 10
    return mat


# ------------------------------------------------------------------ FASTA: the hit entries
def test_hit_entries(lib, fasta):
    plus = lib.FX_SEARCH_PLUS
    calls = {"search": (lambda ids, cap, counts: fasta.fasta_search(b"ACGT", None, plus, ids, cap, counts), [i64, i64, u8]),
             "approx": (lambda ids, cap, counts: fasta.fasta_search_approx(b"ACGT", None, plus, 1, 0, ids, cap, counts), [i64, i64, u8, u8]),
             "pwm": (lambda ids, cap, counts: fasta.fasta_pwm_scan(_mat(), plus, 40, ids, cap, counts), [i64, i64, u8, i32]),
             "minimizers": (lambda ids, cap, counts: fasta.fasta_minimizers(3, 2, lib.FX_MZ_CANONICAL, ids, cap, counts), [i64, i64, u8, u64])}
    for name, (call, dtypes) in calls.items():
        n, hits, cnt = call(None, 1000, True)
        assert n >= 4 and (name not in ("search", "pwm") or n == 4), name
        assert cnt.dtype == i64 and cnt.shape == (3, 2) and int(cnt.sum()) == n and cnt[2].tolist() == [0, 0], name
        _arrays(lib, hits, dtypes, [n] * len(dtypes))
        n0, hits0, cnt0 = _empty(lambda ids: call(ids, 1000, True))
        assert n0 == 0 and cnt0.dtype == i64 and cnt0.shape == (0, 2), name
        if hits0 is not None:
            _arrays(lib, hits0, dtypes, [0] * len(dtypes))
        _refused(lib, lambda: call(None, n - 1, False), n_hits=n)
    n, hits, _ = calls["search"][0](None, 1000, False)
    assert sorted(zip(hits[0].tolist(), hits[1].tolist())) == [(0, 0), (0, 4), (1, 0), (1, 15)] and set(hits[2].tolist()) == {ord("+")}


def test_pwm_best(lib, fasta):
    scores, starts = fasta.fasta_pwm_best(_mat(), lib.FX_SEARCH_PLUS)
    assert scores.dtype == i32 and starts.dtype == i64 and scores.shape == starts.shape == (3, 2)
    assert scores[:, 0].tolist() == [40, 40, np.iinfo(i32).min] and starts[0, 0] in (0, 4) and starts[1, 0] in (0, 15) and starts[2, 0] == -1
    scores, starts = _empty(lambda ids: fasta.fasta_pwm_best(_mat(), lib.FX_SEARCH_PLUS, ids))
    assert scores.dtype == i32 and starts.dtype == i64 and scores.shape == starts.shape == (0, 2)
    e = _refused(lib, lambda: fasta.fasta_pwm_best(_mat(), lib.FX_SEARCH_PLUS, [0, 3]))
    assert not hasattr(e, "first_bad")                                  # the entry names no query


# ------------------------------------------------------------------ FASTA: the interval entries
def test_interval_entries(lib, fasta):
    calls = {"windows": (lambda ids, cap: fasta.fasta_window_counts(8, 8, True, ids, cap), [i64] * 4),
             "runs": (lambda ids, cap: fasta.fasta_class_runs(SET_A, 1, ids, cap), [i64] * 3),
             "repeats": (lambda ids, cap: fasta.fasta_tandem_repeats([12], 0, ids, cap), [i64] * 3 + [u8, u32]),
             "orfs": (lambda ids, cap: fasta.fasta_orfs(STOPS, ATG, 1, 3, 0, ids, cap), [i64] * 3 + [i8, u8])}
    for name, (call, dtypes) in calls.items():
        out = call(None, 10**6)
        t = out[0].size
        assert isinstance(out, tuple) and t >= 1 and t == {"windows": 5 + 3, "repeats": 2}.get(name, t), (name, t)
        _arrays(lib, out, dtypes, [t] * len(dtypes))
        out0 = _empty(lambda ids: call(ids, 10**6))
        _arrays(lib, out0, dtypes, [0] * len(dtypes))
        assert name != "windows" or (out[3].shape == (t, 7) and out0[3].shape == (0, 7) and out[3].sum(axis=1).tolist() == [8] * 5 + [8, 8, 3])
        _refused(lib, lambda: call(None, t - 1), n_rows=t)


# ------------------------------------------------------------------ FASTA: the k-mer entries
def test_fasta_kmer_entries(lib, fasta, kset):
    sk = lambda ids: fasta.fasta_sketch(3, 0, ids, max_key=64)                                  # noqa: E731
    windows = sum(max(len(s) - 2, 0) for s in ("".join(TWO), ONE))
    a = fasta.fasta_kmers(3)
    _arrays(lib, [a], [i64], [64])
    assert int(a.sum()) == windows
    a = fasta.fasta_kmers(3, per_record=True)
    _arrays(lib, [a], [i64], [3])
    assert a.shape == (3, 64) and a.sum(axis=1).tolist() == [38, 17, 0]
    codes, counts, nw, parts = fasta.fasta_kmer_table(3)
    _arrays(lib, [codes, counts], [i64, i64], [codes.size, codes.size])
    assert codes.size >= 1 and int(counts.sum()) == nw == windows
    w, h = fasta.fasta_kmer_hits(kset)
    _arrays(lib, [w, h], [i64, i64], [3, 3])
    assert w.tolist() == [37, 16, 0] and h.tolist() == [2, 2, 0]
    o, rounds = sk(None)
    _arrays(lib, o.read(), [i64, u64], [4, o.n_keys])
    assert o.n_sets == 3 and o.n_keys >= 2

    a = _empty(lambda ids: fasta.fasta_kmers(3, ids=ids))
    _arrays(lib, [a], [i64], [64])
    assert not a.any()
    a = _empty(lambda ids: fasta.fasta_kmers(3, ids=ids, per_record=True))
    _arrays(lib, [a], [i64], [0])
    assert a.shape == (0, 64)
    codes, counts, nw, parts = _empty(lambda ids: fasta.fasta_kmer_table(3, ids=ids))
    _arrays(lib, [codes, counts], [i64, i64], [0, 0])
    assert (nw, parts) == (0, 0)
    _arrays(lib, _empty(lambda ids: fasta.fasta_kmer_hits(kset, ids)), [i64, i64], [0, 0])
    o, rounds = _empty(sk)
    assert (o.n_sets, o.n_keys, rounds) == (0, 0, 0) and o.read()[0].tolist() == [0]

    for call in (lambda: fasta.fasta_kmers(3, ids=[0, 3]), lambda: fasta.fasta_kmers(3, ids=[0, 3], per_record=True),
                 lambda: fasta.fasta_kmer_table(3, ids=[0, 3]), lambda: fasta.fasta_kmer_hits(kset, [0, 3])):
        _refused(lib, call, first_bad=1)
    assert not hasattr(_refused(lib, lambda: sk([0, 3])), "first_bad")     # fx_fasta_sketch names no query


# ------------------------------------------------------------------ FASTQ
def _fastq_calls(lib, b, mate, kset):
    """name -> (the call on a selection, the arrays of its answer, their dtypes, their lengths for n queries; None: any)"""
    bc = np.frombuffer(b"ACGTACGA", dtype=np.uint8).reshape(2, 4)
    stats = ("length", "qsum", "qmin", "qmax", "n_low", "n_gc", "n_other")
    pair = ("diag", "overlap", "mismatches", "end1", "end2")
    n_of = lambda ids: 4 if ids is None else len(ids)                                           # noqa: E731
    return {
        "read_stats": (lambda ids: b.fastq_read_stats(ids, phred=33), lambda d: [d[k] for k in stats],
                       [i64] * 2 + [i16] * 2 + [i32] * 3, lambda n: [n] * 7),
        "trim": (lambda ids: b.fastq_trim(ids, phred=33, clip_front=1), list, [i64] * 2, lambda n: [n] * 2),
        "format": (lambda ids: b.fastq_format_alloc(ids), lambda o: list(o[:2]), [u8, i64], lambda n: [None, n + 1]),
        "demux": (lambda ids: b.fastq_demux(bc, [0], [0], [4], [1], 1, ids), lambda d: [d[k] for k in ("sample", "dist", "second", "counts", "order", "bin_off")],
                  [i32] * 3 + [i64] * 3, lambda n: [n, n, n, 4, n, 5]),
        "pair_overlap": (lambda ids: b.fastq_pair_overlap(mate, ids, min_overlap=4), lambda d: [d[k] for k in pair],
                         [i32] * 3 + [i64] * 2, lambda n: [n] * 5),
        "pair_merge": (lambda ids: b.fastq_pair_merge_alloc(mate, np.full(n_of(ids), NONE, dtype=np.int32), ids), lambda o: list(o[:2]),
                       [u8, i64], lambda n: [0, n + 1]),
        "kmers": (lambda ids: b.fastq_kmers(3, ids=ids), lambda a: [a], [i64], lambda n: [64]),
        "kmer_table": (lambda ids: b.fastq_kmer_table(3, ids=ids), lambda o: list(o[:2]), [i64] * 2, lambda n: [None if n else 0] * 2),
        "sketch": (lambda ids: b.fastq_sketch(3, 0, ids, max_key=64), lambda o: list(o[0].read()), [i64, u64], lambda n: [2, None if n else 0]),
        "kmer_hits": (lambda ids: b.fastq_kmer_hits(kset, ids), list, [i32] * 2, lambda n: [n] * 2),
        "kmer_screen": (lambda ids: b.fastq_kmer_screen(kset, ids), lambda a: [a], [i64], lambda n: [n]),        # every read holds ACGT
        "dup_first": (lambda ids: b.fastq_dup_first(ids), lambda o: [o[0]], [i64], lambda n: [n]),
        "dedup": (lambda ids: b.fastq_dedup(ids, want_copies=True), lambda o: list(o[:2]), [i64] * 2, lambda n: [3 if n else 0] * 2),
    }


def test_fastq_entries(lib, fastq, kset):
    b, mate = fastq
    calls = _fastq_calls(lib, b, mate, kset)
    full, none = {}, {}
    for name, (call, arrays, dtypes, lengths) in calls.items():
        full[name], none[name] = call(None), _empty(call)
        _arrays(lib, arrays(full[name]), dtypes, lengths(4))
        _arrays(lib, arrays(none[name]), dtypes, lengths(0))
        _refused(lib, lambda: call([0, 4]), first_bad=1)
    # what the answers hold, where the inputs make it plain
    assert full["read_stats"]["length"].tolist() == [10, 5, 20, 10] and full["read_stats"]["qmin"].tolist() == [40] * 4
    assert [x.tolist() for x in full["trim"]] == [[1] * 4, [10, 5, 20, 10]]
    buf, offs, kept = full["format"]
    assert buf.tobytes() == FASTQ and kept == 4 and offs.tolist() == np.cumsum([0] + [2 * len(s) + 8 for s in READS]).tolist()
    assert none["format"][1].tolist() == [0] and none["format"][2] == 0
    assert sorted(full["demux"]) == sorted(none["demux"]) == ["bin_off", "counts", "dist", "order", "sample", "second"]
    assert int(full["demux"]["counts"].sum()) == 4 and none["demux"]["counts"].tolist() == [0] * 4 and none["demux"]["bin_off"].tolist() == [0] * 5
    assert sorted(full["pair_overlap"]) == sorted(none["pair_overlap"]) == sorted(("diag", "overlap", "mismatches", "end1", "end2"))
    assert full["pair_merge"][1].tolist() == [0] * 5 and full["pair_merge"][2] == none["pair_merge"][2] == 0
    assert int(full["kmers"].sum()) == sum(len(s) - 2 for s in READS) and not none["kmers"].any()
    assert full["kmer_table"][2] == int(full["kmer_table"][1].sum()) == int(full["kmers"].sum()) and none["kmer_table"][2:] == (0, 0)
    assert (full["sketch"][0].n_sets, none["sketch"][0].n_sets, none["sketch"][1]) == (1, 1, 0)
    assert [x.tolist() for x in full["kmer_hits"]] == [[7, 2, 17, 7], [2, 1, 5, 2]]
    assert full["kmer_screen"].tolist() == [0, 1, 2, 3]
    assert full["dup_first"][0].tolist() == [0, 1, 2, 0] and full["dup_first"][1] == 3 and none["dup_first"][1] == 0
    assert full["dedup"][0].tolist() == [0, 1, 2] and full["dedup"][1].tolist() == [2, 1, 1] and none["dedup"][2] == 0
    pos, copies, groups, _ = b.fastq_dedup(want_copies=False)
    assert pos.tolist() == [0, 1, 2] and copies is None and groups == 3
    cols = b.fastq_demux(np.frombuffer(b"ACGTACGA", dtype=np.uint8).reshape(2, 4), [0], [0], [4], [1], 1, want_order=False)
    assert sorted(cols) == ["counts", "dist", "sample", "second"]
