"""CPU: the paired-end definitions (tests/pair_truth.py) on hand-worked pairs, the argument rules of pyfastx_amd/pair.py, the
errors of the FastqPair constructor, and the host-side logic of FastqPair.trim / write / insert_histogram on stub objects."""
import types

import numpy as np
import pytest

from pair_truth import COMP, NONE, diagonals, insert_of, merged_truth, mismatches_on, overlap_truth, revcomp

EXACT = dict(min_overlap=4, max_diff=0, err=(0, 1))


def frag_of(n, seed):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def pair_of(frag, L1, L2, seed=99):
    """The mates of a fragment: its first L1 letters, the first L2 of its reverse complement; past the fragment's end random
    letters stand for the adapter."""
    fill = frag_of(L1 + L2, seed)
    return (frag + fill[:L1])[:L1], (revcomp(frag) + fill[L1:])[:L2]


def plant(s, pos, c=None):
    """s with the letter at pos replaced by c (default: another letter of A C G T)."""
    b = bytearray(s)
    b[pos] = c if c is not None else b"CATG"[b"ACGT".index(b[pos])]
    return bytes(b)


def test_trial_order_and_complement_table():
    assert diagonals(3, 4) == [0, 1, 2, -1, -2, -3] and diagonals(0, 2) == [-1] and diagonals(2, 0) == [0, 1]
    assert revcomp(b"ACGTNacgtRYu") == b"aRYacgtNACGT"
    assert COMP[ord("M")] == ord("K") and COMP[ord("w")] == ord("w") and COMP[200] == 200 and COMP[ord("U")] == ord("A")


def test_worked_example():
    # read 1 ACGTTGCA, reverse complement of read 2 TGCAGGAT: the only diagonal without a mismatch is d = 4, TGCA on TGCA
    s1, s2 = b"ACGTTGCA", revcomp(b"TGCAGGAT")
    assert s2 == b"ATCCTGCA"
    assert [mismatches_on(s1, s2, d) for d in (0, 3, 4, 5, -1)] == [(8, 7), (5, 4), (4, 0), (3, 3), (7, 6)]
    assert overlap_truth(s1, s2, **EXACT) == {"diag": 4, "overlap": 4, "mismatches": 0, "end1": 8, "end2": 8, "insert": 12}
    # three letters of overlap are fewer than min_overlap
    assert overlap_truth(s1, s2, min_overlap=5, max_diff=0, err=(0, 1))["diag"] == NONE
    # one mismatch in four allowed: d = 4 is still the first accepted (d = 0 .. 3 have 7, 4, 6, 4)
    assert overlap_truth(s1, s2, min_overlap=4, max_diff=1, err=(1, 4))["diag"] == 4
    got = merged_truth(b"@r", s1, b"IIIIIIII", s2, b"ABCDEFGH", 4)
    assert got == b"@r\nACGTTGCAGGAT\n+\nIIIIIIIIDCBA\n"


@pytest.mark.parametrize("F,d", [(60, 20), (40, 0), (25, -15), (79, 39), (1, -39)])
def test_perfect_overlap(F, d):
    s1, s2 = pair_of(frag_of(F, F), 40, 40)
    r = overlap_truth(s1, s2, min_overlap=1, max_diff=0, err=(0, 1))
    m = 80 - F if d >= 0 else F
    assert r == {"diag": d, "overlap": m, "mismatches": 0, "end1": 40 if d >= 0 else F, "end2": 40 if d >= 0 else F, "insert": F}
    assert mismatches_on(s1, s2, d) == (m, 0)


@pytest.mark.parametrize("F", [60, 40, 25])
def test_planted_mismatches_against_max_diff(F):
    L, max_diff = 40, 2
    s1, s2 = pair_of(frag_of(F, 7 + F), L, L)
    d = F - L
    lo, hi = max(0, d), min(L, d + L)
    pos = [lo, hi - 1, (lo + hi) // 2]
    a = s1
    for p in pos[:max_diff]:
        a = plant(a, p)
    r = overlap_truth(a, s2, min_overlap=10, max_diff=max_diff, err=(1, 2))
    assert (r["diag"], r["overlap"], r["mismatches"]) == (d, hi - lo, max_diff)
    a = plant(a, pos[2])
    assert mismatches_on(a, s2, d) == (hi - lo, max_diff + 1)
    assert overlap_truth(a, s2, min_overlap=10, max_diff=max_diff, err=(1, 2))["diag"] == NONE
    # the same letters planted in read 2 instead
    b = s2
    for p in pos[:max_diff]:
        b = plant(b, L - 1 - (p - d))
    assert overlap_truth(s1, b, min_overlap=10, max_diff=max_diff, err=(1, 2))["mismatches"] == max_diff


def test_ratio_met_exactly_and_exceeded_by_one():
    s1, s2 = pair_of(frag_of(60, 3), 40, 40)                  # d = 20, 20 letters of overlap
    a = plant(plant(s1, 22), 31)
    r = overlap_truth(a, s2, min_overlap=10, max_diff=5, err=(1, 10))                # 2 * 10 <= 1 * 20
    assert (r["diag"], r["mismatches"]) == (20, 2)
    a = plant(a, 39)
    assert mismatches_on(a, s2, 20) == (20, 3)
    assert overlap_truth(a, s2, min_overlap=10, max_diff=5, err=(1, 10))["diag"] == NONE   # 3 * 10 > 1 * 20
    assert overlap_truth(a, s2, min_overlap=10, max_diff=5, err=(3, 20))["diag"] == 20     # 3 * 20 <= 3 * 20


def test_n_and_lower_case_mismatch_in_either_mate():
    s1, s2 = pair_of(frag_of(60, 5), 40, 40)
    for a, b in ((plant(s1, 30, ord("N")), s2), (plant(s1, 30, s1[30] | 0x20), s2), (s1, plant(s2, 25, ord("N"))), (s1, plant(s2, 25, s2[25] | 0x20)),
                 (plant(s1, 30, ord("R")), s2)):
        assert mismatches_on(a, b, 20) == (20, 1)
        r = overlap_truth(a, b, min_overlap=10, max_diff=1, err=(1, 5))
        assert (r["diag"], r["mismatches"]) == (20, 1)
        assert overlap_truth(a, b, min_overlap=10, max_diff=0, err=(1, 5))["diag"] == NONE
    # an N under an N is a mismatch too
    assert mismatches_on(b"ACGNT", revcomp(b"ACGNT"), 0) == (5, 1)


def test_unequal_and_empty_reads():
    s1, s2 = pair_of(frag_of(50, 11), 33, 47)
    assert overlap_truth(s1, s2, min_overlap=8, max_diff=0, err=(0, 1)) == {"diag": 3, "overlap": 30, "mismatches": 0, "end1": 33, "end2": 47, "insert": 50}
    s1, s2 = pair_of(frag_of(20, 12), 33, 47)                 # read-through in both: d = 20 - 47
    assert overlap_truth(s1, s2, min_overlap=8, max_diff=0, err=(0, 1)) == {"diag": -27, "overlap": 20, "mismatches": 0, "end1": 20, "end2": 20, "insert": 20}
    none = {"diag": NONE, "overlap": 0, "mismatches": 0, "insert": -1}
    assert overlap_truth(b"", b"ACGTACGTAC", min_overlap=1) == dict(none, end1=0, end2=10)
    assert overlap_truth(b"ACGT", b"", min_overlap=1) == dict(none, end1=4, end2=0)
    assert overlap_truth(b"", b"", min_overlap=1) == dict(none, end1=0, end2=0)
    assert merged_truth(b"@x", b"", b"", b"ACGT", b"IIII", NONE) == b""


def test_min_overlap_larger_than_both_reads():
    s1, s2 = pair_of(frag_of(40, 13), 40, 40)
    assert overlap_truth(s1, s2, min_overlap=40, max_diff=0, err=(0, 1))["diag"] == 0
    assert overlap_truth(s1, s2, min_overlap=41, max_diff=5, err=(1, 1))["diag"] == NONE


def test_poly_g_pair():
    # two-colour instruments read a dark cycle as G: read 1 poly-G over read 2 poly-C is a perfect overlap at d = 0
    r = overlap_truth(b"G" * 40, b"C" * 40)
    assert (r["diag"], r["overlap"], r["mismatches"], r["insert"]) == (0, 40, 0, 40)
    assert overlap_truth(b"G" * 40, b"G" * 40)["diag"] == NONE


def test_merge_rules():
    # d = 2: fragment positions 2..5 carry both mates; x = read 1, y = the complement of read 2 read backwards
    s1, q1 = b"AACCGG", b"555555"
    y, b = b"CCTGAT", b"5694AB"                              # letters k = 0..5 of the reverse complement and their qualities
    s2, q2 = revcomp(y), b[::-1]
    rec = merged_truth(b"@h", s1, q1, s2, q2, 2)
    # f=2: C/C agree, max(5, 5) -> 5;  f=3: C/C agree, max(5, 6) -> 6;  f=4: G against T, 5 < 9 -> T 9;  f=5: G against G, max(5, 4) -> 5
    assert rec == b"@h\nAACCTGAT\n+\n55569" + b"5AB\n"
    # a tie between different letters keeps read 1's; a higher quality of read 1 keeps it too
    assert merged_truth(b"@h", b"A", b"5", revcomp(b"C"), b"5", 0) == b"@h\nA\n+\n5\n"
    assert merged_truth(b"@h", b"A", b"6", revcomp(b"C"), b"5", 0) == b"@h\nA\n+\n6\n"
    assert merged_truth(b"@h", b"A", b"4", revcomp(b"C"), b"5", 0) == b"@h\nC\n+\n5\n"
    # lower case differs from upper case as bytes; the complement keeps the case; qualities compare as raw bytes
    assert merged_truth(b"@h", b"a", b"\x80", revcomp(b"A"), b"\x7f", 0) == b"@h\na\n+\n\x80\n"
    assert merged_truth(b"@h", b"a", b"\x7f", b"t", b"\x80", 0) == b"@h\na\n+\n\x80\n"
    # min_len
    assert merged_truth(b"@h", s1, q1, s2, q2, 2, min_len=8) == rec and merged_truth(b"@h", s1, q1, s2, q2, 2, min_len=9) == b""
    # d < 0: the fragment is what read 2 has left, read 1's letters past it (adapter) are dropped
    assert merged_truth(b"@h", b"ACGTTT", b"999999", revcomp(b"GGACG"), b"11111", -2) == b"@h\nACG\n+\n999\n"


def test_read_2_inside_read_1():
    frag = frag_of(40, 17)
    s1, s2 = frag, revcomp(frag[10:30])
    r = overlap_truth(s1, s2, min_overlap=8, max_diff=0, err=(0, 1))
    assert r == {"diag": 10, "overlap": 20, "mismatches": 0, "end1": 40, "end2": 20, "insert": 40}
    q1, q2 = bytes(range(40, 80)), bytes([90] * 20)
    rec = merged_truth(b"@in", s1, q1, s2, q2, 10)
    assert rec == b"@in\n" + frag + b"\n+\n" + q1[:10] + bytes([90] * 20) + q1[30:] + b"\n"


def test_vectorised_truth_agrees_with_the_letter_loop():
    rng = np.random.default_rng(5)
    for _ in range(60):
        L1, L2 = int(rng.integers(0, 25)), int(rng.integers(0, 25))
        F = int(rng.integers(1, 50))
        s1, s2 = pair_of(frag_of(F, int(rng.integers(1 << 30))), L1, L2, seed=int(rng.integers(1 << 30)))
        if L1 and rng.random() < 0.5:
            s1 = plant(s1, int(rng.integers(L1)), ord("N"))
        kw = dict(min_overlap=int(rng.integers(1, 8)), max_diff=int(rng.integers(0, 3)), err=(int(rng.integers(0, 3)), int(rng.integers(1, 8))))
        want = NONE
        for d in diagonals(L1, L2):
            m, mm = mismatches_on(s1, s2, d)
            if m >= kw["min_overlap"] and mm <= kw["max_diff"] and mm * kw["err"][1] <= kw["err"][0] * m:
                want = d
                break
        r = overlap_truth(s1, s2, **kw)
        assert r["diag"] == want and r["insert"] == insert_of(want, L1, L2)


# ------------------------------------------------------------------ pyfastx_amd/pair.py
def test_argument_rules():
    from pyfastx_amd import pair
    assert pair.overlap_args() == {"min_overlap": 30, "max_diff": 5, "err": (1, 5)}
    assert pair.overlap_args(1, 0, 0) == {"min_overlap": 1, "max_diff": 0, "err": (0, 1)}
    assert pair.overlap_args(max_error_rate="1/3")["err"] == (1, 3) and pair.overlap_args(max_error_rate=0.1234567)["err"][1] <= 1000
    for bad in (dict(min_overlap=0), dict(min_overlap=-3), dict(min_overlap=1.5), dict(min_overlap=True), dict(max_diff=-1), dict(max_diff="2"),
                dict(max_error_rate=-0.1), dict(max_error_rate=float("nan")), dict(max_error_rate=None)):
        with pytest.raises(ValueError):
            pair.overlap_args(**bad)
    assert pair.NONE == NONE == -2**31
    d = np.array([NONE, 0, 5, -3], dtype=np.int32)
    assert pair.insert_of(d, [10, 10, 10, 10], [8, 8, 8, 8]).tolist() == [-1, 10, 13, 5]
    assert pair.insert_of(d, 10, 8).dtype == np.int64
    with pytest.raises(ValueError):
        pair.check_diag(np.zeros(3, dtype=np.int32), 4)
    assert pair.strip_mate("r1/1") == "r1" == pair.strip_mate("r1/2") and pair.strip_mate("r1/3") == "r1/3" and pair.strip_mate("/1") == ""


def test_insert_histogram():
    from pyfastx_amd import pair
    h = pair.insert_histogram(np.array([3, -1, 3, 0, 5, -1], dtype=np.int64))
    assert h.dtype == np.int64 and h.tolist() == [1, 0, 0, 2, 0, 1]
    assert pair.insert_histogram(np.array([-1, -1])).tolist() == [] and pair.insert_histogram([]).size == 0
    assert pair.FastqPair.insert_histogram([2]).tolist() == [0, 0, 1]


def test_both_symbols_in_the_abi_list():
    from pyfastx_amd import _lib
    assert "fx_fastq_pair_overlap" in _lib.SYMBOLS and "fx_fastq_pair_merge_alloc" in _lib.SYMBOLS
    L = _lib.lib()
    assert L.fx_fastq_pair_overlap.argtypes is not None and len(L.fx_fastq_pair_overlap.argtypes) == 15
    assert len(L.fx_fastq_pair_merge_alloc.argtypes) == 11


class StubFastq:
    """What FastqPair touches of a Fastq: the device, the lengths, trim and write (which record their arguments)."""

    def __init__(self, lengths, device=0, sharded=False, names=None, trims=None):
        self._rlen_host = np.asarray(lengths, dtype=np.int64)
        self._tab_host = {"dlen": np.full(len(lengths), 5, dtype=np.int32)}
        self._st = types.SimpleNamespace(device=device)
        self._sharded = sharded
        self.file_name = "stub.fq"
        self.names = names
        self.trims = trims
        self.calls = []

    def __len__(self):
        return self._rlen_host.size

    def __getitem__(self, i):
        return types.SimpleNamespace(name=self.names[i])

    def _qc_blob(self):
        if self._sharded:
            raise NotImplementedError("quality control on a sharded or windowed stream")
        return None

    def trim(self, ids=None, **kw):
        self.calls.append(("trim", ids, kw))
        sel = slice(None) if ids is None else ids
        return {"start": self.trims[0][sel], "end": self.trims[1][sel]}

    def write(self, path, ids=None, start=None, end=None, min_len=0, batch_bytes=1 << 30):
        self.calls.append(("write", path, ids, start, end, min_len, batch_bytes))
        ln = self._rlen_host[ids] if start is None else end - start
        return {"reads": int(ids.size), "bases": int(ln.sum()), "dropped": 0}


@pytest.fixture
def stubbed(monkeypatch):
    from pyfastx_amd import api, pair
    monkeypatch.setattr(api, "Fastq", StubFastq)
    return pair


def test_constructor_errors(stubbed):
    pair = stubbed
    ok = pair.FastqPair(StubFastq([5, 6]), StubFastq([7, 8]))
    assert len(ok) == 2 and "2 pairs" in repr(ok)
    with pytest.raises(TypeError):
        pair.FastqPair(StubFastq([5]), "reads_R2.fq")
    with pytest.raises(TypeError):
        pair.FastqPair(None, StubFastq([5]))
    with pytest.raises(NotImplementedError):
        pair.FastqPair(StubFastq([5], sharded=True), StubFastq([5]))
    with pytest.raises(NotImplementedError):
        pair.FastqPair(StubFastq([5]), StubFastq([5], sharded=True))
    with pytest.raises(ValueError, match="devices"):
        pair.FastqPair(StubFastq([5], device=0), StubFastq([5], device=1))
    with pytest.raises(ValueError, match="numbers of reads"):
        pair.FastqPair(StubFastq([5, 6]), StubFastq([5]))


def test_the_real_constructor_refuses_what_is_no_fastq():
    import pyfastx_amd
    assert pyfastx_amd.FastqPair is pyfastx_amd.pair.FastqPair
    with pytest.raises(TypeError):
        pyfastx_amd.FastqPair("a.fq", "b.fq")


def test_check_names(stubbed):
    pair = stubbed
    n1 = ["r%d/1" % i for i in range(10)]
    n2 = ["r%d/2" % i for i in range(10)]
    p = pair.FastqPair(StubFastq([4] * 10, names=n1), StubFastq([4] * 10, names=n2))
    p.check_names()
    p.check_names(n=2)
    n2[7] = "other/2"
    p.check_names(n=2)                                        # pair 7 is neither among the first nor among the last two
    with pytest.raises(ValueError, match="pair 7"):
        p.check_names(n=3)
    n2[1], n2[8] = "x", "y"
    with pytest.raises(ValueError, match="pair 1:"):
        p.check_names()
    same = ["r%d" % i for i in range(10)]
    pair.FastqPair(StubFastq([4] * 10, names=same), StubFastq([4] * 10, names=list(same))).check_names()


def test_trim_lowers_the_ends_to_the_overlap(stubbed):
    pair = stubbed
    t1 = (np.array([0, 5, 30, 2]), np.array([100, 100, 90, 50]))
    t2 = (np.array([1, 0, 10, 0]), np.array([100, 80, 100, 100]))
    f1, f2 = StubFastq([100] * 4, trims=t1), StubFastq([100] * 4, trims=t2)
    p = pair.FastqPair(f1, f2)
    ov = {"diag": np.array([NONE, -40, -80, 10], dtype=np.int32), "end1": np.array([100, 60, 20, 100]), "end2": np.array([100, 60, 20, 100])}
    seen = []
    p.overlap = lambda ids=None, **kw: seen.append((ids, kw)) or ov
    got = p.trim(front_qual=20)
    assert sorted(got) == ["diag", "end1", "end2", "start1", "start2"]
    assert got["end1"].tolist() == [100, 60, 20, 50] and got["start1"].tolist() == [0, 5, 20, 2]           # a start beyond the new end is clamped to it
    assert got["end2"].tolist() == [100, 60, 20, 100] and got["start2"].tolist() == [1, 0, 10, 0]
    assert got["diag"].tolist() == [NONE, -40, -80, 10] and got["diag"].dtype == np.int32
    assert seen == [(None, {})] and f1.calls == [("trim", None, {"front_qual": 20})] and f2.calls == f1.calls
    assert all(isinstance(v, np.ndarray) for v in got.values())
    # the arguments of overlap as a dict; no overlap at all
    p.trim(overlap={"min_overlap": 12}, tail_qual=3)
    assert seen[1] == (None, {"min_overlap": 12}) and f1.calls[-1] == ("trim", None, {"tail_qual": 3})
    got = p.trim(overlap=False)
    assert len(seen) == 2 and got["end1"].tolist() == [100, 100, 90, 50] and got["diag"].tolist() == [NONE] * 4
    # gathered ids reach all three
    ids = np.array([3, 3, 0])
    ov3 = {k: v[ids] for k, v in ov.items()}
    p.overlap = lambda ids=None, **kw: seen.append((ids, kw)) or ov3
    got = p.trim(ids=ids)
    assert seen[-1][0] is ids and got["end1"].tolist() == [50, 50, 100] and got["diag"].tolist() == [10, 10, NONE]


def test_write_keeps_a_pair_only_when_both_mates_pass(stubbed):
    pair = stubbed
    f1, f2 = StubFastq([50, 10, 50, 50, 0]), StubFastq([50, 50, 9, 50, 0])
    p = pair.FastqPair(f1, f2)
    got = p.write("a", "b", min_len=10)
    assert got == {"pairs": 3, "bases1": 110, "bases2": 150, "dropped": 2}
    (_, p1, i1, s1, e1, m1, bb1), (_, p2, i2, s2, e2, m2, bb2) = f1.calls[-1], f2.calls[-1]
    assert (p1, p2) == ("a", "b") and i1.tolist() == i2.tolist() == [0, 1, 3] and s1 is e1 is s2 is e2 is None and m1 == m2 == 10 and bb1 == bb2 == 1 << 30
    # intervals: the kept length is end - start; ids in any order, with repeats; the intervals are cut with the ids
    ids = np.array([3, 0, 0, 2])
    st1, en1 = np.array([0, 10, 45, 0]), np.array([50, 30, 50, 50])
    st2, en2 = np.array([5, 0, 0, 0]), np.array([25, 50, 50, 9])
    got = p.write("a", "b", ids=ids, start1=st1, end1=en1, start2=st2, end2=en2, min_len=20, batch_bytes=4096)
    assert got == {"pairs": 2, "bases1": 70, "bases2": 70, "dropped": 2}
    (_, _, i1, s1, e1, _, bb1), (_, _, i2, s2, e2, _, _) = f1.calls[-1], f2.calls[-1]
    assert i1.tolist() == i2.tolist() == [3, 0] and s1.tolist() == [0, 10] and e1.tolist() == [50, 30] and s2.tolist() == [5, 0] and e2.tolist() == [25, 50]
    assert bb1 == 4096
    # one mate with intervals, the other whole
    got = p.write("a", "b", start2=np.zeros(5, dtype=np.int64), end2=np.array([50, 50, 9, 3, 0]), min_len=1)
    assert got["pairs"] == 4 and f1.calls[-1][2].tolist() == [0, 1, 2, 3] and f1.calls[-1][3] is None and f2.calls[-1][4].tolist() == [50, 50, 9, 3]
    # nothing passes: both files are still written (empty), in step
    got = p.write("a", "b", min_len=51)
    assert got == {"pairs": 0, "bases1": 0, "bases2": 0, "dropped": 5} and f1.calls[-1][2].size == 0
    with pytest.raises(ValueError):
        p.write("a", "b", start1=st1)
    with pytest.raises(ValueError):
        p.write("a", "b", start1=st1, end1=en1)                # four rows for five pairs
    with pytest.raises(IndexError):
        p.write("a", "b", ids=[5])
    with pytest.raises(ValueError):
        p.write("a", "b", min_len=-1)
