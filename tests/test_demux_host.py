"""CPU: the plain-Python definition tests/demux_truth.py on hand-written reads whose answers are written out, the numpy form
against it on random inputs, the argument rules of pyfastx_amd/demux.py, the Demux object on made-up columns, the C entry
(declared, exported) and the pins of the definition over tests/data/test.fq parsed on the host."""
import os

import numpy as np
import pytest

from conftest import DATA, ROOT
from demux_truth import (ABSENT, AMBIGUOUS, HEADER, NONE, SEQ3, SEQ5, bins_of, cut_header, decide, demux_read, demux_truth,
                         demux_truth_fast, distance, parse_fastq, segments, window)


def W(txt):
    """'AC.' -> [65, 67, ABSENT]"""
    return [ABSENT if c == "." else ord(c) for c in txt]


# ------------------------------------------------------------------ windows
def test_sequence_windows():
    s = b"ACGTTGCA"
    assert window(b"@r", s, SEQ5, 0, 4) == W("ACGT")
    assert window(b"@r", s, SEQ5, 6, 4) == W("CA..")                   # ABSENT at the 3' end
    assert window(b"@r", s, SEQ5, 8, 2) == W("..") and window(b"@r", s, SEQ5, 100, 1) == W(".")
    assert window(b"@r", s, SEQ3, 0, 4) == W("TGCA")
    assert window(b"@r", s, SEQ3, 2, 4) == W("GTTG")
    assert window(b"@r", s, SEQ3, 6, 4) == W("..AC")                   # ABSENT at the 5' end
    assert window(b"@r", s, SEQ3, 8, 3) == W("...") and window(b"@r", s, SEQ3, 0, 10) == W("..ACGTTGCA")
    assert window(b"@r", b"", SEQ5, 0, 3) == W("...") and window(b"@r", b"", SEQ3, 0, 3) == W("...")


def test_header_windows():
    H = b"@M1:7:000:1:1101:1:2 1:N:0:CAATGGAA+CGAGGCTG"
    assert window(H, b"", HEADER, 0, 8) == W("CAATGGAA") and window(H, b"", HEADER, 1, 8) == W("CGAGGCTG")
    assert window(H, b"", HEADER, 0, 6) == W("CAATGG")                 # a part longer than len: a prefix compare
    assert window(H, b"", HEADER, 1, 10) == W("CGAGGCTG..")            # a part shorter than len
    H1 = b"@r 1:N:0:CAATGG"                                            # no '+'
    assert window(H1, b"", HEADER, 0, 8) == W("CAATGG..") and window(H1, b"", HEADER, 1, 4) == W("....")
    assert window(b"@r 1:N:0:", b"", HEADER, 0, 2) == W("..")          # an empty field
    assert window(b"@r 1:N:0:+AC", b"", HEADER, 0, 2) == W("..") and window(b"@r 1:N:0:+AC", b"", HEADER, 1, 2) == W("AC")
    assert window(b"@r 1:N:0:A+C+G", b"", HEADER, 1, 3) == W("C+G")    # only the first '+' splits
    assert window(b"@read7 ACGT", b"", HEADER, 0, 4) == W("....")      # no ':' at all
    assert cut_header(b"@r:ACGT\r") == b"@r:ACGT" and cut_header(b"@r:ACGT\r\r") == b"@r:ACGT\r" and cut_header(b"@r") == b"@r"
    assert window(cut_header(b"@r:ACGT\r"), b"", HEADER, 0, 5) == W("ACGT.")
    F65, F66 = b"A" * 30 + b"+" + b"C" * 34, b"A" * 30 + b"+" + b"C" * 35
    assert len(F65) == 65 and len(F66) == 66
    assert window(b"@r:" + F65, b"", HEADER, 0, 3) == W("AAA") and window(b"@r:" + F65, b"", HEADER, 1, 3) == W("CCC")
    assert window(b"@r:" + F66, b"", HEADER, 0, 3) == W("...") and window(b"@r:" + F66, b"", HEADER, 1, 3) == W("...")


def test_distance():
    assert distance(W("ACGT"), b"ACGT") == 0 and distance(W("ACGA"), b"ACGT") == 1
    assert distance(W("ACGT"), b"NNNN") == 0 and distance(W("...."), b"NNNN") == 0      # N in the barcode matches anything
    assert distance(W("ANGT"), b"ACGT") == 1 and distance(W("NNNN"), b"ACGT") == 4      # N in the read mismatches
    assert distance(W("acgt"), b"ACGT") == 4 and distance(W("ARGT"), b"ACGT") == 1      # lower case, IUPAC
    assert distance(W("AC.."), b"ACGT") == 2 and distance(W("AC.."), b"ACNT") == 1      # ABSENT mismatches a letter that counts


def test_decide_margins_and_ties():
    assert decide([], 1) == (NONE, -1, -1)
    assert decide([(2, 5)], 1) == (5, 2, -1) and decide([(2, 5)], 64) == (5, 2, -1)
    assert decide([(0, 3), (1, 1)], 1) == (3, 0, 1) and decide([(0, 3), (1, 1)], 2) == (AMBIGUOUS, 0, 1)
    assert decide([(2, 0), (0, 3)], 2) == (3, 0, 2) and decide([(2, 0), (0, 3)], 3) == (AMBIGUOUS, 0, 2)
    assert decide([(3, 0), (0, 3)], 3) == (3, 0, 3)
    assert decide([(1, 0), (1, 4)], 1) == (AMBIGUOUS, 1, 1)                             # a tie between two
    assert decide([(1, 0), (1, 4), (1, 2)], 1) == (AMBIGUOUS, 1, 1)                     # and between three
    assert decide([(1, 0), (1, 4), (0, 2)], 1) == (2, 0, 1)


def test_reads_by_hand():
    sheet = [(b"ACGT",), (b"ACGA",), (b"TTTT",)]
    seg = lambda mm: [(SEQ5, 0, 4, mm)]
    assert demux_read(b"@r", b"ACGTCC", seg(0), sheet) == (0, 0, -1)
    assert demux_read(b"@r", b"ACGTCC", seg(1), sheet) == (0, 0, 1)
    assert demux_read(b"@r", b"ACGTCC", seg(1), sheet, margin=2) == (AMBIGUOUS, 0, 1)
    assert demux_read(b"@r", b"ACGCCC", seg(1), sheet) == (AMBIGUOUS, 1, 1)             # one letter from two samples
    assert demux_read(b"@r", b"GGGGCC", seg(1), sheet) == (NONE, -1, -1)
    assert demux_read(b"@r", b"AC", seg(2), sheet) == (AMBIGUOUS, 2, 2)                 # two ABSENT slots
    assert demux_read(b"@r", b"acgt", seg(4), sheet) == (AMBIGUOUS, 4, 4)               # a tie between three
    # a budget per segment, not on the total
    dual = [(b"AAAA", b"CCCC"), (b"GGGG", b"TTTT")]
    two = lambda m0, m1: [(SEQ5, 0, 4, m0), (SEQ3, 0, 4, m1)]
    assert demux_read(b"@r", b"AAATxxCCCC", two(1, 1), dual) == (0, 1, -1)
    assert demux_read(b"@r", b"AATTxxCCCC", two(1, 1), dual) == (NONE, -1, -1)          # 2 + 0: within a total of 2, over the segment's 1
    assert demux_read(b"@r", b"AATTxxCCCC", two(2, 0), dual) == (0, 2, -1)
    assert demux_read(b"@r", b"AAATxxCCCG", two(1, 1), dual) == (0, 2, -1)
    assert demux_read(b"@r", b"AAATxxCCCG", two(1, 0), dual) == (NONE, -1, -1)
    assert demux_read(b"@r", b"AAGGxxCCTT", two(2, 2), dual) == (AMBIGUOUS, 4, 4)
    hdr = [(HEADER, 0, 8, 1), (HEADER, 1, 8, 1)]
    idx = [(b"CAATGGAA", b"CGAGGCTG"), (b"CAATGGAA", b"CGAGGCGG")]
    assert demux_read(b"@x 1:N:0:CAATGGAA+CGAGGCTG", b"", hdr, idx) == (0, 0, 1)
    assert demux_read(b"@x 1:N:0:CAATGGAA+CGAGGCTG", b"", hdr, idx, margin=2) == (AMBIGUOUS, 0, 1)
    assert demux_read(b"@x 1:N:0:CAATGGAA+CGAGGCAG", b"", hdr, idx) == (AMBIGUOUS, 1, 1)
    assert demux_read(b"@x 1:N:0:CAATGGAA", b"", hdr, idx) == (NONE, -1, -1)


def test_fast_truth_equals_slow_truth():
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACGTNacgtR", dtype=np.uint8)
    for trial in range(12):
        n_seg = 1 + trial % 2
        lens = [int(rng.integers(1, 33)) for _ in range(n_seg)]
        ns = int(rng.integers(1, 40))
        sheet = set()
        while len(sheet) < ns:
            sheet.add(tuple(bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, ln, p=[.24, .24, .24, .24, .04])]) for ln in lens))
        sheet = sorted(sheet)
        segs = [(int(rng.integers(0, 3)), 0, ln, int(rng.integers(0, min(ln, 4) + 1))) for ln in lens]
        segs = [(src, int(rng.integers(0, 2)) if src == HEADER else int(rng.integers(0, 12)), ln, mm) for src, _, ln, mm in segs]
        reads = []
        for i in range(120):
            row = sheet[int(rng.integers(0, ns))]
            parts = [bytearray(b) for b in row]
            for p in parts:                                   # up to three letters changed
                for _ in range(int(rng.integers(0, 4))):
                    p[int(rng.integers(0, len(p)))] = int(letters[rng.integers(0, len(letters))])
            body = bytes(letters[rng.integers(0, 4, int(rng.integers(0, 30)))])
            s = bytes(parts[0]) + body + bytes(parts[-1])
            s = s[:int(rng.integers(0, len(s) + 1))] if i % 7 == 0 else s
            H = b"@r%d 1:N:0:" % i + bytes(parts[0]) + (b"+" + bytes(parts[-1]) if i % 5 else b"")
            reads.append((H if i % 11 else b"@plain%d" % i, s))
        for margin in (1, 2, 5):
            slow, fast = demux_truth(reads, segs, sheet, margin), demux_truth_fast(reads, segs, sheet, margin, chunk=50)
            for a, b in zip(slow, fast):
                assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (trial, margin)


# ------------------------------------------------------------------ argument rules
def test_args_defaults_and_conversions():
    from pyfastx_amd import demux
    a = demux.demux_args({"s1": "caatggaa", "s2": b"CGAGGCTN"})
    assert a["names"] == ["s1", "s2"] and a["where"] == ["header"] and a["src"] == [2] and a["off"] == [0] and a["length"] == [8]
    assert a["mm"] == [1] and a["margin"] == 1 and a["barcodes"].dtype == np.uint8 and a["barcodes"].shape == (2, 8)
    assert a["barcodes"].tobytes() == b"CAATGGAACGAGGCTN"
    a = demux.demux_args([("CAATGGAA", "CGAGGCTG"), ("ACGTACGT", "CGAGGCTG")])
    assert a["names"] == ["0", "1"] and a["off"] == [0, 1] and a["src"] == [2, 2] and a["mm"] == [1, 1]     # parts 0 and 1
    assert a["barcodes"].shape == (2, 16) and a["barcodes"][1].tobytes() == b"ACGTACGTCGAGGCTG"
    assert demux.demux_args([("AC", "GT")], offset=(1, 0))["off"] == [1, 0]
    assert demux.demux_args([("AC", "GT")], where=("5p", "header"))["off"] == [0, 0]
    a = demux.demux_args([("AAC", "GGGT")], where=("5p", "3p"), offset=(3, np.int64(9)), mismatches=(0, 4), margin=64, revcomp=(False, True))
    assert (a["src"], a["off"], a["length"], a["mm"], a["margin"]) == ([0, 1], [3, 9], [3, 4], [0, 4], 64)
    assert a["barcodes"].tobytes() == b"AACACCC"
    assert demux.demux_args(["AACN"], where="3p", revcomp=True)["barcodes"].tobytes() == b"NGTT"
    segs, sheet = segments(a)
    assert segs == [(0, 3, 3, 0), (1, 9, 4, 4)] and sheet == [(b"AAC", b"ACCC")]
    assert len(demux.demux_args(["A" * 12 + format(i, "012b").replace("0", "C").replace("1", "G") for i in range(4096)])["names"]) == 4096


@pytest.mark.parametrize("kw", [
    dict(samples={}), dict(samples=[]), dict(samples="ACGT"), dict(samples=5), dict(samples=None),
    dict(samples=["ACGT"] * 2), dict(samples={"a": "ACGT", "b": "acgt"}), dict(samples=["ACGT", "ACG"]),
    dict(samples=["ACGT", ("ACGT", "AC")]), dict(samples=[("ACGT", "AC"), ("ACGT", "ACG")]), dict(samples=[("A", "C", "G")]),
    dict(samples=[()]), dict(samples=["ACGU"]), dict(samples=["AC-T"]), dict(samples=["ACRT"]), dict(samples=["ACGé"]), dict(samples=[""]),
    dict(samples=["A" * 33]), dict(samples=[5]), dict(samples={1: "ACGT"}),
    dict(samples=["A" * 12 + format(i, "013b").replace("0", "C").replace("1", "G") for i in range(4097)]),
    dict(samples=["ACGT"], where="5"), dict(samples=["ACGT"], where=0), dict(samples=["ACGT"], where=("5p", "3p")),
    dict(samples=[("AC", "GT")], where=("5p",)), dict(samples=["ACGT"], offset=-1), dict(samples=["ACGT"], offset=1.0),
    dict(samples=["ACGT"], offset=True), dict(samples=["ACGT"], offset=2), dict(samples=["ACGT"], offset=(0, 1)),
    dict(samples=[("AC", "GT")], offset=(0, 2)), dict(samples=["ACGT"], where="5p", offset=2**31),
    dict(samples=["ACGT"], mismatches=-1), dict(samples=["ACGT"], mismatches=5), dict(samples=["ACGT"], mismatches=1.0),
    dict(samples=[("ACGT", "AC")], mismatches=3), dict(samples=[("ACGT", "AC")], mismatches=(1, 1, 1)),
    dict(samples=["ACGT"], margin=0), dict(samples=["ACGT"], margin=65), dict(samples=["ACGT"], margin=1.5), dict(samples=["ACGT"], margin=True),
    dict(samples=["ACGT"], revcomp=1), dict(samples=["ACGT"], revcomp=(True, False)), dict(samples=["ACGT"], revcomp="yes")])
def test_value_errors(kw):
    from pyfastx_amd import demux
    with pytest.raises(ValueError):
        demux.demux_args(**kw)


# ------------------------------------------------------------------ the Demux object
def made_up():
    from pyfastx_amd import demux
    sample = np.array([1, -1, 0, 1, -2, 1, 0, -1], dtype=np.int32)
    dist = np.array([0, -1, 1, 2, 0, 0, 0, -1], dtype=np.int32)
    second = np.array([-1, -1, 3, -1, 0, 2, -1, -1], dtype=np.int32)
    order, bin_off, counts = bins_of(sample, 3)
    return demux, sample, dist, second, order, bin_off, counts


def test_demux_object_ids_and_summary():
    demux, sample, dist, second, order, bin_off, counts = made_up()
    assert order.tolist() == [2, 6, 0, 3, 5, 1, 7, 4] and bin_off.tolist() == [0, 2, 5, 5, 7, 8] and counts.tolist() == [2, 3, 0, 2, 1]
    dm = demux.Demux(["a", "b", "c"], sample, dist, second, counts, order, bin_off, np.full(8, 50))
    assert len(dm) == 8 and (dm.n_assigned, dm.n_unassigned, dm.n_ambiguous) == (5, 2, 1)
    assert dm.ids("a").tolist() == [2, 6] and dm.ids(1).tolist() == [0, 3, 5] and dm.ids("c").tolist() == []
    assert dm.unassigned_ids.tolist() == [1, 7] and dm.ambiguous_ids.tolist() == [4]
    with pytest.raises(KeyError):
        dm.ids("nobody")
    for bad in (3, -1, 1.0):
        with pytest.raises(ValueError):
            dm.ids(bad)
    assert dm.summary() == [("a", 2, 0.25, 1), ("b", 3, 0.375, 2), ("c", 0, 0.0, 0), ("unassigned", 2, 0.25, 0), ("ambiguous", 1, 0.125, 0)]
    # through ids: positions become read ids, repeats stay
    q = np.array([10, 11, 12, 10, 14, 15, 16, 17], dtype=np.int64)
    dm = demux.Demux(["a", "b", "c"], sample, dist, second, counts, order, bin_off, np.full(8, 50), q)
    assert dm.ids("b").tolist() == [10, 10, 15] and dm.unassigned_ids.tolist() == [11, 17] and dm.ambiguous_ids.tolist() == [14]
    empty = demux.Demux(["a"], *(np.zeros(0, dtype=np.int32),) * 3, np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64),
                        np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert empty.summary() == [("a", 0, 0.0, 0), ("unassigned", 0, 0.0, 0), ("ambiguous", 0, 0.0, 0)] and empty.ids("a").size == 0


def test_demux_object_intervals_and_paths():
    demux, sample, dist, second, order, bin_off, counts = made_up()
    L = np.array([50, 0, 5, 8, 9, 12, 13, 100], dtype=np.int64)
    mk = lambda segs: demux.Demux(["a", "b", "c"], sample, dist, second, counts, order, bin_off, L, None, segs)
    a, b = mk([("header", 0, 8)]).intervals()
    assert a.tolist() == [0] * 8 and b.tolist() == L.tolist() and a.dtype == b.dtype == np.int64
    a, b = mk([("5p", 1, 7)]).intervals()
    assert a.tolist() == [8, 0, 5, 8, 8, 8, 8, 8] and b.tolist() == L.tolist()
    a, b = mk([("3p", 2, 6)]).intervals()
    assert a.tolist() == [0] * 8 and b.tolist() == [42, 0, 0, 0, 1, 4, 5, 92]
    a, b = mk([("5p", 0, 6), ("3p", 0, 6)]).intervals()
    assert a.tolist() == [6, 0, 5, 6, 6, 6, 6, 6] and b.tolist() == [44, 0, 5, 6, 6, 6, 7, 94]
    dm = mk([("5p", 0, 6)])
    assert demux.bin_paths(dm, "/x/{sample}.fq", None, None) == [("a", 0, "/x/a.fq"), ("b", 1, "/x/b.fq"), ("c", 2, "/x/c.fq")]
    assert demux.bin_paths(dm, "{sample}_{sample}", "u.fq", "m.fq")[3:] == [("unassigned", 3, "u.fq"), ("ambiguous", 4, "m.fq")]
    for bad in ("/x/out.fq", "/x/{name}.fq", None):
        with pytest.raises(ValueError):
            demux.bin_paths(dm, bad, None, None)


# ------------------------------------------------------------------ the C entry
def test_declared_and_exported():
    from pyfastx_amd import _lib
    assert "fx_fastq_demux" in _lib.SYMBOLS and hasattr(_lib.Blob, "fastq_demux")
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    for word in ("int fx_fastq_demux(", "FX_DEMUX_SEQ5 0", "FX_DEMUX_SEQ3 1", "FX_DEMUX_HEADER 2", "FX_DEMUX_NONE (-1)", "FX_DEMUX_AMBIGUOUS (-2)"):
        assert word in hdr, word
    from pyfastx_amd import demux
    assert (demux.NONE, demux.AMBIGUOUS, demux.SOURCES) == (NONE, AMBIGUOUS, {"5p": SEQ5, "3p": SEQ3, "header": HEADER})
    from pyfastx_amd.api import Fastq
    from pyfastx_amd.pair import FastqPair
    assert all(hasattr(c, m) for c in (Fastq, FastqPair) for m in ("demux", "demux_write"))


# ------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fixture_reads():
    reads = parse_fastq(open(os.path.join(DATA, "test.fq"), "rb").read())
    assert len(reads) == 800
    return reads


@pytest.mark.parametrize("mm,assigned", [((0, 0), 757), ((0, 1), 789), ((1, 0), 766), ((1, 1), 800)])
def test_fixture_pins(fixture_reads, mm, assigned):
    from pyfastx_amd import demux
    args = demux.demux_args({"s": ("CAATGGAA", "CGAGGCTG")}, mismatches=mm)
    segs, sheet = segments(args)
    sample, dist, second = demux_truth(fixture_reads, segs, sheet, 1)
    assert int((sample == 0).sum()) == assigned and int((sample == NONE).sum()) == 800 - assigned and not (second != -1).any()
    assert np.array_equal(dist[sample == 0] >= 0, np.ones(assigned, dtype=bool))


def test_fixture_distances(fixture_reads):
    pairs = {}
    for H, s in fixture_reads:
        d = (distance(window(H, s, HEADER, 0, 8), b"CAATGGAA"), distance(window(H, s, HEADER, 1, 8), b"CGAGGCTG"))
        pairs[d] = pairs.get(d, 0) + 1
    assert pairs == {(0, 0): 757, (0, 1): 32, (1, 0): 9, (1, 1): 2}
