"""-m gpu: Fastq.demux / demux_write and FastqPair.demux_write (fx_fastq_demux, csrc/fx_fastq_demux.hpp) against the plain-Python
definition tests/demux_truth.py over fq[i].description / fq[i].seq of the same file -- every comparison exact -- on the
fixture, on every input of tests/golden/fastq_edge.json and on a generated file of irregular reads with barcodes planted."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA, load_golden
from demux_truth import AMBIGUOUS, NONE, bins_of, demux_truth, demux_truth_fast, segments
from trim_truth import record

pytestmark = pytest.mark.gpu

EDGE = load_golden("fastq_edge")
DUAL = {"s": ("CAATGGAA", "CGAGGCTG")}


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _lat(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def reads_of(fq):
    """[(H, s)] from the object API: the header as Read.description shows it, the bases."""
    return [(_lat(fq[i].description), _lat(fq[i].seq)) for i in range(len(fq))]


def check(fq, reads, samples, ids=None, truth=demux_truth, **kw):
    """One demux call against the definition: the three columns, the counters, the grouping -> (Demux, the truth's columns)."""
    from pyfastx_amd import demux
    args = demux.demux_args(samples, **kw)
    segs, sheet = segments(args)
    sel = reads if ids is None else [reads[int(i)] for i in ids]
    want = truth(sel, segs, sheet, args["margin"])
    dm = fq.demux(samples, ids=ids, **kw)
    ns = len(sheet)
    assert dm.names == args["names"] and len(dm) == len(sel)
    for name, got, w in zip(("sample", "dist", "second"), (dm.sample, dm.dist, dm.second), want):
        assert got.dtype == np.int32 and np.array_equal(got, w), (name, kw)
    order, bin_off, counts = bins_of(want[0], ns)
    assert dm.counts.dtype == np.int64 and np.array_equal(dm.counts, counts)
    assert dm.order.dtype == dm.bin_off.dtype == np.int64
    assert np.array_equal(dm.bin_off, bin_off) and np.array_equal(dm.order, order)       # stable: ascending inside a bin
    assert (dm.n_assigned, dm.n_unassigned, dm.n_ambiguous) == (int(counts[:ns].sum()), int(counts[ns]), int(counts[ns + 1]))
    return dm, want


def sheet_from(reads, where, off, ln, rng, extra=2):
    """Barcodes that occur: the window of a few reads at that place (a missing or odd byte becomes N), and random ones."""
    from demux_truth import SOURCES, window
    out = []
    for H, s in reads[:3]:
        w = window(H, s, SOURCES[where], off, ln)
        out.append("".join(chr(c) if c is not None and chr(c) in "ACGT" else "N" for c in w))
    for _ in range(extra):
        out.append("".join("ACGT"[int(k)] for k in rng.integers(0, 4, ln)))
    return sorted(set(out))


# ------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fixture(fx, tmp_path_factory):
    p = tmp_path_factory.mktemp("demux") / "test.fq"
    shutil.copy(os.path.join(DATA, "test.fq"), p)
    fq = fx.Fastq(str(p))
    assert len(fq) == 800
    return fq, reads_of(fq)


@pytest.mark.parametrize("mm,assigned", [((0, 0), 757), ((0, 1), 789), ((1, 0), 766), ((1, 1), 800)])
def test_fixture_pins(fixture, mm, assigned):
    fq, reads = fixture
    dm, _ = check(fq, reads, DUAL, mismatches=mm)
    assert dm.n_assigned == assigned and dm.n_unassigned == 800 - assigned and dm.n_ambiguous == 0
    assert dm.ids("s").size == assigned and dm.summary()[0][:2] == ("s", assigned)
    if mm == (1, 1):
        assert np.bincount(dm.dist).tolist() == [757, 41, 2] and dm.summary()[0] == ("s", 800, 1.0, 757)


def test_fixture_one_part_and_a_close_sample(fixture):
    fq, reads = fixture
    dm, _ = check(fq, reads, {"i5": "CGAGGCTG"}, offset=1, mismatches=0)
    assert dm.n_assigned == 757 + 9                                    # part 1 exact: the (0, 0) and the (1, 0) reads
    check(fq, reads, {"i5": "CGAGGCTG"}, offset=1, mismatches=1)
    check(fq, reads, ["CAATGGAA"], offset=0, mismatches=0)
    check(fq, reads, ["CAATGG"], mismatches=0)                         # the sheet is shorter than the index read
    check(fq, reads, ["CAATGGAAAC"], mismatches=2)                     # and longer: two ABSENT slots
    near = {"a": ("CAATGGAA", "CGAGGCTG"), "b": ("CAATGGAA", "CGAGGCGG")}
    d1, w1 = check(fq, reads, near, margin=1)
    d2, w2 = check(fq, reads, near, margin=2)
    assert d1.n_ambiguous < d2.n_ambiguous and d2.n_ambiguous >= 757  # one letter apart: every exact read is ambiguous at margin 2
    check(fq, reads, near, margin=64, mismatches=(8, 8))
    check(fq, reads, near, revcomp=(False, True))
    check(fq, reads, {"n": ("NNNNNNNN", "CGAGGNNN")}, mismatches=0)


@pytest.mark.parametrize("where", ["5p", "3p"])
def test_fixture_inline_windows(fixture, where):
    fq, reads = fixture
    rng = np.random.default_rng(21)
    for ln in (1, 15, 16, 17, 32):
        for off in (0, 7, 140, 149, 150):
            check(fq, reads, sheet_from(reads, where, off, ln, rng), where=where, offset=off, mismatches=min(ln, 2))
    check(fq, reads, [("ACGTAC", "GGT")], where=("5p", "3p"), offset=(2, 1), mismatches=(3, 2))
    check(fq, reads, sheet_from(reads, where, 2**31 - 1, 4, rng), where=where, offset=2**31 - 1, mismatches=4)


@pytest.mark.parametrize("ns", [1, 64, 65, 1024, 1025, 4096])
def test_fixture_sheet_sizes(fixture, ns):
    """Random 8 + 8 sheets with the run's own barcode last, against the numpy form of the truth."""
    fq, reads = fixture
    rng = np.random.default_rng(ns)
    rows = {("CAATGGAA", "CGAGGCTG")}
    while len(rows) < ns:
        rows.add(tuple("".join("ACGT"[int(k)] for k in rng.integers(0, 4, 8)) for _ in range(2)))
    rows = sorted(rows - {("CAATGGAA", "CGAGGCTG")}) + [("CAATGGAA", "CGAGGCTG")]
    ids = None if ns <= 1025 else np.arange(0, 800, 3)
    dm, want = check(fq, reads, rows, ids=ids, truth=demux_truth_fast, mismatches=(3, 3))
    assert int((want[0] == ns - 1).sum()) >= 200                       # a truth that assigns nothing cannot pass silently


def test_fixture_ids(fixture):
    fq, reads = fixture
    ids = np.random.default_rng(5).integers(0, 800, 2500)
    dm, want = check(fq, reads, DUAL, ids=ids, mismatches=(0, 0))
    assert np.array_equal(dm.ids("s"), ids[want[0] == 0]) and np.array_equal(dm.unassigned_ids, ids[want[0] == NONE])
    dm = fq.demux(DUAL, ids=[])
    assert len(dm) == 0 and dm.counts.tolist() == [0, 0, 0] and dm.bin_off.tolist() == [0, 0, 0, 0] and dm.order.size == 0
    assert dm.ids("s").size == 0 and dm.summary()[0] == ("s", 0, 0.0, 0)
    for bad in ([800], [-1], [0, 807, 0]):
        with pytest.raises(IndexError, match="index out of range"):
            fq.demux(DUAL, ids=bad)
    with pytest.raises(ValueError):
        fq.demux(DUAL, margin=0)


def test_errors_at_the_abi(fixture):
    """Below the Python checks: FX_ERANGE with *first_bad, FX_EINVAL for every argument outside its range, FX_ESTATE."""
    from pyfastx_amd import _lib
    fq, _ = fixture
    blob = fq._qc_blob()
    bc = np.frombuffer(b"ACGTACGA", dtype=np.uint8).reshape(2, 4)
    ok = dict(barcodes=bc, src=[0], off=[0], length=[4], mm=[1], margin=1)
    cols = blob.fastq_demux(**ok, want_order=False)
    assert sorted(cols) == ["counts", "dist", "sample", "second"] and int(cols["counts"].sum()) == 800
    with pytest.raises(_lib.FxError) as e:
        blob.fastq_demux(**ok, ids=np.array([0, 1, 800], dtype=np.int64))
    assert e.value.code == _lib.FX_ERANGE and e.value.first_bad == 2
    low = np.frombuffer(b"ACGTacga", dtype=np.uint8).reshape(2, 4)
    for kw in (dict(margin=0), dict(margin=65), dict(src=[3]), dict(src=[-1]), dict(off=[-1]), dict(src=[2], off=[2]), dict(mm=[5]), dict(mm=[-1]),
               dict(barcodes=low), dict(barcodes=np.zeros((2, 33), dtype=np.uint8) + 65, length=[33], mm=[0]),
               dict(barcodes=np.zeros((4097, 4), dtype=np.uint8) + 65), dict(barcodes=np.zeros((0, 4), dtype=np.uint8))):
        with pytest.raises(_lib.FxError) as e:
            blob.fastq_demux(**{**ok, **kw})
        assert e.value.code == _lib.FX_EINVAL, kw
    raw = _lib.Blob.from_bytes(b"@r\nACGT\n+\nIIII\n", device=0)
    with pytest.raises(_lib.FxError) as e:
        raw.fastq_demux(**ok)
    assert e.value.code == _lib.FX_ESTATE


# ------------------------------------------------------------------ edge inputs
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_inputs(fx, tmp_path, name):
    """Every input of fastq_edge.json, opened as a file: empty and short reads, the last read at the end of the stream, CRLF."""
    path = tmp_path / (name + ".fq")
    path.write_bytes(EDGE[name]["text"].encode("latin-1"))
    fq = fx.Fastq(str(path))
    assert len(fq) == EDGE[name]["count"]
    reads = reads_of(fq)
    rng = np.random.default_rng(9)
    for where in ("5p", "3p"):
        for ln, off in ((1, 0), (2, 1), (4, 0), (5, 3), (20, 0), (32, 2)):
            check(fq, reads, sheet_from(reads, where, off, ln, rng), where=where, offset=off, mismatches=min(ln, 2))
    check(fq, reads, DUAL)
    check(fq, reads, ["NN"], mismatches=0)
    check(fq, reads, [("AC", "GT"), ("GG", "NN")], where=("5p", "3p"), mismatches=(1, 2), ids=list(range(len(reads))) * 2)


# ------------------------------------------------------------------ a generated file
def _sheet96(rng):
    """96 dual 8 + 8 barcodes: 80 random ones, and 16 that are one letter from one of the first 16."""
    rows = set()
    while len(rows) < 80:
        rows.add(tuple("".join("ACGT"[int(k)] for k in rng.integers(0, 4, 8)) for _ in range(2)))
    rows = sorted(rows)
    for k in range(16):
        a, b = rows[k]
        j = int(rng.integers(0, 8))
        rows.append((a[:j] + "ACGT"[("ACGT".index(a[j]) + 1) % 4] + a[j + 1:], b))
    assert len(set(rows)) == 96
    return rows


def _irregular(n, seed):
    """n reads of 0..300 bases; the barcodes of a random sample, with 0..3 letters changed, in the header's index field and at
    the two ends of the read; headers with and without an index field, some without any ':', some longer than 80 bytes."""
    rng = np.random.default_rng(seed)
    rows = _sheet96(rng)
    odd = "acgtNRY"
    parts1, parts2 = [], []
    for i in range(n):
        a, b = (list(x) for x in rows[int(rng.integers(0, 96))])
        for _ in range(int(rng.choice(4, p=[0.5, 0.25, 0.15, 0.10]))):
            x = a if rng.random() < 0.5 else b
            x[int(rng.integers(0, 8))] = (odd + "ACGT")[int(rng.integers(0, len(odd) + 4))]
        a, b = "".join(a), "".join(b)
        body = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(0, 285))))
        s = a + body + b
        kind = i % 16
        if kind == 3:
            s = s[:int(rng.integers(0, 17))]                  # shorter than the two windows, down to an empty read
        h = "@r%d" % i
        if kind == 5:
            h += " no index field"
        elif kind == 6:
            h += " 1:N:0:" + a                                # no '+'
        elif kind == 7:
            h += " " + "x" * 90 + " 1:N:0:" + a + "+" + b     # the field lies beyond the first 80 bytes
        elif kind == 8:
            h += ":" + "G" * 40 + "+" + "T" * 26              # a field of 67 bytes
        elif kind == 9:
            h += " 1:N:0:" + a + "AT+" + b + "CC"             # index reads longer than the sheet's barcodes
        else:
            h += " 1:N:0:" + a + "+" + b
        q = "".join("F:,#"[int(k)] for k in rng.choice(4, len(s), p=[0.8, 0.12, 0.06, 0.02]))
        parts1.append("%s\n%s\n+\n%s\n" % (h, s, q))
        parts2.append("%s\n%s\n+\n%s\n" % (h, s[::-1], q[::-1]))
    return rows, "".join(parts1).encode(), "".join(parts2).encode()


@pytest.fixture(scope="module")
def generated(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("demux_gen")
    rows, raw1, raw2 = _irregular(2000, 33)
    (d / "g_1.fq").write_bytes(raw1)
    (d / "g_2.fq").write_bytes(raw2)
    fq1, fq2 = fx.Fastq(str(d / "g_1.fq")), fx.Fastq(str(d / "g_2.fq"))
    assert len(fq1) == len(fq2) == 2000
    return rows, fq1, fq2, reads_of(fq1)


@pytest.mark.parametrize("kw", [dict(), dict(where=("5p", "3p"))])
def test_generated(generated, kw):
    from pyfastx_amd import demux
    rows, fq, _, reads = generated
    kw = dict(kw, mismatches=(1, 1), margin=2)
    segs, sheet = segments(demux.demux_args(rows, **kw))
    s, d, _ = demux_truth_fast(reads, segs, sheet, 2)
    # before the device is compared: a truth that assigns nothing cannot pass silently
    assert int((s >= 0).sum()) >= 50 and int((s == NONE).sum()) >= 50 and int((s == AMBIGUOUS).sum()) >= 50
    assert int(((s >= 0) & (d > 0)).sum()) >= 10
    lens = np.array([len(r[1]) for r in reads])
    assert lens.min() == 0 and lens.max() >= 290
    check(fq, reads, rows, truth=demux_truth_fast, **kw)
    check(fq, reads, rows, truth=demux_truth_fast, **dict(kw, margin=1, mismatches=(2, 3)))
    ids = np.random.default_rng(2).integers(0, 2000, 700)
    check(fq, reads, rows[:7], ids=ids, **kw)                   # the slow truth on a gathered subset


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    return [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]


def test_demux_write_cut(generated, tmp_path):
    from pyfastx_amd import demux
    rows, fq, _, reads = generated
    kw = dict(where=("5p", "3p"), mismatches=(1, 1), margin=2)
    segs, sheet = segments(demux.demux_args(rows, **kw))
    want = demux_truth_fast(reads, segs, sheet, 2)[0]
    order, bin_off, counts = bins_of(want, 96)
    dm = fq.demux(rows, **kw)
    quals = [_lat(fq[i].qual) for i in range(len(fq))]
    min_len = 20
    out = fq.demux_write(dm, str(tmp_path / "s_{sample}.fq"), unassigned=str(tmp_path / "none.fq"), ambiguous=str(tmp_path / "amb.fq"),
                         cut=True, min_len=min_len, batch_bytes=20000)
    total = kept = 0
    for k in range(98):
        key = str(k) if k < 96 else ("unassigned", "ambiguous")[k - 96]
        path = str(tmp_path / ("s_%d.fq" % k)) if k < 96 else str(tmp_path / ("none.fq", "amb.fq")[k - 96])
        pos = order[bin_off[k]:bin_off[k + 1]]
        if pos.size == 0:
            assert key not in out and not os.path.exists(path)
            continue
        parts = []
        for i in pos:
            H, s = reads[int(i)]
            L = len(s)
            a = min(L, 8)
            b = max(a, L - 8)
            if b - a >= min_len:
                parts.append(record(H, np.frombuffer(s, dtype=np.uint8), np.frombuffer(quals[int(i)], dtype=np.uint8), a, b))
        assert open(path, "rb").read() == b"".join(parts), key
        assert out[key] == (path, len(parts))
        total += pos.size
        kept += len(parts)
    assert total == 2000 and sum(r for _, r in out.values()) == kept and 0 < kept < 2000
    # whole reads, the extra bins dropped
    out = fq.demux_write(dm, str(tmp_path / "w_{sample}.fq"))
    assert sum(r for _, r in out.values()) == int(counts[:96].sum()) and "unassigned" not in out and "ambiguous" not in out
    k = int(np.argmax(counts[:96]))
    assert [r[0] for r in _records(out[str(k)][0])] == [reads[int(i)][0] for i in order[bin_off[k]:bin_off[k + 1]]]
    with pytest.raises(ValueError):
        fq.demux_write(dm, str(tmp_path / "nothing.fq"))
    with pytest.raises(ValueError):
        fq.demux_write(fq.demux(rows[:2], ids=[1, 2]).sample, str(tmp_path / "{sample}.fq"))


def test_pair_demux_write(fx, generated, tmp_path):
    rows, fq1, fq2, reads = generated
    pair = fx.FastqPair(fq1, fq2)
    dm = pair.demux(rows, mate=1, mismatches=(1, 1), margin=2)
    ref = fq1.demux(rows, mismatches=(1, 1), margin=2)
    assert dm.mate == 1 and np.array_equal(dm.sample, ref.sample) and np.array_equal(dm.order, ref.order)
    out = pair.demux_write(dm, str(tmp_path / "{sample}_R1.fq"), str(tmp_path / "{sample}_R2.fq"),
                           unassigned=(str(tmp_path / "u_R1.fq"), str(tmp_path / "u_R2.fq")))
    assert "unassigned" in out and "ambiguous" not in out
    pairs = 0
    for key, (p1, p2, n) in out.items():
        k = 96 if key == "unassigned" else int(key)
        r1, r2 = _records(p1), _records(p2)
        pos = dm.positions(k)
        assert len(r1) == len(r2) == n == pos.size > 0
        assert [r[0] for r in r1] == [r[0] for r in r2] == [reads[int(i)][0] for i in pos]      # the two files stay in step
        assert all(a[1] == b[1][::-1] for a, b in zip(r1, r2))
        pairs += n
    assert pairs == dm.n_assigned + dm.n_unassigned
    # the other mate: reversed reads carry the barcodes at the other ends
    d2 = pair.demux(rows, mate=2, where=("3p", "5p"), mismatches=(8, 8), margin=1)
    assert d2.mate == 2 and d2.n_unassigned == 0
    out = pair.demux_write(d2, str(tmp_path / "c_{sample}_R1.fq"), str(tmp_path / "c_{sample}_R2.fq"),
                           ambiguous=(str(tmp_path / "ca_R1.fq"), str(tmp_path / "ca_R2.fq")), cut=True)
    assert sum(n for _, _, n in out.values()) == 2000
    for p1, p2, n in out.values():                            # the windows come off the mate that was looked at, not off the other
        assert all(len(b[1]) == max(0, len(a[1]) - 16) and a[0] == b[0] for a, b in zip(_records(p1), _records(p2)))
    with pytest.raises(ValueError):
        pair.demux(rows, mate=3)
