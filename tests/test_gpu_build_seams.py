"""-m gpu: the FASTA and FASTQ index builds swept across every seam of the scan (tests/seam_cases.py) -- the 16-byte lane
chunk, the 1 KiB wave row, the 4 KiB granule, the 8 / 16 / 32 KiB run of the fused composition scan, the 16 KiB FASTQ record
slot, the 32 KiB scan workgroup, the 64 KiB span and one-read FASTQ run, the 1 MiB prefix chunk, the partial (or empty) tail
granule, the first table capacity.  Each hand-over has code of its own (a look-back at data[gp - 1], prevnl / nl_prefix, the
line-length hint carried from row to row, the overflow list, the table that regrows); a probe that is hard for it is slid
so that the seam falls in front of every byte of it, in LF and in CRLF.  Truth is the CPU oracle, every comparison exact.

One parametrised case is one sweep of small builds: (probe, seam kind, line end or background).  A failure names the
placement: probe, seam kind, the marked byte, d (the marked byte lies at seam + d) and the line end.  Paths are chosen by the
shape of the input alone; three tests read the launch counters to make sure the shapes still choose them."""
import numpy as np
import pytest

import seam_cases as sc
from test_gpu_kernels import assert_fasta_equal

pytestmark = pytest.mark.gpu

FASTA_PROBES = ("H", "H0", "B", "O1", "O3", "G", "T", "CR", "LH")
FASTQ_PROBES = ("R", "RP", "RQ", "R1", "RS", "RL")
WIDTHS = [1, 2, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.fixture(scope="module")
def L():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return _lib


def _rng(*key):
    return np.random.default_rng([11] + [int(x) for x in key])


def _launches(b, call):
    b.prof_enable(1)
    b.prof_reset()
    res = call()
    out = {k: n for k, (_, n) in b.prof_read().items()}
    b.prof_enable(0)
    return res, out


# ----------------------------------------------------------------------------------------------------------- FASTA
def _fasta_both_names(oracle, L, raw, where):
    """all nine columns, n_seq, seq_len, the dense composition, the fused comp=True build column for column and the
    line-regular column (assert_fasta_equal), with the name cut at the first white space and with the whole header line"""
    for full_name in (False, True):
        try:
            b, _, _ = assert_fasta_equal(oracle, L, raw, full_name=full_name)
        except AssertionError as e:
            raise AssertionError("%s full_name=%s (%d bytes): %s" % (where, full_name, len(raw), e)) from None
        b.close()


# What follows the probe decides which code sees the seam.  "short": three lines, so the stream ends inside the granule behind the
# seam -- the partial tail granule, which k_gran_reduce (FASTA) or k_fastq_emit (FASTQ) computes with bounds-checked loads.
# "long": more than two granules, so the granules on both sides of the seam are whole ones of the scan kernel itself.
TAILS = ("short", "long")


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("eol", ["lf", "crlf"])
@pytest.mark.parametrize("kind", sc.FASTA_SEAMS)
@pytest.mark.parametrize("probe", FASTA_PROBES)
def test_fasta_probe_across_seam(oracle, L, probe, kind, eol, tail):
    E, seam = sc.EOLS[eol], sc.SEAMS[kind]
    text, places = sc.fasta_probes(E)[probe]
    tail_lines = 3 if tail == "short" else 3 + 2 * 4096 // sc.WIDTH
    for i, (mark, d) in enumerate(places):
        raw = sc.place_fasta(text, mark, seam, d, E, _rng(seam, i), tail_lines=tail_lines)
        if tail == "short":
            assert len(raw) // 4096 == seam // 4096 or probe == "LH"      # the granule the seam opens is the partial last one
        else:
            assert len(raw) // 4096 >= (seam + d - mark + len(text)) // 4096 + 2
        _fasta_both_names(oracle, L, raw, "probe %s, %s seam at %d, mark %d, d %+d, %s, %s tail" % (probe, kind, seam, mark, d, eol, tail))


@pytest.mark.parametrize("eol", ["lf", "crlf"])
@pytest.mark.parametrize("kind", sc.FASTA_SEAMS)
@pytest.mark.parametrize("probe", FASTA_PROBES)
def test_fasta_stream_ends_at_seam(oracle, L, probe, kind, eol):
    """END: the stream is seam + d bytes long, d in -2 .. 2 (d = 0: a whole number of granules, the tail granule is empty) and
    ends in front of byte `mark` of the probe -- after a terminated line, in an unterminated one, after a CR, after a bare '>'
    or a bare header, one cut per kind the probe has."""
    E, seam = sc.EOLS[eol], sc.SEAMS[kind]
    text, _ = sc.fasta_probes(E)[probe]
    for mark in sc.end_marks(text):
        for d in (-2, -1, 0, 1, 2):
            raw = sc.truncated_fasta(text, mark, seam, d, E, _rng(seam, mark))
            assert len(raw) == seam + d
            _fasta_both_names(oracle, L, raw, "END of probe %s cut at byte %d, %s seam at %d, d %+d, %s" % (probe, mark, kind, seam, d, eol))


def test_fasta_fused_build_takes_the_scan_comp_kernel(L):
    """the comp=True half of every sweep above is k_scan_comp, the other half k_span_scan; both hand the tail granule to k_gran_reduce"""
    text, _ = sc.fasta_probes(b"\n")["H"]
    b = L.Blob.from_bytes(sc.place_fasta(text, 0, sc.SEAMS["4K"], 0, b"\n", _rng(0)))
    _, fused = _launches(b, lambda: b.fasta_build(False, comp=True))
    _, plain = _launches(b, lambda: b.fasta_build(False))
    assert fused.get("k_scan_comp") == 1 and "k_span_scan" not in fused, fused
    assert plain.get("k_span_scan") == 1 and "k_scan_comp" not in plain, plain
    for k in (fused, plain):
        assert k.get("k_gran_reduce") == 1 and k.get("k_gran_prefix") == 1 and k.get("k_hdr_rec", 0) >= 1, k
    b.close()


@pytest.mark.parametrize("eol", ["lf", "crlf"])
def test_fasta_line_widths(oracle, L, eol):
    """One record of at least three granules per line width, short last line, all in one stream: the widths around which the
    scan's fast path (at most one newline per lane, the positions an arithmetic progression) turns on and off."""
    raw = sc.width_sweep(WIDTHS, sc.EOLS[eol], _rng(3))
    _fasta_both_names(oracle, L, raw, "line widths, %s" % eol)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_fasta_record_count_at_first_capacity(oracle, L, n):
    """a fresh handle's table holds 4096 records: one less, exactly as many, one more (the table regrows, the records part runs again)"""
    _fasta_both_names(oracle, L, sc.one_line_records(n), "%d one-line records" % n)


def test_fasta_record_count_fills_the_regrown_table(oracle, L):
    """4097 records regrow a fresh handle's table to n + n / 16 + 16 = 4369 rows.  The handle keeps that table: the same device
    buffer is then filled with a stream of exactly 4369 records (the table is full to the last row, nothing regrows) and with
    one of 4370 (it regrows a second time)."""
    import torch
    n0 = 4097
    cap = n0 + n0 // 16 + 16
    streams = [sc.one_line_records(n) for n in (n0, cap, cap + 1)]
    size = len(streams[-1])
    # the shorter streams end in one record whose sequence line is padded to the common size
    streams = [s if len(s) == size else s[:-1] + b"A" * (size - len(s)) + b"\n" for s in streams]
    assert all(len(s) == size for s in streams)
    dev = torch.device("cuda:0")
    t = torch.zeros(size, dtype=torch.uint8, device=dev)
    b = L.Blob.from_device(t.data_ptr(), size, device=0, keepalive=t)
    for raw, n in zip(streams, (n0, cap, cap + 1)):
        t.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        torch.cuda.synchronize(dev)
        recs, tot = oracle.fasta_index(raw)
        assert len(recs) == n
        for comp in (False, True):
            s = b.fasta_build(False, comp=comp)
            assert (s.n_seq, s.seq_len) == (n, tot)
            tab = b.fasta_table(n)
            for col in ("hoff", "boff", "blen", "slen", "llen", "elen", "norm", "dlen", "name_len"):
                np.testing.assert_array_equal(tab[col], recs[col].astype(tab[col].dtype), err_msg="%d records, comp=%s: %s" % (n, comp, col))
            np.testing.assert_array_equal(b.fasta_comp(n), oracle.fasta_comp(raw, n), err_msg="%d records, comp=%s" % (n, comp))
    b.close()


@pytest.mark.parametrize("eol", ["lf", "crlf"])
@pytest.mark.parametrize("mib,gpw", [(64, 4), (256, 8)])
def test_fasta_fused_run_seams(oracle, L, mib, gpw, eol):
    """k_scan_comp with 4 and with 8 granules per run (streams of at least 16384 and 65536 granules: just over 64 MiB and 256
    MiB): probe H with its '>' and with its header's line end at -1, 0 and +1 of six run seams, one fused build, rows and
    composition against the oracle."""
    E = sc.EOLS[eol]
    raw, where = sc.run_seam_stream(mib << 20, gpw * 4096, E, _rng(mib))
    assert len(raw) // 4096 + 1 >= (16384 if gpw == 4 else 65536) and (gpw == 8 or len(raw) // 4096 + 1 < 65536)
    a = np.frombuffer(raw, dtype=np.uint8)
    recs, tot = oracle.fasta_index(a)
    assert len(recs) == 18
    b = L.Blob.from_bytes(a)
    s, k = _launches(b, lambda: b.fasta_build(False, comp=True))
    assert k.get("k_scan_comp") == 1 and "k_span_scan" not in k, k
    assert (s.n_seq, s.seq_len) == (len(recs), tot)
    t = b.fasta_table(s.n_seq)
    for col in ("hoff", "boff", "blen", "slen", "llen", "elen", "norm", "dlen", "name_len"):
        np.testing.assert_array_equal(t[col], recs[col].astype(t[col].dtype), err_msg="%s (probes at %s)" % (col, where))
    np.testing.assert_array_equal(b.fasta_comp(s.n_seq), oracle.fasta_comp(a, len(recs)), err_msg="comp (probes at %s)" % (where,))
    b.close()


# ----------------------------------------------------------------------------------------------------------- FASTQ
def _fastq_equal(oracle, L, raw, where):
    """fastq_build(comp=False) and fastq_build(comp=True): n_reads, size, n_lines, the six columns, base and meta"""
    recs, size, ln = oracle.fastq_index(raw)
    c = oracle.fastq_composition(raw)
    base_w, meta_w = [c["a"], c["c"], c["g"], c["t"], c["n"]], [c["maxlen"], c["minlen"], c["minqs"], c["maxqs"], c["phred"]]
    b = L.Blob.from_bytes(raw)
    for comp in (False, True):
        tag = "%s comp=%s (%d bytes)" % (where, comp, len(raw))
        s = b.fastq_build(comp=comp)
        assert (s.n_reads, s.size, s.n_lines) == (len(recs), size, ln), tag
        t = b.fastq_table(s.n_reads)
        for col in ("name_off", "name_len", "dlen", "rlen", "soff", "qoff"):
            np.testing.assert_array_equal(t[col], recs[col].astype(t[col].dtype), err_msg="%s: %s" % (tag, col))
        base, meta = b.fastq_comp()
        assert base.tolist() == base_w and meta.tolist() == meta_w, (tag, base.tolist(), base_w, meta.tolist(), meta_w)
    b.close()


FASTQ_CASES = [(bg, tail) for bg in sc.FASTQ_BACKGROUNDS for tail in TAILS if not (bg.startswith("island") and tail == "short")]
# (an island stream is padded to 800 KiB behind the probe whatever is asked for: its tail is always long)


def _fastq_seam(text, kind, bg):
    """The offset of the seam kind for this probe and background.  At least five granules lie in front of it: a stream under
    four granules is never sampled for its line density and takes the two-read build whatever its reads are, so the small
    seam kinds move 64 KiB up (still a multiple of no larger seam) and a short-tail stream of 150-base reads is a one-read
    build too -- with the granule the seam opens on k_fastq_emit's list as the partial last one."""
    return sc.seam_offset(kind, max(sc.fastq_need(len(text), bg), 5 * 4096))


def _fastq_stream(text, kind, bg, tail, mark, d, i):
    E = sc.fastq_bg_eol(bg)
    seam = _fastq_seam(text, kind, bg)
    tail_records = 3 if tail == "short" else 4 + 2 * 4096 // sc.fastq_record_size(20 if bg == "r20" else 150, E, b"s" if bg == "r20" else b"bg")
    raw, island = sc.place_fastq(text, mark, seam, d, bg, _rng(seam, i), tail_records=tail_records)
    assert len(raw) >= 4 * 4096
    if tail == "long":
        assert len(raw) // 4096 >= (seam + d - mark + len(text)) // 4096 + 2
    elif len(text) < 1000:
        assert len(raw) // 4096 == seam // 4096                # the granule the seam opens is the partial last one
    return raw, island, seam


@pytest.mark.parametrize("bg,tail", FASTQ_CASES)
@pytest.mark.parametrize("kind", sc.FASTQ_SEAMS)
@pytest.mark.parametrize("probe", FASTQ_PROBES)
def test_fastq_probe_across_seam(oracle, L, probe, kind, bg, tail):
    text, places = sc.fastq_probes(sc.fastq_bg_eol(bg))[probe]
    for i, (mark, d) in enumerate(places):
        raw, _, seam = _fastq_stream(text, kind, bg, tail, mark, d, i)
        _fastq_equal(oracle, L, raw, "probe %s, %s seam at %d, mark %d, d %+d, background %s, %s tail" % (probe, kind, seam, mark, d, bg, tail))


@pytest.mark.parametrize("bg,tail", FASTQ_CASES)
@pytest.mark.parametrize("kind", ["4K", "16K", "1M"])
def test_fastq_backgrounds_take_their_kernels(L, kind, bg, tail):
    """The streams of the sweep above, at a small, a middle and a large seam, short and long tails.  150-base reads: the one-read
    build (k_fastq_lines, fused: its composition form under the same id, then the reduce under k_fastq_comp).  20-base reads:
    the sampled line density chooses the two-read build -- k_span_scan<1> counts, k_fastq_emit reads every granule again, no
    line records.  The island: still the one-read build, and the island's granules hold more lines than a record slot
    (FQL_CAP), which is the rule by which k_fastq_lines puts a granule on the overflow list.  (The length of that list is not
    readable from outside the library and the launch counters hold no grid sizes, so that it is not empty is inferred from the
    newline counts here; the rows of the island's reads, which only k_fastq_emit writes from that list, are compared in the
    sweep.)"""
    text, _ = sc.fastq_probes(sc.fastq_bg_eol(bg))["R"]
    raw, island, _ = _fastq_stream(text, kind, bg, tail, 0, 0, 5)
    b = L.Blob.from_bytes(raw)
    _, plain = _launches(b, lambda: b.fastq_build())
    _, fused = _launches(b, lambda: b.fastq_build(comp=True))
    if bg == "r20":
        for k in (plain, fused):
            assert k.get("k_span_scan") == 1 and k.get("k_fastq_emit") == 1 and "k_fastq_lines" not in k and "k_fastq_rows" not in k, k
        assert b.fastq_comp_info()[2] is False
    else:
        for k in (plain, fused):
            assert k.get("k_fastq_lines") == 1 and k.get("k_fastq_rows") == 1 and k.get("k_fastq_emit") == 1 and "k_span_scan" not in k, k
        assert "k_fastq_comp" not in plain and fused.get("k_fastq_comp", 0) >= 1, (plain, fused)     # k_fastq_lines_comp + k_fastq_comp_reduce
        runs, recounted, one_read = b.fastq_comp_info()
        assert runs == (len(raw) // 4096 + 15) // 16
    if island:
        nl = sc.newlines_per_granule(raw)
        inside = np.arange((island[0] + 4095) // 4096, island[1] // 4096)
        assert inside.size >= 3 and (nl[inside] > sc.FQL_CAP).all() and inside.max() < len(raw) // 4096
    b.close()
