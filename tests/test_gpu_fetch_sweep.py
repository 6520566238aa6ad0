"""-m gpu: the fetch kernels (k_fetch_lines, k_fetch, k_fastq_fetch, k_revcomp) swept over every line phase, answer
length, flag value and output layout, byte for byte against the plain reference of tests/fetch_truth.py (pinned to the
oracle by tests/test_fetch_truth_host.py).  Every test asserts the number of queries it compared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fetch_truth as T
from fetch_sweep_child import check_by_id, expected_of, open_shape

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    from pyfastx_amd import _lib
    _lib.lib()
    assert _lib.lib().fx_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return _lib


def _sweep(L, shapes, mode="all", **kw):
    n = 0
    for sh in shapes:
        b = open_shape(L, sh)
        k, bad = check_by_id(b, sh, T.queries(sh, mode), **kw)
        b.close()
        assert bad is None, bad
        n += k
    return n


# ------------------------------------------------------------------ a. every line phase, default kernels
@pytest.mark.parametrize("el", [1, 2])
def test_line_phase_sweep_small(L, el):
    """bpl 16, 17, 18, 31, 32, 33, slen = 3 bpl + 5: all pairs, all flags; out_len = b - a for every query"""
    assert _sweep(L, [T.shape_a(bpl, el) for bpl in T.A_SMALL]) == 20259 * 8


@pytest.mark.parametrize("el", [1, 2])
@pytest.mark.parametrize("bpl", T.A_LARGE)
def test_line_phase_sweep_two_and_three_steps(L, bpl, el):
    """bpl 60 and 70, slen = 2 bpl + 40: answers of up to 180 bytes, three steps of 64"""
    assert _sweep(L, [T.shape_a(bpl, el)]) == {60: 12880, 70: 16290}[bpl] * 8


# ------------------------------------------------------------------ b. shapes that leave the fast path
def test_shapes_off_the_fast_path(L):
    shapes = T.shapes_b()
    assert [s.name for s in shapes] == [
        "bpl1_el1", "bpl1_el2", "bpl2_el1", "bpl2_el2", "bpl15_el1", "bpl15_el2", "start_el1", "start_el2", "end_el1_nl", "end_el1_nonl",
        "end_el2_nl", "end_el2_nonl", "odd_line", "two_odd_lines", "space", "tab", "gt_inside", "one_line", "one_line_el2", "empty_between"]
    # slen 50: 1275 pairs; the odd-line records 67 and 56 bases; the records around the empty one 50 and 45
    assert _sweep(L, shapes) == 8 * (17 * 1275 + 2278 + 1596 + 1275 + 1035)
    sp = T.shape_space()                                    # the space is dropped, the tab kept
    ids, a, b, fl = T.queries(sp)
    lens = T.expected(sp, ids, a, b, fl)[2]
    assert ((lens == b - a - 1) == ((a <= 27) & (b > 27))).all() and ((lens == b - a) | (lens == b - a - 1)).all()
    tb = [s for s in shapes if s.name == "tab"][0]
    assert (T.expected(tb, *T.queries(tb))[2] == np.diff(T.expected(tb, *T.queries(tb))[1])).all()


# ------------------------------------------------------------------ c. the redo path and the mirror fix-up, forced
def test_forced_redo_and_mirror_fixup(L):
    """A row that claims line-regular for a record with an odd middle line: the fast path takes the query, finds the
    terminator misplaced and hands it to the general path; the answer is the despaced byte range of the arithmetic, cut to
    b - a, possibly shorter (a reversed short answer is moved down by take - got).  The record with a space likewise."""
    odd, sp = T.shapes_forced()
    assert odd.force == (0,) and sp.regular[0]
    lens = T.expected(odd, *T.queries(odd))
    short = lens[2] < np.diff(lens[1])
    assert short.any() and (short & ((T.queries(odd)[3] & 2) != 0)).any()      # short answers, reversed ones among them
    assert _sweep(L, [odd, sp]) == 8 * (2278 + 1275)


# ------------------------------------------------------------------ d. guard bytes
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_no_byte_outside_an_answer_fasta(L):
    import torch
    n = 0
    for sh in T.shapes_guard():
        ids, a, b, fl = q = T.queries(sh)
        buf, offs, lens = expected_of(sh, q)
        assert (lens == b - a).all()
        off, size = T.guard_offsets(b - a)
        assert set((off % 16).tolist()) == set(range(16))
        img = T.guard_image(size, off, [buf[offs[i]:offs[i + 1]].tobytes() for i in range(ids.size)])
        blob = open_shape(L, sh)
        d = [_dev(torch, x) for x in (ids, a, b, fl, off)]
        out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda:0")
        out_len = torch.zeros(ids.size, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        blob.fasta_fetch_dev(ids.size, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), d[4].data_ptr(),
                             flags_per_query=d[3].data_ptr(), out_len=out_len.data_ptr())
        blob.sync()
        got = out.cpu().numpy()
        assert np.array_equal(out_len.cpu().numpy(), b - a), sh.name
        if not np.array_equal(got, img):
            p = int(np.argmax(got != img))
            i = int(np.searchsorted(off, p, side="right")) - 1
            pytest.fail("%s: byte %d of the output (answer %d begins at %d and is %d long, flags %d): 0x%02x, expected 0x%02x"
                        % (sh.name, p, i, off[max(i, 0)], (b - a)[max(i, 0)], fl[max(i, 0)], got[p], img[p]))
        blob.close()
        n += ids.size
    assert n == 8 * (2 * (1431 + 1596 + 12880) + 5 * 1275)


# ------------------------------------------------------------------ e. every instantiation
def _ranges_case(sh, q, skip_form, n_long):
    """The compact sweep as byte ranges: the arithmetic's (off, blen, take), or (boff, blen, take, skip = a); n_long more
    ranges of 64 KiB that run off the end of the stream (read short, as fread does)."""
    ids, a, b, fl = q
    rows = sh.rows
    if skip_form:
        off = np.array([rows[i]["boff"] for i in ids.tolist()], dtype=np.int64)
        blen = np.array([rows[i]["blen"] for i in ids.tolist()], dtype=np.int64)
        skip = a.copy()
    else:
        ar = [T.arith_range(rows[i], x, y) for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())]
        off, blen = np.array([r[0] for r in ar], dtype=np.int64), np.array([r[1] for r in ar], dtype=np.int64)
        skip = np.zeros_like(a)
    take = b - a
    if n_long:
        j = np.arange(n_long, dtype=np.int64)
        r = rows[sh.ids[0]]
        off = np.concatenate([off, r["boff"] + (j * 3) % r["blen"]])
        blen = np.concatenate([blen, np.full(n_long, 1 << 16, dtype=np.int64)])
        take = np.concatenate([take, 1 + (j * 5) % 64])
        skip = np.concatenate([skip, (j % 7) if skip_form else 0 * j])
        fl = np.concatenate([fl, (j % 8).astype(np.uint8)])
    return off, blen, take, skip, fl


def test_every_entry_in_process(L):
    """The compact sweep through FX_LONG by id (k_fetch<true, 64, 16>), through byte ranges short (k_fetch<false, 8, 16>)
    and long (k_fetch<false, 64, 16>), with and without skip, and through fasta_fetch_alloc."""
    n = 0
    for sh in T.shapes_compact():
        b = open_shape(L, sh)
        q = T.queries(sh, "cycle")
        exp = expected_of(sh, q)
        for kw in (dict(via="fasta_fetch", flags=16), dict(via="fasta_fetch_alloc")):
            k, bad = check_by_id(b, sh, q, exp=exp, **kw)
            assert bad is None, bad
            n += k
        for skip_form in (False, True):
            for n_long in (0, q[0].size // 100 + 1):
                off, blen, take, skip, fl = _ranges_case(sh, q, skip_form, n_long)
                assert (blen.mean() > 512) == bool(n_long)          # what the library chooses the 64-lane kernel by
                buf, offs, out_len = b.fetch_ranges(off, blen, take, flags_per_query=fl, skip=skip if skip_form else None)
                bad = T.first_mismatch(buf, offs, out_len, *T.expected_ranges(sh.raw, off, blen, take, skip, fl))
                assert bad is None, "%s ranges skip=%s long=%d: %s" % (sh.name, skip_form, n_long, bad)
                n += off.size
        b.close()
    base = 2 * (1431 + 1596 + 5460 + 12880) + 5 * 1275 + 2278 + 1275
    longs = sum(T.n_queries(s, "cycle") // 100 + 1 for s in T.shapes_compact())
    assert n == 6 * base + 2 * longs


# The switches are read once per process: one fresh child per switch runs the compact sweep (tests/fetch_sweep_child.py).
# CHILD_SECONDS is what a child takes from start to end.  NOT YET MEASURED on an MI355X: the figure is an estimate (about
# 2 s of library load and device start, 1.5 s of the reference in Python -- measured on the CPU -- and 17 small streams of a
# few launches each); the child prints its own run time ("seconds"), which is to replace it.  The limit is ten times
# that -- it only has to tell slow from hung.
CHILD_SECONDS = 6.0
CHILD_TIMEOUT = 10 * CHILD_SECONDS
_child_died = []                                            # a child that crashed or hung: no further child is started


@pytest.mark.parametrize("switch", ["FX_FETCH_G=2", "FX_FETCH_G=8", "FX_FETCH_G=16", "FX_FETCH_LEAN=0", "FX_FETCH_NP=2", "FX_FETCH_COAL=1"])
def test_every_instantiation_in_a_child(L, switch):
    """k_fetch<true, 2 / 8 / 16, 16>, k_fetch<true, 4, 16> without the list, k_fetch_lines<4, 2>, k_fetch_lines<4, 1, true>"""
    if _child_died:
        pytest.fail("not started: the child for %s crashed or hung" % _child_died[0])
    env = dict(os.environ)
    name, value = switch.split("=")
    env[name] = value
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "fetch_sweep_child.py")], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_died.append(switch)
        pytest.fail("%s: the child did not end within %.0f s" % (switch, CHILD_TIMEOUT))
    if p.returncode < 0 or p.returncode in (134, 139):
        _child_died.append(switch)
        pytest.fail("%s: the child ended on status %d\n%s" % (switch, p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(switch, res)
    assert res["mismatch"] is None, res["mismatch"]
    base = 2 * (1431 + 1596 + 5460 + 12880) + 5 * 1275 + 2278 + 1275
    coal = sum(lead + 192 + (-(lead + 192)) % 16 + 32 for lead in range(4))
    assert res["checked"] == base + (coal if name == "FX_FETCH_COAL" else 0)


# ------------------------------------------------------------------ f. k_fastq_fetch
WANTS = (("seq",), ("qual",), ("quali",), ("seq", "qual", "quali"))
FQ_STREAMS = [(False, True), (False, False), (True, True), (True, False)]


def _fastq_blob(L, raw):
    b = L.Blob.from_bytes(raw)
    s = b.fastq_build()
    rows = T.fastq_rows(raw)
    assert s.n_reads == len(rows) == T.FQ_MAX
    t = b.fastq_table(s.n_reads)
    assert list(zip(t["soff"].tolist(), t["qoff"].tolist(), t["rlen"].tolist())) == rows
    return b, rows


def _fastq_expected(raw, rows, ids, phred, flags):
    parts = [T.fastq_read(raw, *rows[i], phred, flags) for i in ids.tolist()]
    return (np.frombuffer(b"".join(p[0] for p in parts), dtype=np.uint8), np.frombuffer(b"".join(p[1] for p in parts), dtype=np.uint8),
            np.concatenate([p[2] for p in parts]))


def _fastq_check(b, raw, rows, phreds=(0, 33, 64)):
    n = 0
    rlen = np.array([r[2] for r in rows], dtype=np.int64)
    for ids in T.fastq_batches(len(rows)):
        for flags in (0, 2, 4, 6):
            for phred in phreds:
                exp = _fastq_expected(raw, rows, ids, phred, flags)
                for want in WANTS:
                    got = b.fastq_fetch(ids, rlen[ids], phred=phred, seq_flags=flags, want=want)
                    assert np.array_equal(got[3][1:], np.cumsum(rlen[ids]))
                    for k, key in enumerate(("seq", "qual", "quali")):
                        if key in want:
                            assert np.array_equal(got[k], exp[k]), (key, flags, phred, want)
                        else:
                            assert got[k] is None
                    n += ids.size
    return n


@pytest.mark.parametrize("crlf,final_nl", FQ_STREAMS)
def test_fastq_fetch_every_length(L, crlf, final_nl):
    """read lengths 1 .. 300; seq_flags 0, 2, 4, 6; phred 0, 33, 64; each output alone and all three; two batches"""
    raw = T.fastq_stream(crlf, final_nl)
    b, rows = _fastq_blob(L, raw)
    assert _fastq_check(b, raw, rows) == (300 + 307) * 4 * 3 * 4
    b.close()


def test_fastq_quali_wraps_the_same_on_both_paths(L):
    """quality bytes >= 128: the 16-byte path (reads inside the stream) and the byte path (the first and the last read)
    both give byte - phred wrapped to int8"""
    raw = T.fastq_stream(high=True)
    b, rows = _fastq_blob(L, raw)
    assert max(raw[rows[0][1]:rows[0][1] + rows[0][2]] + raw[rows[-1][1]:rows[-1][1] + rows[-1][2]]) >= 128     # on the byte path too
    assert _fastq_check(b, raw, rows) == (300 + 307) * 4 * 3 * 4
    b.close()


def test_no_byte_outside_an_answer_fastq(L):
    import torch
    n = 0
    for crlf, final_nl in FQ_STREAMS:
        raw = T.fastq_stream(crlf, final_nl)
        b, rows = _fastq_blob(L, raw)
        rlen = np.array([r[2] for r in rows], dtype=np.int64)
        for ids in T.fastq_batches(len(rows)):
            off, size = T.guard_offsets(rlen[ids])
            for flags, phred in ((0, 33), (6, 64)):
                exp = _fastq_expected(raw, rows, ids, phred, flags)
                cut = np.concatenate([[0], np.cumsum(rlen[ids])])
                imgs = [T.guard_image(size, off, [e[cut[i]:cut[i + 1]].view(np.uint8).tobytes() for i in range(ids.size)]) for e in exp]
                d_ids, d_off = _dev(torch, ids), _dev(torch, off)
                outs = [torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
                torch.cuda.synchronize()
                L.check(L.lib().fx_fastq_fetch(b._h, L.FX_DEVICE, ids.size, d_ids.data_ptr(), phred, flags, outs[0].data_ptr(),
                                               outs[1].data_ptr(), outs[2].data_ptr(), d_off.data_ptr()))
                b.sync()
                for key, o, img in zip(("seq", "qual", "quali"), outs, imgs):
                    got = o.cpu().numpy()
                    if not np.array_equal(got, img):
                        p = int(np.argmax(got != img))
                        pytest.fail("%s crlf=%s final_nl=%s flags=%d: byte %d is 0x%02x, expected 0x%02x" % (key, crlf, final_nl, flags, p, got[p], img[p]))
                n += ids.size
        b.close()
    assert n == 4 * 2 * (300 + 307)


# ------------------------------------------------------------------ g. k_revcomp
def test_revcomp_every_length_and_byte(L):
    n = 0
    for m in T.revcomp_lengths():
        s = T.revcomp_input(m)
        for mode in (2, 4, 6):
            assert L.revcomp_bytes(s, mode) == T.apply_flags(s, mode), (m, mode)
            n += 1
    every = bytes(range(256))
    for mode in (2, 4, 6):
        assert L.revcomp_bytes(every, mode) == T.apply_flags(every, mode)
    assert n == 3 * (131 + 5)
