"""The plain reference of the fetch sweep (tests/fetch_truth.py) against the oracle and the committed reference vectors,
and the properties of the generated inputs that tests/test_gpu_fetch_sweep.py relies on.  No GPU."""
import numpy as np
import pytest

import fetch_truth as T
from conftest import load_golden
from test_host_logic import _reg_of

ROW_COLS = ("boff", "blen", "slen", "llen", "elen", "norm")


def _all_shapes():
    return T.shapes_a() + T.shapes_b() + T.shapes_forced()


def test_apply_flags_golden_and_all_bytes(oracle):
    for fwd, rc in load_golden("misc")["reverse_complement"]:
        assert T.apply_flags(fwd.encode(), 6) == rc.encode()
    every = bytes(range(256))
    for flags in range(8):
        want = oracle.revcomp(oracle.despace(every, upper=True) if flags & 1 else T.despace(every),
                              ((flags >> 1) & 1) | ((flags >> 1) & 2))
        assert T.apply_flags(T.despace(every), flags) == want, flags
    assert T.despace(every) == oracle.despace(every) and len(T.despace(every)) == 253
    tab = T.comp_table()
    assert len(tab) == 256 and sum(tab[c] != c for c in range(256)) == 26       # 12 paired letters and U, both cases


def test_rows_match_the_oracle(oracle):
    for sh in _all_shapes():
        recs, _ = oracle.fasta_index(sh.raw)
        assert len(recs) == len(sh.rows), sh.name
        for r, mine in zip(recs, sh.rows):
            assert [int(r[c]) for c in ROW_COLS] == [mine[c] for c in ROW_COLS], sh.name


def test_shape_properties(oracle):
    """regular means line-regular; inside means 16 bytes in front and 32 behind; front / back mean not."""
    seen = set()
    for sh in _all_shapes():
        recs, _ = oracle.fasta_index(sh.raw)
        for rid in sh.ids:
            reg = _reg_of(sh.raw, recs[rid])
            if rid in sh.force:
                assert sh.regular[rid] and reg == 0 and int(recs[rid]["norm"]) == 1, sh.name   # what the table has to be told
            else:
                assert reg == int(sh.regular[rid]), sh.name
            front, behind = sh.margins(rid)
            if sh.kind == "inside":
                assert front >= 16 and behind >= 32, (sh.name, front, behind)
            elif sh.kind == "front":
                assert front < 16 and behind >= 32, (sh.name, front, behind)
            else:
                assert sh.kind == "back" and front >= 16 and behind < 32, (sh.name, front, behind)
            bpl = sh.rows[rid]["llen"] - sh.rows[rid]["elen"]
            seen.add((sh.kind, bpl, sh.rows[rid]["elen"]))
    for el in (1, 2):
        for bpl in T.A_SMALL + T.A_LARGE + (1, 2, 15):
            assert ("inside", bpl, el) in seen
    for sh in T.shapes_a():
        (rid,) = sh.ids
        bpl = sh.rows[rid]["llen"] - sh.rows[rid]["elen"]
        assert sh.slen(rid) == T.slen_a(bpl) and len(sh.raw.split(b"\n")[0]) >= 20
        t = T.despace(sh.raw[sh.rows[rid]["boff"]:][:sh.rows[rid]["blen"]])
        assert set(t) <= set(T.ALPHABET) and T.apply_flags(t, 1) != t and T.apply_flags(t, 4) != t and T.apply_flags(t, 5) != T.apply_flags(t, 4)
    assert T.shape_space().rows[0]["slen"] == 50 and b" " in T.shape_space().raw        # the index counts the space
    odd = T.shape_odd_line(False)
    assert [len(x) for x in odd.raw.split(b"\n")[1:5]] == [20, 7, 20, 20]


def test_the_sweep_enumerates_every_pair():
    assert sum(T.n_pairs(T.slen_a(b)) for b in T.A_SMALL) == 20259 and sum(T.n_pairs(T.slen_a(b)) for b in T.A_LARGE) == 29170
    assert sum(T.n_queries(sh) for sh in T.shapes_a()) == (20259 + 29170) * 8 * 2 == 790864
    for sh in [T.shape_a(17, 2), T.shape_empty_between()]:
        for mode, per in (("all", 8), ("cycle", 1)):
            ids, a, b, fl = T.queries(sh, mode)
            assert ids.size == T.n_queries(sh, mode) == per * sum(T.n_pairs(sh.slen(r)) for r in sh.ids)
            got = set(zip(ids.tolist(), a.tolist(), b.tolist(), fl.tolist() if mode == "all" else [0] * ids.size))
            want = {(r, x, y, f) for r in sh.ids for x in range(sh.slen(r)) for y in range(x + 1, sh.slen(r) + 1)
                    for f in (range(8) if mode == "all" else [0])}
            assert got == want
            assert (fl == np.arange(ids.size) % 8).all()
    take = T.queries(T.shape_a(16, 1))[2] - T.queries(T.shape_a(16, 1))[1]
    off, size = T.guard_offsets(take)
    assert off[0] == 3 and set((off % 16).tolist()) == set(range(16)) and size >= off[-1] + take[-1]
    assert ((off[1:] - (off[:-1] + take[:-1])) == (np.arange(1, take.size) * 7) % 19).all()


def _oracle_slice(oracle, sh, rid, a, b, flags, regular):
    r = sh.rows[rid]
    if regular:
        off, bl = oracle.slice_range(r["boff"], r["llen"], r["elen"], a, b)
        return oracle.fetch(sh.raw, off, bl, b - a, flags)
    s = oracle.despace(sh.raw[r["boff"]:r["boff"] + r["blen"]], upper=bool(flags & 1))[a:b]
    return oracle.revcomp(s, ((flags >> 1) & 1) | ((flags >> 1) & 2))


def test_slice_by_id_matches_the_oracle_on_the_compact_sweep(oracle):
    n = 0
    for sh in T.shapes_compact():
        ids, a, b, fl = T.queries(sh, "cycle")
        buf, offs, lens = T.expected(sh, ids, a, b, fl)
        for i in range(ids.size):
            want = _oracle_slice(oracle, sh, int(ids[i]), int(a[i]), int(b[i]), int(fl[i]), sh.regular[int(ids[i])])
            assert buf[offs[i]:offs[i] + lens[i]].tobytes() == want, (sh.name, i)
        if sh.clean:
            assert (lens == b - a).all()
        n += ids.size
    assert n == sum(T.n_queries(sh, "cycle") for sh in T.shapes_compact()) == 2 * (1431 + 1596 + 5460 + 12880) + 5 * 1275 + 2278 + 1275
    short = T.expected(T.shape_odd_line(True), *T.queries(T.shape_odd_line(True), "cycle"))[2]
    assert (short < np.diff(T.expected(T.shape_odd_line(True), *T.queries(T.shape_odd_line(True), "cycle"))[1])).any()   # answers shorter than asked for occur


def test_the_other_shapes_match_the_oracle_too(oracle):
    for sh in T.shapes_b():
        ids, a, b, fl = T.queries(sh, "cycle")
        buf, offs, lens = T.expected(sh, ids, a, b, fl)
        for i in range(ids.size):
            want = _oracle_slice(oracle, sh, int(ids[i]), int(a[i]), int(b[i]), int(fl[i]), sh.regular[int(ids[i])])
            assert buf[offs[i]:offs[i] + lens[i]].tobytes() == want, (sh.name, i)


def test_expected_fast_equals_slice_by_id():
    """the eight-copies shortcut of the big sweep is the reference itself, on every clean shape"""
    for sh in T.shapes_a() + [s for s in T.shapes_b() if s.clean]:
        q = T.queries(sh, "all" if T.n_queries(sh) <= 25000 else "cycle")
        slow, fast = T.expected(sh, *q), T.expected_fast(sh, *q)
        for x, y in zip(slow, fast):
            assert np.array_equal(x, y), sh.name
        assert T.first_mismatch(fast[0], fast[1], fast[2], *slow) is None
        if fast[0].size:
            wrong = fast[0].copy()
            wrong[-1] ^= 1
            assert "query %d" % (q[0].size - 1) in T.first_mismatch(wrong, fast[1], fast[2], *slow)


def test_range_fetch_matches_the_oracle(oracle):
    sh = T.shape_odd_line(False)
    r = sh.rows[0]
    for a in range(0, 67, 3):
        for b in range(a + 1, 68, 5):
            for fl in range(8):
                off, bl = T.arith_range(r, a, b)
                assert (off, bl) == oracle.slice_range(r["boff"], r["llen"], r["elen"], a, b)
                assert T.range_fetch(sh.raw, off, bl, b - a, 0, fl) == oracle.fetch(sh.raw, off, bl, b - a, fl)
                assert T.range_fetch(sh.raw, off, 1 << 16, b - a, 0, fl) == oracle.fetch(sh.raw, off, 1 << 16, b - a, fl)
                assert T.range_fetch(sh.raw, r["boff"], r["blen"], b - a, a, fl) == T.slice_by_id(sh.raw, r, a, b, fl, False)


@pytest.mark.parametrize("crlf,final_nl,high", [(False, True, False), (False, False, False), (True, True, False),
                                                (True, False, False), (False, True, True)])
def test_fastq_read_matches_the_oracle(oracle, crlf, final_nl, high):
    raw = T.fastq_stream(crlf, final_nl, high)
    recs, _, _ = oracle.fastq_index(raw)
    rows = T.fastq_rows(raw)
    assert [(int(r["soff"]), int(r["qoff"]), int(r["rlen"])) for r in recs] == rows
    assert sorted(n for _, _, n in rows) == list(range(1, T.FQ_MAX + 1))
    assert rows[0][0] < 16 and len(raw) - (rows[-1][1] + rows[-1][2]) < 16
    quals = set()
    for so, qo, n in rows:
        quals |= set(raw[qo:qo + n])
        for phred in (0, 33, 64):
            seq, qual, qi = T.fastq_read(raw, so, qo, n, phred, 6)
            assert qual == raw[qo:qo + n] and np.array_equal(qi, oracle.quali(raw, qo, n, phred))
            assert seq == oracle.revcomp(raw[so:so + n], 3)
        assert T.fastq_read(raw, so, qo, n, 33, 0)[0] == raw[so:so + n] and b"\r" not in raw[so:so + n]
    assert quals >= set(range(33, 127)) and (max(quals) >= 128) == high
    assert [b.size for b in T.fastq_batches(len(rows))] == [300, 307]


def test_revcomp_inputs_cover_every_byte():
    assert set(T.revcomp_lengths()) >= set(range(131)) | {4095, 4096, 4097, 65537}
    assert set(b"".join(T.revcomp_input(n) for n in range(131))) == set(range(256))
    assert set(T.revcomp_input(4095)) == set(range(256))
