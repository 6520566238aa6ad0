"""The compact fetch sweep in a process of its own (not collected by pytest): tests/test_gpu_fetch_sweep.py starts it once
per environment switch that chooses a fetch kernel, because the library reads those switches once per process.

Prints one JSON line: {"checked": queries compared, "mismatch": null or the first one, "seconds": run time}.
The helpers that open a shape on the device and compare a batch are shared with the GPU test module."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import fetch_truth as T  # noqa: E402

ROW_COLS = ("boff", "blen", "slen", "llen", "elen", "norm")


def open_shape(L, shape):
    """The shape's stream on the device with its record table: built by the index kernels and compared with the plain
    rows -- or, for a record whose row has to claim line-regular, installed (fasta_set_table decides the line-regular
    column from the stream; fasta_set_row then overrides it for that row)."""
    b = L.Blob.from_bytes(shape.raw)
    rows = shape.rows
    if shape.force:
        b.fasta_set_table(*[np.array([r[c] for r in rows]) for c in ROW_COLS])
        for rid in shape.force:
            assert b.fasta_line_regular(len(rows))[rid] == 0, shape.name
            r = rows[rid]
            b.fasta_set_row(rid, r["boff"], r["blen"], r["slen"], r["llen"], r["elen"], 1, 0, 0, reg=1)
    else:
        s = b.fasta_build()
        assert s.n_seq == len(rows), shape.name
        t = b.fasta_table(s.n_seq)
        for c in ROW_COLS:
            assert t[c].tolist() == [r[c] for r in rows], (shape.name, c)
    reg = b.fasta_line_regular(len(rows))
    for rid in shape.ids:
        assert int(reg[rid]) == int(shape.regular[rid]), (shape.name, rid)
    return b


def expected_of(shape, q):
    return T.expected_fast(shape, *q) if shape.clean else T.expected(shape, *q)


def check_by_id(b, shape, q, exp=None, via="fasta_fetch", flags=0):
    """One batch by record id through an entry of the binding -> (queries, None or the first mismatch)."""
    ids, a, c, fl = q
    exp = exp or expected_of(shape, q)
    if via == "fasta_fetch_alloc":
        buf, offs = b.fasta_fetch_alloc(ids, a, c, flags=flags, flags_per_query=fl)
        out_len = None
    else:
        buf, offs, out_len = b.fasta_fetch(ids, a, c, flags=flags, flags_per_query=fl)
    bad = T.first_mismatch(buf, offs, out_len, *exp)
    return ids.size, None if bad is None else "%s %s flags=%d: %s" % (shape.name, via, flags, bad)


def coal_batches(slen):
    """Batches for the LDS-staged stores of k_fetch_lines<4, 1, true>: answers of 4 .. 128 bytes, a multiple of four each,
    laid back to back -- every 16 consecutive ones span at most 2048 bytes -- behind 0, 1, 2 and 3 answers of 4 bytes, so
    the first byte of a wave's span takes every dword phase of a 16-byte line; then 16 answers with one odd length among
    them (the wave stores directly) and 16 of 200 bytes (a span over the cap)."""
    out = []
    for lead in range(4):
        take = [4] * lead + [4 * (1 + (k * 7) % 32) for k in range(64 * 3)]
        while len(take) % 16:
            take.append(8)
        take += [12] * 7 + [13] + [12] * 8
        take += [200] * 16
        take = np.array(take, dtype=np.int64)
        a = (np.arange(take.size) * 37) % (slen - take)
        out.append((np.zeros(take.size, dtype=np.int64), a.astype(np.int64), (a + take).astype(np.int64),
                    (np.arange(take.size) % 8).astype(np.uint8)))
    return out


def shape_coal():
    return T.shape_lines("coal_bpl60", [60], 1000, 1, clean=True)


def run(L):
    checked, bad = 0, None
    for shape in T.shapes_compact():
        b = open_shape(L, shape)
        n, m = check_by_id(b, shape, T.queries(shape, "cycle"))
        checked += n
        bad = bad or m
        b.close()
    if os.environ.get("FX_FETCH_COAL", "0") not in ("", "0"):
        shape = shape_coal()
        b = open_shape(L, shape)
        phases = set()
        for q in coal_batches(shape.slen(0)):
            take = q[2] - q[1]
            offs = np.concatenate([[0], np.cumsum(take)])
            assert all(offs[k + 16] - offs[k] <= 2048 for k in range(0, take.size - 32, 16))
            phases |= {int(offs[k]) % 16 for k in range(0, take.size - 32, 16)}
            n, m = check_by_id(b, shape, q)
            checked += n
            bad = bad or m
        assert phases == {0, 4, 8, 12}, phases
        b.close()
    return checked, bad


def main():
    t0 = time.perf_counter()
    from pyfastx_amd import _lib as L
    L.lib()
    checked, bad = run(L)
    print(json.dumps({"checked": checked, "mismatch": bad, "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
