"""FASTA record output (fx_fasta_format_alloc, csrc/fx_fasta_format.hpp) on a resident synthetic genome of the C2 shape
(synth.fasta_plan: 3 Gbp, 176 records, 60-column lines): kernel ms (fx_prof_*) of the size pass, the scans and the emit pass for
  rewrap        every record re-wrapped to width 80;
  minus         the same on the minus strand (reverse complement);
  soft_masked   the same soft-masked with the rows of class_runs("masked"), merged on the host;
  one_record    one synthetic stream with a single record of --one-bp letters, against the same number of letters in --many records;
  intervals     --regions intervals of 100 bp at width 0 with `name:start-stop` headers, beside fx_fasta_fetch_alloc of the same
                queries (k_fetch + k_fetch_rest) plus the host join of cli.subseq_records (wall clock).
Every repetition alternates the case with two yardsticks on the same device: raw_many of all records (one gather of the
records' bytes, k_fetch) and a device-to-device copy of as many bytes as the case wrote (torch, timed by events).  The traffic
floor of a case is (stream bytes read + output bytes written) at 6.5 TB/s.  Medians over --reps timed runs after a warm-up, with
the smallest and largest.  One JSON line.

    python tools/fasta_write_bench.py [--bp 3000000000] [--reps 5] [--out profiles/fasta_write.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.5
KERNELS = ["k_fa_format_size", "k_fa_format_scan", "k_fa_format_emit"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--one-bp", type=int, default=250_000_000)
    ap.add_argument("--many", type=int, default=2500)
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, annot, fasta_out, synth
    dev = torch.device("cuda:0")

    def resident(plan):
        blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
        torch.cuda.synchronize(dev)                        # the generator's writes, before the library's own stream reads the blob
        b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
        assert b.fasta_build().n_seq == len(plan["slen"])
        return b

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def d2d_ms(nbytes, src, dst):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst[:nbytes].copy_(src[:nbytes])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def case(b, run, read_bytes, raw_cols=None):
        """run() -> (buf, offs, kept, bases); the kernels of the case alternated with the yardsticks."""
        buf, offs, kept, bases = run()                     # warm-up: allocations, code objects
        written = int(offs[-1])
        del buf
        src = torch.empty(max(written, 1), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        d2d_ms(written, src, dst)
        per, copy, raw = {k: [] for k in KERNELS}, [], []
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            r = run()
            pr = b.prof_read()
            del r
            for k in KERNELS:
                per[k].append(pr[k][0] if k in pr else 0.0)
            copy.append(d2d_ms(written, src, dst))
            if raw_cols is not None:
                b.prof_reset()
                rb = b.fetch_ranges(raw_cols[0], raw_cols[1], raw_cols[1], flags=8)
                pr = b.prof_read()
                del rb
                raw.append(sum(pr[k][0] for k in ("k_fetch", "k_fetch_rest") if k in pr))
            b.prof_enable(0)
        kern = {k: stats(v) for k, v in per.items()}
        emit = kern["k_fa_format_emit"]["median_ms"]
        floor_ms = (read_bytes + written) / (HBM_TBS * 1e12) * 1e3
        out = {"records": int(kept), "letters": int(bases), "bytes_written": written, "stream_bytes_read": int(read_bytes), "kernels": kern,
               "size_and_emit_median_ms": round(sum(v["median_ms"] for v in kern.values()), 4),
               "traffic_floor_ms": round(floor_ms, 4), "emit_fraction_of_traffic_floor": round(floor_ms / emit, 4) if emit else None,
               "d2d_copy_same_bytes": stats(copy), "emit_over_d2d_copy": round(emit / statistics.median(copy), 3)}
        if raw:
            out["raw_many_all_records"] = stats(raw)
            out["emit_over_raw_many"] = round(emit / statistics.median(raw), 3)
        return out

    def raw_columns(b, n):
        t = b.fasta_table(n)
        off = t["boff"] - t["dlen"] - t["elen"] - 1
        ln = np.minimum(t["blen"] + t["dlen"] + t["elen"] + 1, b.size - off)
        return off.astype(np.int64), ln.astype(np.int64)

    out = {"tool": "fasta_write_bench", "reps": a.reps, "hbm_tbs": HBM_TBS, "tile_bytes": fasta_out.tile()}
    # ---- the C2 shape
    plan = synth.fasta_plan(total_bp=a.bp)
    b = resident(plan)
    n = len(plan["slen"])
    nb = int(plan["n_bytes"])
    out.update({"total_bp": int(plan["slen"].sum()), "n_bytes": nb, "n_records": n})
    rawc = raw_columns(b, n)
    out["rewrap_width_80"] = case(b, lambda: b.fasta_format_alloc(n, width=80), nb, rawc)
    out["minus_width_80"] = case(b, lambda: b.fasta_format_alloc(n, flags=6, width=80), nb, rawc)
    runs = annot.runs_blob(b, "masked")
    rows = fasta_out.merge_intervals(runs.ids, runs.starts, runs.stops)
    out["soft_masked_width_80"] = case(b, lambda: b.fasta_format_alloc(n, width=80, mask=rows, mask_mode=1), nb, rawc)
    out["soft_masked_width_80"]["mask_rows"] = int(rows[0].size)
    # ---- intervals of 100 bp at width 0
    rng = np.random.default_rng(7)
    slen = plan["slen"]
    ok = np.nonzero(slen >= 100)[0]
    ids = ok[rng.integers(0, ok.size, a.regions)]
    st = (rng.random(a.regions) * (slen[ids] - 99)).astype(np.int64)
    names = ["s%d" % i for i in ids.tolist()]
    t0 = time.perf_counter()
    hdr, hdr_off = fasta_out.pack_headers(fasta_out.auto_headers(names, st, st + 100, np.zeros(a.regions, dtype=bool)), a.regions)
    headers_s = time.perf_counter() - t0
    iv = case(b, lambda: b.fasta_format_alloc(a.regions, ids, st, st + 100, width=0, hdr=hdr, hdr_off=hdr_off), 102 * a.regions + int(hdr.size))
    fetch, join = [], []
    for _ in range(a.reps + 1):
        b.prof_enable(1)
        b.prof_reset()
        buf, offs = b.fasta_fetch_alloc(ids, st, st + 100)
        pr = b.prof_read()
        b.prof_enable(0)
        fetch.append(sum(pr[k][0] for k in ("k_fetch", "k_fetch_rest") if k in pr))
        t0 = time.perf_counter()
        view, o, parts = memoryview(np.ascontiguousarray(buf)), offs.tolist(), []
        for k, c in enumerate(names):                      # the join of cli.subseq_records
            parts.append((">%s:%d-%d\n" % (c, st[k] + 1, st[k] + 100)).encode())
            parts.append(view[o[k]:o[k + 1]])
            parts.append(b"\n")
        joined = b"".join(parts)
        join.append((time.perf_counter() - t0) * 1e3)
        del buf, view
    assert len(joined) == iv["bytes_written"]
    iv.update({"n": a.regions, "host_headers_s": round(headers_s, 3), "fetch_alloc_same_queries": stats(fetch[1:]), "host_join_wall": stats(join[1:])})
    out["intervals_100bp_width_0"] = iv
    del b
    # ---- one long record against the same letters in many
    def plain_stream(nrec, L, width=60):
        """nrec records `>r<i>` of L random letters of A C G T each, lines of `width` -> (device tensor, bytes)"""
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        full, rem = divmod(L, width)
        body = full * (width + 1) + (rem + 1 if rem else 0)
        hdrs = [(">r%d\n" % i).encode() for i in range(nrec)]
        t = torch.empty(sum(len(h) for h in hdrs) + nrec * body + 65536, dtype=torch.uint8, device=dev)
        pos = 0
        for h in hdrs:
            t[pos:pos + len(h)] = torch.frombuffer(bytearray(h), dtype=torch.uint8).to(dev)
            pos += len(h)
            for c0 in range(0, full, 1 << 20):            # 2^20 lines at a time
                k = min(full - c0, 1 << 20)
                view = t[pos:pos + k * (width + 1)].view(k, width + 1)
                view[:, :width] = lut[torch.randint(0, 4, (k, width), device=dev, generator=g)]
                view[:, width] = 10
                pos += k * (width + 1)
            if rem:
                t[pos:pos + rem] = lut[torch.randint(0, 4, (rem,), device=dev, generator=g)]
                t[pos + rem] = 10
                pos += rem + 1
        torch.cuda.synchronize(dev)
        return t, pos

    for key, nrec in (("one_record", 1), ("many_records", a.many)):
        t, nbytes = plain_stream(nrec, a.one_bp // nrec)
        bb = _lib.Blob.from_device(t.data_ptr(), nbytes, device=0, keepalive=t)
        assert bb.fasta_build().n_seq == nrec
        out[key] = case(bb, lambda: bb.fasta_format_alloc(nrec, width=80), nbytes)
        out[key]["n_records"] = nrec
        del bb, t
    out["one_record_over_many_records_emit"] = round(out["one_record"]["kernels"]["k_fa_format_emit"]["median_ms"] /
                                                     out["many_records"]["kernels"]["k_fa_format_emit"]["median_ms"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
