"""Sparse k-mer tables (Fasta.kmer_table / Fastq.kmer_table, csrc/fx_kmer_table.hpp) on the inputs of tools/kmer_bench.py: the C2
shape (synth.fasta_plan / fasta_generate), the low-complexity FASTA with its (ACG)n and (ACGT)n records, and 2 x 10^7
synthetic reads of 150 bases; k = 13, 21, 31, plain and canonical.  Per leg: kernel ms (fx_prof_*) per stage -- k_kt_kept +
k_kmer_scan (the kept bytes and their scan), k_kt_hist (histogram walk), k_kt_emit (emit walks), k_kt_sort (the radix passes
of all rounds, the waits between them included), k_kt_reduce, k_kt_fold --, n_parts, distinct codes and end-to-end ms.

Two yardsticks, measured in the same run on the same handle:
  (a) the dense global-atomic form at k = 13 (k_kmer_fasta MODE 1 / k_kmer_fastq), the only k both forms share at scale;
  (b) the traffic floor of the design at 6.5 TB/s: the stream read once per walk (kept, histogram, one emit walk per round),
      8 bytes written per window, 16 bytes moved per window and sort pass that moves data.  The passes are counted from the
      returned codes: the 8-bit digits of [0, 2k) in which the codes of the table differ -- an upper count, a digit that is
      constant inside every partition is skipped by the sort but counted here.
Every table is checked against torch.unique over the rolling codes of the flat bases before its time is reported, and the
checker is waited for.  Medians of --reps runs; a measurement whose slowest run is more than 1.5 x its fastest is taken
again and flagged "disturbed" if it stays so.  One JSON line.

    python tools/kmer_table_bench.py [--gbp 3.0] [--reads 20000000] [--low-mbp 500] [--reps 7] [--max-bytes 0] [--out profiles/kmer_table.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmer_bench import HBM_TBS, low_complexity_blob  # noqa: E402

KS = (13, 21, 31)
STAGES = ["k_kt_hist", "k_kt_kept", "k_kmer_scan", "k_kt_emit", "k_kt_sort", "k_kt_reduce", "k_kt_fold"]


def torch_table(torch, flat, rec_end, k, canonical, chunk=1 << 27):
    """(codes, counts) by torch on the device (a checker only); rec_end: one past every record's last base"""
    dev = flat.device
    lut = torch.full((256,), 4, dtype=torch.uint8, device=dev)
    for j, c in enumerate(b"ACGT"):
        lut[c] = j
        lut[c + 32] = j
    parts = []
    n = flat.numel() - k + 1
    for a in range(0, max(n, 0), chunk):
        m = min(chunk, n - a)
        c = lut[flat[a:a + m + k - 1].long()]
        code = torch.zeros(m, dtype=torch.int64, device=dev)
        rc = torch.zeros(m, dtype=torch.int64, device=dev)
        bad = torch.zeros(m, dtype=torch.bool, device=dev)
        for j in range(k):
            w = c[j:j + m]
            bad |= w > 3
            code = code * 4 + (w & 3)
            rc += (3 - (w & 3)) << (2 * j)
        for d in range(1, k):                              # starts whose window runs past the end of their record
            pos = rec_end - d - a
            bad[pos[(pos >= 0) & (pos < m)]] = True
        parts.append((torch.minimum(code, rc) if canonical else code)[~bad])
        del c, code, rc, bad
    return torch.unique(torch.cat(parts), return_counts=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--low-mbp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    st = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed_once(b, run, names):
        torch.cuda.synchronize(dev)
        run()                                              # warm-up: allocations, code objects
        per, e2e = {k: [] for k in names}, []
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            t0 = time.perf_counter()
            r = run()
            e2e.append((time.perf_counter() - t0) * 1e3)
            pr = b.prof_read()
            b.prof_enable(0)
            for k in names:
                per[k].append(pr[k][0] if k in pr else 0.0)
        return r, {k: st(v) for k, v in per.items()}, st(e2e)

    def timed(b, run, names):
        for _ in range(3):
            r, kt, e2e = timed_once(b, run, names)
            if e2e["max_ms"] <= 1.5 * e2e["min_ms"]:
                return r, kt, e2e
        e2e["disturbed"] = True
        return r, kt, e2e

    def legs(b, run_of, dense_of, dense_kernel, flat, rec_end, n_bytes):
        rows, dense = [], {}
        for canonical in (False, True):                    # yardstick (a)
            _, kt, _ = timed(b, dense_of(canonical), [dense_kernel])
            dense[canonical] = kt[dense_kernel]
        for k in KS:
            for canonical in (False, True):
                want = torch_table(torch, flat, rec_end, k, canonical)
                torch.cuda.synchronize(dev)                # the checker's kernels must not run beside the timed ones
                got, kt, e2e = timed(b, run_of(k, canonical), STAGES)
                codes, counts, windows, parts = got
                agree = bool(torch.equal(torch.from_numpy(np.asarray(codes)).to(dev), want[0]) and
                             torch.equal(torch.from_numpy(np.asarray(counts)).to(dev), want[1]))
                assert agree, "k = %d canonical = %s differs from torch" % (k, canonical)
                vary = int(np.bitwise_or.reduce(codes) ^ np.bitwise_and.reduce(codes)) if len(codes) else 0
                passes = sum(1 for s in range(0, 2 * k, 8) if (vary >> s) & 0xFF)
                share = {"walks": (2 + parts) * n_bytes, "emit_store": 8 * windows, "sort": 16 * windows * passes}
                floor = {n: v / (HBM_TBS * 1e12) * 1e3 for n, v in share.items()}
                total = sum(v["median_ms"] for v in kt.values())
                stage_ms = {"walks": kt["k_kt_hist"]["median_ms"] + kt["k_kt_kept"]["median_ms"] + kt["k_kt_emit"]["median_ms"],
                            "sort": kt["k_kt_sort"]["median_ms"]}
                row = {"k": k, "canonical": canonical, "windows": int(windows), "distinct": int(len(codes)), "n_parts": int(parts), "agree": agree,
                       "kernels": kt, "kernel_ms": round(total, 4), "e2e": e2e, "sort_passes_counted": passes,
                       "floor_ms": {n: round(v, 4) for n, v in floor.items()}, "times_floor": round(total / sum(floor.values()), 2),
                       "walks_times_its_floor": round(stage_ms["walks"] / (floor["walks"] + floor["emit_store"]), 2),
                       "sort_times_its_floor": round(stage_ms["sort"] / floor["sort"], 2) if floor["sort"] else None}
                if k == 13:
                    row["times_dense_k13"] = round(total / dense[canonical]["median_ms"], 3)
                rows.append(row)
                del got, codes, counts, want
        return {"dense_k13": {"plain": dense[False], "canonical": dense[True]}, "legs": rows}

    out = {"tool": "kmer_table_bench", "reps": a.reps, "checked_against_torch": True, "max_bytes": a.max_bytes, "hbm_tbs": HBM_TBS}
    # ---- FASTA, the C2 shape
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    torch.cuda.synchronize(dev)
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    rec_end = torch.from_numpy(flat_start + plan["slen"]).to(dev)
    fa_run = lambda bb: (lambda k, c: (lambda: bb.fasta_kmer_table(k, c, max_bytes=a.max_bytes)))
    out["fasta_c2"] = dict(n_bytes=nb, **legs(b, fa_run(b), lambda c: (lambda: b.fasta_kmers(13, c)), "k_kmer_fasta", flat_t, rec_end, nb))
    del b, blob_t, flat_t
    torch.cuda.empty_cache()
    # ---- FASTA, low complexity
    blob_t, nb, flat_t, rec_end = low_complexity_blob(torch, dev, a.low_mbp * 1_000_000 // 4)
    torch.cuda.synchronize(dev)
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fasta_build().n_seq == 4
    out["fasta_low_complexity"] = dict(n_bytes=nb, **legs(b, fa_run(b), lambda c: (lambda: b.fasta_kmers(13, c)), "k_kmer_fasta", flat_t, rec_end, nb))
    del b, blob_t, flat_t
    torch.cuda.empty_cache()
    # ---- FASTQ
    n, rlen = a.reads, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    flat_t = blob_t[:n * rec].view(n, rec)[:, hl:hl + rlen].contiguous().view(-1)
    rec_end = (torch.arange(n, dtype=torch.int64, device=dev) + 1) * rlen
    out["fastq"] = dict(n_reads=n, read_length=rlen, n_bytes=nb,
                        **legs(b, lambda k, c: (lambda: b.fastq_kmer_table(k, c, max_bytes=a.max_bytes)), lambda c: (lambda: b.fastq_kmers(13, c)),
                               "k_kmer_fastq", flat_t, rec_end, (rlen + 16) * n))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
