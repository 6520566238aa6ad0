"""Six-frame ORF search and translation on a resident synthetic genome of the C2 shape (synth.fasta_plan: 3 Gbp, 60-column
lines, ~50 % soft-masked blocks, telomere and centromere N runs): kernel ms (fx_prof_*) of
  k_orf_count / k_orf_scan / k_orf_close for mode "start" (ATG) and mode "stop" at min_len 75 and 300 on the whole genome -- up
  to the offsets: the rows are counted and refused by max_orfs=0, since the tens of millions of rows of random letters are
  not what the passes are measured by;
  the same four settings with k_orf_emit on the scaffolds alone, and k_fetch / k_fetch_rest / k_tr_translate for the
  translation of the rows found there (Orfs.proteins);
  k_an_runs_count of class_runs("N") and k_td_count of tandem_repeats (Krait's defaults) beside them: same process, same
  bytes, same run layout.
Medians over --reps timed runs after a warm-up, with the smallest and largest.  One JSON line.

    python tools/orf_bench.py [--bp 3000000000] [--reps 5] [--out profiles/fasta_orfs.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORF = ["k_orf_count", "k_orf_scan", "k_orf_close", "k_orf_emit"]
TR = ["k_fetch", "k_fetch_rest", "k_tr_translate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, annot, orf, synth, tandem
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=a.bp)
    blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own stream reads the blob
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    slen = plan["slen"]
    assert b.fasta_build().n_seq == len(slen)
    b.fasta_rank_build()

    def timed(run, names):
        run()                                              # warm-up: allocations, code objects
        per = {k: [] for k in names}
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            r = run()
            pr = b.prof_read()
            b.prof_enable(0)
            for k in names:
                per[k].append(pr[k][0] if k in pr else 0.0)
        return r, {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in per.items()}

    def total(t):
        return round(sum(v["median_ms"] for v in t.values()), 4)

    def refused(**kw):
        try:
            orf.orfs_blob(b, max_orfs=0, **kw)
        except ValueError as e:
            return int(str(e).split()[0])
        return 0

    scaffolds = np.arange(plan["n_chrom"], len(slen), dtype=np.int64)
    gaps, t_n = timed(lambda: annot.runs_blob(b, "N"), ["k_an_runs_count", "k_an_runs_scan", "k_an_runs_emit"])
    _, t_td = timed(lambda: tandem.repeats_blob(b, tandem.KRAIT_DEFAULT), ["k_td_count", "k_td_scan", "k_td_close", "k_td_emit"])
    an, td = t_n["k_an_runs_count"]["median_ms"], t_td["k_td_count"]["median_ms"]
    legs = {}
    for mode in ("start", "stop"):
        for min_len in (75, 300):
            kw = dict(min_len=min_len, mode=mode)
            rows, t_whole = timed(lambda: refused(**kw), ORF[:3])
            small, t_small = timed(lambda: orf.orfs_blob(b, ids=scaffolds, **kw), ORF)
            (buf, offs), t_tr = timed(small.proteins, TR)
            c = t_whole["k_orf_count"]["median_ms"]
            legs["%s_%d" % (mode, min_len)] = {
                "mode": mode, "min_len": min_len, "rows": rows, "emit": "refused (max_orfs=0): the rows are counted, not stored",
                "total_median_ms": total(t_whole), "kernels": t_whole,
                "count_over_an_runs_count": round(c / an, 3) if an else None, "count_over_td_count": round(c / td, 3) if td else None,
                "scaffolds": {"rows": len(small), "total_median_ms": total(t_small), "kernels": t_small,
                              "proteins": {"amino_acids": int(offs[-1]), "total_median_ms": total(t_tr), "kernels": t_tr}}}
    out = {"tool": "orf_bench", "total_bp": int(slen.sum()), "n_bytes": nb, "n_records": int(len(slen)), "n_runs": nb // 256, "reps": a.reps,
           "table": 1, "starts": ["ATG"], "strand": "both", "scaffolds": {"records": int(scaffolds.size), "bp": int(slen[scaffolds].sum())},
           "legs": legs, "class_runs_N": {"rows": len(gaps), "kernels": t_n}, "tandem_krait_defaults": {"kernels": t_td}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
