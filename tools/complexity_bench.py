"""Low-complexity masking and per-read complexity on resident synthetic inputs: kernel ms (fx_prof_*) of
  k_dust_count / k_dust_scan (carry scan, list, close, offsets) / k_dust_emit of Fasta.low_complexity at (window, threshold) =
  (64, 20) and (16, 20) on a genome of the C2 shape (synth.fasta_plan: 3 Gbp, 60-column lines, ~50 % soft-masked blocks, N
  runs), with three yardsticks that read the same runs beside them: k_an_runs_count of class_runs("N"), k_td_count of
  tandem_repeats (Krait's defaults) and k_search_count of the pattern A ('+' strand, counts only);
  k_fq_complexity on synthetic reads of 150 (synth.fastq_generate) beside k_fq_read_stats.
The legs of a group alternate inside every repetition, so a drift of the clocks falls on all of them alike.  Medians over
--reps timed runs after a warm-up, with the smallest and largest.  One JSON line.

    python tools/complexity_bench.py [--bp 3000000000] [--reads 20000000] [--reps 5] [--out profiles/fasta_complexity.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DUST = ["k_dust_count", "k_dust_scan", "k_dust_emit"]


def alternate(b, legs, reps):
    """legs: {name: (run, kernel names)} -> ({name: last result}, {name: {kernel: median / min / max ms}})"""
    res = {k: run() for k, (run, _) in legs.items()}           # warm-up: allocations, code objects
    per = {k: {n: [] for n in names} for k, (_, names) in legs.items()}
    for _ in range(reps):
        for k, (run, names) in legs.items():
            b.prof_enable(1)
            b.prof_reset()
            res[k] = run()
            pr = b.prof_read()
            b.prof_enable(0)
            for n in names:
                per[k][n].append(pr[n][0] if n in pr else 0.0)
    fig = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return res, {k: {n: fig(v) for n, v in t.items()} for k, t in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, annot, complexity, search, synth, tandem
    dev = torch.device("cuda:0")
    out = {"tool": "complexity_bench", "reps": a.reps}

    if a.bp > 0:
        plan = synth.fasta_plan(total_bp=a.bp)
        blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
        torch.cuda.synchronize(dev)                        # the generator's writes, before the library's own stream reads the blob
        nb = int(plan["n_bytes"])
        b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
        assert b.fasta_build().n_seq == len(plan["slen"])
        b.fasta_rank_build()
        legs = {"dust_w64_t20": (lambda: complexity.mask_blob(b, 64, 20), DUST),
                "dust_w16_t20": (lambda: complexity.mask_blob(b, 16, 20), DUST),
                "class_runs_N": (lambda: annot.runs_blob(b, "N"), ["k_an_runs_count", "k_an_runs_scan", "k_an_runs_emit"]),
                "tandem_krait_defaults": (lambda: tandem.repeats_blob(b, tandem.KRAIT_DEFAULT), ["k_td_count"]),
                "search_count_A_plus": (lambda: search.count_blob(b, "A", "+"), ["k_search_count"])}
        res, t = alternate(b, legs, a.reps)
        an, td, sc = (t[k][n]["median_ms"] for k, n in (("class_runs_N", "k_an_runs_count"), ("tandem_krait_defaults", "k_td_count"),
                                                        ("search_count_A_plus", "k_search_count")))
        fa = {"total_bp": int(plan["slen"].sum()), "n_bytes": nb, "n_records": int(len(plan["slen"])), "n_runs": nb // 256}
        for k in ("dust_w64_t20", "dust_w16_t20"):
            c = t[k]["k_dust_count"]["median_ms"]
            fa[k] = {"rows": len(res[k]), "letters": int(res[k].lengths.sum()), "total_median_ms": round(sum(v["median_ms"] for v in t[k].values()), 4),
                     "kernels": t[k], "count_over_an_runs_count": round(c / an, 3) if an else None,
                     "count_over_td_count": round(c / td, 3) if td else None, "count_over_search_count": round(c / sc, 3) if sc else None}
        fa["class_runs_N"] = {"rows": len(res["class_runs_N"]), "kernels": t["class_runs_N"]}
        fa["tandem_krait_defaults"] = {"rows": len(res["tandem_krait_defaults"]), "kernels": t["tandem_krait_defaults"]}
        fa["search_count_A_plus"] = t["search_count_A_plus"]
        out["fasta"] = fa
        del b, blob_t, res
        torch.cuda.empty_cache()

    if a.reads > 0:
        n, rlen = a.reads, 150
        blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
        torch.cuda.synchronize(dev)
        nb = int(cols["n_bytes"])
        q = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
        assert q.fastq_build().n_reads == n
        legs = {"complexity": (lambda: q.fastq_complexity(), ["k_fq_complexity"]),
                "read_stats": (lambda: q.fastq_read_stats(phred=33, low_qual=20), ["k_fq_read_stats"])}
        res, t = alternate(q, legs, a.reps)
        length, nt, ds, nd = res["complexity"]
        hl = int(cols["soff"][0])
        view = blob_t[:n * int(cols["rec"])].view(n, int(cols["rec"]))[:1_000_000, hl:hl + rlen]
        want = (view[:, 1:] != view[:, :-1]).sum(1).cpu().numpy()  # n_diff of the first million reads against torch
        assert np.array_equal(nd[:1_000_000], want) and int(length.min()) == int(length.max()) == rlen, "n_diff differs from torch"
        cx, rs = t["complexity"]["k_fq_complexity"]["median_ms"], t["read_stats"]["k_fq_read_stats"]["median_ms"]
        out["fastq"] = {"n_reads": n, "read_length": rlen, "n_bytes": nb, "complexity": t["complexity"]["k_fq_complexity"],
                        "read_stats": t["read_stats"]["k_fq_read_stats"], "complexity_over_read_stats": round(cx / rs, 3) if rs else None,
                        "mean_dust": round(float(complexity.dust_score(ds, nt).mean()), 3), "n_diff_checked_against_torch": 1_000_000}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
