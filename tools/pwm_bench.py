"""Position weight matrix scan on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB): kernel ms
(fx_prof_*) of k_pwm_count, k_pwm_emit and k_pwm_best and the hit counts, for matrices of W = 8, 12, 20, 32, 33 and 64
columns made from seeded random counts, at p-value 1e-4 and 1e-5, on both strands.  Next to each width, in the same run:
k_search_count of a literal pattern of the same length and k_asearch_count of it at d = 3 -- the two yardsticks -- and the
fraction of the HBM floor (the stream read once at 6.5 TB/s).  Prints one JSON line.

    python tools/pwm_bench.py [--gbp 3.0] [--reps 3] [--out profiles/fasta_pwm.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
WIDTHS = (8, 12, 20, 32, 33, 64)
PVALUES = (1e-4, 1e-5)


def timed(b, reps, run, names):
    """best of reps by wall time -> (result, end-to-end ms, kernel ms of `names`)"""
    run()                                                               # warm-up (allocations, code objects)
    best, kms, res = 1e30, {}, None
    for _ in range(reps):
        b.prof_enable(1)
        b.prof_reset()
        t0 = time.perf_counter()
        r = run()
        dt = (time.perf_counter() - t0) * 1e3
        if dt < best:
            best, res = dt, r
            pr = b.prof_read()
            kms = {k: round(pr[k][0], 4) for k in names if k in pr}
        b.prof_enable(0)
    return res, round(best, 3), kms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyfastx_amd import _lib, pwm, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t = synth.fasta_generate(plan, dev, keep_flat=False)[0]
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    floor_ms = nb / (HBM_TBS * 1e12) * 1e3
    out = {"tool": "pwm_bench", "n_bytes": nb, "n_records": len(plan["slen"]), "hbm_floor_ms": round(floor_ms, 4), "cases": []}
    rng = np.random.default_rng(20261019)
    for W in WIDTHS:
        m = pwm.Pwm.from_counts(rng.integers(0, 40, (4, W)))
        lit = "".join("ACGT"[c] for c in rng.integers(0, 4, W))
        _, _, k_exact = timed(b, a.reps, lambda: search.count_blob(b, lit, "both"), ("k_search_count",))
        _, _, k_approx = timed(b, a.reps, lambda: search.approx_count_blob(b, lit, 3, None, "both"), ("k_asearch_count",))
        best, e2e_b, k_best = timed(b, a.reps, lambda: pwm.best_blob(b, m, "both"), ("k_pwm_count", "k_search_scan", "k_pwm_best"))
        for p in PVALUES:
            t = m.threshold_for_pvalue(p)
            h, e2e, kms = timed(b, a.reps, lambda: pwm.scan_blob(b, m, t, "both", max_hits=10**9), ("k_pwm_count", "k_search_scan", "k_pwm_emit"))
            _, e2e_c, kms_c = timed(b, a.reps, lambda: pwm.count_blob(b, m, t, "both"), ("k_pwm_count",))
            out["cases"].append({
                "width": W, "groups": (W + 3) // 4, "pvalue": p, "min_score": int(t), "score_range": [m.min_score, m.max_score],
                "hits": int(h.ids.size), "hits_plus": int((h.strands == ord("+")).sum()), "expected_hits_at_most": round(2 * p * a.gbp * 1e9),
                "kernel_ms": kms, "e2e_ms": e2e, "counts_only_e2e_ms": e2e_c, "counts_only_k_pwm_count_ms": kms_c.get("k_pwm_count"),
                "best_kernel_ms": k_best, "best_e2e_ms": e2e_b, "best_score_max": int(best.scores.max()),
                "literal_k_search_count_ms": k_exact.get("k_search_count"), "literal_d3_k_asearch_count_ms": k_approx.get("k_asearch_count"),
                "count_ratio_to_search": round(kms["k_pwm_count"] / k_exact["k_search_count"], 3),
                "count_ratio_to_asearch_d3": round(kms["k_pwm_count"] / k_approx["k_asearch_count"], 3),
                "count_pass_fraction_of_hbm_floor": round(floor_ms / kms["k_pwm_count"], 3)})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
