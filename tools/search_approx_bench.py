"""Mismatch-tolerant motif search on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB): kernel ms
(fx_prof_*) of k_asearch_count and k_asearch_emit, hits, and next to each case k_search_count of the SAME pattern searched
exactly -- the yardstick: the d = 0 line against it is what the generalisation costs, every further level is a slope.
Cases: a 20-letter guide + NGG (23 letters, IUPAC, the PAM anchored) at d = 0, 1, 3, 5, 8 and one 40-letter pattern
(two state words per level) at d = 3.  The d = 0 hits are checked against search_blob's.  Prints one JSON line.

    python tools/search_approx_bench.py [--gbp 3.0] [--reps 3] [--out profiles/search_approx.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
GUIDE = "GACGCATAAAGATGAGACGCNGG"
LONG = "ACGRYTNNCAGGRYATNNGCACGTTGCANNRYGGATCCAT"
CASES = [(GUIDE, slice(20, 23), d) for d in (0, 1, 3, 5, 8)] + [(LONG, None, 3)]


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
    from pyfastx_amd import _lib, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t = synth.fasta_generate(plan, dev, keep_flat=False)[0]
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    floor_ms = nb / (HBM_TBS * 1e12) * 1e3
    out = {"tool": "search_approx_bench", "n_bytes": nb, "n_records": len(plan["slen"]), "hbm_floor_ms": round(floor_ms, 4), "cases": []}
    exact = {}
    for p in (GUIDE, LONG):                                             # the yardstick: the same pattern, exact automaton
        h, e2e, kms = timed(b, a.reps, lambda: search.search_blob(b, p, "both", True, max_hits=10**9), ("k_search_count", "k_search_scan", "k_search_emit"))
        exact[p] = {"hits": int(h.ids.size), "kernel_ms": kms, "e2e_ms": e2e, "rows": h}
    for p, anchor, d in CASES:
        h, e2e, kms = timed(b, a.reps, lambda: search.approx_blob(b, p, d, anchor, "both", True, max_hits=10**9),
                            ("k_asearch_count", "k_search_scan", "k_asearch_emit"))
        _, e2e_c, kms_c = timed(b, a.reps, lambda: search.approx_count_blob(b, p, d, anchor, "both", True), ("k_asearch_count",))
        ex = exact[p]
        case = {"pattern": p, "length": len(p), "anchor": None if anchor is None else [anchor.start, anchor.stop], "mismatches": d,
                "hits": int(h.ids.size), "hits_by_distance": [int(x) for x in np.bincount(h.mismatches, minlength=d + 1)],
                "kernel_ms": kms, "e2e_ms": e2e, "counts_only_e2e_ms": e2e_c, "counts_only_k_asearch_count_ms": kms_c.get("k_asearch_count"),
                "exact_k_search_count_ms": ex["kernel_ms"].get("k_search_count"), "exact_k_search_emit_ms": ex["kernel_ms"].get("k_search_emit"),
                "exact_hits": ex["hits"],
                "count_ratio_to_exact": round(kms["k_asearch_count"] / ex["kernel_ms"]["k_search_count"], 3),
                "count_pass_fraction_of_hbm_floor": round(floor_ms / kms["k_asearch_count"], 3)}
        if d == 0:
            r = ex["rows"]
            case["agree_with_exact"] = bool(h.ids.size == r.ids.size and (h.ids == r.ids).all() and (h.starts == r.starts).all() and
                                            (h.strands == r.strands).all() and not h.mismatches.any())
        out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
