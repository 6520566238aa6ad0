"""Edit-distance motif search on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB): kernel ms
(fx_prof_*) of k_esearch_count, k_esearch_emit, the filter (k_esearch_best: flags, scan, list) and k_esearch_start, the ends
and the rows of report = "best", and in the SAME loop, turn by turn, the two yardsticks: k_search_count of the same pattern
searched exactly and k_asearch_count at d = k.  Cases: a 20-letter guide + NGG (23 letters, IUPAC, 32-bit words) and a
40-letter pattern (64-bit words) at k = 0, 1, 3, 8.  Every figure is the median of --reps (5) turns.  The rows are produced
(and k_esearch_start timed) only where the ends number at most --max-ends; above that the case reports the counts-only call,
which runs count, emit and the filter.  k = 0 under report = "all" is checked against search_blob's rows.  Prints one JSON line.

    python tools/search_edit_bench.py [--gbp 3.0] [--reps 5] [--out profiles/search_edit.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
GUIDE = "GACGCATAAAGATGAGACGCNGG"
LONG = "ACGRYTNNCAGGRYATNNGCACGTTGCANNRYGGATCCAT"
BUDGETS = (0, 1, 3, 8)
EDIT_KERNELS = ("k_esearch_count", "k_esearch_emit", "k_esearch_best", "k_esearch_start")


def once(b, run, names):
    """one profiled call -> (result, end-to-end ms, kernel ms of `names`)"""
    b.prof_enable(1)
    b.prof_reset()
    t0 = time.perf_counter()
    r = run()
    dt = (time.perf_counter() - t0) * 1e3
    pr = b.prof_read()
    b.prof_enable(0)
    return r, dt, {k: pr[k][0] for k in names if k in pr}


def med(xs):
    return None if not xs else round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-ends", type=int, default=2 * 10**8)
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
    out = {"tool": "search_edit_bench", "n_bytes": nb, "n_records": len(plan["slen"]), "hbm_floor_ms": round(floor_ms, 4), "reps": a.reps,
           "cases": []}
    for p in (GUIDE, LONG):
        for k in BUDGETS:
            mode, fwd, rev, _, _ = search.compile_edit(p, k, "both", True, "best")
            counts_call = lambda: b.fasta_search_edit(fwd, rev, mode, k, _lib.FX_EDIT_BEST, cap=0, counts=True)
            n_rows, n_ends, _, _ = counts_call()                          # warm-up, and the size of the answer
            with_rows = n_ends <= a.max_ends
            edit_call = (lambda: search.edit_blob(b, p, k, "both", True, "best", max_hits=a.max_ends)) if with_rows else counts_call
            edit_call()
            search.count_blob(b, p, "both", True)
            search.approx_count_blob(b, p, k, None, "both", True)
            ms = {name: [] for name in EDIT_KERNELS + ("k_search_count", "k_asearch_count", "e2e", "counts_only_e2e")}
            for _ in range(a.reps):                                       # the yardsticks alternate with the search they measure
                _, e2e, kms = once(b, edit_call, EDIT_KERNELS)
                for name, v in kms.items():
                    ms[name].append(v)
                ms["e2e"].append(e2e)
                ms["k_search_count"].append(once(b, lambda: search.count_blob(b, p, "both", True), ("k_search_count",))[2]["k_search_count"])
                ms["k_asearch_count"].append(once(b, lambda: search.approx_count_blob(b, p, k, None, "both", True),
                                                  ("k_asearch_count",))[2]["k_asearch_count"])
                ms["counts_only_e2e"].append(once(b, counts_call, ())[1])
            m = {name: med(v) for name, v in ms.items()}
            case = {"pattern": p, "length": len(p), "edits": k, "ends": int(n_ends), "rows_best": int(n_rows), "rows_produced": bool(with_rows),
                    "kernel_ms": {name: m[name] for name in EDIT_KERNELS}, "e2e_ms": m["e2e"], "counts_only_e2e_ms": m["counts_only_e2e"],
                    "exact_k_search_count_ms": m["k_search_count"], "approx_k_asearch_count_ms": m["k_asearch_count"],
                    "count_ratio_to_asearch": round(m["k_esearch_count"] / m["k_asearch_count"], 3),
                    "count_ratio_to_exact": round(m["k_esearch_count"] / m["k_search_count"], 3),
                    "count_pass_fraction_of_hbm_floor": round(floor_ms / m["k_esearch_count"], 3)}
            if k == 0:
                h, e = search.edit_blob(b, p, 0, "both", True, "all", max_hits=10**9), search.search_blob(b, p, "both", True, max_hits=10**9)
                case["agree_with_exact"] = bool(h.ids.size == e.ids.size and (h.ids == e.ids).all() and (h.starts == e.starts).all() and
                                                (h.stops == e.stops).all() and (h.strands == e.strands).all() and not h.edits.any())
            out["cases"].append(case)
            print("L=%d k=%d: %d ends, %d rows" % (len(p), k, n_ends, n_rows), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
