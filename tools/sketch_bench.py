"""Sketching on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB) and the comparison kernel on synthetic
sets.  One JSON line, written to --out as the legs finish.

Sketches, k = 21, canonical: scaled = 1000 and scaled = 100, per record and pooled, and size = 1000 per record with the rounds
it took.  Kernel ms per stage (fx_prof_*): k_sk_count (the filter pass), k_sk_scan (letters, thresholds, kept scan, the cut at
slen, row scan), k_sk_emit, k_sk_sort (both radix steps and the gather), k_sk_reduce (heads, bounds, decisions, the keys that
stay).  Medians of --reps repetitions with minimum and maximum, alternated in the same run, repetition by repetition, with two
yardsticks on the same handle: k_search_count of the pattern 'A' and k_kt_hist of fx_fasta_kmer_table at k = 21 (canonical;
min_count above every count, so no table comes home).  The count pass is reported as a multiple of k_kt_hist of the same run.
The kept share is the keys of the per-record sketch over the window positions and, once the k-mer table's walk has counted
them, over the valid windows, next to 1 / scaled: the hash is a bijection of the 2k-bit words thresholded on its value, and how
evenly it spreads the k-mers of a text is a measurement, not a given.

Comparison: 1000 x 1000 sets of 1000 keys and 100 x 100 sets of 10^5 keys (every set a random half of a pool twice its size, so
the Jaccard index of a pair is about 1/3), at limit 0 and at limit = the set size.  Wall ms of the whole call (upload of nothing,
one kernel, two copies home), medians of --reps; pairs and key probes (one binary search per key of A and pair) per second.
The kernel that ships reads both lists from global memory; a form that stages the B lists of a workgroup in LDS was not built.

    python tools/sketch_bench.py [--gbp 3.0] [--reps 5] [--kt-reps 3] [--no-kt] [--out profiles/fasta_sketch.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 21
STAGES = ("k_sk_count", "k_sk_scan", "k_sk_emit", "k_sk_sort", "k_sk_reduce")


def st(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def alternate(b, reps, legs):
    """legs: {name: (run, kernel names)}; one warm-up each, then reps rounds that run every leg once, in order ->
    {name: (last result, {kernel: stats}, end-to-end stats)}"""
    for run, _ in legs.values():
        run()
    per = {n: {k: [] for k in names} for n, (_, names) in legs.items()}
    e2e, res = {n: [] for n in legs}, {}
    for _ in range(reps):
        for n, (run, names) in legs.items():
            b.prof_enable(1)
            b.prof_reset()
            t0 = time.perf_counter()
            res[n] = run()
            e2e[n].append((time.perf_counter() - t0) * 1e3)
            pr = b.prof_read()
            b.prof_enable(0)
            for k in names:
                per[n][k].append(pr[k][0] if k in pr else 0.0)
    return {n: (res[n], {k: st(v) for k, v in per[n].items()}, st(e2e[n])) for n in legs}


def compare_case(n_sets, n_keys, reps, rng):
    from pyfastx_amd.sketch import Sketch
    pool = np.unique(rng.integers(0, 4 ** K, 2 * n_keys + 64, dtype=np.uint64))[:2 * n_keys]

    def sets():
        return [np.sort(pool[rng.permutation(pool.size)[:n_keys]]) for _ in range(n_sets)]
    a, b = Sketch.from_hashes(sets(), K, size=n_keys), Sketch.from_hashes(sets(), K, size=n_keys)
    out = {"sets": [n_sets, n_sets], "keys_per_set": n_keys, "form": "global memory (ships)"}
    for name, limit in (("limit_0", 0), ("limit_size", n_keys)):
        a.compare(b, limit=limit, max_pairs=n_sets * n_sets)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            shared, total = a.compare(b, limit=limit, max_pairs=n_sets * n_sets)
            ms.append((time.perf_counter() - t0) * 1e3)
        s = st(ms)
        sec = s["median_ms"] / 1e3
        out[name] = {"call": s, "pairs_per_s": round(n_sets * n_sets / sec, 1), "key_probes_per_s": round(n_sets * n_sets * n_keys / sec, 1),
                     "mean_jaccard": round(float((shared / np.maximum(total, 1)).mean()), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kt-reps", type=int, default=3)
    ap.add_argument("--no-kt", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyfastx_amd import _lib, search, sketch, synth
    dev = torch.device("cuda:0")
    out = {"tool": "sketch_bench", "k": K, "canonical": True, "reps": a.reps, "sketch": [], "k_kt_hist": "not measured", "compare": []}

    def dump():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    rng = np.random.default_rng(20261020)
    for n_sets, n_keys in ((1000, 1000), (100, 100_000)):
        out["compare"].append(compare_case(n_sets, n_keys, a.reps, rng))
        dump()
    out["compare_lds_staged_form"] = "not built"

    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t = synth.fasta_generate(plan, dev, keep_flat=False)[0]
    torch.cuda.synchronize(dev)
    nb = int(plan["n_bytes"])
    slen = np.asarray(plan["slen"], dtype=np.int64)
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    positions = int(np.maximum(slen - K + 1, 0).sum())
    out.update({"n_bytes": nb, "n_records": int(slen.size), "bases": int(slen.sum()), "window_positions": positions})
    forms = (("scaled_1000", dict(scaled=1000), False), ("scaled_1000_pooled", dict(scaled=1000), True), ("scaled_100", dict(scaled=100), False),
             ("scaled_100_pooled", dict(scaled=100), True), ("size_1000", dict(size=1000), False))
    legs = {"search": (lambda: search.count_blob(b, "A", "both"), ("k_search_count",))}
    for name, kw, pooled in forms:
        legs[name] = (lambda kw=kw, pooled=pooled: sketch.fasta_sketch_blob(b, K, canonical=True, pooled=pooled, **kw), STAGES)
    r = alternate(b, a.reps, legs)
    yard = r["search"][1]["k_search_count"]
    out["k_search_count_A"] = yard
    for name, kw, pooled in forms:
        sk, kern, e2e = r[name]
        keys = int(sk.sizes.sum())
        case = {"form": name, "pooled": pooled, "sets": sk.n_sets, "keys": keys, "n_rounds": sk.n_rounds, "kernels": kern, "e2e": e2e,
                "count_times_k_search_count": round(kern["k_sk_count"]["median_ms"] / yard["median_ms"], 3)}
        case.update(kw)
        if "scaled" in kw and not pooled:
            case["kept_share_of_windows"] = round(keys / positions, 7)
            case["one_over_scaled"] = round(1.0 / kw["scaled"], 7)
        out["sketch"].append(case)
    del r
    print(dump())
    if a.no_kt:
        return
    # ---- the k-mer table's histogram walk at k = 21, alternated with the count pass of scaled = 1000
    legs = {"kt": (lambda: b.fasta_kmer_table(K, True, min_count=1 << 40)[2], ("k_kt_hist", "k_kt_kept")),
            "sk": (lambda: sketch.fasta_sketch_blob(b, K, scaled=1000).n_sets, ("k_sk_count",))}
    try:
        r = alternate(b, a.kt_reps, legs)
        hist, cnt = r["kt"][1]["k_kt_hist"], r["sk"][1]["k_sk_count"]
        out["k_kt_hist"] = {"windows": int(r["kt"][0]), "k_kt_hist": hist, "k_kt_kept": r["kt"][1]["k_kt_kept"], "kmer_table_e2e": r["kt"][2], "k_sk_count": cnt,
                            "reps": a.kt_reps, "count_times_k_kt_hist": round(cnt["median_ms"] / hist["median_ms"], 3) if hist["median_ms"] else None}
        for case in out["sketch"]:                           # the valid windows are known now: the positions minus those that hold an N
            if "kept_share_of_windows" in case:
                case["kept_share_of_valid_windows"] = round(case["keys"] / max(int(r["kt"][0]), 1), 7)
    except _lib.FxError as e:
        out["k_kt_hist"] = {"error": str(e)}
    print(dump())


if __name__ == "__main__":
    main()
