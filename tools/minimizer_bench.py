"""Minimizer sampling on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB): kernel ms (fx_prof_*) of
k_mz_count, the scans (k_search_scan: run plan, kept scan, fix at slen, row scan) and k_mz_emit, the rows and their density
next to 2 / (w + 1), for (k, w) = (15, 10), (21, 11), (19, 19), (31, 32), canonical, at hash and at lex order.  Counts-only
calls run on the whole genome; calls that bring rows home run on the shortest records whose rows fit --max-hits.

Two yardsticks from the same run on the same handle, alternated with the minimizer calls repetition by repetition: k_search_count
of the pattern 'A' (both strands) and k_kt_hist of fx_fasta_kmer_table at the same k (canonical; min_count above every count, so
no table comes home) -- both read the same bytes in the same run layout.  Medians of --reps repetitions with their minimum and
maximum; the share of the HBM floor is the stream read once at 6.5 TB/s over the count pass.  The file is written before the
k-mer table legs start and again after them.  One JSON line.

    python tools/minimizer_bench.py [--gbp 3.0] [--reps 5] [--max-hits 20000000] [--no-kt] [--out profiles/fasta_minimizers.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
PARAMS = ((15, 10), (21, 11), (19, 19), (31, 32))
ORDERS = ("hash", "lex")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=20_000_000)
    ap.add_argument("--no-kt", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyfastx_amd import _lib, minimizer, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t = synth.fasta_generate(plan, dev, keep_flat=False)[0]
    torch.cuda.synchronize(dev)
    nb = int(plan["n_bytes"])
    slen = np.asarray(plan["slen"], dtype=np.int64)
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    floor_ms = nb / (HBM_TBS * 1e12) * 1e3
    out = {"tool": "minimizer_bench", "n_bytes": nb, "n_records": int(slen.size), "bases": int(slen.sum()), "reps": a.reps, "canonical": True,
           "hbm_tbs": HBM_TBS, "hbm_floor_ms": round(floor_ms, 4), "cases": [], "k_kt_hist": "not measured"}

    def dump():
        line = json.dumps(out)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    by_len = np.argsort(slen, kind="stable")
    count_names, row_names = ("k_mz_count", "k_search_scan"), ("k_mz_count", "k_search_scan", "k_mz_emit")
    for k, w in PARAMS:
        # the shortest records whose expected rows, with a margin of 15 %, fit max_hits
        fit = np.cumsum(slen[by_len]) * (2.0 / (w + 1)) * 1.15 <= a.max_hits
        ids = np.sort(by_len[:int(fit.sum())])
        legs = {"search": (lambda: search.count_blob(b, "A", "both"), ("k_search_count",))}
        for order in ORDERS:
            legs["counts_" + order] = (lambda o=order: minimizer.count_blob(b, k, w, True, o), count_names)
            legs["rows_" + order] = (lambda o=order: minimizer.minimizers_blob(b, k, w, True, o, ids, a.max_hits), row_names)
        r = alternate(b, a.reps, legs)
        yard = r["search"][1]["k_search_count"]
        for order in ORDERS:
            counts, kc, e2e_c = r["counts_" + order]
            rows, kr, e2e_r = r["rows_" + order]
            n_all, positions = int(counts.sum()), int(np.maximum(slen - k + 1, 0).sum())
            sel_pos = int(np.maximum(slen[ids] - k + 1, 0).sum())
            assert rows.ids.size == int(counts[ids].sum()), "rows and counts of the selected records differ"
            out["cases"].append({
                "k": k, "w": w, "order": order, "expected_density": round(2.0 / (w + 1), 5),
                "genome": {"rows": n_all, "rows_plus": int(counts[:, 0].sum()), "density": round(n_all / positions, 5), "kernels": kc, "e2e": e2e_c},
                "selection": {"records": int(ids.size), "bases": int(slen[ids].sum()), "rows": int(rows.ids.size),
                              "density": round(rows.ids.size / max(sel_pos, 1), 5), "kernels": kr, "e2e": e2e_r},
                "k_search_count_A": yard,
                "count_times_k_search_count": round(kc["k_mz_count"]["median_ms"] / yard["median_ms"], 3),
                "count_pass_fraction_of_hbm_floor": round(floor_ms / kc["k_mz_count"]["median_ms"], 4)})
            del rows
    print(dump())
    if a.no_kt:
        return
    # ---- the k-mer table's histogram walk at the same k, alternated with the count pass at hash order
    out["k_kt_hist"] = []
    for k, w in PARAMS:
        legs = {"kt": (lambda: b.fasta_kmer_table(k, True, min_count=1 << 40)[2], ("k_kt_hist", "k_kt_kept")),
                "mz": (lambda: minimizer.count_blob(b, k, w, True, "hash"), ("k_mz_count",))}
        try:
            r = alternate(b, min(a.reps, 3), legs)
        except _lib.FxError as e:
            out["k_kt_hist"].append({"k": k, "w": w, "error": str(e)})
            continue
        hist, mz = r["kt"][1]["k_kt_hist"], r["mz"][1]["k_mz_count"]
        out["k_kt_hist"].append({"k": k, "w": w, "windows": int(r["kt"][0]), "k_kt_hist": hist, "k_kt_kept": r["kt"][1]["k_kt_kept"],
                                 "kmer_table_e2e": r["kt"][2], "k_mz_count": mz,
                                 "count_times_k_kt_hist": round(mz["median_ms"] / hist["median_ms"], 3) if hist["median_ms"] else None})
        dump()
    print(dump())


if __name__ == "__main__":
    main()
