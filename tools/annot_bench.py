"""Region / window composition and class runs on a resident synthetic genome of the C2 shape (synth.fasta_plan: 3 Gbp, 60-column
lines, ~50 % soft-masked blocks, telomere and centromere N runs): kernel ms (fx_prof_*) of
  rank build   k_an_rank + k_an_scan (the index is given back before every repetition) -- next to k_search_count with the
               pattern A, '+' strand, counts only, in the same process on the same bytes in the same run layout.  The build
               reads the stream once and writes 64 bytes per 256-byte run, so the yardstick is k_search_count x 1.25;
  regions      k_an_region for 10^6 random regions of 100 bp and of 10 kbp -- next to k_fetch (the line-arithmetic gather and
               what it leaves over) for the 100 bp set;
  windows      k_an_region over the tiling 1 kbp windows of every record;
  class runs   k_an_runs_count / _scan / _emit for class_runs("N") and class_runs("masked", min_len=1000).
Medians over --reps timed runs after a warm-up, with the smallest and largest.  One JSON line.

    python tools/annot_bench.py [--bp 3000000000] [--reps 5] [--out profiles/fasta_annot.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, annot, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=a.bp)
    blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own stream reads the blob
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    slen = plan["slen"]
    assert b.fasta_build().n_seq == len(slen)

    def timed(run, names, before=None):
        if before:
            before()
        run()                                              # warm-up: allocations, code objects
        per = {k: [] for k in names}
        for _ in range(a.reps):
            if before:
                before()
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

    _, t_build = timed(b.fasta_rank_build, ["k_an_rank", "k_an_scan"], before=b.fasta_rank_free)
    _, t_search = timed(lambda: search.count_blob(b, "A", "+"), ["k_search_count", "k_search_scan"])
    b.fasta_rank_build()
    rng = np.random.default_rng(7)
    out_regions = {}
    for name, ln in (("100bp", 100), ("10kbp", 10_000)):
        ok = np.nonzero(slen >= ln)[0]
        ids = ok[rng.integers(0, ok.size, a.regions)]
        st = (rng.random(a.regions) * (slen[ids] - ln + 1)).astype(np.int64)
        r, t = timed(lambda: annot.region_blob(b, ids, st, st + ln), ["k_an_region"])
        assert (r.length == ln).all()
        out_regions[name] = t["k_an_region"]
        if ln == 100:
            (buf, offs), tf = timed(lambda: b.fasta_fetch_alloc(ids, st, st + ln), ["k_fetch", "k_fetch_rest"])
            # the fetched letters, counted on the host, against the first rows
            for k in range(200):
                s = buf[offs[k]:offs[k + 1]].tobytes().decode("latin-1")
                want = [sum(s.count(c) for c in pair) for pair in ("Aa", "Cc", "Gg", "Tt", "Nn")]
                assert r.counts[k, :5].tolist() == want and int(r.counts[k, 6]) == sum(c.islower() for c in s), "region differs from the fetched letters"
            out_regions["fetch_100bp"] = {"total_median_ms": total(tf), "kernels": tf}
            del buf
    w, t_win = timed(lambda: annot.window_blob(b, slen, 1000), ["k_an_region", "k_an_scan"])
    n_win = len(w)
    assert int(w.length.sum()) == int(slen.sum())
    del w
    run_names = ["k_an_runs_count", "k_an_runs_scan", "k_an_runs_emit"]
    gaps, t_n = timed(lambda: annot.runs_blob(b, "N"), run_names)
    masked, t_m = timed(lambda: annot.runs_blob(b, "masked", 1000), run_names)

    build_ms, count_ms = total(t_build), t_search["k_search_count"]["median_ms"]
    out = {"tool": "annot_bench", "total_bp": int(slen.sum()), "n_bytes": nb, "n_records": int(len(slen)), "reps": a.reps,
           "rank_build": {"total_median_ms": build_ms, "kernels": t_build, "index_bytes": 64 * (nb // 256)},
           "search_count_A_plus": t_search,
           "yardstick_ms": round(1.25 * count_ms, 4), "build_over_yardstick": round(build_ms / (1.25 * count_ms), 3) if count_ms else None,
           "rank_pass_over_search_count": round(t_build["k_an_rank"]["median_ms"] / count_ms, 3) if count_ms else None,
           "regions": {"n": a.regions, **out_regions},
           "windows_1kbp": {"n": n_win, "kernels": t_win},
           "class_runs_N": {"rows": len(gaps), "total_median_ms": total(t_n), "kernels": t_n},
           "class_runs_masked_min1000": {"rows": len(masked), "total_median_ms": total(t_m), "kernels": t_m}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
