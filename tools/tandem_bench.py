"""Tandem-repeat search on a resident synthetic genome of the C2 shape (synth.fasta_plan: 3 Gbp, 60-column lines, ~50 %
soft-masked blocks, telomere and centromere N runs) with a planted share of perfect repeats (period 1..8, 12..120 letters,
written over the random letters of the chromosomes and scaffolds): kernel ms (fx_prof_*) of
  k_td_count / k_td_scan / k_td_close / k_td_emit for Krait's defaults (12, 7, 5, 4, 4, 4) on the whole genome;
  the same for min_copies = (2,) * 8 -- on the whole genome up to the offsets (the count of rows is read, the rows themselves
  would not fit in host memory and are refused by max_repeats=0), and with the emit pass on the scaffolds alone;
  k_an_runs_count of class_runs("N") and k_search_count of the pattern A ('+' strand, counts only) beside them: same
  process, same bytes, same run layout.
Medians over --reps timed runs after a warm-up, with the smallest and largest.  One JSON line.

    python tools/tandem_bench.py [--bp 3000000000] [--share 0.01] [--reps 5] [--out profiles/fasta_tandem.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TD = ["k_td_count", "k_td_scan", "k_td_close", "k_td_emit"]


def plant(blob_t, plan, share, dev, seed=99):
    """Perfect repeats written over `share` of the letters of the blob -> (number planted, letters planted)."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    slen, boff, w = plan["slen"], plan["boff"], int(plan["width"])
    ok = np.nonzero(slen >= 1000)[0]
    n = int(share * int(slen.sum()) / 66)                      # (lengths 12..120: 66 letters on average)
    if n == 0:
        return 0, 0
    rec = rng.choice(ok, n, p=slen[ok] / slen[ok].sum())
    ln = rng.integers(12, 121, n)
    st = (rng.random(n) * (slen[rec] - ln)).astype(np.int64)
    per = rng.integers(1, 9, n)
    motif = rng.integers(0, 4, (n, 8)).astype(np.uint8)
    first = np.concatenate([[0], np.cumsum(ln)])
    t = lambda a, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    which = torch.repeat_interleave(torch.arange(n, device=dev), t(ln))
    within = torch.arange(int(first[-1]), device=dev) - t(first[:-1])[which]
    x = t(st)[which] + within
    off = t(boff[rec])[which] + x + x // w
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    blob_t[off] = letters[t(motif, torch.uint8)[which, within % t(per)[which]].long()]
    return n, int(first[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, annot, search, synth, tandem
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=a.bp)
    blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
    n_planted, bp_planted = plant(blob_t, plan, a.share, dev)
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

    def refused(mc):
        try:
            tandem.repeats_blob(b, mc, max_repeats=0)
        except ValueError as e:
            return int(str(e).split()[0])
        return 0

    two = (2,) * 8
    scaffolds = np.arange(plan["n_chrom"], len(slen), dtype=np.int64)
    krait, t_krait = timed(lambda: tandem.repeats_blob(b, tandem.KRAIT_DEFAULT), TD)
    n_two, t_two = timed(lambda: refused(two), TD[:3])
    small, t_small = timed(lambda: tandem.repeats_blob(b, two, ids=scaffolds), TD)
    gaps, t_n = timed(lambda: annot.runs_blob(b, "N"), ["k_an_runs_count", "k_an_runs_scan", "k_an_runs_emit"])
    _, t_search = timed(lambda: search.count_blob(b, "A", "+"), ["k_search_count", "k_search_scan"])

    an, sc = t_n["k_an_runs_count"]["median_ms"], t_search["k_search_count"]["median_ms"]
    ratio = lambda t: round(t["k_td_count"]["median_ms"] / an, 3) if an else None
    by_period = {int(p): int(c) for p, c in zip(*np.unique(krait.periods, return_counts=True))}
    out = {"tool": "tandem_bench", "total_bp": int(slen.sum()), "n_bytes": nb, "n_records": int(len(slen)), "n_runs": nb // 256, "reps": a.reps,
           "planted": {"share": a.share, "repeats": n_planted, "letters": bp_planted},
           "krait_defaults": {"min_copies": list(tandem.KRAIT_DEFAULT), "rows": len(krait), "rows_by_period": by_period,
                              "total_median_ms": total(t_krait), "kernels": t_krait, "count_over_an_runs_count": ratio(t_krait)},
           "two_copies": {"min_copies": list(two), "rows": n_two, "emit": "refused (max_repeats=0): the rows are counted, not stored",
                          "total_median_ms": total(t_two), "kernels": t_two, "count_over_an_runs_count": ratio(t_two)},
           "two_copies_scaffolds": {"records": int(scaffolds.size), "bp": int(slen[scaffolds].sum()), "rows": len(small),
                                    "total_median_ms": total(t_small), "kernels": t_small},
           "class_runs_N": {"rows": len(gaps), "kernels": t_n},
           "search_count_A_plus": t_search,
           "count_over_search_count": round(t_krait["k_td_count"]["median_ms"] / sc, 3) if sc else None}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
