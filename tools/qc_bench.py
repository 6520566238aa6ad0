"""FASTQ quality control on a resident synthetic FASTQ (synth.fastq_generate: reads of 150 bases, the C3 shape at
--reads 100000000): kernel ms (fx_prof_*) of the per-read pass (fx_fastq_read_stats), the cycle pass (fx_fastq_cycle_hist) and
select (fx_fastq_select: predicate pass, scans, emit), next to fx_fastq_comp's table kernel on the same handle in the same
run -- the kernel that reads the same sequence and quality bytes -- and the fraction of the HBM floor (the bytes each pass
must read at 6.5 TB/s).  Medians over --reps timed runs after a warm-up, with the smallest and largest.  The results are
checked against torch (per-read sums, one cycle row, the selected count) before the line is printed.  One JSON line.

    python tools/qc_bench.py [--reads 20000000] [--reps 7] [--out profiles/fastq_qc.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.pop("FX_FQ_COMP_STREAM", None)              # the yardstick is the table kernel
    import numpy as np
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    n, rlen = a.reads, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own stream reads the blob
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n                    # fx_fastq_build, not fx_fastq_build_comp: fx_fastq_comp runs its kernel
    view = blob_t[:n * rec].view(n, rec)
    sel = dict(phred=33, low_qual=7, mean_qual=(39, 2), low_frac=(1, 5), max_other=0)      # scores are uniform on 2..37

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

    _, t_comp = timed(lambda: b.fastq_comp(), ["k_fastq_comp"])
    st, t_read = timed(lambda: b.fastq_read_stats(phred=33, low_qual=20), ["k_fq_read_stats"])
    hist, t_cyc = timed(lambda: b.fastq_cycle_hist(rlen), ["k_fq_cycle_hist"])
    ids, t_sel = timed(lambda: b.fastq_select(**sel), ["k_fq_select", "k_fq_select_scan", "k_fq_select_emit"])

    # the checks, in slices of 2 M reads
    qsum = np.empty(n, dtype=np.int64)
    passed = 0
    row = torch.zeros(256, dtype=torch.int64, device=dev)
    cyc = 77
    for c0 in range(0, n, 2_000_000):
        q = view[c0:c0 + 2_000_000, hl + rlen + 3:hl + 2 * rlen + 3].to(torch.int64)
        s = view[c0:c0 + 2_000_000, hl:hl + rlen]
        d = q - 33
        qs = d.sum(1)
        qsum[c0:c0 + 2_000_000] = qs.cpu().numpy()
        other = ((s != 65) & (s != 67) & (s != 71) & (s != 84)).sum(1)
        passed += int(((qs * 2 >= 39 * rlen) & ((d < 7).sum(1) * 5 <= rlen) & (other <= 0)).sum())
        row += torch.bincount(q[:, cyc], minlength=256)
    assert np.array_equal(st["qsum"], qsum), "per-read sums differ from torch"
    assert np.array_equal(hist[0][cyc], row.cpu().numpy()), "cycle row differs from torch"
    assert len(ids) == passed and int(hist[2][0]) == n, "selected count differs from torch"

    line_bytes = 2 * rlen * n
    floor_ms = (line_bytes + 24 * n) / (HBM_TBS * 1e12) * 1e3          # both lines of every read and its table row
    sel_ms = sum(t_sel[k]["median_ms"] for k in t_sel)
    comp_ms = t_comp["k_fastq_comp"]["median_ms"]
    out = {"tool": "qc_bench", "n_reads": n, "read_length": rlen, "n_bytes": nb, "reps": a.reps, "checked_against_torch": True,
           "hbm_floor_ms": round(floor_ms, 4), "fastq_comp_table_kernel": t_comp["k_fastq_comp"],
           "read_stats": t_read["k_fq_read_stats"], "cycle_hist": t_cyc["k_fq_cycle_hist"],
           "select": {"total_median_ms": round(sel_ms, 4), "kernels": t_sel, "selected": int(len(ids))},
           "fraction_of_hbm_floor": {"fastq_comp_table_kernel": round(floor_ms / comp_ms, 3) if comp_ms else None,
                                     "read_stats": round(floor_ms / t_read["k_fq_read_stats"]["median_ms"], 3),
                                     "cycle_hist": round(floor_ms / t_cyc["k_fq_cycle_hist"]["median_ms"], 3),
                                     "select": round(floor_ms / sel_ms, 3)},
           "times_the_table_kernel": {"read_stats": round(t_read["k_fq_read_stats"]["median_ms"] / comp_ms, 2) if comp_ms else None,
                                      "cycle_hist": round(t_cyc["k_fq_cycle_hist"]["median_ms"] / comp_ms, 2) if comp_ms else None,
                                      "select": round(sel_ms / comp_ms, 2) if comp_ms else None}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
