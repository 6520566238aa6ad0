"""Barcode demultiplexing on a resident synthetic FASTQ (synth.fastq_generate's reads of 150 bases, their headers ending in an
8 + 8 index field `1:N:0:XXXXXXXX+YYYYYYYY`, the same two barcodes planted in the first 16 bases; 2 % of the letters of either
changed): kernel ms (fx_prof_*) of k_fq_demux at 96, 1024 and 4096 samples, for one and two segments, in the header and at the
5' end, and of the grouping step (k_fq_demux_group: the radix sort on the bin, the scan of the counters, the order) -- next to
k_fq_read_stats on the same handle in the same run, and the HBM floor at 6.5 TB/s of one 128-byte line of the stream, the
table row and the three result columns per read.  Medians over --reps timed runs after a warm-up, with the smallest and
largest.  The columns of the 96-sample runs are checked against torch on the first 2 M reads before the line is printed.
One JSON line.

    python tools/demux_bench.py [--reads 20000000] [--reps 5] [--out profiles/fastq_demux.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
SIZES = (96, 1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    n, rlen = a.reads, 150
    blob0, cols = synth.fastq_generate(n, dev, rlen=rlen)
    rec0, hl0 = int(cols["rec"]), int(cols["soff"][0])
    # the sheet: 4096 8 + 8 barcodes, distinct in either half; the reads carry those of its first 96 rows
    rng = np.random.default_rng(17)
    halves = []
    for _ in range(2):
        h = np.unique(rng.integers(0, 4, (8000, 8)), axis=0)
        halves.append(h[rng.permutation(len(h))[:SIZES[-1]]])
    sheet = np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate(halves, axis=1)]
    assert sheet.shape == (SIZES[-1], 16)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    planted = torch.randint(0, SIZES[0], (n,), device=dev, generator=g)
    idx = torch.from_numpy(sheet[:SIZES[0]].copy()).to(dev)[planted]                   # n x 16
    wrong = torch.rand((n, 16), device=dev, generator=g) < 0.02
    idx = torch.where(wrong, torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n, 16), device=dev, generator=g)], idx)
    # the records again, with "ACGT\n" of the header replaced by the index field
    hl = hl0 - 5 + 18                                         # header line with its newline
    rec = rec0 - hl0 + hl
    t = torch.empty((n, rec), dtype=torch.uint8, device=dev)
    src = blob0[:n * rec0].view(n, rec0)
    t[:, :hl0 - 5] = src[:, :hl0 - 5]
    t[:, hl - 18:hl - 10] = idx[:, :8]
    t[:, hl - 10] = ord("+")
    t[:, hl - 9:hl - 1] = idx[:, 8:]
    t[:, hl - 1] = 10
    t[:, hl:] = src[:, hl0:]
    t[:, hl:hl + 16] = idx
    del src, blob0
    nb = n * rec
    blob_t = torch.zeros(nb + 131072, dtype=torch.uint8, device=dev)
    blob_t[:nb] = t.view(-1)
    del t
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own stream reads the blob
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n

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

    _, t_read = timed(lambda: b.fastq_read_stats(phred=33, low_qual=20), ["k_fq_read_stats"])
    modes = {"header_1": dict(src=[2], off=[0], seg=[0]), "header_2": dict(src=[2, 2], off=[0, 1], seg=[0, 1]),
             "5p_1": dict(src=[0], off=[0], seg=[0]), "5p_2": dict(src=[0, 0], off=[0, 8], seg=[0, 1])}
    names = ["k_fq_demux", "k_fq_demux_group"]
    results, keep = {}, {}
    for mode, m in modes.items():
        for ns in SIZES:
            bc = np.ascontiguousarray(np.concatenate([sheet[:ns, 8 * s:8 * s + 8] for s in m["seg"]], axis=1))
            nseg = len(m["seg"])
            r, tm = timed(lambda: b.fastq_demux(bc, m["src"], m["off"], [8] * nseg, [1] * nseg, margin=1), names)
            results["%s_%d" % (mode, ns)] = {"samples": int(bc.shape[0]), "kernel": tm["k_fq_demux"], "grouping": tm["k_fq_demux_group"],
                                            "assigned": int(r["counts"][:bc.shape[0]].sum()), "none": int(r["counts"][-2]),
                                            "ambiguous": int(r["counts"][-1])}
            if ns == SIZES[0]:
                keep[mode] = (bc.copy(), {k: np.array(r[k][:2_000_000]) for k in ("sample", "dist", "second")})
            del r

    # the checks: the 96-sample columns of the first 2 M reads, by torch
    m = min(n, 2_000_000)
    for mode, (bc, got) in keep.items():
        nseg = len(modes[mode]["seg"])
        B = torch.from_numpy(bc).to(dev)
        for c0 in range(0, m, 500_000):
            w = idx[c0:min(c0 + 500_000, m)]
            ok = torch.ones((w.shape[0], B.shape[0]), dtype=torch.bool, device=dev)
            tot = torch.zeros((w.shape[0], B.shape[0]), dtype=torch.int32, device=dev)
            for s in range(nseg):
                d = (w[:, None, 8 * s:8 * s + 8] != B[None, :, 8 * s:8 * s + 8]).sum(2, dtype=torch.int32)
                ok &= d <= 1
                tot += d
            tot = torch.where(ok, tot, torch.full_like(tot, 1 << 20))
            t1, i1 = tot.min(1)
            t2 = tot.scatter(1, i1[:, None], (1 << 20) + 1).min(1).values
            none, one = t1 >= (1 << 20), t2 >= (1 << 20)
            smp = torch.where(none, -1, torch.where(~one & (t2 - t1 < 1), -2, i1)).to(torch.int32).cpu().numpy()
            assert np.array_equal(got["sample"][c0:c0 + w.shape[0]], smp), "samples differ from torch (%s)" % mode
            assert np.array_equal(got["dist"][c0:c0 + w.shape[0]], torch.where(none, -1, t1).cpu().numpy()), "distances differ from torch"
            assert np.array_equal(got["second"][c0:c0 + w.shape[0]], torch.where(none | one, -1, t2).cpu().numpy()), "runners-up differ from torch"

    floor = (128 + 20 + 12) * n / (HBM_TBS * 1e12) * 1e3
    read_ms = t_read["k_fq_read_stats"]["median_ms"]
    out = {"tool": "demux_bench", "n_reads": n, "read_length": rlen, "n_bytes": nb, "reps": a.reps, "checked_against_torch": True,
           "read_stats": t_read["k_fq_read_stats"], "demux": results, "hbm_floor_ms": round(floor, 4),
           "ns_per_read_and_sample": {k: round(v["kernel"]["median_ms"] * 1e6 / (n * v["samples"]), 5) for k, v in results.items()},
           "kernel_over_read_stats": {k: round(v["kernel"]["median_ms"] / read_ms, 2) for k, v in results.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
