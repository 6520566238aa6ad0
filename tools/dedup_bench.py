"""Exact duplicate detection (Fastq.dedup, csrc/fx_fastq_dedup.hpp) on 2 x 10^7 synthetic reads of 150 bases of which a stated
share are copies of earlier reads: every --every-th read is overwritten with the sequence of a random earlier read that is no
copy itself, so first[] is known by construction.

The input is checked against numpy first: `first` of the whole file must equal the constructed one, the originals of a sample
must be distinct (np.unique over their bytes) and a sample of the copies must equal their first occurrence byte for byte.

Reported: kernel ms (fx_prof_*) of the four stages of one fx_fastq_dedup call -- k_dd_hash, k_dd_sort (the radix passes),
k_dd_verify (head scan, rank, verify, group sizes, the count of what is left), k_dd_select (predicate, scan, emit, gather) --
and two yardsticks measured on the same handle in the same run:
  (a) k_fq_read_stats on the same reads: it reads the same sequence bytes (and the quality bytes besides);
  (b) a pair sort alone on the same n: torch.sort of n random int64 keys with their indices (device events).
No target ratio is fixed.  Medians of --reps runs; a measurement whose slowest run is more than 1.5 x its fastest is taken again
and flagged "disturbed" if it stays so.  One JSON line.

    python tools/dedup_bench.py [--reads 20000000] [--every 4] [--reps 7] [--revcomp] [--out profiles/fastq_dedup.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RLEN = 150
STAGES = ("k_dd_hash", "k_dd_sort", "k_dd_verify", "k_dd_select")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--every", type=int, default=4, help="every every-th read is a copy of an earlier one")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=200000, help="reads checked byte for byte against numpy")
    ap.add_argument("--revcomp", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    st = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed_once(b, run, names):
        torch.cuda.synchronize(dev)
        run()                                                  # warm-up: allocations, code objects
        ms = {k: [] for k in names}
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            r = run()
            pr = b.prof_read()
            b.prof_enable(0)
            for k in names:
                ms[k].append(pr[k][0] if k in pr else 0.0)
        return r, {k: st(v) for k, v in ms.items()}

    def timed(b, run, names):
        for _ in range(3):
            r, t = timed_once(b, run, names)
            if all(x["max_ms"] <= 1.5 * x["min_ms"] for x in t.values()):
                return r, t
        for x in t.values():
            if x["max_ms"] > 1.5 * x["min_ms"]:
                x["disturbed"] = True
        return r, t

    n, every = a.reads, max(a.every, 2)
    blob_t, cols = synth.fastq_generate(n, dev, rlen=RLEN)
    torch.cuda.synchronize(dev)
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    seq_view = blob_t[:n * rec].view(n, rec)[:, hl:hl + RLEN]
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261018)
    rows = torch.arange(every - 1, n, every, device=dev)       # the copies
    src = (torch.rand(rows.numel(), device=dev, generator=gen, dtype=torch.float64) * rows).long()
    src = src - (src % every == every - 1).long()              # a copy is never copied: its source is an original in front of it
    for lo in range(0, rows.numel(), 1 << 20):
        seq_view[rows[lo:lo + (1 << 20)]] = seq_view[src[lo:lo + (1 << 20)]]
    torch.cuda.synchronize(dev)
    want = np.arange(n, dtype=np.int64)
    want[rows.cpu().numpy()] = src.cpu().numpy()
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    # the check: numpy on the constructed answer and on the bytes of a sample
    first, groups, rounds = b.fastq_dup_first(revcomp=a.revcomp)
    sample = np.unique(np.concatenate([np.arange(min(a.sample, n)), np.arange(0, n, max(n // a.sample, 1))])).astype(np.int64)
    host = seq_view[torch.from_numpy(sample).to(dev)].cpu().numpy()
    firsts = seq_view[torch.from_numpy(np.ascontiguousarray(first[sample])).to(dev)].cpu().numpy()
    orig = host[sample % every != every - 1]
    agree = bool(np.array_equal(first, want) and groups == n - rows.numel() and np.array_equal(host, firsts)
                 and np.unique(orig, axis=0).shape[0] == orig.shape[0])
    assert agree, "first[] differs from the constructed answer or from the bytes of the sample"
    (pos, cp, g2, r2), stage_ms = timed(b, lambda: b.fastq_dedup(revcomp=a.revcomp, want_copies=True), STAGES)
    assert pos.size == groups == g2 and int(cp.sum()) == n and np.array_equal(pos, np.nonzero(want == np.arange(n))[0])
    _, first_ms = timed(b, lambda: b.fastq_dup_first(revcomp=a.revcomp), STAGES[:3])
    _, stats_ms = timed(b, lambda: b.fastq_read_stats(), ("k_fq_read_stats",))

    def torch_sort():
        keys = torch.randint(-2 ** 62, 2 ** 62, (n,), device=dev, generator=gen)
        ms = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.sort(keys, stable=True)
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        return st(ms[1:])

    sort_ms = torch_sort()
    total = sum(stage_ms[k]["median_ms"] for k in STAGES)
    out = {"tool": "dedup_bench", "n_reads": n, "read_length": RLEN, "n_bytes": nb, "reps": a.reps, "revcomp": a.revcomp,
           "copies_share": round(rows.numel() / n, 6), "n_groups": int(groups), "n_rounds": int(rounds), "checked_against_numpy": agree,
           "dedup": stage_ms, "dedup_kernel_ms": round(total, 4), "dup_first": first_ms,
           "k_fq_read_stats": stats_ms["k_fq_read_stats"], "torch_sort_pairs": sort_ms,
           "hash_times_k_fq_read_stats": round(stage_ms["k_dd_hash"]["median_ms"] / stats_ms["k_fq_read_stats"]["median_ms"], 3),
           "sort_times_torch_sort_pairs": round(stage_ms["k_dd_sort"]["median_ms"] / sort_ms["median_ms"], 3)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
