"""k-mer screening (Fastq.kmer_hits, csrc/fx_kmer_screen.hpp) of 2 x 10^7 synthetic reads of 150 bases against device k-mer sets
of 10^3 (probed in LDS), 10^5, 10^7 and 10^8 codes; k = 21 and 31, plain and canonical.  The source of a set is a random
sequence with as many windows as the set has codes; every --spike-th read is overwritten with a slice of it, so a known share
of the reads hits with every window and the rest with next to none.

Per leg: kernel ms of k_ks_fastq (fx_prof_*), probes per second (valid windows / kernel time), the set's build (k_ks_insert ms
and the whole fx_kmer_set_create call with its upload), and two yardsticks measured on the same handle in the same run:
  (a) k_kt_hist of fx_fastq_kmer_table at the same k and strand rule: k_kt_fastq<CANON, false> reads the same bytes and rolls the
      same codes, with an add to a bin in LDS where the screen has a probe;
  (b) k_fq_read_stats: the sequence and quality bytes of every read once.
No target ratio is fixed: this run is what measures a random 8-byte probe against tables of these sizes.
The columns of a sample of the reads are checked against numpy (rolling codes, membership by searchsorted in the sorted codes)
before a time is reported.  Medians of --reps runs; a measurement whose slowest run is more than 1.5 x its fastest is taken
again and flagged "disturbed" if it stays so.  One JSON line.

    python tools/kmer_screen_bench.py [--reads 20000000] [--sets 1000,100000,10000000,100000000] [--reps 7] [--out profiles/kmer_screen.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (21, 31)
RLEN = 150


def rolling_codes(xp, codes4, k, canonical):
    """The counted code of every window of a 2-bit coded int64 sequence (xp: numpy or torch; every letter valid)."""
    n = codes4.shape[-1] - k + 1
    code = xp.zeros_like(codes4[..., :n])
    rc = xp.zeros_like(codes4[..., :n])
    for j in range(k):
        w = codes4[..., j:j + n]
        code = code * 4 + w
        rc = rc + ((3 - w) << (2 * j))
    return xp.minimum(code, rc) if canonical else code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--sets", default="1000,100000,10000000,100000000")
    ap.add_argument("--spike", type=int, default=16, help="every spike-th read is cut from the set's source")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=20000, help="reads checked against numpy per leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, kmer, synth
    dev = torch.device("cuda:0")
    st = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def timed_once(b, run, name):
        torch.cuda.synchronize(dev)
        run()                                                  # warm-up: allocations, code objects
        ms = []
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            r = run()
            pr = b.prof_read()
            b.prof_enable(0)
            ms.append(pr[name][0] if name in pr else 0.0)
        return r, st(ms)

    def timed(b, run, name):
        for _ in range(3):
            r, t = timed_once(b, run, name)
            if t["max_ms"] <= 1.5 * t["min_ms"]:
                return r, t
        t["disturbed"] = True
        return r, t

    n = a.reads
    blob_t, cols = synth.fastq_generate(n, dev, rlen=RLEN)
    torch.cuda.synchronize(dev)
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    seq_view = blob_t[:n * rec].view(n, rec)[:, hl:hl + RLEN]
    lut = torch.full((256,), 4, dtype=torch.int64, device=dev)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    for j, c in enumerate(b"ACGT"):
        lut[c] = j
    spiked = torch.arange(0, n, a.spike, device=dev)
    sample = np.unique(np.concatenate([np.arange(min(a.sample, n)), np.arange(0, n, max(n // a.sample, 1))])).astype(np.int64)
    out = {"tool": "kmer_screen_bench", "n_reads": n, "read_length": RLEN, "n_bytes": nb, "reps": a.reps, "spiked_share": round(spiked.numel() / n, 6),
           "lds_keys": kmer.SCREEN_LDS_KEYS, "checked_against_numpy": True, "legs": []}
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261017)
    for target in [int(x) for x in a.sets.split(",")]:
        for k in KS:
            # the source, the reads cut from it, the stream indexed again
            src4 = torch.randint(0, 4, (target + k - 1,), device=dev, generator=gen)
            at = torch.randint(0, max(target + k - 1 - RLEN, 0) + 1, (spiked.numel(),), device=dev, generator=gen)
            span = min(RLEN, target + k - 1)                   # a source shorter than a read fills its front
            for lo in range(0, spiked.numel(), 1 << 20):
                rows = spiked[lo:lo + (1 << 20)]
                idx = at[lo:lo + (1 << 20), None] + torch.arange(span, device=dev)[None, :]
                seq_view[rows, :span] = letters[src4[idx]]
            torch.cuda.synchronize(dev)
            b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
            assert b.fastq_build().n_reads == n
            _, stats_ms = timed(b, lambda: b.fastq_read_stats(), "k_fq_read_stats")
            host4 = lut[seq_view[torch.from_numpy(sample).to(dev)].long()].cpu().numpy()
            assert (host4 < 4).all()
            for canonical in (False, True):
                codes = torch.unique(rolling_codes(torch, src4, k, canonical)).cpu().numpy()
                torch.cuda.synchronize(dev)
                b.prof_enable(1)
                b.prof_reset()
                t0 = time.perf_counter()
                s = b.kmer_set(k, canonical, codes)
                build_ms = (time.perf_counter() - t0) * 1e3
                insert_ms = b.prof_read().get("k_ks_insert", (0.0, 0))[0]
                b.prof_enable(0)
                # the check: a sample of the reads against numpy
                w = rolling_codes(np, host4, k, canonical)
                pos = np.minimum(np.searchsorted(codes, w), codes.size - 1)
                want_h = (codes[pos] == w).sum(axis=1)
                nw, nh = b.fastq_kmer_hits(s, ids=sample)
                agree = bool((nw == RLEN - k + 1).all() and np.array_equal(nh, want_h))
                assert agree, "set of %d codes, k = %d, canonical = %s differs from numpy" % (target, k, canonical)
                (nw, nh), ks_ms = timed(b, lambda: b.fastq_kmer_hits(s), "k_ks_fastq")
                windows = int(np.asarray(nw, dtype=np.int64).sum())
                full = int((np.asarray(nh) == np.asarray(nw)).sum())
                _, hist_ms = timed(b, lambda: b.fastq_kmer_table(k, canonical)[2], "k_kt_hist")
                out["legs"].append({
                    "set_codes": int(codes.size), "form": "lds" if codes.size <= kmer.SCREEN_LDS_KEYS else "global",
                    "table_bytes": 8 * max(64, 1 << int(2 * codes.size - 1).bit_length()), "k": k, "canonical": canonical, "agree": agree,
                    "windows": windows, "hits": int(np.asarray(nh, dtype=np.int64).sum()), "reads_hit_by_every_window": full,
                    "k_ks_fastq": ks_ms, "probes_per_s": round(windows / (ks_ms["median_ms"] * 1e-3), 1) if ks_ms["median_ms"] else None,
                    "set_build_ms": round(build_ms, 3), "k_ks_insert_ms": round(insert_ms, 4),
                    "k_kt_hist": hist_ms, "k_fq_read_stats": stats_ms,
                    "times_k_kt_hist": round(ks_ms["median_ms"] / hist_ms["median_ms"], 3) if hist_ms["median_ms"] else None,
                    "times_k_fq_read_stats": round(ks_ms["median_ms"] / stats_ms["median_ms"], 3) if stats_ms["median_ms"] else None})
                s.close()
                del codes, s
            del b, src4
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
