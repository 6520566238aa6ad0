"""BGZF written on the device (csrc/fx_deflate.hpp) on the two record writers' shapes: the C2 genome (synth.fasta_plan) re-wrapped
to width 80 through fx_fasta_format_bgzf_alloc, and --reads synthetic reads of 150 (synth.fastq_generate) through
fx_fastq_format_bgzf_alloc, in batches of --batch-mb of records as the writers make them.  Per shape and level 0, 1, 2: kernel
ms (fx_prof_*) of k_bgzf_store / k_bgzf_deflate / k_bgzf_crc_put / k_bgzf_scan / k_bgzf_pack, the compressed size, and beside
them, alternated in every repetition on the same device:
  d2d_copy          a device-to-device copy of the bytes the batch compressed (torch, timed by events);
  decode_par        the BGZF open of the stream just written (kernel ms of k_bgzf_decode + k_bgzf_copy + k_bgzf_crc);
  plain             the plain entry of the same records: wall ms and the bytes that cross the link, next to the compressed
                    entry's wall ms and bytes;
  host_zlib_1       zlib level 1 over the same member payloads on --threads host threads (wall ms), and the sizes zlib levels 1
                    and 6 give on a sample of the members.
Medians over --reps timed runs after a warm-up, with the smallest and largest.  One JSON line.  Runs by hand on an MI355X.

    python tools/bgzf_write_bench.py [--bp 3000000000] [--reads 20000000] [--batch-mb 600] [--reps 5] [--out profiles/bgzf_write.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEMBER = 65280
KERNELS = ["k_bgzf_store", "k_bgzf_deflate", "k_bgzf_crc_put", "k_bgzf_scan", "k_bgzf_pack"]
DECODE = ["k_bgzf_decode", "k_bgzf_copy", "k_bgzf_crc"]


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=3_000_000_000)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--batch-mb", type=int, default=600)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sample", type=int, default=512, help="members zlib levels 1 and 6 are sized on")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, bgzf, synth
    dev = torch.device("cuda:0")

    def d2d_ms(nbytes, src, dst):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst[:nbytes].copy_(src[:nbytes])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_zlib(plain, level, pool):
        view = memoryview(plain)
        parts = [view[i:i + MEMBER] for i in range(0, len(view), MEMBER)]
        def one(p):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            return len(c.compress(p)) + len(c.flush()) + 26
        t0 = time.perf_counter()
        total = sum(pool.map(one, parts, chunksize=64))
        return (time.perf_counter() - t0) * 1e3, total

    def shape(b, plain_call, bgzf_call, tmp):
        """One batch of records through the plain entry and, per level, through the compressed one."""
        out = {}
        wall_plain = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            r = plain_call()
            wall_plain.append((time.perf_counter() - t0) * 1e3)
            plain = r[0]
        n = int(plain.size)
        out["bytes"] = n
        out["members"] = (n + MEMBER - 1) // MEMBER
        out["plain"] = {"wall": stats(wall_plain[1:]), "bytes_over_the_link": n + 8 * int(r[1].size)}
        src = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        d2d_ms(n, src, dst)
        with ThreadPoolExecutor(a.threads) as pool:
            z1 = [host_zlib(plain, 1, pool) for _ in range(a.reps)]
            step = max(out["members"] // a.sample, 1)
            sample = b"".join(bytes(plain[i * MEMBER:(i + 1) * MEMBER]) for i in range(0, out["members"], step))
            out["zlib_sample"] = {"bytes": len(sample), "level_1": host_zlib(sample, 1, pool)[1], "level_6": host_zlib(sample, 6, pool)[1]}
        out["host_zlib_1"] = {"threads": a.threads, "wall": stats([t for t, _ in z1]), "bytes": z1[0][1]}
        for level in (0, 1, 2):
            per, copy, dec, wall = {k: [] for k in KERNELS}, [], [], []
            bgzf_call(level)                               # warm-up: allocations, code objects
            for _ in range(a.reps):
                b.prof_enable(1)
                b.prof_reset()
                t0 = time.perf_counter()
                r = bgzf_call(level)
                wall.append((time.perf_counter() - t0) * 1e3)
                pr = b.prof_read()
                b.prof_enable(0)
                for k in KERNELS:
                    per[k].append(pr[k][0] if k in pr else 0.0)
                copy.append(d2d_ms(n, src, dst))
                stream, moff = r[0], r[1]
                path = os.path.join(tmp, "level%d.gz" % level)
                with open(path, "wb") as f:
                    f.write(memoryview(stream))
                    f.write(bgzf.EOF)
                _lib.lib().fx_prof_default(1)              # handles made from here on time their kernels: the open's own
                back = _lib.Blob.from_file(path, device=0)
                _lib.lib().fx_prof_default(0)
                pd = back.prof_read()
                dec.append(sum(pd[k][0] for k in DECODE if k in pd))
                assert back.size == n
                del back
            zb = int(stream.size)
            out["level_%d" % level] = {"kernels": {k: stats(v) for k, v in per.items()}, "kernel_sum_median_ms": round(sum(statistics.median(v) for v in per.values()), 4),
                                       "compressed_bytes": zb, "ratio": round(zb / max(n, 1), 4), "wall": stats(wall),
                                       "bytes_over_the_link": zb + 8 * int(moff.size) + 8 * int(r[2].size),
                                       "d2d_copy_same_bytes": stats(copy), "decode_of_the_stream": stats(dec)}
        return out

    out = {"tool": "bgzf_write_bench", "reps": a.reps, "batch_mb": a.batch_mb}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the C2 genome re-wrapped to width 80: the leading records whose output fits the batch
        plan = synth.fasta_plan(total_bp=a.bp)
        blob_t, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
        torch.cuda.synchronize(dev)
        b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
        assert b.fasta_build().n_seq == len(plan["slen"])
        cum = np.cumsum(plan["slen"] * 81 // 80 + 64)
        nrec = max(int(np.searchsorted(cum, a.batch_mb << 20)), 1)
        out["fasta_width_80"] = shape(b, lambda: b.fasta_format_alloc(nrec, width=80), lambda lv: b.fasta_format_alloc(nrec, width=80, level=lv), tmp)
        out["fasta_width_80"]["records"] = nrec
        del b, blob_t
        # ---- reads of 150
        blob_t, cols = synth.fastq_generate(a.reads, dev, rlen=150)
        torch.cuda.synchronize(dev)
        b = _lib.Blob.from_device(blob_t.data_ptr(), int(cols["n_bytes"]), device=0, keepalive=blob_t)
        assert b.fastq_build().n_reads == a.reads
        nq = min(a.reads, max((a.batch_mb << 20) // int(cols["rec"]), 1))
        ids = np.arange(nq, dtype=np.int64)
        out["fastq_reads_150"] = shape(b, lambda: b.fastq_format_alloc(ids), lambda lv: b.fastq_format_alloc(ids, level=lv), tmp)
        out["fastq_reads_150"]["reads"] = nq
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
