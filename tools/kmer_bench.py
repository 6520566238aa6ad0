"""k-mer counting on resident synthetic inputs (synth.fasta_plan / fasta_generate: the C2 shape, 3.05 GB; synth.fastq_generate:
2 x 10^7 reads of 150 bases; and a low-complexity FASTA made here: one record each of A, AC, ACG and ACGT repeated): kernel ms (fx_prof_*) of
k_kmer_fasta / k_kmer_scan / k_kmer_fix / k_kmer_fastq and end-to-end ms of the calls under Fasta.kmer_counts /
Fastq.kmer_counts, plain and canonical, medians over --reps timed runs after a warm-up with the smallest and largest.  Beside
them, in the same run, the yardsticks that read the same bytes in the same layout -- k_search_count with the one-letter
pattern A (search_counts) for FASTA, k_fq_read_stats for FASTQ -- and the HBM floor (bytes / 6.5 TB/s).  For the table in
global memory also windows per second and that rate times 64 bytes against 1.3 TB/s of atomic requests.  Every spectrum is
checked against torch on the device (rolling codes over the flat bases, windows masked at record ends) before its time is
reported.  One JSON line.

A measurement whose slowest run is more than 1.5 x its fastest is repeated and, if it stays so, flagged "disturbed".
--only-low runs the low-complexity legs alone (for an experiment build of the library chosen by FX_LIBFXGPU).

    python tools/kmer_bench.py [--gbp 3.0] [--reads 20000000] [--reps 7] [--only-low] [--out profiles/kmer.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
ATOMIC_TBS = 1.3
FASTA_KS = (1, 4, 6, 7, 11, 13)                   # 6: the largest k with the table in LDS, 7: the smallest with it in global memory
FASTQ_KS = (4, 11)
LOW_KS = (6, 11)


def torch_counts(torch, flat, rec_end, k, chunk=1 << 27):
    """plain spectrum of the flat bases by torch on the device (a checker only); rec_end: one past every record's last base"""
    dev = flat.device
    lut = torch.full((256,), 4, dtype=torch.uint8, device=dev)
    for j, c in enumerate(b"ACGT"):
        lut[c] = j
        lut[c + 32] = j
    out = torch.zeros(4 ** k, dtype=torch.int64, device=dev)
    n = flat.numel() - k + 1
    for a in range(0, max(n, 0), chunk):
        m = min(chunk, n - a)
        c = lut[flat[a:a + m + k - 1].long()]
        code = torch.zeros(m, dtype=torch.int64, device=dev)
        bad = torch.zeros(m, dtype=torch.bool, device=dev)
        for j in range(k):
            w = c[j:j + m]
            bad |= w > 3
            code = code * 4 + (w & 3)
        for d in range(1, k):                              # starts whose window runs past the end of their record
            pos = rec_end - d - a
            bad[pos[(pos >= 0) & (pos < m)]] = True
        out += torch.bincount(code[~bad], minlength=4 ** k)
        del c, code, bad
    return out


def fold_canonical(torch, counts, k):
    idx = torch.arange(4 ** k, dtype=torch.int64, device=counts.device)
    rc, t = torch.zeros_like(idx), idx.clone()
    for _ in range(k):
        rc = rc * 4 + (3 - (t & 3))
        t >>= 2
    return torch.bincount(torch.minimum(idx, rc), weights=counts.double(), minlength=4 ** k).long()     # exact below 2^53


LOW_UNITS = (b"A", b"AC", b"ACG", b"ACGT")       # one record each: periods 1..4


def low_complexity_blob(torch, dev, n_each, width=60):
    """One record per unit of LOW_UNITS, the unit repeated to n_each bases, in lines of `width` -> (blob, n_bytes, flat, rec_end)"""
    n_rec = len(LOW_UNITS)
    flat = torch.empty(n_rec * n_each, dtype=torch.uint8, device=dev)
    for i, u in enumerate(LOW_UNITS):
        for j, c in enumerate(u):
            flat[i * n_each + j:(i + 1) * n_each:len(u)] = c
    parts, pos = [], 0
    for i in range(n_rec):
        hdr = torch.tensor(list(b">low%d\n" % i), dtype=torch.uint8, device=dev)
        s = flat[i * n_each:(i + 1) * n_each]
        full = n_each // width
        body = torch.full((full, width + 1), 10, dtype=torch.uint8, device=dev)
        body[:, :width] = s[:full * width].view(full, width)
        tail = torch.cat([s[full * width:], torch.tensor([10], dtype=torch.uint8, device=dev)]) if n_each % width else s[:0]
        parts += [hdr, body.view(-1), tail]
        pos += hdr.numel() + body.numel() + tail.numel()
    blob = torch.cat(parts + [torch.zeros(131072, dtype=torch.uint8, device=dev)])
    rec_end = (torch.arange(n_rec, dtype=torch.int64, device=dev) + 1) * n_each
    return blob, pos, flat, rec_end


def finish(out, a):
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def fasta_c2(a, torch, synth, _lib, search, dev, timed, legs, out, fa_names):
    """the C2 shape"""
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    torch.cuda.synchronize(dev)
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    rec_end = torch.from_numpy(flat_start + plan["slen"]).to(dev)
    floor = nb / (HBM_TBS * 1e12) * 1e3
    _, yt, _ = timed(b, lambda: search.count_blob(b, "A", "both", False), ["k_search_count"])
    yard = yt["k_search_count"]["median_ms"]
    out["fasta_c2"] = {"n_bytes": nb, "n_records": len(plan["slen"]), "hbm_floor_ms": round(floor, 4), "yardstick_k_search_count_A": yt["k_search_count"],
                       "legs": legs(b, lambda k, c: (lambda: b.fasta_kmers(k, c)), FASTA_KS, lambda k: torch_counts(torch, flat_t, rec_end, k),
                                    yard, floor, "k_kmer_fasta", fa_names)}
    del b, blob_t, flat_t
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--low-mbp", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-low", action="store_true", help="the low-complexity legs alone (for a variant build of the library)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, search, synth
    dev = torch.device("cuda:0")

    def timed(b, run, names):
        """medians of --reps timed runs; a measurement whose slowest run of the first kernel is more than 1.5 x its fastest had
        company on the device: it is taken again, up to three times, and flagged if it stays that way"""
        for attempt in range(3):
            r, kt, e2e = timed_once(b, run, names)
            first = kt[names[0]]
            if first["max_ms"] <= 1.5 * first["min_ms"]:
                return r, kt, e2e
        kt[names[0]]["disturbed"] = True
        return r, kt, e2e

    def timed_once(b, run, names):
        torch.cuda.synchronize(dev)
        run()                                              # warm-up: allocations, code objects
        per, e2e = {k: [] for k in names}, []
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            t0 = time.perf_counter()
            r = run()
            e2e.append((time.perf_counter() - t0) * 1e3)
            pr = b.prof_read()
            b.prof_enable(0)
            for k in names:
                per[k].append(pr[k][0] if k in pr else 0.0)
        st = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        return r, {k: st(v) for k, v in per.items()}, st(e2e)

    def legs(b, run_of, ks, truth_of, yard_ms, floor_ms, main_kernel, names):
        rows = []
        for k in ks:
            plain = truth_of(k)
            torch.cuda.synchronize(dev)                    # the checker's kernels must not run beside the timed ones
            for canonical in (False, True):
                got, kt, e2e = timed(b, run_of(k, canonical), names)
                want = fold_canonical(torch, plain, k) if canonical else plain
                agree = bool(torch.equal(torch.from_numpy(np.asarray(got)).to(dev), want))
                assert agree, "k = %d canonical = %s differs from torch" % (k, canonical)
                ms = kt[main_kernel]["median_ms"]
                windows = int(plain.sum())
                row = {"k": k, "canonical": canonical, "table": "lds" if k <= 6 else "global", "windows": windows, "agree": agree,
                       "kernels": kt, "e2e": e2e, "times_yardstick": round(ms / yard_ms, 2), "fraction_of_hbm_floor": round(floor_ms / ms, 3)}
                if k > 6:
                    rate = windows / (ms * 1e-3)
                    row["windows_per_s"] = round(rate, 0)
                    row["atomic_request_bytes_per_s_over_1.3TBs"] = round(rate * 64 / (ATOMIC_TBS * 1e12), 3)
                rows.append(row)
                del got
            del plain
        return rows

    out = {"tool": "kmer_bench", "reps": a.reps, "checked_against_torch": True, "library": os.path.basename(_lib._SO)}
    fa_names = ["k_kmer_fasta", "k_kmer_scan", "k_kmer_fix"]
    if not a.only_low:
        fasta_c2(a, torch, synth, _lib, search, dev, timed, legs, out, fa_names)
    # ---- FASTA, low complexity
    blob_t, nb, flat_t, rec_end = low_complexity_blob(torch, dev, a.low_mbp * 1_000_000 // len(LOW_UNITS))
    torch.cuda.synchronize(dev)
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fasta_build().n_seq == len(LOW_UNITS)
    floor = nb / (HBM_TBS * 1e12) * 1e3
    _, yt, _ = timed(b, lambda: search.count_blob(b, "A", "both", False), ["k_search_count"])
    yard = yt["k_search_count"]["median_ms"]
    out["fasta_low_complexity"] = {"n_bytes": nb, "records": ["(%s) x n" % u.decode() for u in LOW_UNITS], "hbm_floor_ms": round(floor, 4),
                                   "yardstick_k_search_count_A": yt["k_search_count"],
                                   "legs": legs(b, lambda k, c: (lambda: b.fasta_kmers(k, c)), LOW_KS, lambda k: torch_counts(torch, flat_t, rec_end, k),
                                                yard, floor, "k_kmer_fasta", fa_names)}
    del b, blob_t, flat_t
    torch.cuda.empty_cache()
    if a.only_low:
        return finish(out, a)
    # ---- FASTQ
    n, rlen = a.reads, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    flat_t = blob_t[:n * rec].view(n, rec)[:, hl:hl + rlen].contiguous().view(-1)
    rec_end = (torch.arange(n, dtype=torch.int64, device=dev) + 1) * rlen
    _, yt, _ = timed(b, lambda: b.fastq_read_stats(phred=33, low_qual=20), ["k_fq_read_stats"])
    yard = yt["k_fq_read_stats"]["median_ms"]
    floor = (rlen + 16) * n / (HBM_TBS * 1e12) * 1e3           # the sequence line and two columns of the read table
    out["fastq"] = {"n_reads": n, "read_length": rlen, "n_bytes": nb, "hbm_floor_ms": round(floor, 4), "yardstick_k_fq_read_stats": yt["k_fq_read_stats"],
                    "legs": legs(b, lambda k, c: (lambda: b.fastq_kmers(k, c)), FASTQ_KS, lambda k: torch_counts(torch, flat_t, rec_end, k),
                                 yard, floor, "k_kmer_fastq", ["k_kmer_fastq"])}
    finish(out, a)


if __name__ == "__main__":
    main()
