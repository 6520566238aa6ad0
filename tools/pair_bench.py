"""Paired-end overlap and merge on two resident synthetic FASTQ streams (synth.fastq_pair_generate: pairs of 150 bases, inserts
normal(200, 60)): kernel ms (fx_prof_*) of
  overlap leg  k_fp_overlap over every pair -- next to k_fq_trim with the 13-letter adapter and to k_fq_read_stats on read 1 of
               the same pairs in the same run (each reads half the bytes k_fp_overlap reads);
  merge leg    k_fp_merge_count / _scan / _emit over every pair with the diagonals of the overlap leg -- next to
               k_fq_format_count / _scan / _emit of read 1 of the same pairs, whole.
Also: the diagonal-words per second of k_fp_overlap (a diagonal-word = one 16-letter word of one diagonal's overlap that the
kernel walks: for every lane's set of 16 diagonals whose longest overlap reaches min_overlap, 16 x the words of that overlap),
its issue-rate bound (INSTR_PER_DIAGONAL_WORD vector instructions per diagonal-word and lane, 64 lanes per wave-instruction,
1.67 ns per wave-instruction and SIMD, 1024 SIMDs: the coefficient of DESIGN.md section 0), and the share of pairs whose insert
overlap recovers against the generator's truth.  Medians over --reps timed runs after a warm-up, with the smallest and largest.
A slice of the results is checked against the plain-Python definition (tests/pair_truth.py) before the line is printed.  One
JSON line.

    python tools/pair_bench.py [--pairs 20000000] [--reps 7] [--out profiles/fastq_pair.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ADAPTER = b"AGATCGGAAGAGC"
INSTR_PER_DIAGONAL_WORD = 7        # what the compiler made: 2 v_alignbit, v_xor, v_lshrrev, v_bitop3 (or + and), v_or3, v_bcnt (it adds)
NS_PER_WAVE_INSTR, SIMDS = 1.67, 1024


def diagonal_words(rlen, min_overlap):
    """Diagonal-words k_fp_overlap walks for a pair of two reads of rlen letters."""
    lpr = (rlen + 15) // 16
    words = 0
    for ws in range(lpr):                                     # the forward set of lane ws, the backward set of lane lpr - 1 - ws
        mmax = rlen - 16 * ws
        if mmax >= min_overlap and mmax > 0:
            words += 2 * 16 * ((mmax + 15) // 16)
    return words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, pair, synth
    from pair_truth import merged_truth, overlap_truth
    dev = torch.device("cuda:0")
    n, rlen = a.pairs, 150
    t1, c1, t2, c2, ins = synth.fastq_pair_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own streams read the blobs
    nb = int(c1["n_bytes"])
    b1 = _lib.Blob.from_device(t1.data_ptr(), nb, device=0, keepalive=t1)
    b2 = _lib.Blob.from_device(t2.data_ptr(), nb, device=0, keepalive=t2)
    assert b1.fastq_build().n_reads == n and b2.fastq_build().n_reads == n
    args = pair.overlap_args()

    def timed(run, names):
        run()                                              # warm-up: allocations, code objects
        per = {k: [] for k in names}
        for _ in range(a.reps):
            b1.prof_enable(1)
            b1.prof_reset()
            r = run()
            pr = b1.prof_read()
            b1.prof_enable(0)
            for k in names:
                per[k].append(pr[k][0] if k in pr else 0.0)
        return r, {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in per.items()}

    cols, t_ov = timed(lambda: b1.fastq_pair_overlap(b2, None, **args), ["k_fp_overlap"])
    cols = {k: v.copy() for k, v in cols.items()}
    _, t_read = timed(lambda: b1.fastq_read_stats(phred=33, low_qual=20), ["k_fq_read_stats"])
    _, t_trim = timed(lambda: b1.fastq_trim(phred=33, adapter=ADAPTER, min_overlap=3, err=(1, 10)), ["k_fq_trim"])
    mg_names = ["k_fp_merge_count", "k_fp_merge_scan", "k_fp_merge_emit"]
    fmt_names = ["k_fq_format_count", "k_fq_format_scan", "k_fq_format_emit"]
    (buf, offs, merged), t_mg = timed(lambda: b1.fastq_pair_merge_alloc(b2, cols["diag"]), mg_names)
    merged_bytes = int(offs[n])
    # a slice against the definition
    got = pair.insert_of(cols["diag"], rlen, rlen)
    rec, hl = int(c1["rec"]), int(c1["soff"][0])
    m = min(n, 2000)
    h1, h2 = t1[:m * rec].cpu().numpy().reshape(m, rec), t2[:m * rec].cpu().numpy().reshape(m, rec)
    for i in range(m):
        s1, q1, s2, q2 = (h[i, o:o + rlen] for h in (h1, h2) for o in (hl, hl + rlen + 3))
        w = overlap_truth(s1, s2, **args)
        assert all(int(cols[k][i]) == w[k] for k in ("diag", "overlap", "mismatches", "end1", "end2")), "overlap differs from the definition"
        assert buf[offs[i]:offs[i + 1]].tobytes() == merged_truth(h1[i, :hl - 1].tobytes(), s1, q1, s2, q2, w["diag"]), "record differs from the definition"
    del buf
    (fbuf, foffs, fkept), t_fmt = timed(lambda: b1.fastq_format_alloc(None, None, None, 0), fmt_names)
    format_bytes = int(foffs[n])
    del fbuf

    ov_ms = t_ov["k_fp_overlap"]["median_ms"]
    dw = diagonal_words(rlen, args["min_overlap"])
    bound_ms = dw * INSTR_PER_DIAGONAL_WORD / 64 * NS_PER_WAVE_INSTR / SIMDS * n * 1e-6
    can = (ins >= args["min_overlap"]) & (ins <= 2 * rlen - args["min_overlap"])
    mg_ms, fmt_ms = sum(t_mg[k]["median_ms"] for k in mg_names), sum(t_fmt[k]["median_ms"] for k in fmt_names)
    out = {"tool": "pair_bench", "n_pairs": n, "read_length": rlen, "n_bytes_per_file": nb, "reps": a.reps, "checked_against_definition": m,
           "overlap": t_ov["k_fp_overlap"], "trim_adapter_13_read1": t_trim["k_fq_trim"], "read_stats_read1": t_read["k_fq_read_stats"],
           "overlap_ns_per_pair": round(ov_ms * 1e6 / n, 3),
           "diagonal_words_per_pair": dw, "diagonal_words_per_second": round(dw * n / (ov_ms * 1e-3), 0) if ov_ms else None,
           "issue_rate_bound_ms": round(bound_ms, 3), "fraction_of_issue_rate_bound": round(bound_ms / ov_ms, 3) if ov_ms else None,
           "merge": {"total_median_ms": round(mg_ms, 4), "kernels": t_mg, "merged": int(merged), "bytes": merged_bytes},
           "format_read1_whole": {"total_median_ms": round(fmt_ms, 4), "kernels": t_fmt, "kept": int(fkept), "bytes": format_bytes},
           "ratios": {"overlap_over_trim_adapter": round(ov_ms / t_trim["k_fq_trim"]["median_ms"], 2),
                      "overlap_over_read_stats": round(ov_ms / t_read["k_fq_read_stats"]["median_ms"], 2),
                      "merge_emit_over_format_emit": round(t_mg["k_fp_merge_emit"]["median_ms"] / t_fmt["k_fq_format_emit"]["median_ms"], 2),
                      "merge_emit_ps_per_byte": round(t_mg["k_fp_merge_emit"]["median_ms"] * 1e9 / max(merged_bytes, 1), 3),
                      "format_emit_ps_per_byte": round(t_fmt["k_fq_format_emit"]["median_ms"] * 1e9 / max(format_bytes, 1), 3)},
           "truth": {"pairs_merged": int((got >= 0).sum()), "share_merged": round(float((got >= 0).mean()), 4),
                     "share_with_true_insert": round(float((got == ins).mean()), 4),
                     "pairs_with_insert_in_reach": int(can.sum()), "share_of_those_recovered": round(float((got[can] == ins[can]).mean()), 4),
                     "wrong_insert": int(((got >= 0) & (got != ins)).sum())}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
