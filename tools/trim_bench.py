"""FASTQ trimming and trimmed-record output on a resident synthetic FASTQ (synth.fastq_generate: reads of 150 bases): kernel ms
(fx_prof_*) of k_fq_trim for (a) the quality steps only and (b) the quality steps + a 13-letter adapter, and of the three
format kernels (k_fq_format_count / _scan / _emit) for all reads with their trimmed intervals (min_len 60) and for all reads
whole -- next to k_fq_read_stats on
the same handle in the same run (it reads exactly the bytes k_fq_trim reads) and to fx_fastq_fetch_alloc of ("seq", "qual")
for the same ids (it moves about the bytes the format pass moves), and the HBM floor at 6.5 TB/s (trim: 2 * rlen + 24 bytes
per read; format: header + 2 x kept bytes read, the record written).  Medians over --reps timed runs after a warm-up, with
the smallest and largest.  The results are checked against torch (the intervals of the quality steps on every read, with the
adapter on the first 2 M reads, the record sizes)
before the line is printed.  One JSON line.

    python tools/trim_bench.py [--reads 20000000] [--reps 7] [--out profiles/fastq_trim.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
ADAPTER = b"AGATCGGAAGAGC"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pyfastx_amd import _lib, synth
    dev = torch.device("cuda:0")
    n, rlen = a.reads, 150
    blob_t, cols = synth.fastq_generate(n, dev, rlen=rlen)
    torch.cuda.synchronize(dev)                            # the generator's writes, before the library's own stream reads the blob
    rec, hl, nb = int(cols["rec"]), int(cols["soff"][0]), int(cols["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    assert b.fastq_build().n_reads == n
    view = blob_t[:n * rec].view(n, rec)
    fq_, tq, w, wn, wd = 12, 9, 6, 31, 2                   # scores are uniform on 2..37
    qual = dict(phred=33, front_qual=fq_, window=(w, wn, wd), tail_qual=tq)
    min_len = 60

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
    (st, en), t_q = timed(lambda: b.fastq_trim(**qual), ["k_fq_trim"])
    st, en = st.copy(), en.copy()
    (st2, en2), t_qa = timed(lambda: b.fastq_trim(adapter=ADAPTER, min_overlap=3, err=(1, 10), **qual), ["k_fq_trim"])
    fmt_names = ["k_fq_format_count", "k_fq_format_scan", "k_fq_format_emit"]
    (buf, offs, kept), t_fmt = timed(lambda: b.fastq_format_alloc(None, st, en, min_len), fmt_names)
    sizes = np.diff(offs)
    del buf
    (wbuf, woffs, wkept), t_whole = timed(lambda: b.fastq_format_alloc(None, None, None, 0), fmt_names)      # every read whole: the bytes fetch moves
    assert wkept == n and int(woffs[n]) == n * (hl - 1 + 2 * rlen + 5)
    whole_bytes = int(woffs[n])
    del wbuf
    ids = np.arange(n, dtype=np.int64)
    _, t_fetch = timed(lambda: b.fastq_fetch_alloc(ids, phred=33, want=("seq", "qual")), ["k_fastq_fetch"])

    # the checks, in slices of 2 M reads (the adapter step on the first slice)
    j = torch.arange(rlen, device=dev, dtype=torch.int64)
    A = torch.tensor(list(ADAPTER), dtype=torch.uint8, device=dev)

    def by_torch(s, d, adapter):
        m = d.shape[0]
        full = torch.full((m,), rlen, device=dev)
        tb = full
        if adapter:
            pad = torch.cat([s, torch.zeros((m, len(A)), dtype=torch.uint8, device=dev)], 1).unfold(1, len(A), 1)[:, :rlen]
            ov = torch.clamp(rlen - j, max=len(A))                                  # letters compared at offset j
            mm = ((pad != A) & (torch.arange(len(A), device=dev)[None, :] < ov[:, None])[None]).sum(2)
            hit = (ov[None, :] >= 3) & (mm * 10 <= ov[None, :])
            tb = torch.where(hit.any(1), hit.to(torch.int8).argmax(1), full)
        ge = (d >= fq_) & (j[None, :] < tb[:, None])
        ta = torch.where(ge.any(1), ge.to(torch.int8).argmax(1), tb)
        cs = torch.cat([torch.zeros((m, 1), dtype=torch.int64, device=dev), d.cumsum(1)], 1)
        we = torch.clamp(tb - ta, max=w)
        ws = cs.gather(1, torch.clamp(j[None, :] + we[:, None], max=rlen)) - cs[:, :rlen]
        fail = (ws * wd < wn * we[:, None]) & (j[None, :] >= ta[:, None]) & (j[None, :] + we[:, None] <= tb[:, None]) & ((tb - ta)[:, None] > 0)
        tb = torch.where(fail.any(1), fail.to(torch.int8).argmax(1), tb)
        ok = (d >= tq) & (j[None, :] >= ta[:, None]) & (j[None, :] < tb[:, None])
        tb = torch.where(ok.any(1), rlen - ok.flip(1).to(torch.int8).argmax(1), ta)
        return ta.cpu().numpy(), tb.cpu().numpy()

    for c0 in range(0, n, 2_000_000):
        d = view[c0:c0 + 2_000_000, hl + rlen + 3:hl + 2 * rlen + 3].to(torch.int64) - 33
        m = d.shape[0]
        ta, tb = by_torch(None, d, False)
        assert np.array_equal(st[c0:c0 + m], ta) and np.array_equal(en[c0:c0 + m], tb), "intervals differ from torch"
        k = tb - ta
        assert np.array_equal(sizes[c0:c0 + m], np.where(k >= min_len, hl - 1 + 2 * k + 5, 0)), "record sizes differ from torch"
        if c0 == 0:
            ta, tb = by_torch(view[:m, hl:hl + rlen], d, True)
            assert np.array_equal(st2[:m], ta) and np.array_equal(en2[:m], tb), "intervals with the adapter differ from torch"
            assert int((tb < en[:m]).sum()) > 0

    kept_bases = int((en - st)[sizes > 0].sum())
    trim_floor = (2 * rlen + 24) * n / (HBM_TBS * 1e12) * 1e3
    fmt_floor = (int(kept) * (hl - 1) + 2 * kept_bases + int(sizes.sum())) / (HBM_TBS * 1e12) * 1e3
    read_ms, q_ms, qa_ms = t_read["k_fq_read_stats"]["median_ms"], t_q["k_fq_trim"]["median_ms"], t_qa["k_fq_trim"]["median_ms"]
    fmt_ms = sum(t_fmt[k]["median_ms"] for k in fmt_names)
    fetch_ms = t_fetch["k_fastq_fetch"]["median_ms"]
    whole_ms = sum(t_whole[k]["median_ms"] for k in fmt_names)
    whole_floor = (whole_bytes - 5 * n + whole_bytes) / (HBM_TBS * 1e12) * 1e3
    out = {"tool": "trim_bench", "n_reads": n, "read_length": rlen, "n_bytes": nb, "reps": a.reps, "checked_against_torch": True,
           "read_stats": t_read["k_fq_read_stats"], "trim_quality": t_q["k_fq_trim"], "trim_quality_adapter": t_qa["k_fq_trim"],
           "format": {"total_median_ms": round(fmt_ms, 4), "kernels": t_fmt, "kept": int(kept), "bytes": int(sizes.sum())},
           "format_whole_reads": {"total_median_ms": round(whole_ms, 4), "kernels": t_whole, "kept": int(wkept), "bytes": whole_bytes},
           "fetch_seq_qual": t_fetch["k_fastq_fetch"],
           "hbm_floor_ms": {"trim": round(trim_floor, 4), "format": round(fmt_floor, 4), "format_whole_reads": round(whole_floor, 4)},
           "fraction_of_hbm_floor": {"trim_quality": round(trim_floor / q_ms, 3), "trim_quality_adapter": round(trim_floor / qa_ms, 3),
                                     "format": round(fmt_floor / fmt_ms, 3), "format_whole_reads": round(whole_floor / whole_ms, 3)},
           "ratios": {"trim_quality_over_read_stats": round(q_ms / read_ms, 2), "trim_quality_adapter_over_trim_quality": round(qa_ms / q_ms, 2),
                      "format_over_fetch_seq_qual": round(fmt_ms / fetch_ms, 2) if fetch_ms else None,
                      "format_whole_reads_over_fetch_seq_qual": round(whole_ms / fetch_ms, 2) if fetch_ms else None},
           "adapter_step": {"ns_per_read": round((qa_ms - q_ms) * 1e6 / n, 3), "ps_per_offset": round((qa_ms - q_ms) * 1e9 / (n * rlen), 3)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
