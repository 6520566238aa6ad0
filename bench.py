#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on MI355X: seconds to build the index + M random
sub-sequence fetches / s on a synthetic 3 Gbp hg38-shaped plain FASTA (configs[1]).

The JSON line (rank 0) carries

* the contract keys: `value` = throughput of one STEP = index build (one-read granule scan ->
  prefixes -> record table) + 1 M (id, start, stop, strand) fetches, with the stream, the query
  arrays and the results RESIDENT IN HBM (as the task statement prescribes for `value`);
* `roofline`: the dominant kernel (k_span_scan), HIP events on the library's own stream;
* `e2e`: the SAME workload end to end, like for like with the reference's own benchmark idioms
  (benchmark/pyfastx_fasta_build_index.py:1-4, benchmark/pyfastx_fasta_extract_subsequences.py:8-12):
  a FILE on disk (page cache) -> fx_open_file (pinned pieces, H2D) -> index -> host table -> `.fxi`
  on disk, and 1 M queries from host arrays to a host buffer through `Fasta.fetch_many`; every one of
  the 1 M answers is compared with the string the reference returned for the same query;
* `cpu_baseline`: the real reference (oracle/_ref, compiled from /root/reference where it exists)
  on this host, same file, 1 core; `speedup_vs_cpu` = its seconds / the e2e seconds (PCIe, page
  cache, SQLite and Python included on both sides);
* `c3` / `c4`: BASELINE configs[2] and [3] (FASTQ 100 M x 150 bp; the C2 bytes BGZF-framed) with their
  dominant-kernel rooflines and the reference beside them on a stated sample.

A plain run (one GPU) prints only the contract keys: set-up, warm-up, the timed steps and, with
`--dump-outputs DIR`, what the last step computed.  Everything else above, and the full-size parity
checks, run with `--full`.

N > 1: one process per GPU, ONE file sharded by byte range (configs[4] shape): every rank reads only its
own range (+ nothing else: bytes never move between GPUs), one all-gather of the 28-word boundary
summaries stitches the record that crosses each cut.
"""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gbp", type=float, default=3.0, help="Gbp of FASTA per GPU (3.0 = BASELINE config)")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="N > 1: weak = --gbp per GPU, the pieces of all ranks form ONE file (configs[4]: 24 Gbp at 8 GPUs), with the strong leg "
                         "reported beside it; strong = ONE --gbp file (the metric's 3 Gbp FASTA) split by byte range over the N GPUs")
    ap.add_argument("--c3-reads", type=float, default=1e8, help="reads of the FASTQ leg resident in HBM (1e8 = BASELINE configs[2])")
    ap.add_argument("--c3-sample", type=float, default=2e6, help="reads of the FASTQ file that the reference also indexes")
    ap.add_argument("--fastq-reads", type=float, default=2e7, help="reads of the ONE FASTQ file that an N > 1 run shards over its ranks (fastq_strong)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-c3", action="store_true")
    ap.add_argument("--no-c4", action="store_true")
    ap.add_argument("--gz-stream", action="store_true", help="also the single-stream gzip sub-leg of c4 (the C2 bytes as ONE gzip member: 17 s of deflate on this box's "
                                                               "16-CPU quota to make it + 3 s; its numbers of the round are in profiles/r04_single_stream_gzip.json)")
    ap.add_argument("--no-gz-stream", action="store_true", help=argparse.SUPPRESS)      # (the default now)
    ap.add_argument("--no-pmc", action="store_true", help="skip the two rocprofv3 --pmc passes that measure the scan kernel's HBM traffic (about a minute)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)      # the workload of one counter pass: generate, build three times, exit
    ap.add_argument("--no-c3-file", action="store_true", help="skip the full-size FASTQ file leg (35 GB file + 10 GB index in /dev/shm)")
    ap.add_argument("--c3-integrity", action="store_true", help="PRAGMA integrity_check of the 10 GB index file of the full-size FASTQ leg (SQLite reads all of it: about a minute)")
    ap.add_argument("--c3-reference-full", action="store_true", help="the compiled reference on the FULL configs[2] file as well (pyfastx.Fastq(path, full_index=True): ~5 minutes on one core, "
                                                                      "a second 10 GB index file), every `read` row + base / meta / stat compared (profiles/r05_c3_full_reference.json holds one such run)")
    ap.add_argument("--c4-ref-queries", type=int, default=100_000, help="queries of the C4 leg that the reference answers too (ascending offsets, through its restart points)")
    ap.add_argument("--c4-reference-full", action="store_true", help="ALL queries of the C4 leg through the reference (builder-run: profiles/r06_c4_full_reference.json; minutes of one core)")
    ap.add_argument("--pmc-file", default=None, help=argparse.SUPPRESS)                  # the counter passes' child opens this file instead of generating the stream
    ap.add_argument("--full", action="store_true", help="everything beyond the headline step (one GPU): full-size parity, per-kernel times and rooflines, "
                                                        "the end-to-end file leg, the CPU baseline, the counter passes, the C3 / C4 legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps (one GPU), write what the last step computed as DIR/<name>.npy")
    return ap.parse_args()


_T0 = time.perf_counter()
_LAPS = []


def _lap(name):
    """wall time of the bench's own legs (set-up included), for the line's `bench_wall_s`: the default run has a budget of minutes"""
    global _T0
    t = time.perf_counter()
    _LAPS.append((name, round(t - _T0, 2)))
    _T0 = t


def _median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def _reference():
    """The compiled reference (oracle/_ref), or None where it did not travel."""
    p = os.path.join(ROOT, "oracle", "_ref")
    if p not in sys.path:
        sys.path.insert(0, p)
    try:
        import pyfastx
        return pyfastx
    except Exception:
        return None


def _settle_device_memory(dev, limit_s=12.0):
    """Wait until the driver has finished taking down device memory that was freed just before: it does that in the background
    (~12 GB/s) and ANY hipMalloc that comes before it is done may wait for it -- seconds after torch released tens of GB
    (tools/first_open_probe.py; 5.7 s inside the allocations of the 0.7 GB sample's index build in about half of the
    full runs of round 5).  A timed region must not begin in that state: a 2 GiB allocation, a kernel on it and a small pinned host
    allocation are made and released until three rounds in a row come back at once.  -> seconds waited."""
    import torch
    t0 = time.perf_counter()
    quick = 0
    while quick < 3 and time.perf_counter() - t0 < limit_s:
        t = time.perf_counter()
        x = torch.empty(2 << 30, dtype=torch.uint8, device=dev)       # (large enough to be a request to the driver, not a piece of a cached chunk)
        x[:4096].zero_()                                      # (... and a kernel on it with its wait: the device itself may be busy with the take-down)
        torch.cuda.synchronize(dev)
        pin = torch.empty(4096, dtype=torch.uint8).pin_memory()      # (... and a small pinned host allocation, which every new handle makes)
        del x, pin
        torch.cuda.empty_cache()
        quick = quick + 1 if time.perf_counter() - t < 0.005 else 0
    return round(time.perf_counter() - t0, 3)


def _device_cpulist(dev):
    """local_cpulist of the device's PCI function: where libfxgpu pins the staging threads of that device (FX_STAGE_NUMA=0: nowhere)."""
    try:
        import torch
        pr = torch.cuda.get_device_properties(dev)
        bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        with open("/sys/bus/pci/devices/%s/local_cpulist" % bdf) as f:
            return {"pci": bdf, "local_cpulist": f.read().strip()}
    except Exception as e:                                    # noqa: BLE001
        return {"error": str(e)[:80]}


def _tables(path, names):
    import sqlite3
    db = sqlite3.connect(path)
    out = {t: db.execute("SELECT * FROM %s" % t).fetchall() for t in names}
    db.close()
    return out


def _rm(*paths):
    for p in paths:
        try:
            os.unlink(p)
        except OSError:
            pass


# ------------------------------------------------------------------------------------------ C2, end to end
def e2e_fasta(path, plan, q, out):
    """File on disk -> index -> 1 M answers in host memory, through the product's public surface."""
    import pyfastx_amd as fx
    from pyfastx_amd import _lib
    ids, st, sp, strand = q
    names = plan["names"]
    qnames = [names[i] for i in ids]                      # the reference idiom addresses sequences by name
    _lib.Blob.from_file(path).close()                     # first touch (pinned staging pool, HIP context): not part of a warm open
    t_open, t_ready, t_ctor, t_fetch = [], [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        b = _lib.Blob.from_file(path)                     # page cache -> pinned pieces -> HBM
        t1 = time.perf_counter()
        s = b.fasta_build()
        b.fasta_table(s.n_seq)                            # the host table exists
        t2 = time.perf_counter()
        b.close()
        t_open.append(t1 - t0); t_ready.append(t2 - t0)
    fa = None
    for _ in range(3):
        if fa is not None:
            del fa
        _rm(path + ".fxi")
        t0 = time.perf_counter()
        fa = fx.Fasta(path)                               # stage + scan + names + .fxi on disk (benchmark/pyfastx_fasta_build_index.py)
        t1 = time.perf_counter()
        t_ctor.append(t1 - t0)
    buf = offs = None
    t_first = None
    for _ in range(6):
        buf = offs = None                                 # the previous answer goes back to the library's pinned pool
        t0 = time.perf_counter()
        buf, offs = fa.fetch_many(qnames, st, sp, strand=strand)     # host arrays (1 M str names) -> host buffer
        t1 = time.perf_counter()
        if t_first is None:
            t_first = t1 - t0                             # the first call pins its buffers (fx_pinned_alloc): reported, not in the median
        else:
            t_fetch.append(t1 - t0)
    t_byid = []
    for _ in range(5):
        bi = oi = None
        t0 = time.perf_counter()
        bi, oi = fa.fetch_many(ids, st, sp, strand=strand)           # the same batch by record id
        t_byid.append(time.perf_counter() - t0)
    same_by_id = bool(np.array_equal(bi, buf) and np.array_equal(oi, offs))
    del bi, oi
    out.update(fetch_many_1M_first_call_s=round(t_first, 4), fetch_many_1M_by_id_host_to_host_s=round(_median(t_byid), 4),
               fetch_by_id_equals_by_name=same_by_id, fetch_phases_ms=_lib.fetch_phases())
    out.update(file_bytes=os.path.getsize(path), open_file_s=round(_median(t_open), 4),
               open_file_GBps=round(os.path.getsize(path) / _median(t_open) / 1e9, 1),
               index_ready_s=round(_median(t_ready), 4), fxi_durable_s=round(_median(t_ctor), 4),
               fetch_many_1M_host_to_host_s=round(_median(t_fetch), 4), n_queries=int(len(ids)),
               note="medians of 3 (fetches: of 5 after a first call that pins the pooled buffers); file in the page cache; open = pread into pinned 8 MiB pieces + hipMemcpyAsync (bound by the copy out of the page cache: a plain pinned copy runs at 57 GB/s here); "
                    "fxi_durable = pyfastx_amd.Fasta(path) with no .fxi present; fetch = Fasta.fetch_many(names, starts, stops, strand)")
    ours_rows = _tables(path + ".fxi", ("seq", "stat"))
    del fa
    _rm(path + ".fxi")
    return buf, offs, ours_rows


def cpu_fasta(path, plan, q, out, gpu_buf, gpu_offs, ours_rows):
    """The reference on the same file, same host, one core: constructor (index build + .fxi) and the
    fa[name][s:e].seq / .antisense loop; its 1 M strings are kept and compared with the GPU's answers."""
    ref = _reference()
    if ref is None:
        return False
    ids, st, sp, strand = q
    names = plan["names"]
    # three repeats, the median -- of the constructor (the index file removed in between) and of the query loop
    t_index, t_loop = [], []
    fa = None
    for _ in range(3):
        del fa
        _rm(path + ".fxi")
        t0 = time.perf_counter()
        fa = ref.Fasta(path)                              # benchmark/pyfastx_fasta_build_index.py idiom
        t_index.append(time.perf_counter() - t0)
    ii, ss, ee, neg = ids.tolist(), st.tolist(), sp.tolist(), strand.tolist()
    got = None
    for _ in range(3):
        got = []
        app = got.append
        t2 = time.perf_counter()
        for j in range(len(ii)):                          # benchmark/pyfastx_fasta_extract_subsequences.py idiom
            s = fa[names[ii[j]]][ss[j]:ee[j]]
            app(s.antisense if neg[j] else s.seq)
        t_loop.append(time.perf_counter() - t2)
    t0, t1, t2, t3 = 0.0, _median(t_index), 0.0, _median(t_loop)
    theirs = _tables(path + ".fxi", ("seq", "stat"))
    rows_equal = theirs["seq"] == ours_rows["seq"] and theirs["stat"][0][:2] == ours_rows["stat"][0][:2]
    bytes_equal = None
    if gpu_buf is not None:
        theirs_b = "".join(got).encode("latin-1")
        bytes_equal = (len(theirs_b) == int(gpu_offs[-1])) and theirs_b == gpu_buf[:int(gpu_offs[-1])].tobytes()
    out.update(kind="reference", cores=1, index_s=round(t1 - t0, 3), fetch_s=round(t3 - t2, 3), repeats=3,
               index_runs_s=[round(x, 3) for x in t_index], fetch_runs_s=[round(x, 3) for x in t_loop],
               rows_equal_gpu=bool(rows_equal), fetch_bytes_equal_gpu=bytes_equal,
               sample="full workload, medians of 3 (BASELINE.md 3.3): pyfastx.Fasta() on the %.2f GB file (no .fxi present) + %d fa[name][s:e].seq/.antisense, "
                      "every returned string compared with the GPU batch" % (os.path.getsize(path) / 1e9, len(ii)))
    del fa
    _rm(path + ".fxi")
    return True


def cpu_fasta_port(host, q, out):
    """oracle/_ref did not travel: the C restatement (oracle/fx_oracle.c) on the same bytes."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import fxoracle
    ids, st, sp, strand = q
    t0 = time.perf_counter()
    recs, tot = fxoracle.fasta_index(host)
    t1 = time.perf_counter()
    nq = min(len(ids), 200_000)
    r = recs[ids[:nq]]
    bpl = r["llen"] - r["elen"]
    off = r["boff"] + st[:nq] + r["elen"] * (st[:nq] // bpl)
    bl = (sp[:nq] - st[:nq]) + (sp[:nq] // bpl - st[:nq] // bpl) * r["elen"]
    fxoracle.fetch_batch(host, off, bl, sp[:nq] - st[:nq], np.where(strand[:nq] > 0, 6, 0))
    t2 = time.perf_counter()
    out.update(kind="port", cores=1, index_s=round(t1 - t0, 3), fetch_s=round((t2 - t1) * len(ids) / nq, 3),
               sample="C port of the scan on the full %.2f GB + %d fetches (scaled to %d); the compiled reference did not travel"
                      % (len(host) / 1e9, nq, len(ids)))


# ------------------------------------------------------------------------------------------ C3: FASTQ
def leg_c3(a, dev, tmpdir):
    """configs[2]: FASTQ index build + composition + 1 M read fetches with phred conversion.
    (i) the full configuration resident in HBM (kernel times, rooflines, every row against the generator's truth);
    (ii) a file of the first `c3_sample` reads end to end -- product and reference side by side, tables compared."""
    import torch
    import pyfastx_amd as fx
    from pyfastx_amd import _lib, synth
    out = {}
    n = int(a.c3_reads)
    blob_t, cols = synth.fastq_generate(n, dev)
    nb = int(cols["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=dev.index, keepalive=blob_t)
    b.fastq_build(); b.fastq_comp()                       # warm-up (allocations)
    b.prof_enable(1); b.prof_reset()
    R = 3
    t0 = time.perf_counter()
    for _ in range(R):
        s = b.fastq_build()
    t1 = time.perf_counter()
    for _ in range(R):
        base, meta = b.fastq_comp()
    t2 = time.perf_counter()
    prof_two = {k: v[0] / v[1] for k, v in b.prof_read().items()}
    b.prof_reset()
    # Fastq(path, full_index=True) since round 4: index AND composition in one read of the stream (fx_fastq_build_comp)
    b.fastq_build(comp=True); b.fastq_comp()
    t3a = time.perf_counter()
    for _ in range(R):
        b.fastq_build(comp=True)
        base1, meta1 = b.fastq_comp()
    t3b = time.perf_counter()
    one_read_ms = (t3b - t3a) / R * 1e3
    same_one_read = bool((base1 == base).all() and (meta1 == meta).all())
    prof_one = {k: v[0] / v[1] for k, v in b.prof_read().items()}     # (the slots k_fastq_lines / k_fastq_comp hold the fused kernels here)
    b.prof_reset()
    s = b.fastq_build()
    ok = (s.n_reads, s.size) == (n, n * 150) and same_one_read
    t = b.fastq_table(n)
    for k in ("name_off", "name_len", "dlen", "rlen", "soff", "qoff"):
        ok = ok and bool((t[k] == cols[k]).all())
    rec = cols["rec"]
    v = blob_t[:nb].view(n, rec)
    so, qo = int(cols["soff"][0]), int(cols["qoff"][0])
    seqs, quals = v[:, so:so + 150], v[:, qo:qo + 150]
    want = [int((seqs == c).sum()) for c in b"ACGT"]
    want.append(n * 150 - sum(want))
    ok = ok and base.tolist() == want and meta.tolist() == [150, 150, int(quals.min()), int(quals.max()), 33]
    nq = a.queries
    rng = np.random.default_rng(99)
    ids = torch.from_numpy(rng.integers(0, n, nq)).to(dev)
    off = torch.arange(nq, device=dev, dtype=torch.int64) * 150
    o_seq = torch.zeros(nq * 150, dtype=torch.uint8, device=dev); o_q = torch.zeros_like(o_seq)
    o_qi = torch.zeros(nq * 150, dtype=torch.int8, device=dev)
    L = _lib.lib()

    def fetch():
        _lib.check(L.fx_fastq_fetch(b._h, _lib.FX_DEVICE, nq, ids.data_ptr(), 33, 0, o_seq.data_ptr(), o_q.data_ptr(),
                                    o_qi.data_ptr(), off.data_ptr()))
        b.sync()
    fetch()
    t3 = time.perf_counter()
    for _ in range(R):
        fetch()
    t4 = time.perf_counter()
    ok = ok and bool((o_seq.view(nq, 150) == seqs[ids]).all()) and bool((o_q.view(nq, 150) == quals[ids]).all())
    ok = ok and bool((o_qi.view(nq, 150) == (quals[ids].to(torch.int16) - 33).to(torch.int8)).all())
    prof = {k: v[0] / v[1] for k, v in b.prof_read().items()}
    prof.update({k: v for k, v in prof_two.items() if k in ("k_fastq_lines", "k_fastq_comp")})   # the two-read timings of these slots
    b.prof_enable(0)
    n_lines = 4 * n
    build_alg = nb + 4 * n_lines + 44 * n                 # stream once + one 4-byte line record per line + the 44-byte row
    comp_alg = 2 * 150 * n + 12 * n                       # sequence and quality line of every read + its table entries
    fetch_alg = 782 * nq                                  # 150+150 read, 3 x 150 written, descriptor + offset
    kl = prof.get("k_fastq_lines", 0.0)
    out["full"] = {
        "workload": "configs[2]: synthetic FASTQ %d x 150 bp (%.2f GB) resident in HBM, index build + composition + %d random reads "
                    "(seq + qual + int8 quali)" % (n, nb / 1e9, nq),
        "index_build_ms": round((t1 - t0) / R * 1e3, 3), "composition_ms": round((t2 - t1) / R * 1e3, 3),
        "full_index_one_read_ms": round(one_read_ms, 3), "full_index_two_reads_ms": round((t2 - t0) / R * 1e3, 3),
        "kernels_one_read_ms_avg": {"k_fastq_lines_comp": round(prof_one.get("k_fastq_lines", 0.0), 4),
                                    "k_fastq_comp_reduce": round(prof_one.get("k_fastq_comp", 0.0), 4)},
        "fetch_1M_ms": round((t4 - t3) / R * 1e3, 3), "M_reads_per_s": round(nq / ((t4 - t3) / R) / 1e6, 1),
        "kernels_ms_avg": {k: round(v, 4) for k, v in prof.items()},
        "rows_base_meta_fetch_equal_generator": bool(ok),
        "roofline": {"kernel": "fx::k_fastq_lines", "bound": "hbm", "achieved": round(nb / (kl * 1e-3) / 1e9, 1) if kl else None,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(nb / (kl * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kl else None,
                     "algorithmic_bytes_per_launch": nb, "avg_launch_ms": round(kl, 4), "traffic": None},
        # the scan kernels of the FASTQ build are bound by the vector instructions they issue, not by HBM (VERDICT r4 missing #6): the
        # floor is instructions per 4 KiB granule and wave (SQ_INSTS_VALU / granules, PMC pass of the round) x 4 cycles of a SIMD each
        # / (1024 SIMDs x 2.4 GHz); frac = floor / measured time
        "roofline_issue": {name: _issue_roofline(name, nb, ms) for name, ms in (("k_fastq_lines", kl), ("k_fastq_lines_comp", prof_one.get("k_fastq_lines", 0.0))) if ms},
        "roofline_build": {"algorithmic_bytes": build_alg, "frac": round(build_alg / ((t1 - t0) / R) / 1e9 / HBM_PEAK_GBS, 4)},
        "roofline_comp": {"kernel": "fx::k_fastq_comp", "algorithmic_bytes": comp_alg,
                          "frac": round(comp_alg / (prof.get("k_fastq_comp", 1e9) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
        # traffic: from the builder's counter passes (profiles/r06_pmc_fetch.txt: 1 M random reads of 150 bases -> FETCH_SIZE 409 700 KB x 2 read,
        # WRITE_SIZE 440 040 KB written per launch), scaled to this launch's reads; the factor 2 is the calibration of profiles/r06_gathercal.txt
        "roofline_fetch": {"kernel": "fx::k_fastq_fetch", "algorithmic_bytes": fetch_alg,
                           "frac": round(fetch_alg / (prof.get("k_fastq_fetch", 1e9) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "traffic": int(nq * (409700 * 1024 * 2 + 440040 * 1024) / 1e6),
                           "traffic_source": "profiles/r06_pmc_fetch.txt (builder-run rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over tools/fetch_probe.py, 1 M reads per launch), per read x this launch's reads",
                           "calibration": "profiles/r06_gathercal.txt (FETCH_SIZE x 2 for gathers as for streams)",
                           "lines_of_128_bytes_fetched_per_read": round(409700 * 1024 * 2 / 1e6 / 128.0, 2),
                           "frac_of_measured_traffic": round(nq * (409700 * 1024 * 2 + 440040 * 1024) / 1e6 / (prof.get("k_fastq_fetch", 1e9) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
    }
    if not ok:
        raise SystemExit("PARITY FAILURE (C3 at full size)")
    # ---- (ii) the file leg: the first m reads as a file, product and reference end to end
    m = int(min(a.c3_sample, n))
    path = os.path.join(tmpdir, "c3.fq")
    blob_t[:m * rec].cpu().numpy().tofile(path)
    # ---- (iii) the WHOLE configuration as a file (space permitting): written here, while the bytes are at hand
    full_dir = full_path = None
    if not a.no_c3_file and n > m:
        try:
            need = nb + n * 110 + (8 << 30)                   # the file, its index file (~100 B per read), slack
            if shutil.disk_usage("/dev/shm").free > need * 1.15:
                full_dir = tempfile.mkdtemp(prefix="fxc3", dir="/dev/shm")
                full_path = os.path.join(full_dir, "c3_full.fq")
                with open(full_path, "wb") as f:
                    for x in range(0, nb, 1 << 30):
                        f.write(memoryview(blob_t[x:min(x + (1 << 30), nb)].cpu().numpy()))
        except OSError:
            full_path = None
    b.close()
    del b, blob_t, v, seqs, quals, o_seq, o_q, o_qi
    # torch's 35 GB go back to the driver HERE, as early as possible: the driver takes freed device memory down in the background
    # (35 GB: ~2.8 s) and a hipMalloc that comes before it is done may wait for it (tools/first_open_probe.py; that wait in front of
    # the 0.7 GB file below was the 5.9 s "constructor" of one round-4 run).  The reference's leg below (5 s) gives it the time;
    # keeping the memory in torch's pool instead made the full-size constructors further down erratic (2.2-3.6 s against 1.4).
    torch.cuda.empty_cache()
    out["device_memory_settled_after_s"] = _settle_device_memory(dev)      # (not part of any timed region)
    nqs = min(nq, 200_000)
    sid = np.random.default_rng(7).integers(0, m, nqs)
    _lib.Blob.from_file(path).close()
    t0 = time.perf_counter()
    fq = fx.Fastq(path, full_index=True)                  # stage + scan + names + sort + .fxi pages + composition
    t1 = time.perf_counter()
    got = fq.fetch_many(sid, want=("seq", "qual", "quali"))
    t2 = time.perf_counter()
    ours = _tables(path + ".fxi", ("read", "stat", "base", "meta"))
    ctor_ph = {k: (round(v, 4) if isinstance(v, float) else v) for d in (getattr(fq, "ctor_phases", None), getattr(fq, "build_phases", None)) if d
               for k, v in d.items() if isinstance(v, (float, dict))}
    del fq
    _rm(path + ".fxi")
    smp = {"reads": m, "file_bytes": os.path.getsize(path), "Fastq_ctor_full_index_s": round(t1 - t0, 3),
           "fetch_many_%d_s" % nqs: round(t2 - t1, 4),
           # (one run of round 4 showed 5.9 s here against 0.17 s in all others: the parts are in the line since round 5)
           "ctor_phases_s": ctor_ph}
    ref = None if a.no_cpu_baseline else _reference()
    if ref is not None:
        t0 = time.perf_counter()
        rq = ref.Fastq(path, full_index=True)
        t1 = time.perf_counter()
        rs, rqq, rqi = [], [], []
        t2 = time.perf_counter()
        for i in sid.tolist():                            # fq[i].seq / .qual / .quali: the reference's per-read getters
            r = rq[i]
            rs.append(r.seq); rqq.append(r.qual); rqi.append(r.quali)
        t3 = time.perf_counter()
        theirs = _tables(path + ".fxi", ("read", "stat", "base", "meta"))
        o = got["offsets"]
        eq = "".join(rs).encode() == got["seq"][:int(o[-1])].tobytes() and "".join(rqq).encode() == got["qual"][:int(o[-1])].tobytes()
        eq = eq and bool((np.concatenate([np.asarray(x, dtype=np.int8) for x in rqi]) == got["quali"][:int(o[-1])]).all())
        smp["cpu_baseline"] = {"kind": "reference", "cores": 1, "index_s": round(t1 - t0, 3), "fetch_s": round(t3 - t2, 3),
                               "sample": "pyfastx.Fastq(path, full_index=True) on the first %d reads (%.2f GB) + %d x fq[i].seq/.qual/.quali"
                                         % (m, os.path.getsize(path) / 1e9, nqs)}
        smp["rows_equal_reference"] = bool(all(theirs[k] == ours[k] for k in ("read", "base", "meta")) and theirs["stat"] == ours["stat"])
        smp["fetch_bytes_equal_reference"] = bool(eq)
        smp["speedup_vs_cpu"] = round((t1 - t0 + t3 - t2) / max(float(smp["Fastq_ctor_full_index_s"]) + float(smp["fetch_many_%d_s" % nqs]), 1e-9), 1)
        del rq
        if not (smp["rows_equal_reference"] and eq):
            raise SystemExit("PARITY FAILURE (C3 file leg vs the reference)")
    # Fastx (fastx.c + kseq.c:138-179): index-free iteration over the same file -- stage, line table, parallel prefix passes /
    # walk, gather, tuples built by the C iterator -- beside the reference's kseq loop; every tuple compared
    _rm(path + ".fxi")
    t0 = time.perf_counter()
    mine = list(fx.Fastx(path))
    t1 = time.perf_counter()
    smp["fastx"] = {"tuples": len(mine), "iterate_s": round(t1 - t0, 3)}
    if ref is not None:
        t2 = time.perf_counter()
        theirs_x = list(ref.Fastx(path))
        t3 = time.perf_counter()
        smp["fastx"].update(reference_iterate_s=round(t3 - t2, 3), tuples_equal_reference=bool(mine == theirs_x),
                            note="list(Fastx(path)): both sides create one (name, seq, qual) tuple of str per read, which is most of either time")
        if mine != theirs_x:
            raise SystemExit("PARITY FAILURE (Fastx vs the reference)")
        del theirs_x
    del mine
    _rm(path, path + ".fxi")
    out["file_sample"] = smp
    if full_path is not None:
        try:
            out["e2e_full"] = c3_full_file(a, full_path, n, cols, theirs_rows=(theirs["read"] if ref is not None else None), m=m)
        finally:
            shutil.rmtree(full_dir, ignore_errors=True)
    else:
        out["e2e_full"] = None if a.no_c3_file or n <= m else "skipped: /dev/shm has no room for the %.0f GB file and its index" % (nb / 1e9)
    return out


def c3_full_file(a, path, n, cols, theirs_rows, m):
    """configs[2] at FULL size from a FILE, the job of pyfastx_fastq_create_index (fastq.c:8-182) end to end: the 35 GB file
    (page cache) -> Fastq(path): staging, scan, rows, names, GPU sort, the 10 GB .fxi durable on disk -> 1 M reads (seq +
    qual + int8 quali) into host memory.  Checked: SQLite's own integrity check of the index file (page structure, every
    index entry against its row, order, uniqueness), the rows of the first `m` reads against the rows the REFERENCE wrote
    for that prefix (offsets are from the start of the file: the same rows), rows and fetched bytes of a sample all over
    the file against the file's own bytes."""
    import sqlite3
    import pyfastx_amd as fx
    from pyfastx_amd import _lib
    nb = os.path.getsize(path)
    _lib.Blob.from_file_range(path, 0, 1 << 24, 0).close()
    # Three constructors, the MEDIAN reported (as every end-to-end figure of this file), all three listed: an allocation of tens of GB
    # can wait seconds for the driver's background clean-up of memory freed just before -- by this process or the one before it --
    # and the first copies into fresh device memory run at a third of the rate (tools/first_open_probe.py); the
    # library's pool keeps the blob of the last large stream so that later opens ask the driver for nothing.
    import gc
    runs, fq = [], None
    for rep in range(3):
        if fq is not None:
            st_ = getattr(fq, "_st", None)
            if st_ is not None and getattr(st_, "_blob", None) is not None:
                st_._blob.close()                             # (explicitly: the blob goes back to the library's pool now, not when the collector gets to it)
            fq = None
            gc.collect()
            _rm(path + ".fxi")
        t0 = time.perf_counter()
        fq = fx.Fastq(path)                                  # stage + scan + rows + names sorted + b-tree pages formatted on the device + pages to the file
        t1 = time.perf_counter()
        runs.append((t1 - t0, dict(getattr(fq, "build_phases", None) or {}), dict(getattr(fq, "index_phases", None) or {})))
    order = sorted(range(3), key=lambda i: runs[i][0])
    t_ctor, bp, ip = runs[order[1]]                          # the median run: its phases are the ones reported
    t0, t1 = 0.0, t_ctor
    first = {"Fastq_ctor_s": round(runs[0][0], 3), **{k: round(v, 3) for k, v in runs[0][1].items() if isinstance(v, float)}}
    all_runs = [{"Fastq_ctor_s": round(r[0], 3), "device_alloc_s": round(r[1].get("device_alloc_s", 0.0), 3), "page_cache_to_hbm_s": round(r[1].get("page_cache_to_hbm_s", 0.0), 3),
                 "fxi_s": round(r[1].get("fxi_s", 0.0), 3)} for r in runs]
    nq = a.queries
    ids = np.random.default_rng(99).integers(0, n, nq)
    fq.fetch_many(ids[:1000], want=("seq", "qual", "quali"))
    t2 = time.perf_counter()
    got = fq.fetch_many(ids, want=("seq", "qual", "quali"))
    t3 = time.perf_counter()
    rec = int(cols["rec"])
    so, qo = int(cols["soff"][0]), int(cols["qoff"][0])
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    pick = np.arange(0, nq, max(nq // 20000, 1))
    o = got["offsets"]
    ok = bool((np.diff(o) == 150).all())
    base = ids[pick].astype(np.int64) * rec
    idx = base[:, None] + np.arange(150)[None, :]
    want_s, want_q = mm[idx + so], mm[idx + qo]
    gs = got["seq"][:int(o[-1])].reshape(nq, 150)[pick]
    gq = got["qual"][:int(o[-1])].reshape(nq, 150)[pick]
    gi = got["quali"][:int(o[-1])].reshape(nq, 150)[pick]
    ok = ok and bool((gs == want_s).all()) and bool((gq == want_q).all()) and bool((gi == (want_q.astype(np.int16) - 33).astype(np.int8)).all())
    del mm, fq
    t4 = time.perf_counter()
    db = sqlite3.connect(path + ".fxi")
    # SQLite's own check reads all 10 GB (66 s in the round-3 driver run): behind --c3-integrity; the default run probes 2 000 rows
    # by ID and 2 000 by name through the b-trees instead (tests/test_gpu_api.py::test_bulk_written_index_is_sound runs the
    # integrity check on files of every shape)
    integrity = db.execute("PRAGMA integrity_check").fetchone()[0] if a.c3_integrity else "skipped (--c3-integrity)"
    t5 = time.perf_counter()
    cnt = db.execute("SELECT counts, size FROM stat").fetchone()
    samp = np.unique(np.concatenate([np.arange(1, 6), np.random.default_rng(5).integers(1, n + 1, 2000), [n]]))
    rows_ok = cnt == (n, n * 150)
    for i in samp.tolist():
        r = db.execute("SELECT dlen, rlen, soff, qoff FROM read WHERE ID=?", (i,)).fetchone()
        rows_ok = rows_ok and r == (int(cols["dlen"][i - 1]), 150, int(cols["soff"][i - 1]), int(cols["qoff"][i - 1]))
    prefix_equal = None
    if theirs_rows is not None:
        mine = db.execute("SELECT * FROM read WHERE ID<=? ORDER BY ID", (m,)).fetchall()
        prefix_equal = mine == theirs_rows
    by_name = db.execute("SELECT ID FROM read WHERE name=(SELECT name FROM read WHERE ID=?)", (n // 2,)).fetchone()[0] == n // 2
    for i in samp.tolist():                                   # ... and every sampled row through the name index
        by_name = by_name and db.execute("SELECT ID FROM read WHERE name=(SELECT name FROM read WHERE ID=?)", (i,)).fetchone()[0] == i
    db.close()
    full_ref = None
    if a.c3_reference_full and _reference() is not None:
        # the reference on the whole file (fastq.c:8-182 + 663-795), its index file beside ours, every row compared by one join on the rowid
        ref = _reference()
        ours_path = path + ".ours.fxi"
        os.rename(path + ".fxi", ours_path)
        base_meta = None
        try:
            import pyfastx_amd as fx2
            t6 = time.perf_counter()
            fq2 = fx2.Fastq(path, index_file=ours_path, full_index=True)      # our base / meta for the whole file (the index is there: composition only)
            t7 = time.perf_counter()
            del fq2
            rq = ref.Fastq(path, full_index=True)
            t8 = time.perf_counter()
            del rq
            db = sqlite3.connect(path + ".fxi")
            db.execute("ATTACH DATABASE ? AS ours", (ours_path,))
            same = db.execute("SELECT count(*) FROM main.read r JOIN ours.read q ON q.ID = r.ID WHERE r.name = q.name AND r.dlen = q.dlen "
                              "AND r.rlen = q.rlen AND r.soff = q.soff AND r.qoff = q.qoff").fetchone()[0]
            counts = (db.execute("SELECT count(*) FROM main.read").fetchone()[0], db.execute("SELECT count(*) FROM ours.read").fetchone()[0])
            base_meta = all(db.execute("SELECT * FROM main.%s" % t).fetchall() == db.execute("SELECT * FROM ours.%s" % t).fetchall() for t in ("base", "meta", "stat"))
            t9 = time.perf_counter()
            db.close()
            full_ref = {"reference_Fastq_full_index_s": round(t8 - t7, 1), "ours_composition_on_the_indexed_file_s": round(t7 - t6, 3),
                        "rows_compared": int(counts[0]), "rows_equal": int(same), "row_counts": list(counts), "base_meta_stat_equal": bool(base_meta),
                        "compare_s": round(t9 - t8, 1), "cores": 1}
        finally:
            _rm(path + ".fxi")
            os.rename(ours_path, path + ".fxi")
        if full_ref["rows_equal"] != n or counts != (n, n) or not base_meta:
            raise SystemExit("PARITY FAILURE (C3 at full size against the reference on the whole file): %r" % (full_ref,))
    res = {"workload": "configs[2] from a FILE: %d x 150 bp FASTQ (%.1f GB, page cache) -> pyfastx_amd.Fastq(path) with no .fxi present -> the index "
                       "file durable on disk (%.1f GB) -> %d random reads (seq + qual + int8 quali) into host memory" % (n, nb / 1e9, os.path.getsize(path + ".fxi") / 1e9, nq),
           "Fastq_ctor_s": round(t1 - t0, 3), "Fastq_ctor_s_is": "the median of three constructors (constructor_runs lists them; phases_s are the median run's)",
           "M_rows_per_s": round(n / (t1 - t0) / 1e6, 2),
           # both times -- the read table resident in HBM (batches can be served), the .fxi durable on disk
           "index_ready_s": round(bp["index_ready_s"], 3) if bp else None, "fxi_durable_s": round(bp["fxi_durable_s"], 3) if bp else None,
           "first_constructor_of_the_process": first, "constructor_runs": all_runs,
           "phases_s": {"staging": round(bp.get("staging_s", 0.0), 3), "device_alloc": round(bp.get("device_alloc_s", 0.0), 4),
                        "page_cache_to_hbm": round(bp.get("page_cache_to_hbm_s", 0.0), 3), "index_kernels": round(bp.get("scan_s", 0.0), 4),
                        "name_sort_and_index_shape_not_hidden_by_the_table_copy_out": round(ip.get("sort_and_index_shape_not_hidden", 0.0), 3) if ip else None,
                        "sqlite_schema_and_reopen": round(ip.get("sqlite_schema", 0.0) + ip.get("sqlite_reopen", 0.0), 3) if ip else None,
                        "unaccounted_in_the_write_call": round(ip.get("write_call", 0.0) - sum(ip.get(k, 0.0) for k in _lib.Blob.FXI_LAPS if k != "index_shape") - ip.get("sort_and_index_shape_not_hidden", 0.0), 3) if ip else None,
                        "page_shapes": round(ip.get("table_shape", 0.0), 4) if ip else None,
                        "page_kernels": round(ip.get("table_kernels", 0.0) + ip.get("index_kernels", 0.0), 4) if ip else None,
                        "file_grown": round(ip.get("file_grown", 0.0), 3) if ip else None,
                        "pages_d2h_and_into_the_file": round(ip.get("table_to_file", 0.0) + ip.get("index_to_file", 0.0), 3) if ip else None,
                        "host_levels_and_header": round(ip.get("host_levels_and_header", 0.0), 3) if ip else None,
                        "fxi_total": round(bp.get("fxi_s", 0.0), 3), "room_set_aside_while_staging": bp.get("room_set_aside_early"),
                        "pages_formatted_on": "device" if ip else "host"} if bp else None,
           "fetch_many_1M_s": round(t3 - t2, 4),
           "sqlite_integrity_check": integrity, "integrity_check_s": round(t5 - t4, 1), "rows_sample_equal_generator": bool(rows_ok),
           "rows_of_the_first_%d_reads_equal_reference" % m: prefix_equal, "name_probe_ok": bool(by_name), "fetch_sample_equal_file_bytes": bool(ok),
           # (the reference takes ~3 minutes of one core for the whole file: not part of the default run)
           "reference_on_the_whole_file": full_ref if full_ref is not None else "builder-run, see profiles/r06_c3_full_reference.json (all 10^8 read rows + base / meta / stat equal, 179 s of the reference; `--c3-reference-full` repeats it)"}
    if (a.c3_integrity and integrity != "ok") or not rows_ok or not ok or prefix_equal is False or not by_name:
        raise SystemExit("PARITY FAILURE (C3 at full size from a file): %r" % (res,))
    return res


# ------------------------------------------------------------------------------------------ C4: BGZF
def _bgzf_part(chunk):
    from pyfastx_amd import synth
    return synth.bgzf_compress(chunk)[:-28]               # drop the per-chunk EOF member


def leg_c4(a, host, plan, q, tmpdir, plain_digest=None):
    """configs[3]: the C2 bytes BGZF-framed; open (member walk, H2D of the compressed bytes, GPU inflate) + index build +
    gzindex restart points + 1 M fetches, the reference on the same .gz beside it."""
    import pyfastx_amd as fx
    from multiprocessing import get_context
    from pyfastx_amd import _lib, synth
    ids, st, sp, strand = q
    names = plan["names"]
    nb = len(host)
    step = 65280 * 64
    t0 = time.perf_counter()
    path = os.path.join(tmpdir, "c4.fa.gz")
    with open(path, "wb") as f:
        f.write(synth.bgzf_compress_parallel(host, step=step))      # all host cores, the bytes shared by fork (setup, untimed)
    t1 = time.perf_counter()
    csize = os.path.getsize(path)
    L = _lib.lib()
    L.fx_prof_default(1)
    if os.environ.get("FX_BENCH_TRACE"):                  # (FX_BENCH_TRACE=1: the laps of every BGZF open of this leg on stderr; off in the default run)
        os.environ.setdefault("FX_TRACE_BGZF", "1")
    _lib.Blob.from_file(path).close()                     # first touch
    t_open = []
    prof = {}
    for _ in range(3):
        t2 = time.perf_counter()
        b = _lib.Blob.from_file(path)
        t3 = time.perf_counter()
        t_open.append(t3 - t2)
        pr = b.prof_read()
        prof = {k: v[0] for k, v in pr.items()}            # per OPEN: a large file is inflated in groups behind its staging, a launch per group
        launches = {k: int(v[1]) for k, v in pr.items()}
        ok_size = b.size == nb
        b.close()
    # the same file taken all at once (staged whole, then one launch of every kernel): the kernels' own time without a copy beside them
    os.environ["FX_BGZF_GROUP"] = "0"
    t_one = []
    prof_one = {}
    for _ in range(2):
        t2 = time.perf_counter()
        b = _lib.Blob.from_file(path)
        t3 = time.perf_counter()
        t_one.append(t3 - t2)
        prof_one = {k: v[0] / v[1] for k, v in b.prof_read().items()}
        b.close()
    del os.environ["FX_BGZF_GROUP"]
    L.fx_prof_default(0)
    qnames = [names[i] for i in ids]
    t_ctor, t_fetch = [], []
    fa = None
    for _ in range(2):
        if fa is not None:
            del fa
        _rm(path + ".fxi")
        t2 = time.perf_counter()
        fa = fx.Fasta(path)
        t3 = time.perf_counter()
        t_ctor.append(t3 - t2)
    for _ in range(2):
        t2 = time.perf_counter()
        buf, offs = fa.fetch_many(qnames, st, sp, strand=strand)
        t3 = time.perf_counter()
        t_fetch.append(t3 - t2)
    ours = _tables(path + ".fxi", ("seq", "stat"))
    npoints = len(_tables(path + ".fxi", ("gzindex",))["gzindex"])
    del fa
    _rm(path + ".fxi")
    infl = sum(v for k, v in prof_one.items() if k.startswith("k_bgzf"))
    alg = csize + nb
    out = {"workload": "configs[3]: the %.2f GB C2 FASTA BGZF-framed (%d members, %.2f GB compressed), zran restart points + index "
                       "build + %d random 100 bp intervals" % (nb / 1e9, (nb + 65279) // 65280, csize / 1e9, len(ids)),
           "host_compress_s_setup_only": round(t1 - t0, 1), "open_file_s": round(_median(t_open), 4),
           "inflated_size_ok": bool(ok_size), "kernels_ms_avg": {k: round(v, 3) for k, v in prof_one.items()},
           "open_file_all_at_once_s": round(min(t_one), 4),
           "kernels_ms_per_open_in_groups": {k: round(v, 3) for k, v in prof.items()}, "launches_per_open_in_groups": launches,
           "fxi_durable_s": round(_median(t_ctor), 4), "fetch_many_1M_host_to_host_s": round(_median(t_fetch), 4),
           "gzindex_rows": npoints,
           # what bounds the inflate (counters of profiles/r06_pmc_bgzf_c4.txt, whole file in one launch): the decode is one
           # wave per member, 16 waves per CU; of a wave's cycles 71 % are spent parked at s_waitcnt for vector memory, 23 % issuing,
           # 6 % in issue stalls.  What it waits for: the per-CU vL1D has requests outstanding at the L2 70 % of the kernel's time
           # (TCP_PENDING_STALL_CYCLES) -- 170 M reads (16-byte chunks of the compressed bytes, one per ~8 symbols and lane) at 474 cycles
           # each and 471 M 8-byte stores at 64 places of a member per instruction at 253; 41 % of the L2's requests miss (4096 members x
           # 84 KiB are open at a time, the L2s hold 32 MiB: lines are evicted between their sixteen 8-byte stores and come back:
           # 15 GB fetched + 17 GB written for 4 GB of compressed and inflated bytes).  Round 6 took the reads from 732 M to 170 M
           # (phase A through the chunk reader: 12.6 -> 10.4 ms); whole 64-byte blocks put together in LDS, streaming stores, a second
           # chunk ahead, the block header staged in LDS were measured and are slower.
           "roofline": {"kernel": "fx::k_bgzf_*", "bound": "vector-memory latency of k_bgzf_decode_par (s_waitcnt on divergent 8-byte stores and 16-byte chunk loads: "
                                 "the vL1D has L2 requests outstanding 70 % of the kernel); not HBM bandwidth, not vector issue",
                        "stall_classes_of_wave_cycles": {"parked_at_s_waitcnt": 0.714, "issuing_instructions": 0.228, "issue_stalls": 0.058,
                                                         "source": "profiles/r06_pmc_bgzf_c4.txt: SQ_WAIT_ANY, SQ_ACTIVE_INST_ANY, SQ_WAIT_INST_ANY over SQ_WAVE_CYCLES"},
                        "achieved": round(alg / (infl * 1e-3) / 1e9, 1) if infl else None,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / (infl * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if infl else None,
                        "hbm_frac": round(alg / (infl * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if infl else None,
                        "decode_traffic_measured": {"hbm_read_bytes": 15425574912, "hbm_written_bytes": 17345473536, "ratio_to_algorithmic": 8.1,
                                                    "source": "profiles/r06_pmc_bgzf_c4.txt: FETCH_SIZE x 1024 x 2 (profiles/r06_gathercal.txt), WRITE_SIZE x 1024"},
                        "decode_valu_issue_floor_ms": round(63900.0 * ((nb + 65279) // 65280) * 1.66e-9 / N_SIMD * 1e3, 2),
                        "decode_avg_launch_ms": round(prof_one.get("k_bgzf_decode", 0.0), 3),
                        "symbols": "11 863 per 65 280-byte member at zlib level 6: 73.7 % matches of 7.1 bytes, 26.3 % literals (tools/deflate_symbol_mix.c)",
                        "algorithmic_bytes_per_launch": alg, "avg_launch_ms": round(infl, 3), "traffic": None}}
    if plain_digest is not None:
        # all 1 M answers against the run on the plain file -- every string of which was compared with the reference's
        import hashlib
        out["fetch_1M_equal_plain_file_run"] = bool(hashlib.blake2b(buf.tobytes(), digest_size=16).hexdigest() == plain_digest[0]
                                                   and hashlib.blake2b(offs.tobytes(), digest_size=16).hexdigest() == plain_digest[1])
        if not out["fetch_1M_equal_plain_file_run"]:
            raise SystemExit("PARITY FAILURE (C4: answers differ from the plain-file run)")
    ref = None if a.no_cpu_baseline else _reference()
    if ref is not None:
        t2 = time.perf_counter()
        rf = ref.Fasta(path)                              # gzread through zlib + the same scan, single thread
        t3 = time.perf_counter()
        theirs = _tables(path + ".fxi", ("seq", "stat"))
        # fetches: indexed_gzip (zran) is NOT vendored in the reference tree; oracle/refshim stands in for it with gzseek, which
        # only moves forward cheaply.  So: a sample of queries in ascending file order (one forward pass), every string compared.
        boff = np.array([x[2] for x in ours["seq"]], dtype=np.int64)
        pool_n = len(ids) if a.c4_reference_full else min(200_000, len(ids))
        nref = pool_n if a.c4_reference_full else max(1, min(int(a.c4_ref_queries), pool_n))
        pick = np.argsort(boff[ids[:pool_n]] + st[:pool_n], kind="stable")[::max(1, pool_n // nref)]   # ascending offsets: one forward pass, a restart at every point it crosses
        t4 = time.perf_counter()
        eq = True
        for j in pick.tolist():
            s = rf[names[int(ids[j])]][int(st[j]):int(sp[j])]
            w = s.antisense if strand[j] else s.seq
            eq = eq and w.encode() == buf[int(offs[j]):int(offs[j + 1])].tobytes()
        t5 = time.perf_counter()
        del rf
        out["cpu_baseline"] = {"kind": "reference", "cores": 1, "index_s": round(t3 - t2, 3),
                               "fetch_sample_s": round(t5 - t4, 3), "fetch_sample_n": int(pick.size),
                               "sample": "pyfastx.Fasta() on the same %.2f GB .gz (gzread + scan + .fxi); fetches: %d queries in ascending "
                                         "file order through the zran work-alike (oracle/refshim/zran.c; indexed_gzip is not in the reference tree) "
                                         "seeking from the restart points the PRODUCT wrote into the index file, compared string by string" % (csize / 1e9, int(pick.size))}
        out["rows_equal_reference"] = bool(theirs["seq"] == ours["seq"] and theirs["stat"][0][:2] == ours["stat"][0][:2])
        out["fetch_sample_equal_reference"] = bool(eq)
        if not a.c4_reference_full:
            out["reference_on_all_queries"] = "builder-run, see profiles/r06_c4_full_reference.json (all 1 000 000 queries equal; `--c4-reference-full` repeats it)"
        out["index_speedup_vs_cpu"] = round((t3 - t2) / max(_median(t_ctor), 1e-9), 1)
        if not (out["rows_equal_reference"] and eq):
            raise SystemExit("PARITY FAILURE (C4 vs the reference)")
    _rm(path, path + ".fxi")
    # ---- the same bytes as ONE gzip stream (no member boundaries): zran-style restart points.  First open:
    # serial inflate on the host, points captured; every later open: the segments between the points inflated in parallel
    if a.gz_stream and not a.no_gz_stream:
        t0 = time.perf_counter()
        gz = synth.gzip_single_stream_parallel(host)
        p2 = os.path.join(tmpdir, "c4s.fa.gz")
        with open(p2, "wb") as f:
            f.write(gz)
        gsize = len(gz)
        del gz
        t1 = time.perf_counter()
        fa = fx.Fasta(p2)                                     # parallel first inflate + scan + .fxi with the restart points
        t2 = time.perf_counter()
        first_mode = fa._st.blob.gz_open_mode
        npts = len(_tables(p2 + ".fxi", ("gzindex",))["gzindex"])
        del fa
        t3 = time.perf_counter()
        fa = fx.Fasta(p2)                                     # loads the index ...
        fa._st.blob                                           # ... stages the stream: the segments between the points inflated in parallel
        t3b = time.perf_counter()
        nchk = min(200_000, len(qnames))
        b2, o2 = fa.fetch_many(qnames[:nchk], st[:nchk], sp[:nchk], strand=strand[:nchk])
        t4 = time.perf_counter()
        same = b2.tobytes() == buf[:int(offs[nchk])].tobytes()
        par = fa._st.blob.gz_checkpoints()["windows"].size == 0      # (a serial inflate would have captured windows again)
        del fa
        out["single_stream_gzip"] = {"compressed_bytes": gsize, "host_compress_s_setup_only": round(t1 - t0, 1),
                                     "first_open_ctor_s": round(t2 - t1, 3), "gzindex_rows": npts,
                                     "reopen_staged_s": round(t3b - t3, 3), "fetch_200k_after_reopen_s": round(t4 - t3b, 4), "reopen_used_the_points": bool(par),
                                     "fetches_equal_bgzf_run": bool(same),
                                     "first_open_mode": first_mode,
                                     "note": "one gzip member of the C2 bytes; first open = the stream inflated on all host cores (fx_pgzip.hpp: block starts "
                                             "searched behind the cuts, pieces decoded with markers, resolved in order; mode 3 -- mode 2 would be zlib on one "
                                             "core, 7 s) with restart points captured every >= 1 MiB, scan, index file with the points; re-open = the index's "
                                             "points, segments inflated by host threads in parallel"}
        if not same:
            raise SystemExit("PARITY FAILURE (single-stream gzip re-open)")
        _rm(p2, p2 + ".fxi")
    return out


# ------------------------------------------------------------------------------------------ N > 1: ONE file, byte-range shards
def _scratch_dir(need_bytes):
    """A directory for the bench's files: /dev/shm when it has the room (the page cache either way), else the temp dir."""
    try:
        if shutil.disk_usage("/dev/shm").free > need_bytes * 1.2 + (1 << 30):
            return tempfile.mkdtemp(prefix="fxbench", dir="/dev/shm")
    except OSError:
        pass
    return tempfile.mkdtemp(prefix="fxbench")


def _host_truth(mm, G, g, a, b, neg):
    """Bases [a, b) of global record g straight from the file bytes (well-formed 60-column LF record), for checking."""
    w = 60
    off = int(G["boff"][g]) + a + a // w
    raw = bytes(mm[off:off + (b - a) + (b // w - a // w)]).replace(b"\n", b"")
    if neg:
        raw = raw.translate(_COMP)[::-1]
    return raw


_COMP = bytes.maketrans(b"ACGTacgtMKRYVBHDmkryvbhdUu", b"TGCAtgcaKMYRBVDHkmyrbvdhAa")


# vector instructions per 4 KiB granule and wave (SQ_INSTS_VALU of a PMC pass / granules of its stream); source file beside each
VALU_PER_GRANULE = {"k_fastq_lines": (473, "profiles/r05_pmc_fastq_plain.txt: 803 238 357 / 1 699 219 granules (506 in round 1)"),
                    "k_fastq_lines_comp": (800, "profiles/r05_pmc_fastq_sq.txt: k_fastq_lines_comp<false> 1 358 541 574 / 1 699 219 granules (855 in round 4)")}
N_SIMD = 1024                                               # 256 CUs x 4 SIMDs
VALU_CAL = os.path.join("profiles", "r06_valuprobe.txt")    # tools/valuprobe.hip + tools/mixprobe.py on an MI355X (tools/gpu.sh valuprobe)


def _valu_calibration():
    """Measured issue times, from the committed calibration file: ns a wave64 instruction occupies a SIMD with the device full --
    fast class (v_sub_u32), slow class (v_dot4_u32_u8: also v_perm, v_alignbit, v_bfe, v_mul_lo, v_bcnt, v_mbcnt, v_readlane, the
    64-bit shifts), and per product kernel the time of ITS opcode mix as a probe kernel + the fraction of slow-class opcodes in it."""
    out = {"mix": {}}
    try:
        for ln in open(os.path.join(ROOT, VALU_CAL)):
            m = re.match(r"(v_sub_u32|v_dot4_u32_u8)\s+full:\s+([0-9.]+) ms", ln)
            if m:                                           # 2000 iterations x 64 instructions x 8 waves per SIMD
                out["fast_ns" if m.group(1) == "v_sub_u32" else "slow_ns"] = float(m.group(2)) * 1e6 / (2000 * 64 * 8)
            m = re.match(r"MIX (\S+) ns_per_instr=([0-9.]+) slow_class_fraction=([0-9.]+)", ln)
            if m:
                out["mix"][m.group(1)] = (float(m.group(2)), float(m.group(3)))
    except OSError:
        pass
    return out


def _issue_roofline(kernel, stream_bytes, measured_ms):
    """The vector-issue bound of a scan kernel, from MEASURED instruction times (VERDICT r5 #4a).  floor: the kernel's instruction
    count (SQ_INSTS_VALU of a PMC pass) x the time of its mix if every opcode issued at the best rate measured for its class -- a
    lower bound (opcodes not measured one by one count as fast).  mix_probe: the same count x the time its own opcode mix took as a
    probe kernel (shuffled, no memory) -- an estimate, not a bound: the product kernels issue their mix a few per cent FASTER than the
    shuffled probe (mix_probe_over_measured > 1), i.e. they run at the issue rate of their mix."""
    per, src = VALU_PER_GRANULE[kernel]
    cal = _valu_calibration()
    key = {"k_fastq_lines": "k_fastq_linesE", "k_fastq_lines_comp": "k_fastq_lines_compILb0E"}[kernel]
    if "fast_ns" not in cal or "slow_ns" not in cal or key not in cal["mix"]:
        return {"bound": "valu issue", "calibration": None, "note": "no calibration file (%s)" % VALU_CAL}
    mix_ns, slow = cal["mix"][key]
    floor_ns = (1.0 - slow) * cal["fast_ns"] + slow * cal["slow_ns"]
    n_instr = per * (stream_bytes / 4096.0)
    floor_ms, probe_ms = n_instr * floor_ns / N_SIMD * 1e-6, n_instr * mix_ns / N_SIMD * 1e-6
    return {"bound": "valu issue", "calibration": VALU_CAL, "valu_instructions_per_granule_and_wave": per, "counter_source": src, "granules": int(stream_bytes // 4096),
            "ns_per_wave64_instruction": {"fast_class": round(cal["fast_ns"], 3), "slow_class": round(cal["slow_ns"], 3), "slow_class_fraction": slow,
                                          "floor_of_this_mix": round(floor_ns, 3), "this_mix_as_a_probe_kernel": mix_ns},
            "floor_ms": round(floor_ms, 3), "avg_launch_ms": round(measured_ms, 4), "frac": round(floor_ms / measured_ms, 4),
            "floor_over_measured": round(floor_ms / measured_ms, 4),
            "mix_probe_ms": round(probe_ms, 3), "mix_probe_over_measured": round(probe_ms / measured_ms, 4),
            "hbm_frac": round(stream_bytes / (measured_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


_FETCH_PMC = {}                                              # FETCH_SIZE / WRITE_SIZE (KiB per launch) of k_fetch_lines from the same two passes


def live_pmc_traffic(a, file_bytes, file_path=None):
    """HBM bytes per k_span_scan launch, measured NOW: two rocprofv3 passes (--pmc FETCH_SIZE, --pmc WRITE_SIZE: separate runs,
    counters only -- MI355X_MICROARCH.md, HBM section) over a child of this script that generates the same stream and builds
    its index three times.  FETCH_SIZE is in KiB and, on gfx950, counts half of a wide coalesced stream (x 2, same section);
    WRITE_SIZE in KiB as it is.  -> (bytes per launch, source text) or (None, why not)."""
    import csv
    import glob
    import subprocess
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return None, "this run is itself under a profiler"
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="fxpmc", dir="/tmp")
    per = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(out, counter)
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                   sys.executable, os.path.join(ROOT, "bench.py"), "--pmc-child", "--gbp", repr(a.gbp), "--no-verify"]
            if file_path:
                cmd += ["--pmc-file", file_path]           # the child opens the file this run wrote: no torch, no generator (seconds, not half a minute)
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                return None, "rocprofv3 --pmc %s failed (rc %d): %s" % (counter, r.returncode, (r.stderr or r.stdout)[-200:])
            tot, ids = 0.0, set()
            ftot, fids = 0.0, set()
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                with open(f, newline="") as fh:
                    for row in csv.DictReader(fh):
                        if row.get("Counter_Name") != counter:
                            continue
                        kn = row.get("Kernel_Name", "")
                        if "k_span_scan<0>" in kn:
                            tot += float(row["Counter_Value"])
                            ids.add(row.get("Dispatch_Id", len(ids)))
                        elif "k_fetch_lines" in kn:
                            ftot += float(row["Counter_Value"])
                            fids.add(row.get("Dispatch_Id", len(fids)))
            if not ids:
                return None, "no k_span_scan<0> rows in the %s pass" % counter
            per[counter] = tot / len(ids)
            if fids:
                _FETCH_PMC[counter] = ftot / len(fids)
    except Exception as e:                                  # a profiler that is missing, hangs or writes another format: the committed figure stands
        return None, "%s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    rd, wr = int(per["FETCH_SIZE"] * 1024 * 2), int(per["WRITE_SIZE"] * 1024)
    return rd + wr, ("measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes over `bench.py --pmc-child` (same stream, "
                     "3 builds); FETCH_SIZE %.0f KiB x 1024 x 2 (gfx950 counts half of a wide coalesced stream, MI355X_MICROARCH.md) + WRITE_SIZE "
                     "%.0f KiB x 1024; %.4f x the algorithmic bytes" % (per["FETCH_SIZE"], per["WRITE_SIZE"], (rd + wr) / file_bytes))


def _collective_name(job, backend):
    if getattr(job, "fxcomm", None) is not None:
        return "fx_comm: ncclAllGather (RCCL) on the library's own stream, under the C ABI (fx_fasta_build_sharded_begin)"
    if backend == "nccl":
        return "torch.distributed all_gather_into_tensor (RCCL)" + ("; fx_comm unavailable: %s" % job.fxcomm_error if getattr(job, "fxcomm_error", None) else "")
    return "torch.distributed all_gather over %s (host path: the ranks share devices)" % backend


def main_sharded(a, dev, rank, world, backend):
    """configs[4] shape: the pieces of all ranks form ONE file; rank r opens only bytes [size*r/N, size*(r+1)/N) of it
    (fx_open_file_range), scans them, and ONE all-gather of the 28-word summaries stitches the records that cross the cuts."""
    import torch
    import torch.distributed as dist
    from pyfastx_amd import synth, shard
    total_bp = int(a.gbp * 1e9)
    plan = synth.fasta_plan(total_bp=total_bp, seed=20260612 + rank, tag="p%d_" % rank)
    piece, flat, flat_start = synth.fasta_generate(plan, dev, keep_flat=not a.no_verify)
    nb = int(plan["n_bytes"])
    comm = dev if backend == "nccl" else torch.device("cpu")
    mine = torch.tensor([nb], dtype=torch.int64, device=comm)
    outs = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(outs, mine)
    sizes = np.array([int(o.item()) for o in outs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(starts[-1])
    box = [None]
    if rank == 0:
        box[0] = os.path.join(_scratch_dir(total), "c5.fa")
        with open(box[0], "wb") as f:
            f.truncate(total)
    dist.broadcast_object_list(box, src=0)
    path = box[0]
    dist.barrier()
    with open(path, "r+b") as f:                           # every rank writes its piece where it belongs in the one file
        f.seek(int(starts[rank]))
        piece[:nb].cpu().numpy().tofile(f)
    del piece
    torch.cuda.empty_cache()
    dist.barrier()
    try:
        t0 = time.perf_counter()
        job = shard.ShardedFasta.from_file(path, dev, rank, world, force_collective=world == 1)   # page cache -> pinned pieces -> HBM, this rank's range only
        t_open = time.perf_counter() - t0
        lo, hi = job.base, job.base + job.n_bytes
        # analytic rows of the whole file (pure numpy, every rank computes them) and the rows this shard must hold
        plans = [plan if r == rank else synth.fasta_plan(total_bp=total_bp, seed=20260612 + r, tag="p%d_" % r) for r in range(world)]
        G = {k: np.concatenate([plans[r][k] + (starts[r] if k in ("hoff", "boff") else 0) for r in range(world)])
             for k in ("hoff", "boff", "blen", "slen", "llen", "dlen", "name_len")}
        gnames = [n for r in range(world) for n in plans[r]["names"]]
        g0, g1 = int(np.searchsorted(G["hoff"], lo, "left")), int(np.searchsorted(G["hoff"], hi, "left"))
        nrec = len(plan["slen"])
        qlen = 100
        own = np.arange(rank * nrec, (rank + 1) * nrec)
        ok = own[(G["hoff"][own] >= lo) & (G["boff"][own] + G["blen"][own] <= hi) & (G["slen"][own] >= qlen)]
        rng = np.random.default_rng(12345 + rank)           # contigs of my piece that lie wholly in my shard: no collective on this path
        pr = G["slen"][ok].astype(np.float64)
        gid = ok[rng.choice(ok.size, a.queries, p=pr / pr.sum())]
        st = (rng.random(a.queries) * (G["slen"][gid] - qlen + 1)).astype(np.int64)
        sp = st + qlen
        strand = (rng.random(a.queries) < 0.5).astype(np.uint8)
        d_ids = torch.from_numpy(gid - g0).to(dev); d_st = torch.from_numpy(st).to(dev); d_sp = torch.from_numpy(sp).to(dev)
        d_fl = torch.from_numpy((strand * 6).astype(np.uint8)).to(dev)
        d_off = torch.arange(a.queries, device=dev, dtype=torch.int64) * qlen
        d_out = torch.zeros(a.queries * qlen, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(a.queries, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def step():
            job.build_async()                                 # scan + tables + summary -> all-gather (RCCL) -> stitch, all enqueued
            job.fetch_local(a.queries, d_ids, d_st, d_sp, d_fl, d_out, d_off, d_len)
            job.finish()                                      # the step's one host synchronisation
            job.sync()

        for _ in range(a.warmup):
            step()
        job.blob.prof_enable(2)
        job.blob.prof_reset()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        dist.barrier()
        el = time.perf_counter() - t0                         # the timed region: exactly a.steps steps between barriers
        t_index = 0.0
        for _ in range(a.steps):
            ts = time.perf_counter()
            job.build()
            t_index += time.perf_counter() - ts
        prof = job.blob.prof_read()
        job.blob.prof_enable(1)
        job.blob.prof_reset()
        for _ in range(5):
            step()
        prof_all = job.blob.prof_read()
        job.blob.prof_enable(0)
        # ---------------- parity at full size: this shard's rows (the stitched one included) against the analytic rows
        verified = None
        if not a.no_verify:
            rows = job.local_rows()
            verified = len(rows["boff"]) == g1 - g0
            for k in G:
                verified = verified and bool((rows[k] == G[k][g0:g1]).all())
            verified = verified and bool((rows["norm"] == 1).all()) and bool((rows["elen"] == 1).all())
            exp = synth.expected_fetch(flat, flat_start, gid - rank * nrec, st, qlen, strand, dev)
            verified = verified and bool((d_out.view(a.queries, qlen) == exp).all()) and bool((d_len == qlen).all())
            del exp
            if not verified:
                raise SystemExit("PARITY FAILURE at full size on rank %d: refusing to report a speed-up" % rank)
        # ---------------- composition across the cuts
        comp_ms = None
        if not a.no_verify:
            tc = time.perf_counter()
            comp = job.composition()
            comp_ms = (time.perf_counter() - tc) * 1e3
            okc = True
            for g in ok.tolist():
                i = g - rank * nrec
                L = int(plan["slen"][i])
                seg = flat[int(flat_start[i]):int(flat_start[i]) + L]
                okc &= bool((torch.bincount(seg.long(), minlength=128)[:128].cpu() == torch.from_numpy(comp[g - g0])).all())
            tot = torch.from_numpy(comp.sum(axis=0) if len(comp) else np.zeros(128, dtype=np.int64)).to(dev)
            want = torch.zeros(128, dtype=torch.int64, device=dev)
            for i in range(nrec):
                L = int(plan["slen"][i])
                want += torch.bincount(flat[int(flat_start[i]):int(flat_start[i]) + L].long(), minlength=128)[:128]
            both = torch.stack([tot, want]).to(comm)
            dist.all_reduce(both, op=dist.ReduceOp.SUM)
            okc &= bool((both[0] == both[1]).all())
            if not okc:
                raise SystemExit("PARITY FAILURE (composition across shards) at full size")
        # ---------------- ONE index file for the whole stream, and fetches over all of it (cross-cut queries included)
        t0 = time.perf_counter()
        table = job.write_index(path + ".fxi")
        t_fxi = time.perf_counter() - t0
        fxi_ok = None
        if rank == 0 and not a.no_verify:
            import sqlite3
            db = sqlite3.connect(path + ".fxi")
            got = db.execute("SELECT chrom,boff,blen,slen,llen,elen,norm,dlen FROM seq ORDER BY ID").fetchall()
            db.close()
            fxi_ok = len(got) == len(gnames) and all(
                tuple(r) == (gnames[i], int(G["boff"][i]), int(G["blen"][i]), int(G["slen"][i]), int(G["llen"][i]), 1, 1, int(G["dlen"][i]))
                for i, r in enumerate(got))
            if not fxi_ok:
                raise SystemExit("PARITY FAILURE: the merged .fxi differs from the analytic rows of the whole file")
        fetcher = job.fetcher(table)
        rq = np.random.default_rng(777)                      # the same batch on every rank: 1 M queries over the WHOLE stream
        pw = np.maximum(G["slen"] - qlen + 1, 0).astype(np.float64)
        qg = rq.choice(len(pw), a.queries, p=pw / pw.sum())
        qa = (rq.random(a.queries) * (G["slen"][qg] - qlen + 1)).astype(np.int64)
        qneg = (rq.random(a.queries) < 0.5)
        qfl = np.where(qneg, 6, 0).astype(np.uint8)
        fetcher.fetch(qg[:1000], qa[:1000], qa[:1000] + qlen, flags_per_query=qfl[:1000])
        dist.barrier()
        t0 = time.perf_counter()
        qidx, fbuf, foffs = fetcher.fetch(qg, qa, qa + qlen, flags_per_query=qfl)
        dist.barrier()
        t_sf = time.perf_counter() - t0
        off_, bl_, _, _ = shard.slice_ranges(table, qg, qa, qa + qlen)
        cross = int((shard.route_ranges(table["bases"], table["ends"], off_, bl_)["cnt"] > 1).sum())
        sf_ok = None
        if not a.no_verify:
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            pos = np.full(a.queries, -1, dtype=np.int64)
            pos[qidx] = np.arange(qidx.size)
            crossing = np.nonzero(shard.route_ranges(table["bases"], table["ends"], off_, bl_)["cnt"] > 1)[0]
            sample = np.unique(np.concatenate([qidx[::max(qidx.size // 2000, 1)], crossing[pos[crossing] >= 0]]))
            sf_ok = True
            for qi in sample.tolist():
                j = int(pos[qi])
                sf_ok = sf_ok and fbuf[foffs[j]:foffs[j + 1]].tobytes() == _host_truth(mm, G, int(qg[qi]), int(qa[qi]), int(qa[qi]) + qlen, bool(qneg[qi]))
            del mm
            cnt = torch.tensor([qidx.size, int(sf_ok)], dtype=torch.int64, device=comm)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
            sf_ok = bool(int(cnt[0]) == a.queries and int(cnt[1]) == world)      # every query answered exactly once, every sample right
            if not sf_ok:
                raise SystemExit("PARITY FAILURE: fetches over the byte-range shards")
        times = torch.tensor([el, t_index, t_open, t_fxi, t_sf], dtype=torch.float64, device=comm)
        dist.all_reduce(times, op=dist.ReduceOp.MAX)          # the slowest rank counts
        el, t_index, t_open, t_fxi, t_sf = (float(x) for x in times.cpu())
    finally:
        dist.barrier()
        if rank == 0:
            shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    if rank != 0:
        return None
    ms = el / a.steps * 1e3
    fetch_ms = sum(prof_all.get(k, (0.0, 1))[0] / max(prof_all.get(k, (0.0, 1))[1], 1) for k in ("k_fetch", "k_fetch_rest"))
    scan_ms, scan_n = prof.get("k_span_scan", (0.0, 0))
    scan_avg = scan_ms / max(scan_n, 1)
    achieved = job.n_bytes / (scan_avg * 1e-3) / 1e9 if scan_avg > 0 else 0.0
    return {
        "metric": "FASTA index build + 1M random 100bp subseq fetches, 3 Gbp plain FASTA per GPU (throughput of the whole step, stream resident in HBM)",
        "value": round(world * a.gbp / (el / a.steps), 3), "unit": "Gbp/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": "configs[4] shape: ONE synthetic %.1f Gbp hg38-shaped plain FASTA (%d x %.1f Gbp pieces, %d contigs) sharded by byte "
                               "range over %d GPUs; per GPU and step: index build of its range + all-gather of the boundary summaries + stitch + "
                               "%d random %d bp intervals (50%% '-' strand) on contigs it holds" % (world * a.gbp, world, a.gbp, len(gnames), world, a.queries, qlen),
                   "file_bytes": total, "file_bytes_per_gpu": int(job.n_bytes),
                   "parallelism": "byte-range shards of one file x%d (each rank reads only its range), 1 all-gather (%s)" % (world, backend),
                   "collective": _collective_name(job, backend),
                   # the host threads that stage a rank's byte range run on the CPUs next to its device (csrc/fxgpu.hip: device_cpus)
                   "staging_cpus_of_rank0_device": _device_cpulist(dev)},
        "index_build_s": round(t_index / a.steps, 6),
        "fetch_M_per_s": round(world * a.queries / max(fetch_ms * 1e-3, 1e-9) / 1e6, 2),
        "parity_verified_full_size": verified,
        "composition_pass_ms": None if comp_ms is None else round(comp_ms, 3),
        "kernels_ms_avg": {k: round(v[0] / v[1], 4) for k, v in prof_all.items()},
        "roofline": {"kernel": "fx::k_span_scan<0>", "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                     "algorithmic_bytes_per_launch": int(job.n_bytes), "avg_launch_ms": round(scan_avg, 4)},
        "sharded_file": {"open_range_s": round(t_open, 4), "open_GBps_aggregate": round(total / max(t_open, 1e-9) / 1e9, 1),
                         "merged_fxi_s": round(t_fxi, 4), "merged_fxi_rows_equal_plan": fxi_ok,
                         "shard_fetch_1M_host_to_host_s": round(t_sf, 4), "queries_crossing_a_cut": cross,
                         "every_query_answered_once_and_sample_equals_file": sf_ok,
                         "note": "max over ranks; open = every rank stages only its byte range of the one file (page cache -> pinned -> HBM); "
                                 "merged_fxi = all_gather_object of the per-rank rows + rank 0 writes ONE .fxi; shard_fetch = the same 1 M queries over "
                                 "the WHOLE stream on every rank through shard.ShardFetcher, each answered by the rank that holds its first byte"},
    }


# ------------------------------------------------------------------------------------------ strong scaling: ONE file over N GPUs
def strong_leg(a, dev, rank, world, backend, collective):
    """BASELINE.json's metric as it is worded -- ONE 3 Gbp FASTA on 1/2/4/8 GPUs: the file is cut into `world` byte ranges
    (the cuts fall inside contigs and lines), rank r stages only ITS range over its own PCIe link, builds its part of the
    index, ONE all-gather of the 28-word summaries stitches the record across every cut, rank 0 writes ONE .fxi, and the
    SAME 1 M queries of the single-GPU run are answered over the whole stream: each by the rank that holds its first byte
    (fx_shard_route), queries that cross a cut put together from their pieces.  Reported: (i) the step with everything
    resident in HBM -- build + all-gather + stitch + this rank's routed share of the queries, K timed steps between barriers
    -- and (ii) the same job END TO END, file to answers in host memory, every phase max over ranks.
    collective: a process group exists (world > 1, or the forced single-rank RCCL run)."""
    import torch
    import torch.distributed as dist
    from pyfastx_amd import _lib, synth, shard
    total_bp = int(a.gbp * 1e9)
    comm = dev if backend == "nccl" else torch.device("cpu")

    def barrier():
        if collective:
            dist.barrier()

    def allmax(vals):
        t = torch.tensor(vals, dtype=torch.float64, device=comm if collective else "cpu")
        if collective:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(x) for x in t.cpu()]

    def allsum(vals):
        t = torch.tensor(vals, dtype=torch.int64, device=comm if collective else "cpu")
        if collective:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return [int(x) for x in t.cpu()]

    plan = synth.fasta_plan(total_bp=total_bp, seed=20260612)          # the single-GPU run's file and queries (configs[1])
    nb = int(plan["n_bytes"])
    ids, st, sp, strand = synth.fasta_queries(plan, n=a.queries, seed=12345)
    qfl = (strand * 6).astype(np.uint8)
    qlen = int(sp[0] - st[0])
    box = [None]
    if rank == 0:
        box[0] = os.path.join(_scratch_dir(nb), "c2.fa")
        piece, _, _ = synth.fasta_generate(plan, dev, keep_flat=False)
        piece[:nb].cpu().numpy().tofile(box[0])
        del piece
        torch.cuda.empty_cache()
    if collective:
        dist.broadcast_object_list(box, src=0)
    path = box[0]
    barrier()
    try:
        _lib.Blob.from_file_range(path, nb * rank // world, min(1 << 20, nb // world), 0, device=dev.index).close()   # first touch: HIP context, pinned pool
        barrier()
        # ---------------- (ii) end to end, once per phase (the phases are seconds-scale host work; max over ranks)
        t0 = time.perf_counter()
        job = shard.ShardedFasta.from_file(path, dev, rank, world, force_collective=collective and world == 1)
        t_open = time.perf_counter() - t0
        barrier()
        t0 = time.perf_counter()
        job.build()
        t_build = time.perf_counter() - t0
        barrier()
        t0 = time.perf_counter()
        table = job.write_index(path + ".fxi")                            # gather of the rows + rank 0 writes ONE .fxi
        t_fxi = time.perf_counter() - t0
        fetcher = job.fetcher(table)
        fetcher.fetch(ids[:1000], st[:1000], sp[:1000], flags_per_query=qfl[:1000])
        barrier()
        t0 = time.perf_counter()
        qidx, fbuf, foffs = fetcher.fetch(ids, st, sp, flags_per_query=qfl)   # host arrays -> host buffer, this rank's share
        barrier()
        t_fetch = time.perf_counter() - t0
        # ---------------- parity: the merged index against the plan's analytic rows, every query answered once, the bytes
        ok_rows = ok_bytes = None
        off_, bl_, _, _ = shard.slice_ranges(table, ids, st, sp)
        route = shard.route_ranges(table["bases"], table["ends"], off_, bl_)
        n_cross = int((route["cnt"] > 1).sum())
        if not a.no_verify:
            if rank == 0:
                import sqlite3
                db = sqlite3.connect(path + ".fxi")
                got = db.execute("SELECT chrom,boff,blen,slen,llen,elen,norm,dlen FROM seq ORDER BY ID").fetchall()
                tot = db.execute("SELECT seqnum, seqlen FROM stat").fetchone()
                db.close()
                ok_rows = len(got) == len(plan["names"]) and tuple(tot) == (len(got), int(plan["slen"].sum())) and all(
                    tuple(r) == (plan["names"][i], int(plan["boff"][i]), int(plan["blen"][i]), int(plan["slen"][i]), int(plan["llen"][i]), 1, 1, int(plan["dlen"][i]))
                    for i, r in enumerate(got))
                if not ok_rows:
                    raise SystemExit("PARITY FAILURE (strong scaling): the merged .fxi differs from the analytic rows of the file")
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            G = {"boff": plan["boff"]}
            pos = np.full(a.queries, -1, dtype=np.int64)
            pos[qidx] = np.arange(qidx.size)
            crossing = np.nonzero(route["cnt"] > 1)[0]
            sample = np.unique(np.concatenate([qidx[::max(qidx.size // 4000, 1)], crossing[pos[crossing] >= 0]]))
            good = True
            for qi in sample.tolist():
                j = int(pos[qi])
                good = good and fbuf[foffs[j]:foffs[j + 1]].tobytes() == _host_truth(mm, G, int(ids[qi]), int(st[qi]), int(sp[qi]), bool(strand[qi]))
            del mm
            n_ans, n_good = allsum([qidx.size, int(good)])
            ok_bytes = bool(n_ans == a.queries and n_good == world)
            if not ok_bytes:
                raise SystemExit("PARITY FAILURE (strong scaling): fetches over the byte-range shards")
        del fbuf
        # ---------------- (i) the step, HBM-resident: this rank's routed share of the batch as device arrays (routing is
        # setup here -- it is inside the end-to-end fetch above), pieces of cut-crossing queries of other ranks included
        R = _lib.shard_route(ids, st, sp, fetcher._cols, fetcher.bases, fetcher.ends, 0, qfl)
        lo_, hi_ = int(R["shard_start"][rank]), int(R["shard_start"][rank + 1])
        r_off, r_len, r_take, r_fl = R["off"][lo_:hi_], R["len"][lo_:hi_], R["take"][lo_:hi_], R["fl"][lo_:hi_]
        other = (route["r"] == rank) & (route["first"][route["q"]] != rank)   # pieces I hold of queries another rank answers
        if other.any():
            r_off = np.concatenate([r_off, route["poff"][other]]); r_len = np.concatenate([r_len, route["plen"][other]])
            r_take = np.concatenate([r_take, route["plen"][other]]); r_fl = np.concatenate([r_fl, qfl[route["q"][other]]])
        n_mine = int(r_off.size)
        d_off = torch.from_numpy(np.ascontiguousarray(r_off)).to(dev); d_bl = torch.from_numpy(np.ascontiguousarray(r_len)).to(dev)
        d_tk = torch.from_numpy(np.ascontiguousarray(r_take)).to(dev); d_fl = torch.from_numpy(np.ascontiguousarray(r_fl)).to(dev)
        dst_off = np.zeros(n_mine + 1, dtype=np.int64)
        np.cumsum(np.maximum(r_take, 0), out=dst_off[1:])
        d_do = torch.from_numpy(dst_off[:-1].copy()).to(dev)
        d_out = torch.zeros(max(int(dst_off[-1]), 16), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(max(n_mine, 1), dtype=torch.int64, device=dev)
        L = _lib.lib()
        torch.cuda.synchronize()

        def step():
            job.build_async()                                 # scan + tables + summary -> all-gather -> stitch, enqueued
            if n_mine:
                _lib.check(L.fx_fetch_ranges(job.blob._h, _lib.FX_DEVICE, n_mine, d_off.data_ptr(), d_bl.data_ptr(), d_tk.data_ptr(), 0,
                                             d_fl.data_ptr(), d_out.data_ptr(), d_do.data_ptr(), d_len.data_ptr()))
            job.finish()
            job.sync()

        for _ in range(a.warmup):
            step()
        job.blob.prof_enable(2)
        job.blob.prof_reset()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        barrier()
        el = time.perf_counter() - t0                         # exactly a.steps steps between barriers
        prof = job.blob.prof_read()
        job.blob.prof_enable(1)
        job.blob.prof_reset()
        for _ in range(5):
            step()
        prof_all = job.blob.prof_read()
        job.blob.prof_enable(0)
        t_index = 0.0
        for _ in range(a.steps):
            ts = time.perf_counter()
            job.build()
            t_index += time.perf_counter() - ts
        step_ok = None
        if not a.no_verify:                                   # the device step's answers: whole queries against the file
            out_h, len_h = d_out.cpu().numpy(), d_len.cpu().numpy()
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            G = {"boff": plan["boff"]}
            order = R["order"][lo_:hi_]
            good = True
            for k in range(0, hi_ - lo_, max((hi_ - lo_) // 2000, 1)):
                if R["cnt"][lo_ + k] != 1:
                    continue
                qi = int(order[k])
                good = good and int(len_h[k]) == qlen and out_h[dst_off[k]:dst_off[k] + qlen].tobytes() == _host_truth(mm, G, int(ids[qi]), int(st[qi]), int(sp[qi]), bool(strand[qi]))
            del mm
            step_ok = bool(allsum([int(good)])[0] == world)
            if not step_ok:
                raise SystemExit("PARITY FAILURE (strong scaling): the device-resident routed fetch")
        el, t_index, t_open, t_build, t_fxi, t_fetch = allmax([el, t_index, t_open, t_build, t_fxi, t_fetch])
        n_max = allmax([float(n_mine)])[0]
    finally:
        barrier()
        if rank == 0:
            shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    if rank != 0:
        return None
    ms = el / a.steps * 1e3
    scan_ms, scan_n = prof.get("k_span_scan", (0.0, 0))
    scan_avg = scan_ms / max(scan_n, 1)
    achieved = job.n_bytes / (scan_avg * 1e-3) / 1e9 if scan_avg > 0 else 0.0
    e2e_total = t_open + t_build + t_fxi + t_fetch
    return {
        "workload": "configs[1] on %d GPU(s): ONE synthetic %.1f Gbp hg38-shaped plain FASTA (%d contigs, %.2f GB) cut into %d byte ranges; index build "
                    "(scan of the range + all-gather of the boundary summaries + stitch) + the SAME %d random %d bp intervals (50%% '-' strand) over the "
                    "whole stream, routed to the rank that holds their first byte" % (world, a.gbp, len(plan["names"]), nb / 1e9, world, a.queries, qlen),
        "Gbp_per_s": round(a.gbp / (el / a.steps), 3), "ms_per_step": round(ms, 4), "index_build_s": round(t_index / a.steps, 6),
        "file_bytes": nb, "file_bytes_per_gpu": int(job.n_bytes), "queries_per_gpu_max": int(n_max), "queries_crossing_a_cut": n_cross,
        "collective": _collective_name(job, backend),
        "kernels_ms_avg": {k: round(v[0] / v[1], 4) for k, v in prof_all.items()},
        "roofline": {"kernel": "fx::k_span_scan<0>", "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "algorithmic_bytes_per_launch": int(job.n_bytes),
                     "avg_launch_ms": round(scan_avg, 4)},
        "e2e": {"open_range_s": round(t_open, 4), "open_GBps_aggregate": round(nb / max(t_open, 1e-9) / 1e9, 1), "build_s": round(t_build, 4),
                "merged_fxi_s": round(t_fxi, 4), "fetch_1M_host_to_host_s": round(t_fetch, 4), "total_s": round(e2e_total, 4),
                "note": "one pass per phase, max over ranks, barriers between phases: every rank stages only its byte range of the one file (page "
                        "cache -> pinned -> HBM over its own PCIe link); build = scan + all-gather (%s) + stitch + totals; merged_fxi = gather of "
                        "the rows + rank 0 writes ONE .fxi; fetch = the whole batch through fx_shard_route on every rank, its share through the "
                        "fetch kernel and back to host memory, pieces of cut-crossing queries exchanged" % backend},
        "parity": {"merged_fxi_rows_equal_plan": ok_rows, "every_query_answered_once_and_sample_equals_file": ok_bytes,
                   "device_step_sample_equals_file": step_ok},
    }


def fastq_strong_leg(a, dev, rank, world, backend, collective):
    """configs[2]'s job on N GPUs (round 4: what was left of multi-GPU FASTQ): ONE FASTQ file cut into `world` byte ranges, rank r
    stages its range + a halo, ONE all-gather of two words numbers the lines, every rank builds the rows of the reads it owns,
    ONE more all-gather of ten words gives base / meta of the whole file on every rank, rank 0 writes ONE .fxi, and a batch of
    random reads (the same on every rank) is answered by the ranks that own them -- no bytes between GPUs.  Every phase max
    over ranks; rows, base / meta and fetched bytes against the generator's analytic truth."""
    import torch
    import torch.distributed as dist
    from pyfastx_amd import _lib, synth, shard
    n = int(min(a.c3_reads, a.fastq_reads))
    comm = dev if backend == "nccl" else torch.device("cpu")

    def barrier():
        if collective:
            dist.barrier()

    def allmax(vals):
        t = torch.tensor(vals, dtype=torch.float64, device=comm if collective else "cpu")
        if collective:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(x) for x in t.cpu()]

    def allgather_i64(v):
        t = torch.from_numpy(np.asarray(v, dtype=np.int64).copy()).to(comm if collective else "cpu")
        if not collective:
            return t.cpu().numpy().reshape(1, -1)
        outs = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(outs, t)
        return np.stack([o.cpu().numpy() for o in outs])

    box = [None]
    rec = so = qo = hl = None
    if rank == 0:
        blob, cols = synth.fastq_generate(n, dev)
        nb = int(cols["n_bytes"])
        box[0] = (os.path.join(_scratch_dir(nb * 1.4), "c3s.fq"), nb, int(cols["rec"]), int(cols["soff"][0]), int(cols["qoff"][0]), int(cols["dlen"][0]))
        blob[:nb].cpu().numpy().tofile(box[0][0])
        del blob, cols
        torch.cuda.empty_cache()
    if collective:
        dist.broadcast_object_list(box, src=0)
    path, nb, rec, so, qo, dl = box[0]
    barrier()
    try:
        _lib.Blob.from_file_range(path, nb * rank // world, min(1 << 20, nb // world), 0, device=dev.index).close()
        barrier()
        t0 = time.perf_counter()
        sq = shard.ShardedFastq(path, rank, world, device=dev.index, gather=(lambda m: allgather_i64(m)), index_file=path + ".fxi")     # stage + scan + all-gather + rows (rank 0: room for the .fxi set aside meanwhile)
        t_build = time.perf_counter() - t0
        barrier()
        t0 = time.perf_counter()
        base, meta = sq.composition(gather=(lambda m: allgather_i64(m)))
        t_comp = time.perf_counter() - t0
        barrier()
        t0 = time.perf_counter()
        n_total = sq.write_index(path + ".fxi", gather=allgather_i64)     # every rank formats its table leaves on its device; names to rank 0 (RCCL / gloo), one sort, the index
        t_fxi = time.perf_counter() - t0
        first = np.concatenate([[0], np.cumsum(allgather_i64([sq.n_local])[:, 0])])
        nq = int(min(a.queries, 1_000_000))
        ids = np.random.default_rng(99).integers(0, n, nq)
        sq.fetch(ids[:1000], first, phred=int(meta[4]))
        barrier()
        t0 = time.perf_counter()
        pos, seq, qual, qi, offs = sq.fetch(ids, first, phred=int(meta[4]))
        barrier()
        t_fetch = time.perf_counter() - t0
        ok = None
        if not a.no_verify:
            # rows: the generator's records are `rec` bytes apart; this rank owns ids [first_id, first_id + n_local)
            t = sq.blob.fastq_table(sq.n_local)
            gid = sq.first_id + np.arange(sq.n_local, dtype=np.int64)
            ok = bool((t["soff"] == gid * rec + so).all() and (t["qoff"] == gid * rec + qo).all() and (t["rlen"] == 150).all() and (t["dlen"] == dl).all())
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            pick = np.arange(0, pos.size, max(pos.size // 5000, 1))
            g = ids[pos[pick]].astype(np.int64) * rec
            idx = g[:, None] + np.arange(150)[None, :]
            sv = np.asarray(seq).reshape(-1, 150)[pick] if pos.size else np.zeros((0, 150), np.uint8)
            qv = np.asarray(qual).reshape(-1, 150)[pick] if pos.size else np.zeros((0, 150), np.uint8)
            ok = ok and bool((sv == mm[idx + so]).all()) and bool((qv == mm[idx + qo]).all())
            del mm
            answered = int(allgather_i64([pos.size])[:, 0].sum())
            ok = ok and answered == nq and int(first[-1]) == n and int(base.sum()) == n * 150 and int(meta[0]) == 150 and int(meta[4]) == 33
            if collective:
                t_ok = torch.tensor([1 if ok else 0], dtype=torch.int32, device=comm)
                dist.all_reduce(t_ok, op=dist.ReduceOp.MIN)
                ok = bool(int(t_ok.item()))
            if not ok:
                raise SystemExit("PARITY FAILURE (sharded FASTQ, rank %d)" % rank)
        tb, tc, tf, tq = allmax([t_build, t_comp, t_fxi, t_fetch])
        return {"workload": "ONE %d x 150 bp FASTQ file (%.2f GB) over %d ranks by byte range: build (stage + scan + one all-gather of 2 words + rows), "
                            "composition (one all-gather of 10 words), ONE .fxi, %d random reads routed to the ranks that own them" % (n, nb / 1e9, world, nq),
                "build_s": round(tb, 4), "composition_s": round(tc, 4), "fxi_written_s": round(tf, 3), "fetch_routed_s": round(tq, 4),
                "fxi_steps_rank0_s": getattr(sq, "index_steps", None), "fxi_laps_rank0_s": {k: round(v, 4) for k, v in getattr(sq, "index_laps", {}).items()},
                "reads_indexed": int(n_total) if n_total is not None else int(first[-1]), "halo_reopened": int(sq.reopened),
                "rows_base_meta_fetch_equal_generator": ok, "M_reads_per_s_build": round(n / max(tb, 1e-9) / 1e6, 1)}
    finally:
        barrier()
        if rank == 0:
            _rm(path, path + ".fxi")


def main_strong(a, dev, rank, world, backend, collective):
    """--scaling strong: the strong leg IS the line."""
    s = strong_leg(a, dev, rank, world, backend, collective)
    if rank != 0:
        return None
    return {
        "metric": "FASTA index build + 1M random 100bp subseq fetches on ONE 3 Gbp plain FASTA split by byte range over the GPUs (throughput of the whole step, stream resident in HBM)",
        "value": s["Gbp_per_s"], "unit": "Gbp/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": s["ms_per_step"],
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": s["workload"], "file_bytes": s["file_bytes"], "file_bytes_per_gpu": s["file_bytes_per_gpu"],
                   "parallelism": "byte-range shards of one file x%d (each rank reads only its range), 1 all-gather (%s)" % (world, backend)},
        "index_build_s": s["index_build_s"], "parity_verified_full_size": all(v is not False for v in s["parity"].values()) and None not in s["parity"].values(),
        "kernels_ms_avg": s["kernels_ms_avg"], "roofline": s["roofline"], "strong": s,
    }


def _self_launch(a):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (torch.distributed.run, one process per GPU)."""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    os.execve(sys.executable, cmd, dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))


_LINE_FD = None


def _stdout_for_the_line_only():
    """stdout carries the ONE JSON line and nothing else: what libraries print there (gloo's "[Gloo] Rank 3 is connected to 7 peer
    ranks" for every rank, RCCL's lines under NCCL_DEBUG) goes to stderr from here on."""
    global _LINE_FD
    try:
        sys.stdout.flush()
        fd = os.dup(1)
        os.dup2(2, 1)
        _LINE_FD = fd
    except OSError:
        _LINE_FD = None


def _emit(line):
    text = json.dumps(line) + "\n"
    if _LINE_FD is None:
        sys.stdout.write(text)
        sys.stdout.flush()
        return
    sys.stdout.flush()
    data = text.encode()
    while data:
        data = data[os.write(_LINE_FD, data):]


DUMP_QUERIES = 65536                                         # answers written by --dump-outputs: 65536 x 100 bases as float32 = 26 MB


def dump_outputs(d, job, d_out, d_len, n_queries, qlen):
    """--dump-outputs: what the timed step hands its caller after the last step, as DIR/<name>.npy -- every column of the
    record table (float64: offsets pass 2^24) and, for a fixed seeded sample of the batch's queries, the answer's length
    and its bases (float32), so that two builds run with the same arguments can be compared output for output."""
    import torch
    os.makedirs(d, exist_ok=True)
    for k, v in job.local_rows().items():
        np.save(os.path.join(d, "index_%s.npy" % k), v.astype(np.float64))
    pick = np.sort(np.random.default_rng(4242).choice(n_queries, min(n_queries, DUMP_QUERIES), replace=False))
    idx = torch.from_numpy(pick).to(d_out.device)
    np.save(os.path.join(d, "fetch_len.npy"), d_len[idx].cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "fetch_bases.npy"), d_out.view(n_queries, qlen)[idx].cpu().numpy().astype(np.float32))


# ------------------------------------------------------------------------------------------ main
def main():
    a = parse()
    if a.dump_outputs and (a.gpus > 1 or a.scaling == "strong" or os.environ.get("FX_BENCH_FORCE_SHARDED")):
        raise SystemExit("--dump-outputs: only the single-GPU weak run writes its outputs")
    if a.pmc_child and a.pmc_file:                           # one counter pass of live_pmc_traffic: the file, three builds, nothing else in the process
        os.environ["FX_NO_TORCH"] = "1"
        from pyfastx_amd import _lib
        b = _lib.Blob.from_file(a.pmc_file)
        for _ in range(3):
            b.fasta_build()
        b.sync()
        # ... and the run's own batch of queries, three times (k_fetch_lines: the traffic of roofline_fetch); plan and queries are numpy
        from pyfastx_amd import synth
        plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
        ids, st, sp, strand = synth.fasta_queries(plan, n=a.queries, seed=12345)
        for _ in range(3):
            b.fasta_fetch_alloc(ids, st, sp, flags_per_query=(strand * 6).astype(np.uint8))
        b.close()
        return
    import torch
    import torch.distributed as dist
    from pyfastx_amd import _lib, synth, shard

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(a)                                     # does not return: the N ranks run this file again under torch.distributed.run
    _stdout_for_the_line_only()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    ndev = max(torch.cuda.device_count(), 1)
    # "nccl" IS RCCL on ROCm.  RCCL refuses two ranks on one device, so a box with fewer GPUs than ranks (the 1-GPU test box)
    # runs the same code over gloo with the ranks sharing the devices -- a plumbing run, and the line says so.
    backend = os.environ.get("FX_BENCH_BACKEND", "nccl" if ndev >= world else "gloo")
    local = local % ndev if backend != "nccl" else local
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # FX_BENCH_FORCE_SHARDED=1: the N > 1 code path with a process group of ONE rank (how the 1-GPU test box runs every
    # collective of that path over RCCL; needs MASTER_ADDR / MASTER_PORT / RANK / WORLD_SIZE like any torch.distributed run)
    forced = bool(os.environ.get("FX_BENCH_FORCE_SHARDED"))
    if world > 1 or forced:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        if a.scaling == "strong":
            line = main_strong(a, dev, rank, world, backend, True)
        else:
            line = main_sharded(a, dev, rank, world, backend)
            if not os.environ.get("FX_BENCH_NO_STRONG"):
                # the metric as BASELINE.json words it (ONE 3 Gbp file on N GPUs), beside the weak line: a 3 Gbp file whatever --gbp says
                # for the weak pieces -- unless the run is a small one (tests), which keeps its size
                b = argparse.Namespace(**vars(a))
                b.gbp = 3.0 if a.gbp >= 3.0 else a.gbp
                st_ = strong_leg(b, dev, rank, world, backend, True)
                if rank == 0:
                    line["strong"] = st_
                if not a.no_c3:
                    fq_ = fastq_strong_leg(a, dev, rank, world, backend, True)      # configs[2]'s job over the same ranks
                    if rank == 0:
                        line["fastq_strong"] = fq_
        if rank == 0:
            _emit(line)
        dist.destroy_process_group()
        return
    if a.scaling == "strong":
        _emit(main_strong(a, dev, 0, 1, "none", False))
        return

    # ---------------- workload: the whole stream, resident in HBM
    total_bp = int(a.gbp * 1e9)
    plan = synth.fasta_plan(total_bp=total_bp, seed=20260612)      # (N > 1 never gets here: main_sharded / main_strong above)
    blob, flat, flat_start = synth.fasta_generate(plan, dev, keep_flat=a.full and not a.no_verify)
    q = synth.fasta_queries(plan, n=a.queries, seed=12345)
    ids, st, sp, strand = q
    qlen = int(sp[0] - st[0])
    job = shard.ShardedFasta(blob, int(plan["n_bytes"]), dev, 0, 1)
    if a.pmc_child:
        for _ in range(3):
            job.build()
        job.sync()
        return
    d_ids = torch.from_numpy(ids).to(dev); d_st = torch.from_numpy(st).to(dev); d_sp = torch.from_numpy(sp).to(dev)
    d_fl = torch.from_numpy((strand * 6).astype(np.uint8)).to(dev)               # '-' = reverse|complement
    d_off = torch.arange(a.queries, device=dev, dtype=torch.int64) * qlen
    d_out = torch.zeros(a.queries * qlen, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(a.queries, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def step():
        job.build_async()                                 # scan + tables, enqueued
        job.fetch_local(a.queries, d_ids, d_st, d_sp, d_fl, d_out, d_off, d_len)      # reads the record count on the device
        job.finish()                                      # the step's one host synchronisation: totals of the build
        job.sync()

    def build_only():
        ts = time.perf_counter()
        job.build()
        return time.perf_counter() - ts

    for _ in range(a.warmup):
        step()
    job.blob.prof_enable(2)                               # events around the dominant kernel only (k_span_scan; on in a plain run too: the same timed region)
    job.blob.prof_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    el = t1 - t0
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, job, d_out, d_len, a.queries, qlen)
    line = {
        "metric": "FASTA index build + 1M random 100bp subseq fetches, 3 Gbp plain FASTA per GPU (throughput of the whole step, stream resident in HBM)",
        "value": round(world * a.gbp / (el / a.steps), 3), "unit": "Gbp/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(el / a.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": "configs[1]: synthetic %.1f Gbp hg38-shaped plain FASTA per GPU (200 contigs, 60-col LF, soft-masked, N runs), "
                               "index build + %d random %d bp intervals (50%% '-' strand)" % (a.gbp, a.queries, qlen),
                   "file_bytes_per_gpu": int(plan["n_bytes"]), "parallelism": "one GPU, the whole stream resident in its HBM"},
    }
    if not a.full:
        _emit(line)
        return
    # the index build on its own (its own synchronisation), outside the timed region: the first half of the metric
    ti = sum(build_only() for _ in range(a.steps))
    prof = job.blob.prof_read()
    # per-kernel table from a separate, untimed pass (timing every kernel costs ~20 events per step)
    job.blob.prof_enable(1)
    job.blob.prof_reset()
    for _ in range(5):
        step()
    prof_all = job.blob.prof_read()
    job.blob.prof_enable(0)

    # ---------------- parity at full size (size-independent properties + analytic truth)
    verified = None
    if not a.no_verify:
        rows = job.local_rows()                           # records that START in this shard, as host arrays
        verified = bool(job.check_against_plan(plan, rows, None))
        exp = synth.expected_fetch(flat, flat_start, ids, st, qlen, strand, dev)
        verified = verified and bool((d_out.view(a.queries, qlen) == exp).all()) and bool((d_len == qlen).all())
        del exp
        if not verified:
            raise SystemExit("PARITY FAILURE at full size: refusing to report a speed-up")
    comp_ms = None
    full_index = None
    if not a.no_verify:
        # per-record composition (fasta.c:901-950) at full size vs torch.bincount of the un-wrapped bases
        # (extra information, outside the timed region: full_index is lazy in the reference too)
        nrec = len(plan["slen"])
        d_comp = torch.zeros((nrec, 128), dtype=torch.int64, device=dev)
        job.blob.fasta_comp_dev(d_comp.data_ptr())
        job.sync()
        tc = time.perf_counter()
        for _ in range(3):
            job.blob.fasta_comp_dev(d_comp.data_ptr())
        job.sync()
        comp_ms = (time.perf_counter() - tc) / 3 * 1e3
        okc = True
        for i in range(nrec):
            L = int(plan["slen"][i])
            if L:
                seg = flat[int(flat_start[i]):int(flat_start[i]) + L]
                okc &= bool((torch.bincount(seg.long(), minlength=128)[:128] == d_comp[i]).all())
        if not okc:
            raise SystemExit("PARITY FAILURE (composition) at full size")
        # index AND composition in one read of the stream: the counters ride on the scan (fx_fasta_build with
        # FX_BUILD_COMP: k_scan_comp, then k_comp_attribute + the edge runs), against build + composition pass above
        d_comp2 = torch.zeros_like(d_comp)
        job.blob.fasta_build(False, comp=True)
        job.blob.fasta_comp_dev(d_comp2.data_ptr())
        job.sync()
        tc = time.perf_counter()
        for _ in range(3):
            job.blob.fasta_build(False, comp=True)
            job.blob.fasta_comp_dev(d_comp2.data_ptr())
        job.sync()
        fused_ms = (time.perf_counter() - tc) / 3 * 1e3
        if not bool((d_comp2 == d_comp).all()):
            raise SystemExit("PARITY FAILURE (composition counted on the scan) at full size")
        tc = time.perf_counter()
        for _ in range(3):
            job.blob.fasta_build(False)
            job.blob.fasta_comp_dev(d_comp2.data_ptr())
        job.sync()
        two_ms = (time.perf_counter() - tc) / 3 * 1e3       # leaves the plain build behind
        full_index = {"index_and_composition_one_read_ms": round(fused_ms, 3), "index_then_composition_two_reads_ms": round(two_ms, 3),
                      "rows_equal": True}
        del d_comp2

    shard_bytes = job.n_bytes
    fetch_ms = sum(prof_all.get(k, (0.0, 1))[0] / max(prof_all.get(k, (0.0, 1))[1], 1) for k in ("k_fetch", "k_fetch_rest"))   # kernel time of one batch: the line-arithmetic kernel + the general one over its leftovers
    scan_ms, scan_n = prof.get("k_span_scan", (0.0, 0))
    scan_avg = scan_ms / max(scan_n, 1)
    achieved = shard_bytes / (scan_avg * 1e-3) / 1e9 if scan_avg > 0 else 0.0
    fetch_alg = 234 * a.queries                           # ~102 B read + 100 B written + 32 B descriptor / offset per query
    line.update({
        "index_build_s": round(ti / a.steps, 6),
        "fetch_M_per_s": round(world * a.queries / max(fetch_ms * 1e-3, 1e-9) / 1e6, 2),
        "parity_verified_full_size": verified,
        "composition_pass_ms": None if comp_ms is None else round(comp_ms, 3),
        "full_index": full_index,
        "kernels_ms_avg": {k: round(v[0] / v[1], 4) for k, v in prof_all.items()},
        "roofline": {"kernel": "fx::k_span_scan<0>", "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": shard.pmc_traffic(ROOT, shard_bytes),
                     "traffic_source": "profiles/pmc_k_span_scan.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes of this "
                                       "workload (counters cannot be read inside the run); null when the committed pass was on another size",
                     "algorithmic_bytes_per_launch": int(shard_bytes), "avg_launch_ms": round(scan_avg, 4)},
        "roofline_fetch": {"kernel": "fx::k_fetch_lines<4,1> (+ fx::k_fetch<true,4,16> over what it leaves over)", "bound": "hbm", "algorithmic_bytes_per_launch": fetch_alg,
                           "avg_launch_ms": round(fetch_ms, 4),
                           "frac": round(fetch_alg / max(fetch_ms * 1e-3, 1e-9) / 1e9 / HBM_PEAK_GBS, 4)},
    })
    _lap("generate + timed steps + parity at full size")
    if True:
        # release the device-resident copies before the file legs (the same bytes go to a file first)
        host = None
        tmpdir = tempfile.mkdtemp(prefix="fxbench")
        try:
            want_file = not (a.no_e2e and a.no_cpu_baseline and a.no_c4)
            if want_file:
                host = blob[:int(plan["n_bytes"])].cpu().numpy()
            del job, blob, flat, d_out, d_ids, d_st, d_sp, d_fl, d_off, d_len
            torch.cuda.empty_cache()
            path = os.path.join(tmpdir, "c2.fa")
            gbuf = goffs = ours_rows = None
            if want_file:
                host.tofile(path)
            line["device_memory_settled_after_s"] = _settle_device_memory(dev)     # (the timed opens below must not wait for the driver to take torch's tensors down)
            if not a.no_e2e:
                e2e = {}
                gbuf, goffs, ours_rows = e2e_fasta(path, plan, q, e2e)
                line["e2e"] = e2e
            _lap("e2e from a file")
            if not a.no_cpu_baseline:
                cb = {}
                if ours_rows is None:
                    import pyfastx_amd as fx
                    fx.Fasta(path)
                    ours_rows = _tables(path + ".fxi", ("seq", "stat"))
                if not cpu_fasta(path, plan, q, cb, gbuf, goffs, ours_rows):
                    cpu_fasta_port(host, q, cb)
                cpu_s = cb["index_s"] + cb["fetch_s"]
                cb["value"] = round(a.gbp / cpu_s, 4)
                cb["unit"] = "Gbp/s"
                cb["cpu"] = "%d logical cores on the box, 1 used (reference is single-threaded)" % (os.cpu_count() or 0)
                line["cpu_baseline"] = cb
                if cb.get("rows_equal_gpu") is False or cb.get("fetch_bytes_equal_gpu") is False:
                    raise SystemExit("PARITY FAILURE against the reference at full size: refusing to report a speed-up")
                if "e2e" in line:
                    e = line["e2e"]
                    e["rows_equal_reference"] = cb.get("rows_equal_gpu")
                    e["fetch_bytes_equal_reference"] = cb.get("fetch_bytes_equal_gpu")
                    gpu_s = e["fxi_durable_s"] + e["fetch_many_1M_host_to_host_s"]
                    e["gpu_total_s"] = round(gpu_s, 4)
                    e["cpu_total_s"] = round(cpu_s, 3)
                    e["index_speedup_vs_cpu"] = round(cb["index_s"] / e["fxi_durable_s"], 1)
                    e["fetch_speedup_vs_cpu"] = round(cb["fetch_s"] / e["fetch_many_1M_host_to_host_s"], 1)
                    line["speedup_vs_cpu"] = round(cpu_s / gpu_s, 1)          # like for like: file -> .fxi + host -> host answers
                    line["speedup_definition"] = "(cpu index_s + fetch_s) / (e2e fxi_durable_s + fetch_many_1M_host_to_host_s), same file, same host"
                line["hbm_resident_step_vs_cpu_file_run"] = round(line["value"] / cb["value"], 1)   # NOT like for like: kept for continuity with round 1
            _lap("cpu_baseline (reference on the whole file)")
            plain_digest = None
            if gbuf is not None:
                import hashlib
                plain_digest = (hashlib.blake2b(gbuf.tobytes(), digest_size=16).hexdigest(), hashlib.blake2b(np.asarray(goffs).tobytes(), digest_size=16).hexdigest())
            del gbuf
            if not a.no_pmc and want_file:
                # the dominant kernel's HBM traffic from the counters, now: the file is still there and the device is idle
                torch.cuda.empty_cache()
                tr, src = live_pmc_traffic(a, shard_bytes, path)
                if tr is not None:
                    line["roofline"]["traffic"], line["roofline"]["traffic_source"] = tr, src
                else:
                    line["roofline"]["traffic_source"] += "; a live measurement was tried and failed: " + src
                if "FETCH_SIZE" in _FETCH_PMC and "WRITE_SIZE" in _FETCH_PMC:
                    # FETCH_SIZE tallies every request to memory at 64 bytes and every request fetches 128 -- streams AND gathers
                    # (profiles/r06_gathercal.txt: 10^6 random aligned 128-byte lines = 128 MB known, 64 MB reported; 10^6 random
                    # 64-byte half lines: the same 128 MB fetched) -- so the reads are FETCH_SIZE x 2 here as for the scan kernel
                    rf = line["roofline_fetch"]
                    rd, wr = int(_FETCH_PMC["FETCH_SIZE"] * 1024 * 2), int(_FETCH_PMC["WRITE_SIZE"] * 1024)
                    rf["traffic"] = rd + wr
                    rf["calibration"] = "profiles/r06_gathercal.txt (tools/gathercal.hip under --pmc FETCH_SIZE: factor 2.0 for a stream, for aligned 128-byte lines and for 64-byte half lines; 1.93 for unaligned 100-byte spans counted in 128-byte blocks)"
                    rf["lines_of_128_bytes_fetched_per_query"] = round(rd / a.queries / 128.0, 2)
                    rf["traffic_source"] = ("the same two rocprofv3 passes, rows of k_fetch_lines (3 launches of the run's own %d queries): FETCH_SIZE %.0f KiB x 2 + WRITE_SIZE %.0f KiB "
                                            "per launch = %.2f x the algorithmic bytes; %.0f B fetched per query = %.2f lines of 128 B: the interval's own 1.8 lines (100 bases at a random "
                                            "offset of a 61-byte-per-line record), its descriptor, its row of the record table; the kernel moves %.1f TB/s of lines to deliver its answers"
                                            % (a.queries, _FETCH_PMC["FETCH_SIZE"], _FETCH_PMC["WRITE_SIZE"], (rd + wr) / max(rf["algorithmic_bytes_per_launch"], 1),
                                               rd / a.queries, rd / a.queries / 128.0, (rd + wr) / max(rf["avg_launch_ms"] * 1e-3, 1e-12) / 1e12))
                    rf["frac_of_measured_traffic"] = round((rd + wr) / max(rf["avg_launch_ms"] * 1e-3, 1e-12) / 1e9 / HBM_PEAK_GBS, 4)
                a.no_pmc = True
            _rm(path)
            _lap("pmc passes")
            if not a.no_c4:
                line["c4"] = leg_c4(a, host, plan, q, tmpdir, plain_digest)
            del host
            _lap("c4")
            if not a.no_c3:
                line["c3"] = leg_c3(a, dev, tmpdir)
            _lap("c3")
        finally:
            shutil.rmtree(tmpdir, ignore_errors=True)
    if not a.no_pmc:
        # the dominant kernel's HBM traffic from the counters, now (the device is idle: everything above is done)
        torch.cuda.empty_cache()
        tr, src = live_pmc_traffic(a, shard_bytes)
        if tr is not None:
            line["roofline"]["traffic"], line["roofline"]["traffic_source"] = tr, src
        else:
            line["roofline"]["traffic_source"] += "; a live measurement was tried and failed: " + src
    line["bench_wall_s"] = dict(_LAPS)
    _emit(line)


if __name__ == "__main__":
    main()
