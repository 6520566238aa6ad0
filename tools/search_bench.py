"""Motif search on the C2-shaped synthetic genome (synth.fasta_plan / fasta_generate, 3.05 GB): kernel ms (fx_prof_*),
end-to-end ms of search_blob / count_blob (the calls under Fasta.search_all / search_counts), hit counts, and the fraction
of the HBM floor (one read of the stream at 6.5 TB/s).  The counts are checked against a torch count over the flat
sequence that fasta_generate returns.  Prints one JSON line.

    python tools/search_bench.py [--gbp 3.0] [--reps 3] [--out profiles/search_c2.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.5
CASES = [("GAATTC", "both", False, "all"), ("ACGRYTNNCAGGRYATNNGC", "both", True, "all"), ("A", "both", False, "counts")]
BASES = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
         "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def flat_count(torch, flat, cflat, rec_end, p, deg):
    """windows of the flat sequence that match p and lie inside one record (torch on the device: a checker only).
    cflat: the IUPAC base-set code of every flat byte (0: no IUPAC letter)."""
    L = len(p)
    N = flat.numel() - L + 1
    m = torch.ones(N, dtype=torch.bool, device=flat.device)
    for j, ch in enumerate(p):
        if deg:
            cw = cflat[j:j + N]
            m &= (cw != 0) & ((cw & (15 & ~CODE[ord(ch)])) == 0)
        else:
            m &= flat[j:j + N] == ord(ch)
    for d in range(1, L):                          # starts whose window runs past the end of their record
        pos = rec_end - d
        m[pos[(pos >= 0) & (pos < N)]] = False
    return int(m.sum())


CODE = [0] * 256
for _k, _v in BASES.items():
    CODE[ord(_k)] = CODE[ord(_k.lower())] = sum({"A": 1, "C": 2, "G": 4, "T": 8}[b] for b in _v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyfastx_amd import _lib, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=int(a.gbp * 1e9), seed=20260612)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    nb = int(plan["n_bytes"])
    b = _lib.Blob.from_device(blob_t.data_ptr(), nb, device=0, keepalive=blob_t)
    b.fasta_build()
    rec_end = torch.from_numpy(flat_start + plan["slen"]).to(dev)
    lut = torch.tensor(CODE, dtype=torch.uint8, device=dev)
    cflat = torch.empty_like(flat_t)
    for c0 in range(0, flat_t.numel(), 1 << 28):
        cflat[c0:c0 + (1 << 28)] = lut[flat_t[c0:c0 + (1 << 28)].long()]
    floor_ms = nb / (HBM_TBS * 1e12) * 1e3
    out = {"tool": "search_bench", "n_bytes": nb, "n_records": len(plan["slen"]), "hbm_floor_ms": round(floor_ms, 4), "cases": []}
    for p, strand, deg, kind in CASES:
        rp = search.iupac_revcomp(p) if deg else _lib.revcomp_bytes(p.encode()).decode()
        want = (flat_count(torch, flat_t, cflat, rec_end, p, deg), flat_count(torch, flat_t, cflat, rec_end, rp, deg))
        run = (lambda: search.search_blob(b, p, strand, deg, max_hits=10**9)) if kind == "all" else \
            (lambda: search.count_blob(b, p, strand, deg))
        run()                                                       # warm-up (allocations)
        best, kms = 1e30, {}
        for _ in range(a.reps):
            b.prof_enable(1)
            b.prof_reset()
            t0 = time.perf_counter()
            r = run()
            dt = (time.perf_counter() - t0) * 1e3
            if dt < best:
                best = dt
                pr = b.prof_read()
                kms = {k: round(pr[k][0], 4) for k in ("k_search_count", "k_search_scan", "k_search_emit") if k in pr}
            b.prof_enable(0)
        if kind == "all":
            got = (int((r.strands == ord("+")).sum()), int((r.strands == ord("-")).sum()))
        else:
            got = (int(r[:, 0].sum()), int(r[:, 1].sum()))
        kern = sum(kms.values())
        out["cases"].append({"pattern": p, "strand": strand, "degenerate": deg, "call": "search_all" if kind == "all" else "search_counts",
                             "hits_plus": got[0], "hits_minus": got[1], "flat_count": list(want), "agree": got == want,
                             "kernel_ms": kms, "kernels_total_ms": round(kern, 4), "e2e_ms": round(best, 3),
                             "count_pass_fraction_of_hbm_floor": round(floor_ms / kms["k_search_count"], 3) if kms.get("k_search_count") else None})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
