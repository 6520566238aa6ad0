"""The definition of Fastq.trim / Fastq.records in plain Python (helper of test_fastq_trim_host.py and
test_gpu_fastq_trim.py; the contract of fx_fastq_trim and fx_fastq_format_alloc in include/fxgpu.h)."""
import numpy as np


def trim_truth(s, q, p=33, clip_front=0, clip_tail=0, adapter=None, min_overlap=3, err=(1, 10),
               front_qual=None, window=None, tail_qual=None):      # s, q: uint8 arrays; window = (w, num, den)
    L = len(s); d = q.astype(np.int64) - p
    a = min(clip_front, L); b = max(a, L - clip_tail)               # 1 fixed clip
    if adapter is not None:                                          # 2 3' adapter, Hamming, prefix of the adapter may hang off the end
        A = np.frombuffer(adapter, dtype=np.uint8)                   #   1..64 letters of A C G T N; N matches any byte
        for j in range(a, b):
            m = min(len(A), b - j)
            if m < min_overlap: break
            mm = int(((s[j:j+m] != A[:m]) & (A[:m] != ord('N'))).sum())   # read bytes as they are: lower case, N, IUPAC mismatch
            if mm * err[1] <= err[0] * m: b = j; break              #   the FIRST j that matches
    if front_qual is not None:                                       # 3 5' end
        while a < b and d[a] < front_qual: a += 1
    if window is not None and b > a:                                 # 4 sliding window, mean below num/den
        w, num, den = window; we = min(w, b - a)
        for j in range(a, b - we + 1):
            if int(d[j:j+we].sum()) * den < num * we: b = j; break  #   cut at the first failing window's start
    if tail_qual is not None:                                        # 5 3' end
        while b > a and d[b-1] < tail_qual: b -= 1
    return a, b


def truth_kwargs(args):
    """trim.trim_args(...) -> the keyword arguments of trim_truth."""
    return dict(clip_front=args["clip_front"], clip_tail=args["clip_tail"], adapter=args["adapter"], min_overlap=args["min_overlap"],
                err=args["err"], front_qual=args["front_qual"], window=args["window"], tail_qual=args["tail_qual"])


def record(header, s, q, a, b):
    """One formatted record: header (bytes, begins with '@', no trailing '\\r'), s / q uint8 arrays."""
    return header + b"\n" + s[a:b].tobytes() + b"\n+\n" + q[a:b].tobytes() + b"\n"


def trim_truth_fast(s, q, p=33, clip_front=0, clip_tail=0, adapter=None, min_overlap=3, err=(1, 10),
                    front_qual=None, window=None, tail_qual=None):
    """trim_truth with the loops over positions turned into numpy expressions, for files of 10^5 reads;
    test_fastq_trim_host.py holds it to trim_truth on random reads."""
    L = len(s); d = q.astype(np.int64) - p
    a = min(clip_front, L); b = max(a, L - clip_tail)
    if adapter is not None and b > a:
        A = np.frombuffer(adapter, dtype=np.uint8); n = len(A)
        win = np.lib.stride_tricks.sliding_window_view(np.concatenate([s[a:b], np.zeros(n, dtype=np.uint8)]), n)[:b - a]
        m = np.minimum(n, b - np.arange(a, b))
        mm = ((win != A) & (A != ord('N')) & (np.arange(n)[None, :] < m[:, None])).sum(1)
        ok = np.nonzero((m >= min_overlap) & (mm * err[1] <= err[0] * m))[0]
        if len(ok): b = a + int(ok[0])
    if front_qual is not None:
        ge = np.nonzero(d[a:b] >= front_qual)[0]
        a = a + int(ge[0]) if len(ge) else b
    if window is not None and b > a:
        w, num, den = window; we = min(w, b - a)
        cs = np.concatenate([[0], np.cumsum(d[a:b])])
        bad = np.nonzero((cs[we:] - cs[:len(cs) - we]) * den < num * we)[0]
        if len(bad): b = a + int(bad[0])
    if tail_qual is not None:
        ge = np.nonzero(d[a:b] >= tail_qual)[0]
        b = a + int(ge[-1]) + 1 if len(ge) else a
    return a, b
