"""The definition of Fastq.demux in plain Python, slot by slot (helper of test_demux_host.py and test_gpu_fastq_demux.py; the
contract of fx_fastq_demux in include/fxgpu.h), and demux_truth_fast, the same in numpy for sheets of thousands of samples;
test_demux_host.py holds the fast one to the slow one on random inputs."""
import numpy as np

NONE, AMBIGUOUS = -1, -2
SEQ5, SEQ3, HEADER = 0, 1, 2
SOURCES = {"5p": SEQ5, "3p": SEQ3, "header": HEADER}
ABSENT = None


def cut_header(line):
    """The header line as it stands in the file (from '@' up to, not including, the newline) -> H: one trailing '\\r' off."""
    return line[:-1] if line.endswith(b"\r") else line


def window(H, s, src, off, ln):
    """The ln slots of a segment: each a byte (int) or ABSENT.  H: bytes (cut_header), s: bytes of the read."""
    L = len(s)
    out = []
    if src == SEQ5:
        for j in range(ln):
            out.append(s[off + j] if off + j < L else ABSENT)
        return out
    if src == SEQ3:
        for j in range(ln):
            p = L - off - ln + j
            out.append(s[p] if 0 <= p < L else ABSENT)
        return out
    assert src == HEADER and off in (0, 1)
    k = H.rfind(b":")
    if k < 0:                                                 # no ':' at all
        return [ABSENT] * ln
    F = H[k + 1:]                                             # the longest suffix without ':'
    if len(F) > 65:
        return [ABSENT] * ln
    plus = F.find(b"+")
    if off == 0:
        part = F if plus < 0 else F[:plus]
    else:
        part = b"" if plus < 0 else F[plus + 1:]
    for j in range(ln):
        out.append(part[j] if j < len(part) else ABSENT)      # bytes of the part beyond ln are ignored
    return out


def distance(win, barcode):
    d = 0
    for j, c in enumerate(barcode):
        if c == ord("N"):
            continue
        if win[j] is ABSENT or win[j] != c:
            d += 1
    return d


def decide(totals, margin):
    """totals: [(t, sample index)] of the passing samples -> (sample, dist, second)."""
    if not totals:
        return NONE, -1, -1
    totals = sorted(totals)
    if len(totals) == 1:
        return totals[0][1], totals[0][0], -1
    t1, t2 = totals[0][0], totals[1][0]
    if t2 - t1 >= margin:
        return totals[0][1], t1, t2
    return AMBIGUOUS, t1, t2


def demux_read(H, s, segs, sheet, margin=1):
    """One read.  segs: [(src, off, len, mm)] (1 or 2); sheet: per sample a tuple of bytes, one per segment."""
    wins = [window(H, s, src, off, ln) for src, off, ln, _ in segs]
    totals = []
    for k, row in enumerate(sheet):
        d = [distance(wins[g], row[g]) for g in range(len(segs))]
        if all(d[g] <= segs[g][3] for g in range(len(segs))):
            totals.append((sum(d), k))
    return decide(totals, margin)


def demux_truth(reads, segs, sheet, margin=1):
    """reads: [(H, s)] -> sample, dist, second (int32 arrays)."""
    rows = [demux_read(H, s, segs, sheet, margin) for H, s in reads]
    return tuple(np.array([r[c] for r in rows], dtype=np.int32).reshape(len(rows)) for c in range(3))


def demux_truth_fast(reads, segs, sheet, margin=1, chunk=256):
    """demux_truth with the loop over the samples turned into numpy expressions.  The windows still come from window()."""
    n, ns = len(reads), len(sheet)
    big = 1 << 20
    W, B = [], []
    for g, (src, off, ln, _) in enumerate(segs):
        w = np.full((n, ln), -1, dtype=np.int16)
        for i, (H, s) in enumerate(reads):
            w[i] = [-1 if x is ABSENT else x for x in window(H, s, src, off, ln)]
        W.append(w)
        B.append(np.array([list(row[g]) for row in sheet], dtype=np.int16).reshape(ns, ln))
    sample, dist, second = (np.empty(n, dtype=np.int32) for _ in range(3))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        ok = np.ones((hi - lo, ns), dtype=bool)
        t = np.zeros((hi - lo, ns), dtype=np.int64)
        for g, (_, _, _, mm) in enumerate(segs):
            d = ((W[g][lo:hi, None, :] != B[g][None, :, :]) & (B[g][None, :, :] != ord("N"))).sum(2)
            ok &= d <= mm
            t += d
        t = np.where(ok, t, big)
        rows = np.arange(hi - lo)
        i1 = t.argmin(1)
        t1 = t[rows, i1]
        t[rows, i1] = big + 1
        t2 = t.min(1)
        none, one = t1 >= big, t2 >= big
        amb = ~none & ~one & (t2 - t1 < margin)
        sample[lo:hi] = np.where(none, NONE, np.where(amb, AMBIGUOUS, i1))
        dist[lo:hi] = np.where(none, -1, t1)
        second[lo:hi] = np.where(none | one, -1, t2)
    return sample, dist, second


def segments(args):
    """demux.demux_args(...) -> (segs, sheet) as demux_truth takes them."""
    segs = list(zip(args["src"], args["off"], args["length"], args["mm"]))
    sheet = []
    for row in args["barcodes"]:
        b, at = bytes(row.tobytes()), 0
        parts = []
        for ln in args["length"]:
            parts.append(b[at:at + ln])
            at += ln
        sheet.append(tuple(parts))
    return segs, sheet


def parse_fastq(raw):
    """A well-formed four-line FASTQ on the host -> [(H, s)]."""
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [(cut_header(lines[i]), cut_header(lines[i + 1])) for i in range(0, len(lines), 4)]


def bins_of(sample, n_samples):
    """The stable grouping: order (query positions sorted by (bin, position)) and bin_off (n_samples + 3 entries)."""
    b = np.where(sample >= 0, sample, np.where(sample == NONE, n_samples, n_samples + 1)).astype(np.int64)
    order = np.argsort(b, kind="stable").astype(np.int64)
    counts = np.bincount(b, minlength=n_samples + 2).astype(np.int64)
    return order, np.concatenate(([0], np.cumsum(counts))).astype(np.int64), counts
