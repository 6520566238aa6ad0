"""Low-complexity sequence by the DUST triplet score on the resident streams: the windowed mask of a FASTA table
(Fasta.low_complexity) and the per-read columns of a FASTQ table (Fastq.complexity).  Extensions: the reference has no such
call.  The argument rules and the derived columns live here; the scoring is fx_fasta_low_complexity / fx_fastq_complexity
(csrc/fx_dust.hpp), and include/fxgpu.h holds the definition in full.

This is the WINDOWED form of DUST: every window of `window` letters whose score passes the threshold is masked as a whole, so
a repeat takes flanks of up to window minus about 23 letters with it at window=64, threshold=20; a smaller window is the
finer knob.  sdust's perfect intervals are not implemented and parity with sdust / dustmasker is not claimed."""
import numpy as np

from . import _lib, annot, fasta_out, trim

MIN_WINDOW, MAX_WINDOW, MAX_THRESHOLD, MAX_WINDOWS = 4, 64, 1000, 4


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (what, v))
    return int(v)


def check_mask(window=64, threshold=20, min_len=1, max_rows=10**8):
    """-> (tuple of window lengths, threshold, min_len, max_rows).  window: one length of 4..64 or a tuple of 1 to 4 of them;
    threshold: 1..1000, in tenths (20 is a score of 2.0); min_len >= 1; max_rows >= 0.  ValueError otherwise."""
    if isinstance(window, (tuple, list)):
        if not 1 <= len(window) <= MAX_WINDOWS:
            raise ValueError("window takes 1 to %d lengths, not %d" % (MAX_WINDOWS, len(window)))
        windows = tuple(_int(w, "window") for w in window)
    else:
        windows = (_int(window, "window"),)
    for w in windows:
        if not MIN_WINDOW <= w <= MAX_WINDOW:
            raise ValueError("window=%d outside %d..%d" % (w, MIN_WINDOW, MAX_WINDOW))
    threshold = _int(threshold, "threshold")
    if not 1 <= threshold <= MAX_THRESHOLD:
        raise ValueError("threshold=%d outside 1..%d (tenths: 20 is a score of 2.0)" % (threshold, MAX_THRESHOLD))
    min_len = _int(min_len, "min_len")
    if min_len < 1:
        raise ValueError("min_len=%d must be at least 1" % min_len)
    max_rows = _int(max_rows, "max_rows")
    if max_rows < 0:
        raise ValueError("max_rows must not be negative")
    return windows, threshold, min_len, max_rows


def mask_blob(blob, window=64, threshold=20, min_len=1, ids=None, max_rows=10**8, names=None):
    """annot.ClassRuns of the low-complexity intervals on a Blob whose FASTA table is resident; ids: ascending distinct record
    ids or None.  Several windows: one device call each, the rows joined (fasta_out.merge_intervals) before min_len; max_rows
    then bounds the rows of every call as well as the joined ones."""
    windows, threshold, min_len, max_rows = check_mask(window, threshold, min_len, max_rows)
    try:
        if len(windows) == 1:
            rec, a, b = blob.fasta_low_complexity(windows[0], threshold, min_len, ids, cap=max_rows)
            return annot.ClassRuns(rec, a, b, names)
        parts = [blob.fasta_low_complexity(w, threshold, 1, ids, cap=max_rows) for w in windows]
    except _lib.FxError as e:
        raise _lib.too_many(e, "intervals", "max_rows", max_rows)
    rec, a, b = fasta_out.merge_intervals(*(np.concatenate([p[c] for p in parts]) for c in range(3)))
    keep = b - a >= min_len
    rec, a, b = rec[keep], a[keep], b[keep]
    if rec.size > max_rows:
        raise ValueError("%d intervals, more than max_rows=%d" % (rec.size, max_rows))
    return annot.ClassRuns(rec, a, b, names)


def dust_score(dust_sum, n_triplets):
    """10 * dust_sum / (n_triplets - 1), 0 where n_triplets < 2: prinseq's scale (a homopolymer scores about 5 n, 7 is its
    usual cut), over the whole interval -- without prinseq's averaging over windows of 64."""
    s, n = np.asarray(dust_sum, dtype=np.float64), np.asarray(n_triplets, dtype=np.float64)
    out = np.zeros(n.shape, dtype=np.float64)
    np.divide(10.0 * s, n - 1.0, out=out, where=n >= 2)
    return out


def fastp_complexity(n_diff, length):
    """n_diff / (length - 1), 0 where length < 2: the fraction of letters that differ from the next one (fastp's measure)."""
    d, n = np.asarray(n_diff, dtype=np.float64), np.asarray(length, dtype=np.float64)
    out = np.zeros(n.shape, dtype=np.float64)
    np.divide(d, n - 1.0, out=out, where=n >= 2)
    return out


def columns(length, n_triplets, dust_sum, n_diff):
    """The dict Fastq.complexity returns: the four device columns and the two derived ones."""
    return {"length": length, "n_triplets": n_triplets, "dust_sum": dust_sum, "n_diff": n_diff,
            "dust": dust_score(dust_sum, n_triplets), "complexity": fastp_complexity(n_diff, length)}


def complexity_blob(blob, n_reads, ids=None, start=None, end=None):
    """The columns of seq[start:end] of the reads `ids`; ids, start and end by the rules of Fastq.kmer_counts.  A bad id or an
    interval outside its read: IndexError."""
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    try:
        return columns(*blob.fastq_complexity(ids, start, end))
    except _lib.FxError as e:
        if e.code == _lib.FX_ERANGE and getattr(e, "first_bad", -1) >= 0:
            raise IndexError("the interval of query %d lies outside its read" % e.first_bad)
        raise
