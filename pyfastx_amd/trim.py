"""FASTQ read trimming and trimmed-record output on the resident stream (extension; the reference trims nothing and writes
verbatim copies only, read.c:124-150).

Fastq.trim / records / write check their arguments here and hand them to fx_fastq_trim and fx_fastq_format_alloc
(csrc/fx_fastq_trim.hpp).  Everything is integer: the error rate of the adapter match and the mean of the sliding window
become ratios of two integers (qc.as_ratio) before they reach the device."""
import numpy as np

from . import _lib, qc

MAX_ADAPTER = 64
LETTERS = frozenset(b"ACGTN")


def _int(v, what, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int" % what)
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s %d outside %d..%s" % (what, v, lo, "" if hi is None else hi))
    return v


def check_adapter(adapter):
    """str or bytes -> upper-case bytes, 1..64 letters of A C G T N."""
    if isinstance(adapter, str):
        try:
            adapter = adapter.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("adapter letters must be A C G T N")
    if not isinstance(adapter, (bytes, bytearray)):
        raise ValueError("adapter must be a str or bytes")
    a = bytes(adapter).upper()
    if not 1 <= len(a) <= MAX_ADAPTER:
        raise ValueError("adapter length %d outside 1..%d" % (len(a), MAX_ADAPTER))
    if not set(a) <= LETTERS:
        raise ValueError("adapter letters must be A C G T N")
    return a


def trim_args(clip_front=0, clip_tail=0, adapter=None, min_overlap=3, max_error_rate=0.1, front_qual=None, window=None,
              tail_qual=None):
    """The steps of Fastq.trim as fx_fastq_trim takes them -> dict(clip_front, clip_tail, adapter, min_overlap, err,
    front_qual, window, tail_qual): adapter None or upper-case bytes, err = (num, den), window None or (length, num, den),
    a threshold None (not asked) or 0..255.  ValueError for anything else."""
    out = {"clip_front": _int(clip_front, "clip_front", 0), "clip_tail": _int(clip_tail, "clip_tail", 0),
           "adapter": None, "min_overlap": 1, "err": (0, 1), "window": None,
           "front_qual": None if front_qual is None else _int(front_qual, "front_qual", 0, 255),
           "tail_qual": None if tail_qual is None else _int(tail_qual, "tail_qual", 0, 255)}
    if adapter is not None:
        a = check_adapter(adapter)
        out["adapter"] = a
        out["min_overlap"] = _int(min_overlap, "min_overlap", 1, len(a))
        out["err"] = qc.as_ratio(max_error_rate, "max_error_rate")
    if window is not None:
        try:
            length, mean = window
        except (TypeError, ValueError):
            raise ValueError("window must be a pair (length, mean quality)")
        num, den = qc.as_ratio(mean, "window mean")
        out["window"] = (_int(length, "window length", 1, 2**31 - 1), num, den)
    return out


def check_ids(ids, n_reads):
    """None, or a one-dimensional int64 array of ids inside the table (IndexError otherwise)."""
    if ids is None:
        return None
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if ids.ndim != 1:
        raise ValueError("ids must be one-dimensional")
    if ids.size and (ids.min() < 0 or ids.max() >= n_reads):
        raise IndexError("index out of range")
    return ids


def check_intervals(start, end, n):
    """start / end as Fastq.trim returned them for the same queries: both None, or two int64 arrays of n rows."""
    if start is None and end is None:
        return None, None
    if start is None or end is None:
        raise ValueError("start and end come together")
    start, end = np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
    if start.ndim != 1 or start.shape != end.shape or start.size != n:
        raise ValueError("start and end must have one row per query (%d)" % n)
    return start, end


def trim_blob(blob, n_reads, ids, phred, args):
    ids = check_ids(ids, n_reads)
    start, end = blob.fastq_trim(ids, phred=phred, **args)
    return {"start": start, "end": end}


def records_blob(blob, n_reads, ids, start, end, min_len, level=None):
    """-> (buffer, offsets, kept); with a BGZF level (bgzf.level_of): (stream, member offsets, offsets, kept)"""
    ids = check_ids(ids, n_reads)
    start, end = check_intervals(start, end, n_reads if ids is None else ids.size)
    min_len = _int(min_len, "min_len", 0)
    try:
        if level is not None:
            return blob.fastq_format_alloc(ids, start, end, min_len, level=level)
        return blob.fastq_format_alloc(ids, start, end, min_len)
    except _lib.FxError as e:
        raise _lib.outside(e)


def batches(tab, ids, n_reads, batch_bytes):
    """Consecutive runs [lo, hi) of the queries whose upper bound dlen + 2 * rlen + 6 per read fits batch_bytes (a single
    read larger than that is a batch of its own)."""
    batch_bytes = _int(batch_bytes, "batch_bytes", 1)
    sel = slice(None) if ids is None else ids
    ub = tab["dlen"][sel].astype(np.int64) + 2 * tab["rlen"][sel].astype(np.int64) + 6
    n = n_reads if ids is None else ids.size
    cum = np.cumsum(ub)
    lo = 0
    while lo < n:
        base = int(cum[lo - 1]) if lo else 0
        hi = int(np.searchsorted(cum, base + batch_bytes, side="right"))
        hi = max(hi, lo + 1)
        yield lo, min(hi, n)
        lo = min(hi, n)
