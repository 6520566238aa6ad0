"""FASTA records written back out from the resident stream (extension; the reference writes verbatim copies only,
sequence.c:314-335, and `pyfastx subseq` one interval at a time).

Fasta.records / write check their arguments here and hand them to fx_fasta_format_alloc (csrc/fx_fasta_format.hpp): whole
records or intervals, re-wrapped at a line width, upper-cased, masked, reverse-complemented and laid out back to back on the
device.  What stays on the host is small: names to ids, the strand flags, the `name:start-stop` headers of intervals and
the merge of the mask rows."""
import numpy as np

from . import _lib

MASK_MODES = {"none": 0, "soft": 1, "hard": 2, "upper": 3}
_F_UP, _F_REV, _F_COMP = 1, 2, 4


def tile():
    """Bytes of the output one workgroup of the emit kernel owns."""
    return int(_lib.lib().fx_fasta_format_tile())


def _int(v, what, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int" % what)
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s %d outside %d..%s" % (what, v, lo, "" if hi is None else hi))
    return v


def check_width(width):
    return _int(width, "width", 0)


def check_mask_mode(mask_mode):
    if not isinstance(mask_mode, str) or mask_mode not in MASK_MODES:
        raise ValueError("mask_mode must be one of 'soft', 'hard', 'upper', 'none'")
    return MASK_MODES[mask_mode]


def check_mask_char(mask_char):
    """One byte: a str or bytes of length 1 -> its value."""
    if isinstance(mask_char, str):
        try:
            mask_char = mask_char.encode("latin-1")
        except UnicodeEncodeError:
            raise ValueError("mask_char must be one byte")
    if not isinstance(mask_char, (bytes, bytearray)) or len(mask_char) != 1:
        raise ValueError("mask_char must be one byte")
    return mask_char[0]


def merge_intervals(ids, starts, stops):
    """Rows (id, start, stop) in any order -> the same set of positions as rows sorted by (id, start) in which no two
    rows of a record overlap or touch; empty rows are dropped.  int64 arrays."""
    ids, starts, stops = (np.ascontiguousarray(x, dtype=np.int64).ravel() for x in (ids, starts, stops))
    if not (ids.size == starts.size == stops.size):
        raise ValueError("mask ids, starts and stops differ in length")
    keep = stops > starts
    ids, starts, stops = ids[keep], starts[keep], stops[keep]
    if ids.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    order = np.lexsort((starts, ids))
    ids, starts, stops = ids[order], starts[order], stops[order]
    # the furthest stop seen so far within the record: ids are ascending, so a running maximum of (id, stop) as one key
    span = int(max(int(stops.max()), int(starts.max()), 0)) + 1
    if int(ids.max()) < (1 << 62) // span and int(ids.min()) >= 0 and int(starts.min()) >= 0:
        reach = np.maximum.accumulate(ids * span + stops) - ids * span
    else:                                                  # (coordinates the key cannot carry: the same per record)
        reach = stops.copy()
        for lo, hi in zip(*_runs(ids)):
            reach[lo:hi] = np.maximum.accumulate(stops[lo:hi])
    head = np.ones(ids.size, dtype=bool)                   # a row opens a new interval unless it begins within the reach of those before it
    head[1:] = (ids[1:] != ids[:-1]) | (starts[1:] > reach[:-1])
    first = np.flatnonzero(head)
    last = np.append(first[1:], ids.size) - 1
    return ids[first], starts[first], reach[last]


def _runs(ids):
    cut = np.flatnonzero(np.diff(ids)) + 1
    return np.concatenate(([0], cut)), np.concatenate((cut, [ids.size]))


def mask_rows(mask):
    """An object with .ids / .starts / .stops or a 3-tuple of arrays -> merged rows (merge_intervals); None -> None."""
    if mask is None:
        return None
    if all(hasattr(mask, k) for k in ("ids", "starts", "stops")):
        cols = (mask.ids, mask.starts, mask.stops)
    else:
        try:
            cols = tuple(mask)
        except TypeError:
            cols = ()
        if len(cols) != 3:
            raise ValueError("mask must have .ids / .starts / .stops or be a 3-tuple of arrays")
    return merge_intervals(*cols)


def strand_flags(strand, n):
    """None, '+', '-' or one of '+' / '-' (0 / 1) per row -> bool array of n rows: the row is on the minus strand."""
    if strand is None:
        return np.zeros(n, dtype=bool)
    if isinstance(strand, str):
        if strand not in ("+", "-"):
            raise ValueError("strand must be '+', '-' or one of them per row")
        return np.full(n, strand == "-", dtype=bool)
    if isinstance(strand, np.ndarray) and strand.dtype.kind in "iub":
        neg = (strand != 0) & (strand != ord("+"))
    else:
        strand = list(strand)
        for s in strand:
            if s not in ("+", "-", 0, 1, True, False):
                raise ValueError("strand must be '+', '-' or one of them per row")
        neg = np.array([s in ("-", 1, True) for s in strand], dtype=bool)
    if neg.size != n:
        raise ValueError("strand must have one entry per row (%d)" % n)
    return neg


def check_intervals(starts, stops, n):
    if starts is None and stops is None:
        return None, None
    if starts is None or stops is None:
        raise ValueError("starts and stops come together")
    starts, stops = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(stops, dtype=np.int64)
    if starts.ndim != 1 or starts.shape != stops.shape or starts.size != n:
        raise ValueError("starts and stops must have one row per query (%d)" % n)
    return starts, stops


def auto_headers(names, starts, stops, neg):
    """The `pyfastx subseq` form name:start+1-stop of every interval, "(-)" appended on the minus strand -> list of bytes."""
    out = []
    for k, name in enumerate(names):
        h = "%s:%d-%d" % (name, int(starts[k]) + 1, int(stops[k]))
        if neg[k]:
            h += "(-)"
        out.append(h.encode("utf-8", "surrogateescape"))
    return out


def pack_headers(headers, n):
    """A sequence of str / bytes, one per row -> (uint8 bytes, int64 offsets[n + 1])."""
    if isinstance(headers, (str, bytes, bytearray)):
        raise ValueError("headers must be 'auto' or a sequence with one str / bytes per row")
    rows = []
    for h in headers:
        if isinstance(h, str):
            h = h.encode("utf-8", "surrogateescape")
        elif not isinstance(h, (bytes, bytearray)):
            raise ValueError("a header must be a str or bytes")
        rows.append(bytes(h))
    if len(rows) != n:
        raise ValueError("headers must have one entry per row (%d)" % n)
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    blob = b"".join(rows)
    return np.frombuffer(blob if blob else b"\0", dtype=np.uint8), offs


def size_bound(hdr_len, letters, width):
    """Upper bound of a record's bytes: header + 2 + letters + lines (int64 arrays or ints)."""
    letters = np.asarray(letters, dtype=np.int64)
    lines = np.where(letters > 0, 1, 0) if width == 0 else (letters + width - 1) // width
    return np.asarray(hdr_len, dtype=np.int64) + 2 + letters + lines


def batches(bound, batch_bytes):
    """Consecutive runs [lo, hi) of the queries whose size bounds fit batch_bytes together (a single query larger than
    that is a batch of its own)."""
    batch_bytes = _int(batch_bytes, "batch_bytes", 1)
    n = int(bound.size)
    cum = np.cumsum(bound)
    lo = 0
    while lo < n:
        base = int(cum[lo - 1]) if lo else 0
        hi = int(np.searchsorted(cum, base + batch_bytes, side="right"))
        hi = min(max(hi, lo + 1), n)
        yield lo, hi
        lo = hi


def slice_mask(rows, ids):
    """The merged rows whose record is among `ids` (fewer rows for the device to search; the order is kept)."""
    if rows is None or rows[0].size == 0:
        return rows
    keep = np.isin(rows[0], ids)
    return (rows[0][keep], rows[1][keep], rows[2][keep]) if not keep.all() else rows


def bad_query(e, ids, n_seq, base=0):
    """The exception for the FxError of fx_fasta_format_alloc: FX_ERANGE that names a query becomes the IndexError /
    ValueError of fetch_many with the row (base: the row of the batch's first query), anything else is `e` itself."""
    k = getattr(e, "first_bad", -1)
    if e.code != _lib.FX_ERANGE or k < 0:
        return e
    if ids is not None and (ids[k] < 0 or ids[k] >= n_seq):
        err = IndexError("index out of range (query %d)" % (base + k))
    else:
        err = ValueError("interval outside the sequence (query %d)" % (base + k))
    err.first_bad = base + k
    return err
