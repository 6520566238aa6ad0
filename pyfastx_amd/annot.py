"""Composition of regions and windows, and the maximal runs of a letter class, on the resident FASTA stream.

Fasta.region_stats replaces slicing and counting on the host, one interval at a time (Sequence.composition, gc_content and
gc_skew of fa[name][a:b], sequence.c:562-749); Fasta.window_stats and Fasta.class_runs are extensions.  The argument rules
and the result objects live here; the counting is fx_fasta_region_counts / fx_fasta_window_counts / fx_fasta_class_runs
(csrc/fx_annot.hpp) on the rank index of the table.

The text of a record is `fa[i].seq` as the file has it (uppercase= plays no part); coordinates are 0-based half-open, as
fetch_many and search_all use them.  Seven columns: A C G T N (either case), other (every other letter, U included: the
reference's gc_content counts A C G T only), masked (letters in a..z, overlapping the first six)."""
import numpy as np

from . import _lib

COLUMNS = ("A", "C", "G", "T", "N", "other", "masked")
KINDS = {"N": b"Nn", "masked": bytes(range(ord("a"), ord("z") + 1)), "unmasked": bytes(range(ord("A"), ord("Z") + 1))}


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(den.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


class RegionStats:
    """ids, starts, stops (int64[n]) and counts (int64[n, 7], columns A C G T N other masked) of n intervals; the derived
    figures are float64, nan where their denominator is 0."""

    columns = COLUMNS

    def __init__(self, ids, starts, stops, counts):
        self.ids, self.starts, self.stops = ids, starts, stops
        self.counts = np.asarray(counts).reshape(-1, len(COLUMNS))

    def __len__(self):
        return int(self.counts.shape[0])

    @property
    def length(self):
        """Letters of every interval (the first six columns sum to it)."""
        return self.counts[:, :6].sum(axis=1)

    @property
    def gc_content(self):
        """Percent, (G + C) / (A + C + G + T) * 100, as Sequence.gc_content."""
        c = self.counts
        return _ratio((c[:, 1] + c[:, 2]) * 100.0, c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3])

    @property
    def gc_skew(self):
        """(G - C) / (G + C), as Sequence.gc_skew."""
        c = self.counts
        return _ratio(c[:, 2] - c[:, 1], c[:, 2] + c[:, 1])

    @property
    def masked_fraction(self):
        return _ratio(self.counts[:, 6], self.length)


class ClassRuns:
    """ids, starts, stops (int64[n]) of the maximal runs of one letter class, ordered by (record, start)."""

    def __init__(self, ids, starts, stops, names=None):
        self.ids, self.starts, self.stops = ids, starts, stops
        self._names = names                                  # callable: record id -> name (write_bed)

    def __len__(self):
        return int(self.ids.size)

    @property
    def lengths(self):
        return self.stops - self.starts

    def write_bed(self, path):
        """name<TAB>start<TAB>stop rows, one per run, with the names of the index."""
        name_of, cache = self._names, {}
        with open(path, "w") as f:
            for r, a, b in zip(self.ids.tolist(), self.starts.tolist(), self.stops.tolist()):
                if r not in cache:
                    cache[r] = name_of(r)
                f.write("%s\t%d\t%d\n" % (cache[r], a, b))


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (what, v))
    return int(v)


def check_windows(window, step=None, max_windows=10**8):
    """-> (window, step): step None means tiling; ValueError for a window or step below 1, a negative max_windows or no
    integer."""
    window = _int(window, "window")
    step = window if step is None else _int(step, "step")
    if window < 1:
        raise ValueError("window=%d must be at least 1" % window)
    if step < 1:
        raise ValueError("step=%d must be at least 1" % step)
    if _int(max_windows, "max_windows") < 0:
        raise ValueError("max_windows must not be negative")
    return window, step


def count_windows(slen, window, step, partial=True):
    """Windows of every record of lengths slen -> int64 array (the rule of fx_fasta_window_counts, on the host)."""
    s = np.asarray(slen, dtype=np.int64)
    if partial:
        return np.where(s > 0, (s - 1) // step + 1, 0)
    return np.where(s >= window, (s - window) // step + 1, 0)


def byte_set(letters):
    """An explicit set of byte values, used exactly as written (no case folding) -> its 32-byte form: bit (c & 7) of byte
    (c >> 3) is set when byte value c is in it.  ValueError for an empty set or a character outside latin-1."""
    if isinstance(letters, str):
        try:
            letters = letters.encode("latin-1")
        except UnicodeEncodeError:
            raise ValueError("letters hold a character outside latin-1")
    elif not isinstance(letters, (bytes, bytearray)):
        raise ValueError("letters must be str or bytes, not %r" % (letters,))
    if len(letters) == 0:
        raise ValueError("an empty letter set has no runs")
    out = bytearray(32)
    for c in bytes(letters):
        out[c >> 3] |= 1 << (c & 7)
    return bytes(out)


def class_set(kind=None, letters=None):
    """kind 'N' / 'masked' / 'unmasked', or an explicit set: letters=..., or a kind of more than one distinct letter -> the
    32-byte set.  ValueError for anything else."""
    if letters is not None:
        if kind is not None:
            raise ValueError("give kind or letters, not both")
        return byte_set(letters)
    if isinstance(kind, str) and kind in KINDS:
        return byte_set(KINDS[kind])
    if isinstance(kind, (str, bytes, bytearray)) and len(set(kind)) > 1:
        return byte_set(kind)
    raise ValueError("kind must be 'N', 'masked', 'unmasked' or a set of letters (letters=...), not %r" % (kind,))


def check_runs(min_len=1, max_runs=10**8):
    min_len = _int(min_len, "min_len")
    if min_len < 1:
        raise ValueError("min_len=%d must be at least 1" % min_len)
    if _int(max_runs, "max_runs") < 0:
        raise ValueError("max_runs must not be negative")
    return min_len, int(max_runs)


def region_blob(blob, ids, starts, stops):
    """RegionStats of (record id, start, stop) on a Blob whose FASTA table is resident; an invalid query raises
    FxError(FX_ERANGE) with .first_bad."""
    ids, starts, stops = (np.ascontiguousarray(x, dtype=np.int64) for x in (ids, starts, stops))
    return RegionStats(ids, starts, stops, blob.fasta_region_counts(ids, starts, stops))


def window_blob(blob, slen, window, step=None, ids=None, partial=True, max_windows=10**8):
    """RegionStats of the windows of the selected records; slen: the lengths of all records (the count is checked against
    max_windows here, before the device is asked)."""
    window, step = check_windows(window, step, max_windows)
    s = np.asarray(slen, dtype=np.int64)
    total = int(count_windows(s if ids is None else s[ids], window, step, partial).sum())
    if total > max_windows:
        raise ValueError("%d windows, more than max_windows=%d" % (total, max_windows))
    try:
        rec, a, b, counts = blob.fasta_window_counts(window, step, partial, ids, cap=int(max_windows))
    except _lib.FxError as e:
        raise _lib.too_many(e, "windows", "max_windows", max_windows)
    return RegionStats(rec, a, b, counts)


def runs_blob(blob, kind=None, min_len=1, ids=None, max_runs=10**8, letters=None, names=None):
    """ClassRuns of one letter class on a Blob whose FASTA table is resident."""
    bits = class_set(kind, letters)
    min_len, max_runs = check_runs(min_len, max_runs)
    try:
        rec, a, b = blob.fasta_class_runs(bits, min_len, ids, cap=max_runs)
    except _lib.FxError as e:
        raise _lib.too_many(e, "runs", "max_runs", max_runs)
    return ClassRuns(rec, a, b, names)
