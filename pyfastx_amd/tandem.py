"""Perfect tandem repeats (microsatellites) of period 1..8 on the resident FASTA stream: Fasta.tandem_repeats.  Extension --
the reference has no repeat search (its author ships Krait and pytrf beside it).  The argument rules and the result object
live here; the search is fx_fasta_tandem_repeats (csrc/fx_tandem.hpp).

A repeat of period p is a maximal stretch of A C G T letters (either case) in which every letter equals the one p places
before it, at least max(2 p, p * min_copies[p], min_len) long, whose motif is not a shorter word written several times.
Repeats of different periods may overlap and all are reported (maximal repetitions, not a greedy left-to-right scan)."""
import numpy as np

from . import _lib

MAX_PERIOD = 8
KRAIT_DEFAULT = (12, 7, 5, 4, 4, 4)


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (what, v))
    return int(v)


def check_min_copies(min_copies):
    """A sequence of 1 to 8 integers (entry p - 1: period p) or a dict {period: copies} -> int32 array, one entry per period
    up to the longest one searched.  Each entry is 0 (period not searched) or at least 2, and one at least is not 0."""
    if isinstance(min_copies, dict):
        mc = [0] * MAX_PERIOD
        for p, c in min_copies.items():
            p = _int(p, "a period")
            if not 1 <= p <= MAX_PERIOD:
                raise ValueError("period %d outside 1..%d" % (p, MAX_PERIOD))
            mc[p - 1] = _int(c, "min_copies[%d]" % p)
    elif isinstance(min_copies, (str, bytes)) or not hasattr(min_copies, "__len__"):
        raise ValueError("min_copies must be a sequence of 1 to %d integers or a dict {period: copies}, not %r" % (MAX_PERIOD, min_copies))
    else:
        if not 1 <= len(min_copies) <= MAX_PERIOD:
            raise ValueError("min_copies has %d entries; periods 1..%d can be searched" % (len(min_copies), MAX_PERIOD))
        mc = [_int(c, "min_copies[%d]" % (i + 1)) for i, c in enumerate(min_copies)]
    for p, c in enumerate(mc, 1):
        if c == 1 or c < 0:
            raise ValueError("min_copies of period %d is %d: 0 (not searched) or at least 2" % (p, c))
        if c >= 1 << 31:
            raise ValueError("min_copies of period %d is too large" % p)
    if not any(mc):
        raise ValueError("no period is searched")
    while mc[-1] == 0:
        mc.pop()
    return np.asarray(mc, dtype=np.int32)


def check_limits(min_len=0, max_repeats=10**8):
    min_len = _int(min_len, "min_len")
    if min_len < 0:
        raise ValueError("min_len=%d must not be negative" % min_len)
    if _int(max_repeats, "max_repeats") < 0:
        raise ValueError("max_repeats must not be negative")
    return min_len, int(max_repeats)


def motif_string(code, period):
    """The letters of a 2-bit motif code (first letter most significant, as kmer.kmer_code packs them)."""
    return "".join("ACGT"[(int(code) >> (2 * (period - 1 - i))) & 3] for i in range(period))


_CANON = {}


def canonical_table(period):
    """uint32[4 ** period]: for every motif code the smallest code among all rotations of the motif and of its reverse
    complement (made once per period, on the host)."""
    t = _CANON.get(period)
    if t is None:
        n, bits = 4 ** period, 2 * period
        code = np.arange(n, dtype=np.uint32)
        rc = np.zeros(n, dtype=np.uint32)
        for i in range(period):                              # letter i of the reverse complement = 3 - letter period - 1 - i
            rc |= (3 - ((code >> np.uint32(2 * i)) & 3)) << np.uint32(2 * (period - 1 - i))
        t = np.minimum(code, rc)
        for word in (code, rc):
            for r in range(1, period):
                t = np.minimum(t, ((word << np.uint32(2 * r)) | (word >> np.uint32(bits - 2 * r))) & np.uint32(n - 1))
        _CANON[period] = t
    return t


class TandemRepeats:
    """ids, starts, stops (int64[n]), periods (uint8[n]) and motif_codes (uint32[n]) of the repeats, ordered by record, stop,
    period."""

    def __init__(self, ids, starts, stops, periods, motif_codes, names=None):
        self.ids, self.starts, self.stops, self.periods, self.motif_codes = ids, starts, stops, periods, motif_codes
        self._names = names                                  # callable: record id -> name (write_bed)

    def __len__(self):
        return int(self.ids.size)

    @property
    def lengths(self):
        return self.stops - self.starts

    @property
    def copies(self):
        """Whole copies of the motif: length // period."""
        return self.lengths // self.periods.astype(np.int64)

    @property
    def motifs(self):
        return [motif_string(c, p) for c, p in zip(self.motif_codes.tolist(), self.periods.tolist())]

    @property
    def canonical_motifs(self):
        """uint32[n]: per repeat the smallest code among the rotations of its motif and of the motif's reverse complement."""
        out = np.zeros(len(self), dtype=np.uint32)
        for p in np.unique(self.periods).tolist():
            m = self.periods == p
            out[m] = canonical_table(p)[self.motif_codes[m]]
        return out

    def counts_by_motif(self, canonical=True):
        """{motif string: number of repeats}, of the canonical motifs or of the motifs as they stand in the text."""
        codes = self.canonical_motifs if canonical else self.motif_codes
        key = codes.astype(np.int64) * (MAX_PERIOD + 1) + self.periods
        uniq, cnt = np.unique(key, return_counts=True)
        return {motif_string(k // (MAX_PERIOD + 1), k % (MAX_PERIOD + 1)): int(c) for k, c in zip(uniq.tolist(), cnt.tolist())}

    def sorted_by_start(self):
        """The same repeats ordered by record, start, period (records keep the order they have)."""
        _, first, inverse = np.unique(self.ids, return_index=True, return_inverse=True)
        o = np.lexsort((self.periods, self.starts, first[inverse]))      # a record ranks by where it first appears
        return TandemRepeats(self.ids[o], self.starts[o], self.stops[o], self.periods[o], self.motif_codes[o], self._names)

    def write_bed(self, path):
        """name<TAB>start<TAB>stop<TAB>(MOTIF)copies rows, one per repeat, with the names of the index."""
        name_of, cache = self._names, {}
        with open(path, "w") as f:
            for r, a, b, m, c in zip(self.ids.tolist(), self.starts.tolist(), self.stops.tolist(), self.motifs, self.copies.tolist()):
                if r not in cache:
                    cache[r] = name_of(r)
                f.write("%s\t%d\t%d\t(%s)%d\n" % (cache[r], a, b, m, c))


def repeats_blob(blob, min_copies=KRAIT_DEFAULT, min_len=0, ids=None, max_repeats=10**8, names=None):
    """TandemRepeats on a Blob whose FASTA table is resident."""
    mc = check_min_copies(min_copies)
    min_len, max_repeats = check_limits(min_len, max_repeats)
    try:
        cols = blob.fasta_tandem_repeats(mc, min_len, ids, cap=max_repeats)
    except _lib.FxError as e:
        raise _lib.too_many(e, "repeats", "max_repeats", max_repeats)
    return TandemRepeats(*cols, names=names)
