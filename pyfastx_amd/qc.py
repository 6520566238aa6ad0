"""FASTQ quality control on the resident stream (extension; the reference answers whole-file questions only, fastq.c:715-753).

Fastq.read_stats / cycle_profile / select check their arguments here and hand them to fx_fastq_read_stats,
fx_fastq_cycle_hist and fx_fastq_select (csrc/fx_fastq_qc.hpp).  Everything is integer: a mean-quality or low-fraction
threshold becomes a ratio of two integers before it reaches the device."""
from fractions import Fraction

import numpy as np

MAX_CYCLES = 65536
MAX_DENOMINATOR = 1000
BASES = ("A", "C", "G", "T", "other")


def as_ratio(x, what="threshold"):
    """A non-negative threshold -> (numerator, denominator) of the closest fraction with a denominator <= 1000; the
    comparison the device makes is exact for that fraction.  ValueError for a negative, infinite or NaN value."""
    try:
        f = Fraction(x.item() if isinstance(x, np.generic) else x)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s must be a finite number, not %r" % (what, x))
    if f < 0:
        raise ValueError("%s must not be negative" % what)
    f = f.limit_denominator(MAX_DENOMINATOR)
    if f.numerator > 10**9:
        raise ValueError("%s is too large" % what)
    return f.numerator, f.denominator


def check_low_qual(low_qual):
    if isinstance(low_qual, bool) or not isinstance(low_qual, (int, np.integer)):
        raise ValueError("low_qual must be an int in 0..255")
    if not 0 <= int(low_qual) <= 255:
        raise ValueError("low_qual %d outside 0..255" % int(low_qual))
    return int(low_qual)


def check_cycles(cycles):
    if isinstance(cycles, bool) or not isinstance(cycles, (int, np.integer)):
        raise ValueError("cycles must be an int in 1..%d" % MAX_CYCLES)
    if not 1 <= int(cycles) <= MAX_CYCLES:
        raise ValueError("cycles %d outside 1..%d" % (int(cycles), MAX_CYCLES))
    return int(cycles)


def _bound(v, what):
    """None -> -1 (not asked); a non-negative int otherwise."""
    if v is None:
        return -1
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int" % what)
    if int(v) < 0:
        raise ValueError("%s must not be negative" % what)
    return int(v)


def select_args(min_len=None, max_len=None, min_mean_qual=None, max_low_frac=None, max_other=None, low_qual=20):
    """The criteria of Fastq.select as fx_fastq_select takes them -> dict(low_qual, min_len, max_len, mean_qual, low_frac,
    max_other); None becomes -1 (a bound) or (0, 0) (a ratio): not asked."""
    lo, hi = _bound(min_len, "min_len"), _bound(max_len, "max_len")
    if lo >= 0 and hi >= 0 and lo > hi:
        raise ValueError("min_len %d is larger than max_len %d" % (lo, hi))
    return {"low_qual": check_low_qual(low_qual), "min_len": lo, "max_len": hi,
            "mean_qual": (0, 0) if min_mean_qual is None else as_ratio(min_mean_qual, "min_mean_qual"),
            "low_frac": (0, 0) if max_low_frac is None else as_ratio(max_low_frac, "max_low_frac"),
            "max_other": _bound(max_other, "max_other")}


class CycleProfile:
    """What Fastq.cycle_profile returns.  qual int64[cycles, 256]: reads per cycle and RAW quality byte; base int64[cycles, 5]:
    reads per cycle with A, C, G, T, other; depth int64[cycles]: reads longer than the cycle; phred: the offset (33 or 64)."""

    __slots__ = ("qual", "base", "depth", "phred")

    def __init__(self, qual, base, depth, phred):
        self.qual, self.base, self.depth, self.phred = qual, base, depth, int(phred)

    @property
    def cycles(self):
        return int(self.depth.shape[0])

    @property
    def qual_scores(self):
        """A view of qual: column s is the score s = byte - phred, 0..93."""
        return self.qual[:, self.phred:self.phred + 94]

    @property
    def mean_qual(self):
        """Mean score per cycle over the bytes inside qual_scores (float64; NaN where no read reaches the cycle)."""
        qs = self.qual_scores
        tot = (qs * np.arange(qs.shape[1], dtype=np.int64)).sum(1)
        n = qs.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return tot / n

    def __repr__(self):
        return "<CycleProfile> %d cycles, %d reads" % (self.cycles, int(self.depth[0]) if self.cycles else 0)


def read_stats_blob(blob, n_reads, ids, phred, low_qual):
    low_qual = check_low_qual(low_qual)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 1:
            raise ValueError("ids must be one-dimensional")
        if ids.size and (ids.min() < 0 or ids.max() >= n_reads):
            raise IndexError("index out of range")
    return blob.fastq_read_stats(ids, phred=phred, low_qual=low_qual)


def cycle_profile_blob(blob, cycles, phred):
    qual, base, depth = blob.fastq_cycle_hist(check_cycles(cycles))
    return CycleProfile(qual, base, depth, phred or 33)

