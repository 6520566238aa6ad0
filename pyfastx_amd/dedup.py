"""Exact duplicate-read detection on the resident FASTQ stream (csrc/fx_fastq_dedup.hpp): the argument rules of
Fastq.duplicates / Fastq.dedup, the calls into the library, and FastQC's duplication levels from the group sizes (host numpy).

The definition stands in include/fxgpu.h: the key of a query is seq[start:end] as bytes, two queries are duplicates when their
keys are equal (with revcomp: when one key equals the other or its reverse complement), first[q] is the smallest query position
whose key is a duplicate of q's."""
import numpy as np

from . import _lib, trim

# FastQC's duplication-level bins: group sizes 1..9 one by one, then ">10" = 10..49, ">50" = 50..99, ">100" = 100..499,
# ">500" = 500..999, ">1k" = 1000..4999, ">5k" = 5000..9999, ">10k" = 10000 and more
LEVEL_LABELS = ("1", "2", "3", "4", "5", "6", "7", "8", "9", ">10", ">50", ">100", ">500", ">1k", ">5k", ">10k")
LEVEL_EDGES = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000], dtype=np.int64)


def _int(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int" % name)
    return int(v)


def check_copies(min_copies=1, max_copies=None):
    """The group-size bounds of Fastq.dedup as fx_fastq_dedup takes them -> (min_copies, max_copies); max_copies None: -1, not
    asked."""
    lo = _int(min_copies, "min_copies")
    if lo < 1:
        raise ValueError("min_copies %d below 1" % lo)
    if max_copies is None:
        return lo, -1
    hi = _int(max_copies, "max_copies")
    if hi < lo:
        raise ValueError("max_copies %d below min_copies %d" % (hi, lo))
    return lo, hi


def check_hash_bits(hash_bits=0):
    """The fingerprint bits kept: 0 (all 64) or 1..64.  It exists for tests of the collision path; no result depends on it."""
    b = _int(hash_bits, "hash_bits")
    if b < 0 or b > 64:
        raise ValueError("hash_bits %d outside 0..64" % b)
    return b


def check_flag(v, name):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be a bool" % name)
    return bool(v)


def _queries(ids, start, end, n_reads):
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    return ids, start, end


def duplicates_blob(blob, n_reads, ids=None, start=None, end=None, revcomp=False, hash_bits=0):
    """-> (first int64[n], n_groups, n_rounds); ids, start and end by the rules of Fastq.records."""
    revcomp, hash_bits = check_flag(revcomp, "revcomp"), check_hash_bits(hash_bits)
    ids, start, end = _queries(ids, start, end, n_reads)
    try:
        return blob.fastq_dup_first(ids, start, end, revcomp, hash_bits)
    except _lib.FxError as e:
        raise _lib.outside(e)


def dedup_blob(blob, n_reads, ids=None, start=None, end=None, revcomp=False, min_copies=1, max_copies=None, return_counts=False, hash_bits=0):
    """-> (positions int64, copies int64 or None, n_groups, n_rounds)"""
    revcomp, return_counts = check_flag(revcomp, "revcomp"), check_flag(return_counts, "return_counts")
    lo, hi = check_copies(min_copies, max_copies)
    hash_bits = check_hash_bits(hash_bits)
    ids, start, end = _queries(ids, start, end, n_reads)
    try:
        return blob.fastq_dedup(ids, start, end, revcomp, hash_bits, lo, hi, return_counts)
    except _lib.FxError as e:
        raise _lib.outside(e)


def duplication_levels(copies):
    """FastQC's duplication levels from the group sizes `copies` (one entry per distinct sequence, as Fastq.dedup(...,
    return_counts=True) returns them) -> {"labels": LEVEL_LABELS, "groups": int64[16] distinct sequences per bin, "reads":
    int64[16] reads per bin, "n_groups", "n_reads", "unique_fraction": n_groups / n_reads -- the share of the reads that is left
    after deduplication (1.0 for no read at all)}."""
    c = np.asarray(copies)
    if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("copies must be a one-dimensional integer array")
    c = c.astype(np.int64)
    if c.size and c.min() < 1:
        raise ValueError("a group has at least one member")
    bins = np.searchsorted(LEVEL_EDGES, c, side="right") - 1
    groups = np.bincount(bins, minlength=LEVEL_EDGES.size).astype(np.int64)
    reads = np.array([c[bins == b].sum() for b in range(LEVEL_EDGES.size)], dtype=np.int64)       # exact: no float weights
    n_groups, n_reads = int(c.size), int(c.sum())
    return {"labels": LEVEL_LABELS, "groups": groups, "reads": reads, "n_groups": n_groups, "n_reads": n_reads,
            "unique_fraction": n_groups / n_reads if n_reads else 1.0}
