"""k-mer spectra of the resident FASTA and FASTQ streams (extension; the reference counts single letters only).

Fasta.kmer_counts / kmer_profile and Fastq.kmer_counts check their arguments here and hand them to fx_fasta_kmers and
fx_fastq_kmers (csrc/fx_kmer.hpp).  The definition -- alphabet, code of a window, canonical form -- is written down in
include/fxgpu.h and, as plain Python, in tests/kmer_truth.py."""
import numpy as np

from . import _lib, trim

MAX_K = 13                # the dense table is 8 * 4**k bytes: 512 MiB at k = 13
MAX_PROFILE_K = 6         # one row per record


def check_k(k, hi=MAX_K):
    """k as an int in 1..hi; ValueError for a bool, a float, anything else, or a value outside the range."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an int")
    k = int(k)
    if not 1 <= k <= hi:
        raise ValueError("k %d outside 1..%d" % (k, hi))
    return k


def check_profile(k, n_sel, max_bytes):
    """The arguments of kmer_profile -> k; more than max_bytes of rows: ValueError that names the size, before anything is
    allocated."""
    k = check_k(k, MAX_PROFILE_K)
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 0:
        raise ValueError("max_bytes must be a non-negative int")
    size = int(n_sel) * 4 ** k * 8
    if size > max_bytes:
        raise ValueError("%d rows of %d counters take %d bytes, more than max_bytes=%d" % (n_sel, 4 ** k, size, max_bytes))
    return k


def revcomp_code(code, k):
    """The code of the reverse complement of the k-mer with this code (int or numpy array)."""
    code = np.asarray(code, dtype=np.int64)
    out = np.zeros_like(code)
    for _ in range(k):
        out = out * 4 + (3 - (code & 3))
        code = code >> 2
    return out


def kmer_string(code, k):
    """The k letters of a code."""
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def fasta_counts_blob(blob, k, canonical=False, ids=None):
    """One spectrum of the records `ids` (int64 ids or None) of a Blob whose FASTA table is resident -> int64[4**k], pinned."""
    k = check_k(k)
    return blob.fasta_kmers(k, bool(canonical), ids)


def fasta_profile_blob(blob, k, canonical, ids, n_records, max_bytes):
    """One row per selected record -> int64[n_sel, 4**k], pinned."""
    k = check_profile(k, n_records if ids is None else len(ids), max_bytes)
    return blob.fasta_kmers(k, bool(canonical), ids, per_record=True)


def fastq_counts_blob(blob, n_reads, k, canonical=False, ids=None, start=None, end=None):
    """One spectrum of seq[start:end] of the reads `ids`; ids, start and end by the rules of Fastq.records."""
    k = check_k(k)
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    try:
        return blob.fastq_kmers(k, bool(canonical), ids, start, end)
    except _lib.FxError as e:
        if e.code == _lib.FX_ERANGE and getattr(e, "first_bad", -1) >= 0:
            raise ValueError("the interval of query %d lies outside its read" % e.first_bad)
        raise
