"""k-mer spectra of the resident FASTA and FASTQ streams (extension; the reference counts single letters only).

Fasta.kmer_counts / kmer_profile and Fastq.kmer_counts check their arguments here and hand them to fx_fasta_kmers and
fx_fastq_kmers (csrc/fx_kmer.hpp); Fasta.kmer_table and Fastq.kmer_table (1 <= k <= 31, the codes that occur with their
counts: a KmerTable) go to fx_fasta_kmer_table and fx_fastq_kmer_table (csrc/fx_kmer_table.hpp).  The definition -- alphabet, code of a window, canonical form -- is written down in
include/fxgpu.h and, as plain Python, in tests/kmer_truth.py."""
import numpy as np

from . import _lib, trim

MAX_K = 13                # the dense table is 8 * 4**k bytes: 512 MiB at k = 13
MAX_PROFILE_K = 6         # one row per record
MAX_TABLE_K = 31          # the sparse table: a code has 2k <= 62 bits, an exact non-negative int64


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
        raise _lib.outside(e)


# ------------------------------------------------------------------ sparse tables (1 <= k <= 31)
def _check_int(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int" % name)
    if int(v) < lo:
        raise ValueError("%s %d below %d" % (name, int(v), lo))
    return int(v)


def check_table(k, min_count=1, max_bytes=None):
    """The arguments of kmer_table -> (k, min_count, max_bytes as the library takes it: 0 for the default)."""
    k = check_k(k, MAX_TABLE_K)
    min_count = _check_int(min_count, "min_count", 1)
    max_bytes = 0 if max_bytes is None else _check_int(max_bytes, "max_bytes", 1 << 20)
    return k, min_count, max_bytes


_LETTER = np.full(256, -1, dtype=np.int64)
for _j, _c in enumerate("ACGT"):
    _LETTER[ord(_c)] = _LETTER[ord(_c.lower())] = _j


def kmer_code(s, k):
    """The code of a k-letter string; ValueError for another length or a letter outside ACGTacgt."""
    if isinstance(s, str):
        s = s.encode("latin-1", "replace")
    d = _LETTER[np.frombuffer(bytes(s), dtype=np.uint8)]
    if d.size != k:
        raise ValueError("a k-mer of %d letters where k is %d" % (d.size, k))
    if (d < 0).any():
        raise ValueError("a k-mer holds letters of ACGTacgt only")
    code = 0
    for x in d.tolist():
        code = code * 4 + x
    return code


class KmerTable:
    """The k-mers that occur in a selection: codes (int64, ascending, canonical ones only where canonical) and their counts
    (int64); n_windows = valid windows of the selection before min_count, n_parts = sort-and-reduce rounds the call took."""

    def __init__(self, k, canonical, codes, counts, n_windows=None, n_parts=0):
        self.k = int(k)
        self.canonical = bool(canonical)
        self.codes = np.asarray(codes, dtype=np.int64)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.n_windows = int(self.counts.sum()) if n_windows is None else int(n_windows)
        self.n_parts = int(n_parts)
        self._sets = {}                                        # device -> _lib.KmerSet of the codes, made by the first screen there

    @classmethod
    def from_strings(cls, seqs, k, canonical=False):
        """The table of the windows of the strings `seqs` (str or bytes; one alone counts as a list of one), computed on the
        host by the definition of this module: letters outside ACGTacgt break windows, a string shorter than k has none.  An
        adapter or primer list becomes a table without a file."""
        k = check_k(k, MAX_TABLE_K)
        if isinstance(seqs, (str, bytes, bytearray)):
            seqs = [seqs]
        found = [np.zeros(0, dtype=np.int64)]
        for s in seqs:
            if isinstance(s, str):
                s = s.encode("latin-1", "replace")
            d = _LETTER[np.frombuffer(bytes(s), dtype=np.uint8)]
            n = d.size - k + 1
            if n <= 0:
                continue
            code = np.zeros(n, dtype=np.int64)
            bad = np.zeros(n, dtype=bool)
            for j in range(k):
                w = d[j:j + n]
                bad |= w < 0
                code = code * 4 + (w & 3)
            code = code[~bad]
            found.append(np.minimum(code, revcomp_code(code, k)) if canonical else code)
        codes, counts = np.unique(np.concatenate(found), return_counts=True)
        return cls(k, canonical, codes, counts.astype(np.int64), n_parts=0)

    def release(self):
        """Free the device sets the screens of this table have made (they are freed with the table otherwise)."""
        for s in self._sets.values():
            s.close()
        self._sets = {}

    def __len__(self):
        return int(self.codes.size)

    def __repr__(self):
        return "<KmerTable k=%d%s: %d distinct of %d windows>" % (self.k, " canonical" if self.canonical else "", len(self), self.n_windows)

    def count(self, x):
        """How often a k-mer occurs: x a k-letter string or a code -> int; an array of codes -> int64 array.  0 where it is
        absent.  On a canonical table the query is folded to its canonical code first."""
        scalar = isinstance(x, (str, bytes, bytearray, int, np.integer)) and not isinstance(x, bool)
        q = kmer_code(x, self.k) if isinstance(x, (str, bytes, bytearray)) else x
        q = np.atleast_1d(np.asarray(q, dtype=np.int64))
        if self.canonical:
            q = np.minimum(q, revcomp_code(q, self.k))
        at = np.searchsorted(self.codes, q)
        inside = at < self.codes.size
        at = np.where(inside, at, 0)
        out = np.zeros(q.shape, dtype=np.int64)
        if self.codes.size:
            hit = inside & (self.codes[at] == q)
            out[hit] = self.counts[at[hit]]
        return int(out[0]) if scalar else out

    def spectrum(self):
        """int64 array whose entry c is the number of distinct k-mers that occur c times (entry 0 is 0)."""
        if not self.counts.size:
            return np.zeros(1, dtype=np.int64)
        return np.bincount(self.counts).astype(np.int64)

    def strings(self, lo=0, hi=None):
        """The letters of the entries [lo, hi) of the table."""
        return [kmer_string(c, self.k) for c in self.codes[lo:hi].tolist()]


def fasta_table_blob(blob, k, canonical=False, ids=None, min_count=1, max_bytes=None):
    """The table of the records `ids` (int64 ids or None) of a Blob whose FASTA table is resident -> KmerTable."""
    k, min_count, max_bytes = check_table(k, min_count, max_bytes)
    codes, counts, nw, parts = blob.fasta_kmer_table(k, bool(canonical), ids, min_count, max_bytes)
    return KmerTable(k, canonical, codes, counts, nw, parts)


def fastq_table_blob(blob, n_reads, k, canonical=False, ids=None, start=None, end=None, min_count=1, max_bytes=None):
    """The table of seq[start:end] of the reads `ids`; ids, start and end by the rules of Fastq.records -> KmerTable."""
    k, min_count, max_bytes = check_table(k, min_count, max_bytes)
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    try:
        codes, counts, nw, parts = blob.fastq_kmer_table(k, bool(canonical), ids, start, end, min_count, max_bytes)
    except _lib.FxError as e:
        raise _lib.outside(e)
    return KmerTable(k, canonical, codes, counts, nw, parts)


# ------------------------------------------------------------------ screening against a table (csrc/fx_kmer_screen.hpp)
SCREEN_LDS_KEYS = 4096    # a set of at most this many codes is probed in LDS (an image of at most 64 KiB), a larger one in global memory


def check_screen_table(table):
    """The table a screen runs against; anything that is no KmerTable: TypeError."""
    if not isinstance(table, KmerTable):
        raise TypeError("a kmer.KmerTable is needed (Fasta.kmer_table, Fastq.kmer_table, KmerTable.from_strings), not %s" % type(table).__name__)
    return table


def check_screen(min_hits=1, min_frac=None, invert=False):
    """The criteria of Fastq.screen as fx_fastq_kmer_screen takes them -> (min_hits, (numerator, denominator), invert);
    min_frac None: (0, 0), the ratio is not asked; else a fraction in 0..1 by the rule of qc.as_ratio."""
    from . import qc
    if isinstance(min_hits, bool) or not isinstance(min_hits, (int, np.integer)):
        raise ValueError("min_hits must be an int")
    if int(min_hits) < 0:
        raise ValueError("min_hits %d is negative" % int(min_hits))
    frac = (0, 0)
    if min_frac is not None:
        frac = qc.as_ratio(min_frac, "min_frac")
        if frac[0] > frac[1]:
            raise ValueError("min_frac %r outside 0..1" % (min_frac,))
    return int(min_hits), frac, bool(invert)


def device_set(table, blob, device):
    """The device k-mer set of a table on `device`: created through `blob` on first use, kept on the table."""
    check_screen_table(table)
    s = table._sets.get(int(device))
    if s is None:
        s = table._sets[int(device)] = blob.kmer_set(table.k, table.canonical, table.codes)
    return s


def fastq_hits_blob(blob, device, n_reads, table, ids=None, start=None, end=None):
    """(n_windows, n_hits), int32, of seq[start:end] of the reads `ids` against the table; ids, start and end by the rules of
    Fastq.records."""
    check_screen_table(table)
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    try:
        return blob.fastq_kmer_hits(device_set(table, blob, device), ids, start, end)
    except _lib.FxError as e:
        raise _lib.outside(e)


def fastq_screen_blob(blob, device, n_reads, table, min_hits=1, min_frac=None, invert=False, ids=None, start=None, end=None):
    """The ascending positions (int64) of the queries that pass the screen."""
    check_screen_table(table)
    min_hits, frac, invert = check_screen(min_hits, min_frac, invert)
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    try:
        return blob.fastq_kmer_screen(device_set(table, blob, device), ids, start, end, min_hits, frac, invert)
    except _lib.FxError as e:
        raise _lib.outside(e)


def fasta_hits_blob(blob, device, table, ids=None):
    """(n_windows, n_hits), int64, one row per record of `ids` (int64 ids or None) of a Blob whose FASTA table is resident."""
    check_screen_table(table)
    return blob.fasta_kmer_hits(device_set(table, blob, device), ids)
