"""Minimizers on the resident stream (extension; the reference has no k-mer of any kind).

Fasta.minimizers / minimizer_counts hand k, w and two flags to fx_fasta_minimizers (csrc/fx_minimizer.hpp).  The definition,
as include/fxgpu.h has it:

Sequence.  A record's `seq` as the searches see it: bytes 10, 13 and 32 dropped, windows across line ends and never across
records, cut at slen.  uppercase= plays no part.
k-mers.  1 <= k <= 31.  Position p (0 <= p <= slen - k) holds the k-mer seq[p:p+k]; it is valid when all its letters are
ACGTacgt (U, N, IUPAC codes and everything else are not).  fw is its base-4 code, A=0 C=1 G=2 T=3, first letter most
significant; rc the code of its reverse complement.  canonical: code = min(fw, rc), strand '+' when fw <= rc (a k-mer that is
its own reverse complement is '+'), '-' otherwise.  Not canonical: code = fw, strand '+'.
Order.  "lex": key = code.  "hash": key = mix(code, k), a bijection of the 2k-bit words, so equal keys mean equal codes.
Windows.  1 <= w <= 32.  Window j (0 <= j <= slen - k - w + 1) holds the positions j .. j+w-1; its selection is the leftmost
position with the smallest key among its valid k-mers; a window with no valid k-mer has none.  A record shorter than
w + k - 1 letters has no window and gives no row.
Rows.  The distinct selections of all windows of a record, each (record, start = position, strand, code), ordered by
(record, start)."""
from collections import namedtuple

import numpy as np

from . import _lib

MAX_K = 31
MAX_W = 32
ORDERS = ("hash", "lex")
_U = np.uint64
# the odd multipliers of mix and their inverses modulo 2^64
_INV_2_21_M1 = _U(0x7FFFFBFFFFDFFFFF)
_INV_265 = _U(0xD38FF08B1C03DD39)
_INV_21 = _U(0xCF3CF3CF3CF3CF3D)
_INV_2_31_P1 = _U(0x3FFFFFFF80000001)


def check_args(k, w, order="hash"):
    """The argument rules of every entry -> (k, w) as Python ints.  ValueError otherwise."""
    for name, v, top in (("k", k, MAX_K), ("w", w, MAX_W)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, not %r" % (name, v))
        if not 1 <= v <= top:
            raise ValueError("%s = %d outside 1..%d" % (name, v, top))
    if order not in ORDERS:
        raise ValueError("order must be 'hash' or 'lex', not %r" % (order,))
    return int(k), int(w)


def _flags(canonical, order):
    return (_lib.FX_MZ_CANONICAL if canonical else 0) | (_lib.FX_MZ_LEX if order == "lex" else 0)


def _codes(codes, k):
    k, _ = check_args(k, 1)
    x = np.array(codes, dtype=np.uint64, copy=True, ndmin=1)
    m = _U(4 ** k - 1)
    if x.size and (x > m).any():
        raise ValueError("a code is not below 4**%d" % k)
    return x, m


def mix(codes, k):
    """The hash order's key of every code (uint64 array): with m = 4**k - 1 and unsigned 64-bit arithmetic
        x = (~x + (x << 21)) & m;  x ^= x >> 24
        x = (x + (x << 3) + (x << 8)) & m;  x ^= x >> 14
        x = (x + (x << 2) + (x << 4)) & m;  x ^= x >> 28
        x = (x + (x << 31)) & m"""
    x, m = _codes(codes, k)
    with np.errstate(over="ignore"):
        x = (~x + (x << _U(21))) & m
        x ^= x >> _U(24)
        x = (x + (x << _U(3)) + (x << _U(8))) & m
        x ^= x >> _U(14)
        x = (x + (x << _U(2)) + (x << _U(4))) & m
        x ^= x >> _U(28)
        x = (x + (x << _U(31))) & m
    return x


def unmix(keys, k):
    """The inverse of mix: unmix(mix(x, k), k) == x.  The steps undone last to first: an odd multiplier by its inverse modulo
    2^64, y = x ^ (x >> s) by x = y ^ (y >> s) ^ (y >> 2s) ^ ..."""
    x, m = _codes(keys, k)
    with np.errstate(over="ignore"):
        x = (x * _INV_2_31_P1) & m
        x ^= (x >> _U(28)) ^ (x >> _U(56))
        x = (x * _INV_21) & m
        x ^= (x >> _U(14)) ^ (x >> _U(28)) ^ (x >> _U(42)) ^ (x >> _U(56))
        x = (x * _INV_265) & m
        x ^= (x >> _U(24)) ^ (x >> _U(48))
        x = ((x + _U(1)) * _INV_2_21_M1) & m
    return x


class Minimizers(namedtuple("Minimizers", ["ids", "starts", "stops", "strands", "codes"])):
    """The rows of Fasta.minimizers: record ids int64, starts and stops int64 (0-based half-open, forward strand,
    stops = starts + k), strands uint8 ('+' / '-'), codes uint64."""
    __slots__ = ()

    @property
    def k(self):
        """k, read off the rows (None without a row)."""
        return int(self.stops[0] - self.starts[0]) if self.ids.size else None

    def hashes(self):
        """mix(codes, k): the keys of the hash order, whatever order chose the rows."""
        return mix(self.codes, self.k) if self.ids.size else np.zeros(0, dtype=np.uint64)

    def kmers(self):
        """The letters of `codes` as stored -> list of str: the forward-strand letters of a '+' row, their reverse complement
        for a '-' row."""
        if not self.ids.size:
            return []
        k = self.k
        sh = (np.arange(k - 1, -1, -1, dtype=np.uint64) * _U(2))[None, :]
        digits = ((self.codes[:, None] >> sh) & _U(3)).astype(np.intp)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[digits]
        return [row.tobytes().decode() for row in letters]

    def density(self, lengths):
        """Rows per k-mer position of every record -> float64[len(lengths)]: count / (length - k + 1), 0 for a record
        shorter than k.  lengths: the sequence length of every record, e.g. [len(s) for s in fa]."""
        lengths = np.asarray(lengths, dtype=np.int64)
        n = np.bincount(self.ids, minlength=lengths.size).astype(np.float64)
        if n.size > lengths.size:
            raise ValueError("a row's record id lies beyond the %d lengths given" % lengths.size)
        pos = lengths - ((self.k or 1) - 1)
        return np.divide(n, pos, out=np.zeros(lengths.size, dtype=np.float64), where=pos > 0)

    def write_bed(self, path, names):
        """BED6 lines, one per row: name of the record, start, stop, the k-mer (kmers()), 0, strand.  names: the records'
        names by id, e.g. list(fa.keys()).  -> the number of lines."""
        km = self.kmers()
        with open(path, "w") as f:
            for i, a, z, s, word in zip(self.ids.tolist(), self.starts.tolist(), self.stops.tolist(), self.strands.tolist(), km):
                f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (names[i], a, z, word, chr(s)))
        return len(km)


def _empty():
    z = np.zeros(0, dtype=np.int64)
    return Minimizers(z, z.copy(), z.copy(), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64))


def minimizers_blob(blob, k, w, canonical=True, order="hash", ids=None, max_hits=10**8):
    """The rows on a Blob whose FASTA table is resident -> Minimizers (arrays in pinned memory)."""
    k, w = check_args(k, w, order)
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    try:
        total, rows, _ = blob.fasta_minimizers(k, w, _flags(canonical, order), ids=ids, cap=int(max_hits))
    except _lib.FxError as e:
        raise _lib.too_many(e, "minimizers", "max_hits", max_hits)
    if rows is None:
        return _empty()
    rec, starts, strands, codes = rows
    stops = _lib.pinned_empty(total, np.int64)
    np.add(starts, k, out=stops)
    return Minimizers(rec, starts, stops, strands, codes)


def count_blob(blob, k, w, canonical=True, order="hash"):
    """Rows per record on + and on - -> int64[n_records, 2]; the rows themselves never leave the device."""
    k, w = check_args(k, w, order)
    _, _, counts = blob.fasta_minimizers(k, w, _flags(canonical, order), cap=0, counts=True)
    return counts
