"""Open reading frames in all six frames and batched translation on the resident FASTA stream: Fasta.orfs,
Fasta.translate_many.  Extension -- the reference reads no codon.  The genetic codes, the argument rules and the result
object live here; the search is fx_fasta_orfs and the translation fx_fasta_translate_alloc (csrc/fx_orf.hpp).

Per strand and residue class a segment is a maximal run of consecutive codons that are neither a stop nor hold a letter
outside A C G T (either case).  mode "stop" reports the segments, mode "start" the part of a segment from its first START
codon on; rows are kept from max(min_len, 3) letters on and never contain the stop codon that ends them."""
import numpy as np

from . import _lib

# NCBI translation tables, amino acids and starts, in NCBI's own codon order T C A G (first letter slowest)
_NCBI = {
    1: ("FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
        "---M------**--*----M---------------M----------------------------"),
    2: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG",
        "----------**--------------------MMMM----------**---M------------"),
    4: ("FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
        "--MM------**-------M------------MMMM---------------M------------"),
    11: ("FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
         "---M------**--*----M------------MMMM---------------M------------"),
}
_TCAG = "TCAG"
MODES = {"stop": 0, "start": 1}
STRANDS = {"+": 1, "-": 2, "both": 3}


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (what, v))
    return int(v)


def codon_index(codon):
    """16 c0 + 4 c1 + c2 with A C G T = 0..3 of a codon written with T, either case."""
    if not isinstance(codon, str) or len(codon) != 3:
        raise ValueError("a codon is three letters of ACGT, not %r" % (codon,))
    v = 0
    for ch in codon.upper():
        k = "ACGT".find(ch)
        if k < 0:
            raise ValueError("a codon is three letters of ACGT, not %r" % (codon,))
        v = v * 4 + k
    return v


def genetic_code(table=1):
    """table: an NCBI id in {1, 2, 4, 11} or a pair of 64-letter strings in NCBI's TCAG order (amino acids, starts) ->
    (aa64 bytes by codon index 16 c0 + 4 c1 + c2 in A C G T order, stop_mask, start_mask).  '*' among the amino acids marks
    a stop, only 'M' among the starts marks a start."""
    if isinstance(table, (int, np.integer)) and not isinstance(table, bool):
        if int(table) not in _NCBI:
            raise ValueError("genetic code %d is not built in: one of %s, or a pair of 64-letter strings" % (int(table), sorted(_NCBI)))
        aas, starts = _NCBI[int(table)]
    else:
        try:
            aas, starts = table
        except (TypeError, ValueError):
            raise ValueError("table must be an NCBI id or a pair (amino acids, starts) of 64-letter strings")
        if not isinstance(aas, str) or not isinstance(starts, str) or len(aas) != 64 or len(starts) != 64:
            raise ValueError("a custom table is a pair of strings of 64 letters each")
        if not all(ord(ch) < 128 for ch in aas):
            raise ValueError("the amino acids must be ASCII letters")
    aa = bytearray(64)
    stop_mask = start_mask = 0
    for i in range(64):                                      # i: the codon in TCAG order
        codon = _TCAG[i >> 4] + _TCAG[(i >> 2) & 3] + _TCAG[i & 3]
        k = codon_index(codon)
        aa[k] = ord(aas[i])
        if aas[i] == "*":
            stop_mask |= 1 << k
        if starts[i] == "M":
            start_mask |= 1 << k
    return bytes(aa), stop_mask, start_mask


def start_mask_of(starts, table_starts, stop_mask):
    """starts: "table" (the table's own start set) or an iterable of codons -> the mask; one at least must not be a stop."""
    if isinstance(starts, str):
        if starts != "table":
            raise ValueError("starts is an iterable of codons or \"table\", not %r" % (starts,))
        m = table_starts
    else:
        try:
            codons = list(starts)
        except TypeError:
            raise ValueError("starts is an iterable of codons or \"table\", not %r" % (starts,))
        m = 0
        for c in codons:
            m |= 1 << codon_index(c)
    if not m & ~stop_mask:
        raise ValueError("no START codon that is not a stop codon of the table")
    return m


def check_args(min_len=75, mode="start", strand="both", max_orfs=10**8):
    """-> (min_len, mode 0 / 1, strands 1 / 2 / 3, max_orfs)"""
    min_len = _int(min_len, "min_len")
    if min_len < 0:
        raise ValueError("min_len=%d must not be negative" % min_len)
    if _int(max_orfs, "max_orfs") < 0:
        raise ValueError("max_orfs must not be negative")
    if max(min_len, int(max_orfs)) >= 2 ** 63:
        raise ValueError("min_len and max_orfs are 64-bit integers")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode is \"start\" or \"stop\", not %r" % (mode,))
    if not isinstance(strand, str) or strand not in STRANDS:
        raise ValueError("strand is \"+\", \"-\" or \"both\", not %r" % (strand,))
    return min_len, MODES[mode], STRANDS[strand], int(max_orfs)


_STRAND_OF = {"+": False, "-": True, b"+": False, b"-": True}


def _strand_int(s):
    if isinstance(s, (bool, int, np.integer)) and int(s) in (0, 1, ord("+"), ord("-")):
        return int(s) in (1, ord("-"))
    raise ValueError("a strand is '+' or '-' (0 or 1), not %r" % (s,))


def strands_of(strand, n):
    """None, or one '+' / '-' (0 / 1) per query -> None or uint8[n] of 0 / 1"""
    if strand is None:
        return None
    if isinstance(strand, np.ndarray) and strand.dtype.kind in "biu":
        neg = (strand != 0) & (strand != ord("+"))
    else:                                                    # '+' / '-' one by one; an array of strings comes here as well
        if isinstance(strand, np.ndarray):
            strand = strand.ravel().tolist()
        if isinstance(strand, str) and len(strand) != n:
            raise ValueError("strand has %d entries for %d queries" % (len(strand), n))
        neg = np.array([_STRAND_OF[s] if isinstance(s, (str, bytes)) and s in _STRAND_OF else _strand_int(s) for s in strand], dtype=bool)
    if neg.size != n:
        raise ValueError("strand has %d entries for %d queries" % (neg.size, n))
    return neg.astype(np.uint8)


class Orfs:
    """ids, starts, stops (int64[n]), frames (int8[n]: +1..+3, -1..-3) and flags (uint8[n]: 1 a stop codon follows the 3' end,
    2 a stop codon precedes the segment, 4 the first codon is a START) of the open reading frames, ordered by record, the
    coordinate at which a left-to-right walk closes the row's segment, strand."""

    def __init__(self, ids, starts, stops, frames, flags, names=None, translate=None):
        self.ids, self.starts, self.stops, self.frames, self.flags = ids, starts, stops, frames, flags
        self._names = names                                  # callable: record id -> name (write_bed, write_faa)
        self._translate = translate                          # callable: (ids, starts, stops, strands 0 / 1) -> (buffer, offsets)

    def __len__(self):
        return int(self.ids.size)

    @property
    def lengths(self):
        return self.stops - self.starts

    @property
    def strands(self):
        """uint8[n]: ord('+') or ord('-')"""
        return np.where(self.frames > 0, np.uint8(ord("+")), np.uint8(ord("-"))).astype(np.uint8)

    @property
    def has_stop(self):
        return (self.flags & 1) != 0

    @property
    def has_start(self):
        return (self.flags & 4) != 0

    @property
    def complete(self):
        """a START codon first and a stop codon behind the last codon"""
        return (self.flags & 5) == 5

    def _take(self, o):
        return Orfs(self.ids[o], self.starts[o], self.stops[o], self.frames[o], self.flags[o], self._names, self._translate)

    def sorted_by_start(self):
        """The same rows ordered by record, start, stop, strand (records keep the order they have; '+' before '-')."""
        if not len(self):
            return self._take(np.zeros(0, dtype=np.int64))
        _, first, inverse = np.unique(self.ids, return_index=True, return_inverse=True)
        return self._take(np.lexsort((self.frames < 0, self.stops, self.starts, first[inverse])))   # a record ranks by where it first appears

    def _name_cache(self):
        name_of, cache = self._names, {}

        def get(r):
            if r not in cache:
                cache[r] = name_of(r)
            return cache[r]
        return get

    def write_bed(self, path):
        """BED6: name, start, stop, orf<k> (k: the row), score = length, strand."""
        get = self._name_cache()
        with open(path, "w") as f:
            for k, (r, a, b, fr) in enumerate(zip(self.ids.tolist(), self.starts.tolist(), self.stops.tolist(), self.frames.tolist())):
                f.write("%s\t%d\t%d\torf%d\t%d\t%s\n" % (get(r), a, b, k, b - a, "+" if fr > 0 else "-"))

    def proteins(self):
        """-> (uint8 buffer, int64 offsets[n + 1]): the rows translated with the table of the search (plain table translation:
        an alternative START codon is not rewritten to M)."""
        if self._translate is None:
            raise ValueError("these rows do not come from a search: nothing to translate them with")
        return self._translate(self.ids, self.starts, self.stops, (self.frames < 0).astype(np.uint8))

    def write_faa(self, path):
        """FASTA of the proteins, header >name:start-stop(strand)."""
        buf, offs = self.proteins()
        get = self._name_cache()
        data, o = bytes(buf), offs.tolist()
        with open(path, "w") as f:
            for k, (r, a, b, fr) in enumerate(zip(self.ids.tolist(), self.starts.tolist(), self.stops.tolist(), self.frames.tolist())):
                f.write(">%s:%d-%d(%s)\n%s\n" % (get(r), a, b, "+" if fr > 0 else "-", data[o[k]:o[k + 1]].decode("ascii")))


def translate_blob(blob, ids, starts, stops, strand=None, table=1):
    """(amino acids uint8, offsets int64[n + 1]) of the intervals on a Blob whose FASTA table is resident; FxError(FX_ERANGE)
    with .first_bad for a query outside the table or its record."""
    aa64 = genetic_code(table)[0]
    return blob.fasta_translate_alloc(ids, starts, stops, aa64, strand=strands_of(strand, len(ids)))


def search_args(min_len=75, table=1, starts=("ATG",), mode="start", strand="both", max_orfs=10**8):
    """The arguments of a search, checked and resolved once, before the device is touched ->
    (min_len, mode 0 / 1, strands 1 / 2 / 3, max_orfs, stop_mask, start_mask, table)"""
    min_len, m, s, max_orfs = check_args(min_len, mode, strand, max_orfs)
    _, stop_mask, table_starts = genetic_code(table)
    return min_len, m, s, max_orfs, stop_mask, start_mask_of(starts, table_starts, stop_mask), table


def orfs_blob(blob, min_len=75, table=1, starts=("ATG",), mode="start", strand="both", ids=None, max_orfs=10**8, names=None):
    """Orfs on a Blob whose FASTA table is resident."""
    return orfs_run(blob, search_args(min_len, table, starts, mode, strand, max_orfs), ids, names)


def orfs_run(blob, args, ids=None, names=None):
    """orfs_blob with the arguments search_args() has resolved."""
    min_len, m, s, max_orfs, stop_mask, start_mask, table = args
    try:
        cols = blob.fasta_orfs(stop_mask, start_mask, m, s, min_len, ids, cap=max_orfs)
    except _lib.FxError as e:
        raise _lib.too_many(e, "open reading frames", "max_orfs", max_orfs)
    return Orfs(*cols, names=names, translate=lambda i, a, b, sd: translate_blob(blob, i, a, b, sd, table))
