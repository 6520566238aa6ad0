"""Genome-wide motif search on the resident stream (extension; the reference only has Sequence.search, sequence.c:519-558).

Fasta.search_all / search_counts check the pattern here and hand it to fx_fasta_search (csrc/fx_search.hpp): every
overlapping hit in the `seq` of the records, on one or both strands, exact or with IUPAC codes.  Fasta.search_approx /
search_approx_counts allow up to `mismatches` substituted letters per hit, none of them inside an anchor
(fx_fasta_search_approx, csrc/fx_search_approx.hpp).  Fasta.search_edit / search_edit_counts allow up to `edits`
substituted, inserted or deleted letters (fx_fasta_search_edit, csrc/fx_search_edit.hpp)."""
from collections import namedtuple

import numpy as np

from . import _lib

SearchHits = namedtuple("SearchHits", ["ids", "starts", "stops", "strands"])
ApproxHits = namedtuple("ApproxHits", ["ids", "starts", "stops", "strands", "mismatches"])
EditHits = namedtuple("EditHits", ["ids", "starts", "stops", "strands", "edits"])

MAX_PATTERN = 64
MAX_MISMATCH = 8
MAX_EDITS = 8
_REPORTS = {"all": _lib.FX_EDIT_ALL, "best": _lib.FX_EDIT_BEST}

# the base set of every IUPAC letter (U is T)
IUPAC = {k: frozenset(v) for k, v in {
    "A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
    "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}.items()}
_IUPAC_COMP = {"A": "T", "T": "A", "U": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B",
               "D": "H", "H": "D", "S": "S", "W": "W", "N": "N"}
_STRANDS = {"+": _lib.FX_SEARCH_PLUS, "-": _lib.FX_SEARCH_MINUS, "both": _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS}
_SPACE = frozenset(b" \t\n\r\v\f")


def iupac_set(letter):
    """Base set of one IUPAC letter (any case) -> frozenset of 'ACGT'; KeyError for anything else."""
    return IUPAC[letter.upper()]


def iupac_revcomp(pattern):
    """The '-' strand of a degenerate pattern: the reverse of its IUPAC complement (upper case)."""
    return "".join(_IUPAC_COMP[c] for c in reversed(pattern.upper()))


def _as_text(pattern):
    return pattern.decode("latin-1") if isinstance(pattern, (bytes, bytearray)) else str(pattern)


def compile_pattern(pattern, strand="both", degenerate=False, device=0):
    """Check a pattern -> (mode bits, bytes searched on +, bytes searched on -); ValueError for a length outside 1..64, a
    white-space byte in an exact pattern, a non-IUPAC letter in a degenerate one, or a bad strand.  The '-' pattern of an
    exact search is made by fx_revcomp, as Sequence.search makes it."""
    if strand not in _STRANDS:
        raise ValueError("strand must be '+', '-' or 'both', not %r" % (strand,))
    text = _as_text(pattern)
    if not 1 <= len(text) <= MAX_PATTERN:
        raise ValueError("pattern length %d outside 1..%d" % (len(text), MAX_PATTERN))
    mode = _STRANDS[strand]
    if degenerate:
        bad = [c for c in text if c.upper() not in IUPAC]
        if bad:
            raise ValueError("%r is not an IUPAC nucleotide code" % bad[0])
        fwd = text.upper().encode("latin-1")
        rev = iupac_revcomp(text).encode("latin-1") if mode & _lib.FX_SEARCH_MINUS else None
        return mode | _lib.FX_SEARCH_DEGENERATE, fwd, rev
    try:
        fwd = text.encode("latin-1")
    except UnicodeEncodeError:
        raise ValueError("pattern holds a character outside latin-1")
    if any(b in _SPACE for b in fwd):
        raise ValueError("white space in an exact pattern never matches `seq`")
    rev = _lib.revcomp_bytes(fwd, _lib.FX_REVERSE | _lib.FX_COMPLEMENT, device) if mode & _lib.FX_SEARCH_MINUS else None
    return mode, fwd, rev


def search_blob(blob, pattern, strand="both", degenerate=False, uppercase=False, ids=None, max_hits=10**8, device=0):
    """Every hit on a Blob whose FASTA table is resident -> SearchHits (arrays in pinned memory).  ids: ascending 0-based
    record ids or None for all."""
    mode, fwd, rev = compile_pattern(pattern, strand, degenerate, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    try:
        total, hits, _ = blob.fasta_search(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, ids=ids, cap=int(max_hits))
    except _lib.FxError as e:
        raise _lib.too_many(e, "hits", "max_hits", max_hits)
    if hits is None:
        z = np.zeros(0, dtype=np.int64)
        return SearchHits(z, z.copy(), z.copy(), np.zeros(0, dtype=np.uint8))
    rec, starts, strands = hits
    stops = _lib.pinned_empty(total, np.int64)
    np.add(starts, len(fwd), out=stops)
    return SearchHits(rec, starts, stops, strands)


def count_blob(blob, pattern, strand="both", degenerate=False, uppercase=False, device=0):
    """Hits per record on + and on - -> int64[n_records, 2]; the hits themselves never leave the device."""
    mode, fwd, rev = compile_pattern(pattern, strand, degenerate, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    _, _, counts = blob.fasta_search(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, cap=0, counts=True)
    return counts


def compile_approx(pattern, mismatches, anchor=None, strand="both", degenerate=False, device=0):
    """compile_pattern plus the mismatch budget -> (mode bits, bytes on +, bytes on -, mismatches, anchor bit mask).
    anchor: the positions of the FORWARD pattern where no mismatch may fall -- None, a slice, or an iterable of 0-based
    positions; bit j of the mask is letter j (the library mirrors it for '-').  ValueError for what compile_pattern
    refuses, mismatches outside 0..min(8, len(pattern) - 1) or no integer, a position outside the pattern or no integer."""
    mode, fwd, rev = compile_pattern(pattern, strand, degenerate, device)
    L = len(fwd)
    if isinstance(mismatches, bool) or not isinstance(mismatches, (int, np.integer)):
        raise ValueError("mismatches must be an integer, not %r" % (mismatches,))
    if not 0 <= mismatches <= min(MAX_MISMATCH, L - 1):
        raise ValueError("mismatches=%d outside 0..%d for a pattern of %d letters" % (mismatches, min(MAX_MISMATCH, L - 1), L))
    mask = 0
    if isinstance(anchor, slice):
        anchor = range(*anchor.indices(L))
    elif anchor is None:
        anchor = ()
    elif isinstance(anchor, (str, bytes, bytearray)) or not hasattr(anchor, "__iter__"):
        raise ValueError("anchor must be None, a slice or an iterable of positions, not %r" % (anchor,))
    for j in anchor:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)):
            raise ValueError("anchor position %r is not an integer" % (j,))
        if not 0 <= j < L:
            raise ValueError("anchor position %d outside the pattern (0..%d)" % (j, L - 1))
        mask |= 1 << int(j)
    return mode, fwd, rev, int(mismatches), mask


def approx_blob(blob, pattern, mismatches, anchor=None, strand="both", degenerate=False, uppercase=False, ids=None, max_hits=10**8,
                device=0):
    """search_blob with mismatches -> ApproxHits (arrays in pinned memory; mismatches: uint8, the Hamming distance of every
    hit)."""
    mode, fwd, rev, d, mask = compile_approx(pattern, mismatches, anchor, strand, degenerate, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    try:
        total, hits, _ = blob.fasta_search_approx(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, d, mask, ids=ids,
                                                  cap=int(max_hits))
    except _lib.FxError as e:
        raise _lib.too_many(e, "hits", "max_hits", max_hits)
    if hits is None:
        z = np.zeros(0, dtype=np.int64)
        return ApproxHits(z, z.copy(), z.copy(), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
    rec, starts, strands, mis = hits
    stops = _lib.pinned_empty(total, np.int64)
    np.add(starts, len(fwd), out=stops)
    return ApproxHits(rec, starts, stops, strands, mis)


def approx_count_blob(blob, pattern, mismatches, anchor=None, strand="both", degenerate=False, uppercase=False, device=0):
    """Hits of approx_blob per record on + and on - -> int64[n_records, 2]; the hits themselves never leave the device."""
    mode, fwd, rev, d, mask = compile_approx(pattern, mismatches, anchor, strand, degenerate, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    _, _, counts = blob.fasta_search_approx(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, d, mask, cap=0, counts=True)
    return counts


def compile_edit(pattern, edits, strand="both", degenerate=False, report="best", device=0):
    """compile_pattern plus the edit budget and the report -> (mode bits, bytes on +, bytes on -, edits, report code).
    TypeError for edits that is no integer or a report that is no string; ValueError for what compile_pattern refuses, edits
    outside 0..min(8, len(pattern) - 1) or a report other than 'all' / 'best'.  Everything is checked before the '-' pattern
    of an exact search is made."""
    if isinstance(edits, bool) or not isinstance(edits, (int, np.integer)):
        raise TypeError("edits must be an integer, not %r" % (edits,))
    if not isinstance(report, str):
        raise TypeError("report must be 'all' or 'best', not %r" % (report,))
    if report not in _REPORTS:
        raise ValueError("report must be 'all' or 'best', not %r" % (report,))
    if strand not in _STRANDS:
        raise ValueError("strand must be '+', '-' or 'both', not %r" % (strand,))
    L = len(_as_text(pattern))
    if not 1 <= L <= MAX_PATTERN:
        raise ValueError("pattern length %d outside 1..%d" % (L, MAX_PATTERN))
    if not 0 <= edits <= min(MAX_EDITS, L - 1):
        raise ValueError("edits=%d outside 0..%d for a pattern of %d letters" % (edits, min(MAX_EDITS, L - 1), L))
    mode, fwd, rev = compile_pattern(pattern, strand, degenerate, device)
    return mode, fwd, rev, int(edits), _REPORTS[report]


def edit_blob(blob, pattern, edits, strand="both", degenerate=False, report="best", uppercase=False, ids=None, max_hits=10**8,
              device=0):
    """Every end of `pattern` within `edits` edits on a Blob whose FASTA table is resident -> EditHits (arrays in pinned
    memory; edits: uint8, the Levenshtein distance of every row).  max_hits bounds the ENDS, which the device holds before
    report='best' thins them out."""
    mode, fwd, rev, k, rep = compile_edit(pattern, edits, strand, degenerate, report, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    try:
        total, _, rows, _ = blob.fasta_search_edit(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, k, rep, ids=ids, cap=int(max_hits))
    except _lib.FxError as e:
        n = getattr(e, "n_ends", 0)
        if e.code == _lib.FX_ERANGE and n > max_hits:
            raise ValueError("%d ends within %d edits, more than max_hits=%d" % (n, k, max_hits))
        raise
    if rows is None:
        z = np.zeros(0, dtype=np.int64)
        return EditHits(z, z.copy(), z.copy(), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))
    return EditHits(*rows)


def edit_count_blob(blob, pattern, edits, strand="both", degenerate=False, report="best", uppercase=False, device=0):
    """Rows of edit_blob per record on + and on - -> int64[n_records, 2]; the rows themselves never leave the device."""
    mode, fwd, rev, k, rep = compile_edit(pattern, edits, strand, degenerate, report, device)
    if uppercase:
        mode |= _lib.FX_SEARCH_UPPER
    return blob.fasta_search_edit(fwd if mode & _lib.FX_SEARCH_PLUS else None, rev, mode, k, rep, cap=0, counts=True)[3]
