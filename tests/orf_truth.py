"""Plain Python truth of Fasta.orfs and Fasta.translate_many, straight from the definition: per strand and residue class the
maximal runs of consecutive codons that are neither a stop nor invalid; the reverse strand by reverse-complementing the
string and mapping the coordinates back.  It shares nothing with the package.

Coordinates are 0-based and half-open in the `seq` string.  Letters fold to A C G T whatever their case; every other letter is
invalid.  A row is (start, stop, frame, flags): frame +1 + start % 3 on the forward strand, -(1 + (slen - stop) % 3) on the
reverse strand; flags in the ORF's own orientation: 1 a STOP codon follows the 3' end, 2 a STOP codon precedes the segment at
its 5' end, 4 the first codon of the row is a START codon."""

# the standard genetic code, written out
STANDARD = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W",
    "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R",
    "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}
STANDARD_STOPS = ("TAA", "TAG", "TGA")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def fold(seq):
    """The letters as the search sees them: A C G T for either case, '?' for every other letter."""
    return "".join(ch.upper() if ch.upper() in "ACGT" else "?" for ch in seq)


def revcomp(folded):
    return "".join(COMP.get(ch, "?") for ch in reversed(folded))


STOP, START, OTHER, INVALID = "stop", "start", "other", "invalid"


def codon_class(codon, stops, starts):
    if "?" in codon:
        return INVALID
    if codon in stops:
        return STOP
    return START if codon in starts else OTHER


def forward_rows(t, stops, starts, mode, min_len):
    """The rows of the forward strand of the folded text t -> [(start, stop, flags, close)], close = the coordinate at which
    the segment ends."""
    rows, need = [], max(min_len, 3)
    for c in range(3):
        kinds = [(j, codon_class(t[j:j + 3], stops, starts)) for j in range(c, len(t) - 2, 3)]
        if not kinds:
            continue
        a, before = c, None                                  # left end of the open segment, the kind of the break in front of it
        first_start = None
        for j, kind in kinds + [(kinds[-1][0] + 3, None)]:  # (None: the end of the last full codon closes the last segment)
            if kind in (START, OTHER):
                if kind == START and first_start is None:
                    first_start = j
                continue
            b = j
            s = a if mode == "stop" else first_start
            if b > a and s is not None and b - s >= need:
                flags = (1 if kind == STOP else 0) | (2 if before == STOP else 0) | (4 if first_start == s else 0)
                rows.append((s, b, flags, b))
            a, before, first_start = j + 3, kind, None
    return rows


def orfs(seq, stops=STANDARD_STOPS, starts=("ATG",), mode="start", min_len=3, strand="both"):
    """-> [(start, stop, frame, flags)] in the order of the definition: by the forward coordinate at which a left-to-right
    walk closes the row's segment, forward before reverse."""
    t = fold(seq)
    n = len(t)
    stops = set(stops)
    starts = set(starts) - stops                             # where a codon is both, the stop wins
    keyed = []
    if strand in ("+", "both"):
        for s, b, flags, close in forward_rows(t, stops, starts, mode, min_len):
            keyed.append((close, 0, (s, b, 1 + s % 3, flags)))
    if strand in ("-", "both"):
        rc = revcomp(t)
        for s, e, flags, close in forward_rows(rc, stops, starts, mode, min_len):
            # the segment [a', close) of the reverse complement is [n - close, n - a') of the text; a left-to-right walk of the
            # text closes it at its right end n - a', which the walk of the reverse complement knows as the segment's left end
            a_rc = _segment_left(rc, s, stops)
            keyed.append((n - a_rc, 1, (n - e, n - s, -(1 + s % 3), flags)))
    keyed.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in keyed]


def _segment_left(t, s, stops):
    """Left end of the segment of the folded text t that holds the codon at s: walk left while the codon in front is no break."""
    a = s
    while a - 3 >= 0 and codon_class(t[a - 3:a], stops, ()) not in (STOP, INVALID):
        a -= 3
    return a


def close_coordinate(seq, row, stops=STANDARD_STOPS):
    """The forward coordinate at which a left-to-right walk closes the segment of a row (the second key of the row order)."""
    t = fold(seq)
    start, stop, frame, _ = row
    if frame > 0:
        return stop
    rc = revcomp(t)
    return len(t) - _segment_left(rc, len(t) - stop, set(stops))


def translate(seq, strand="+", aa=None, unknown="X"):
    """Table translation of a `seq` string (strand '-': of its reverse complement): len // 3 amino acids, an invalid codon gives
    `unknown`, no codon is rewritten to M."""
    aa = STANDARD if aa is None else aa
    t = fold(seq)
    if strand == "-":
        t = revcomp(t)
    return "".join(aa.get(t[i:i + 3], unknown) if "?" not in t[i:i + 3] else unknown for i in range(0, len(t) - len(t) % 3, 3))
