"""Streams that put a chosen byte of a small probe at a chosen offset: the inputs of the seam sweeps over the FASTA and
FASTQ index builds (test_gpu_build_seams.py; the generator itself is checked in test_seam_cases_host.py).  numpy only.

The build hands state over at fixed byte offsets of the stream: the 16-byte chunk of a lane, the 1 KiB row of a wave, the
4 KiB granule, the 8 KiB run of the fused composition scan, the 16 KiB FASTQ record slot, the 32 KiB scan workgroup, the
64 KiB span, the 1 MiB chunk of the granule prefix.  A probe is a few lines that are hard for one of the hand-overs; it is
slid so that the seam falls in front of every byte of it.  In front of the probe stands one line-regular record (FASTA) or
whole four-line records of one size (FASTQ), so whatever goes wrong goes wrong at the probe."""
import numpy as np

EOLS = {"lf": b"\n", "crlf": b"\r\n"}

# one offset per kind: a multiple of its own seam and of no larger one listed (the 1 MiB ones are multiples of all)
SEAMS = {
    "16B": 3 * 4096 + 5 * 16,
    "1K": 3 * 4096 + 2 * 1024,
    "4K": 3 * 4096,
    "8K": 3 * 8192,
    "16K": 3 * 16384,
    "32K": 3 * 32768,
    "64K": 3 * 65536,
    "1M": 1 << 20,
    "2M": 2 << 20,
}


def seam_offset(kind, need=0):
    """the offset of a seam kind; the next one of the same kind (64 KiB further, still a multiple of no larger seam) that leaves
    `need` bytes in front of it, for a long probe or an island"""
    s = SEAMS[kind]
    while s < need or (s % (1 << 20) == 0 and not kind.endswith("M")):
        s += 65536
    return s


def fastq_need(probe_len, bg):
    """bytes a FASTQ placement needs in front of the seam, whichever byte of the probe is marked"""
    return probe_len + (ISLAND_BYTES + 64 if bg == "island_before" else 0) + 512


FASTA_SEAMS = [k for k in SEAMS if k != "16K"]          # the 16 KiB record slot is a FASTQ seam
FASTQ_SEAMS = list(SEAMS)

WIDTH = 60                                               # letters per filler line
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ACGTN = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _letters(rng, n, alpha=_ACGT):
    return alpha[rng.integers(0, alpha.size, n)].tobytes()


def filler_lines(rng, k, eol, width=WIDTH):
    """k whole lines of `width` random letters, generated in one piece"""
    if k <= 0:
        return b""
    a = np.empty((k, width + len(eol)), dtype=np.uint8)
    a[:, :width] = _ACGT[rng.integers(0, 4, (k, width), dtype=np.uint8)]
    a[:, width:] = np.frombuffer(eol, dtype=np.uint8)
    return a.tobytes()


# ----------------------------------------------------------------------------------------------------------- FASTA
def fasta_segment(start, name, probe, mark, target, eol, rng):
    """One header line `name` + 'x' * pad, whole filler lines, then the probe -- written at offset `start` of a stream, with
    byte `mark` of the probe at offset `target`."""
    line = WIDTH + len(eol)
    room = target - mark - start - len(name) - len(eol)
    assert room >= 0, "the seam lies too close in front of the probe"
    k, pad = divmod(room, line)
    return name + b"x" * pad + eol + filler_lines(rng, k, eol) + probe


def place_fasta(probe, mark, seam, d, eol, rng, tail_lines=3):
    """`>bg` + 'x' * pad + eol, whole 60-letter lines of record bg, the probe, tail_lines more whole lines (of whichever
    record the probe left open): byte `mark` of the probe lies at offset seam + d."""
    return fasta_segment(0, b">bg", probe, mark, seam + d, eol, rng) + filler_lines(rng, tail_lines, eol)


def slide(n):
    """(mark, d) for a probe of n bytes: the seam in front of every byte of it and behind its last, two positions more on
    either side -- n + 5 placements"""
    return [(0, 2), (0, 1)] + [(m, 0) for m in range(n)] + [(n - 1, -1), (n - 1, -2), (n - 1, -3)]


def fasta_probes(eol):
    """name -> (probe bytes, placements).  E below is the file's line end."""
    E = eol
    crlf = E == b"\r\n"
    P = {
        "H": b">p1 w1 w2" + E + b"ACGTACGTAC" + E + b"GTACGTACGT" + E + b"ACG" + E + b">p2" + E,
        "H0": b">a" + E + b">b x" + E + b">" + E + b">c" + E,                  # header-only records, an empty name
        "B": b"ACGT" + E + E + E + b"ACGT" + E,                               # blank lines inside bg
        "O1": b"ACGTNACGTNACGTNACGTNACGTNACGTNACGTNACGTNA" + E,               # one 41-letter line, full lines after it: norm = 1
        "O3": b"ACGTNACGTNACGTNACGTNACGTNACGTNACGTNACGTNA" + E + b"GTGTGTGTGTGTGTGTG" + E + b"TTTTT" + E,   # a third distinct length
        "G": b"AC>GT" + E + b"A>" + E,                                        # '>' that starts no line
        "T": b">t1\tx y" + E + b"ACGT" + E + b">t2\x0bx y" + E + b"ACGT" + E + b">t3 \r\n" + b"ACGT" + E,
        "CR": (b"ACGT\n" if crlf else b"AC\rGT" + E + b"ACGT\r\r" + E),     # a bare LF in a CRLF file; stray CRs in an LF file
    }
    assert len(P["O1"]) == 41 + len(E)
    out = {k: (v, slide(len(v))) for k, v in P.items()}
    # LH: a 5000-byte header line, first space at byte 3000: the seam at '>', at the space and at the line end, each +-1
    lh = b">" + b"h" * 2999 + b" " + b"d" * 1999
    assert len(lh) == 5000 and lh.index(b" ") == 3000
    marks = [0, 3000, 5000] + ([5001] if crlf else [])
    out["LH"] = (lh + E + b"ACGTACGTAC" + E, [(m, d) for m in marks for d in (-1, 0, 1)])
    return out


def _cls(c):
    return {10: "n", 13: "r", 62: "g", 32: "w", 9: "w", 11: "w"}.get(c, "a")


def end_marks(probe):
    """Cut points of a probe, one per kind of (byte before the cut, byte behind it, inside a header line or not): the last line
    terminated, unterminated, ending in CR, a bare '>' or a bare header among them.  0: the stream ends with the filler."""
    seen, out, in_hdr = set(), [0], False
    for m in range(1, len(probe) + 1):
        if probe[m - 1] == 62 and (m == 1 or probe[m - 2] == 10):
            in_hdr = True
        key = (_cls(probe[m - 1]), _cls(probe[m]) if m < len(probe) else "$", in_hdr)
        if probe[m - 1] == 10:
            in_hdr = False
        if key not in seen:
            seen.add(key)
            out.append(m)
    return out


def truncated_fasta(probe, mark, seam, d, eol, rng):
    """the stream that ends right in front of byte `mark` of the probe, seam + d bytes long"""
    raw = place_fasta(probe, mark, seam, d, eol, rng, tail_lines=0)
    return raw[:seam + d]


def width_sweep(widths, eol, rng, min_bytes=3 * 4096 + 100):
    """one stream, one record per line width, each of at least three granules and with a short last line"""
    parts = []
    for w in widths:
        k = -(-min_bytes // (w + len(eol)))
        parts.append(b">w%d width %d" % (w, w) + eol + filler_lines(rng, k, eol, w) + _letters(rng, max(w // 2, 1) if w > 1 else 0) + (eol if w > 1 else b""))
    return b"".join(parts)


def one_line_records(n, eol=b"\n"):
    """n records of one 8-letter line each"""
    a = np.empty((n, 20), dtype=np.uint8)
    a[:] = np.frombuffer(b">r000000 d\nACGTACGT\n", dtype=np.uint8)
    num = np.arange(n)
    for j in range(6):
        a[:, 7 - j] = 48 + (num // 10 ** j) % 10
    raw = a.tobytes()
    return raw if eol == b"\n" else raw.replace(b"\n", eol)


def run_seam_stream(total, run, eol, rng):
    """A stream of a little more than `total` bytes with probe H at six seams of the `run`-byte runs of the fused composition
    scan: '>' at -1, 0, +1 and the header's line end at -1, 0, +1.  -> (bytes, the six (seam, mark, d))."""
    H = fasta_probes(eol)["H"][0]
    e = H.index(b"\n")                                                       # the LF of the header line
    nruns = total // run
    cases = [(0, -1), (0, 0), (0, 1), (e, -1), (e, 0), (e, 1)]
    parts, pos, where = [], 0, []
    for i, (mark, d) in enumerate(cases):
        seam = (3 + i * (nruns - 4) // 5) * run                              # the first near the start, the last near the end
        seg = fasta_segment(pos, b">f%d" % i, H, mark, seam + d, eol, rng)
        parts.append(seg)
        pos += len(seg)
        where.append((seam, mark, d))
    room = total + 100 - pos
    parts.append(filler_lines(rng, max(room // (WIDTH + len(eol)) + 1, 1), eol))
    return b"".join(parts), where


# ----------------------------------------------------------------------------------------------------------- FASTQ
FASTQ_BACKGROUNDS = ("r150", "r150crlf", "r20", "island_before", "island_after")
ISLAND_BYTES = 4 * 4096 + 512                            # at least three whole granules of 8-base reads wherever it starts
ISLAND_MIN_STREAM = 800 * 1024                           # ... in a stream long enough that the sampled line density stays that of 150-base reads
FQL_CAP = 128                                            # line records of a granule slot: more newlines than this and the granule overflows


def fastq_bg_eol(bg):
    return b"\r\n" if bg == "r150crlf" else b"\n"


def _fastq_records(rng, k, rlen, eol, tag):
    """k whole records of one size: @<tag><6 digits> / rlen bases / + / rlen qualities"""
    if k <= 0:
        return b""
    e = len(eol)
    head = 1 + len(tag) + 6
    size = head + e + rlen + e + 1 + e + rlen + e
    a = np.empty((k, size), dtype=np.uint8)
    a[:, 0] = 64
    a[:, 1:1 + len(tag)] = np.frombuffer(tag, dtype=np.uint8)
    num = np.arange(k)
    for j in range(6):
        a[:, head - 1 - j] = 48 + (num // 10 ** j) % 10
    p = head
    a[:, p:p + e] = np.frombuffer(eol, dtype=np.uint8); p += e
    a[:, p:p + rlen] = _ACGTN[rng.integers(0, 5, (k, rlen), dtype=np.uint8)]; p += rlen
    a[:, p:p + e] = np.frombuffer(eol, dtype=np.uint8); p += e
    a[:, p] = 43; p += 1
    a[:, p:p + e] = np.frombuffer(eol, dtype=np.uint8); p += e
    a[:, p:p + rlen] = rng.integers(65, 74, (k, rlen), dtype=np.uint8); p += rlen
    a[:, p:p + e] = np.frombuffer(eol, dtype=np.uint8)
    return a.tobytes()


def fastq_record_size(rlen, eol, tag):
    return 1 + len(tag) + 6 + 2 * rlen + 1 + 4 * len(eol)


def place_fastq(probe, mark, seam, d, bg, rng, tail_records=3):
    """Whole four-line records of one size (the first one's name padded), the probe, tail_records more records: byte `mark` of
    the probe lies at offset seam + d.  bg: one of FASTQ_BACKGROUNDS.  -> (bytes, (island start, island end) or None)."""
    eol = fastq_bg_eol(bg)
    rlen, tag = (20, b"s") if bg == "r20" else (150, b"bg")
    size = fastq_record_size(rlen, eol, tag)
    front = b"" if bg != "island_before" else _island(rng)
    back = b"" if bg != "island_after" else _island(rng)
    room = seam + d - mark - len(front) - size
    assert room >= 0, "the seam lies too close in front of the probe"
    k, pad = divmod(room, size)
    first = _fastq_records(rng, 1, rlen, eol, tag)
    cut = first.index(eol)
    first = first[:cut] + b"x" * pad + first[cut:]
    head = first + _fastq_records(rng, k, rlen, eol, tag)
    body = head + front + probe + back
    if bg.startswith("island"):
        tail_records = max(tail_records, -(-(ISLAND_MIN_STREAM - len(body)) // size))
    raw = body + _fastq_records(rng, tail_records, rlen, eol, tag)
    island = None
    if front:
        island = (len(head), len(head) + len(front))
    elif back:
        island = (len(head) + len(probe), len(head) + len(probe) + len(back))
    return raw, island


def _island(rng):
    size = fastq_record_size(8, b"\n", b"i")
    return _fastq_records(rng, -(-ISLAND_BYTES // size), 8, b"\n", b"i")


def fastq_probes(eol):
    """name -> (probe bytes, placements): well-formed four-line records"""
    E = eol
    P = {
        "R": b"@q1 desc x" + E + b"ACGTN" + E + b"+" + E + b"IIIII" + E,
        "RP": b"@q1 desc x" + E + b"ACGTN" + E + b"+q1 desc x" + E + b"IIIII" + E,            # the '+' line repeats the name
        "RQ": b"@q2" + E + b"ACGT" + E + b"+" + E + b"@+>I" + E + b"@@x" + E + b"AC" + E + b"+" + E + b"II" + E,
        "R1": b"@q3 one" + E + b"A" + E + b"+" + E + b"I" + E,                               # a one-base read
        "RS": (b"@ s1" + E + b"ACG" + E + b"+" + E + b"III" + E + b"@nospace" + E + b"ACG" + E + b"+" + E + b"III" + E +
               b"@tab\tz w" + E + b"ACG" + E + b"+" + E + b"III" + E),
    }
    out = {k: (v, slide(len(v))) for k, v in P.items()}
    # RL: a 9000-base read, the seam at its four line ends, each +-1
    n = 9000
    rl = b"@long read" + E + b"ACGTN" * (n // 5) + E + b"+" + E + b"F" * n + E
    ends, p = [], 0
    for _ in range(4):
        p = rl.index(b"\n", p) + 1
        ends.append(p - 1)
    out["RL"] = (rl, [(m, d) for m in ends for d in (-1, 0, 1)])
    return out


def newlines_per_granule(raw):
    a = np.frombuffer(raw, dtype=np.uint8)
    pos = np.nonzero(a == 10)[0]
    return np.bincount(pos // 4096, minlength=len(raw) // 4096 + 1)
