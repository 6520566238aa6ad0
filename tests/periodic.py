"""Periodic streams and their exact answers: a FASTA record that is R copies of one block B of m letters, a FASTQ stream that
is R copies of one block of reads.  Such a stream is built in device memory in milliseconds at any size, and what a pass
must say about it follows from the CPU truth of two or three copies of the block -- the rules below.  Plain numpy; torch
is imported inside the builders only.  tests/test_periodic_host.py pins every rule to the truth of five copies.

The rules hold for a pass whose every row, and whatever decides that row, fits into fewer than m letters:

  rows      tile_rows: the rows of B*3 that start in the first copy stay, those that start in the middle copy repeat once
            per inner copy, those that start in the last copy move to the last copy.
  counts    tile_counts: c(B^R) = R c(B) + (R - 1) (c(B+B) - 2 c(B)); the second term is what one seam adds.
  sets      the distinct k-mers or sketch keys of B^R are those of B+B.
  regions   region_rule: the class counts of [a, b) from the prefix sums of B.
  letters   letters_at: B indexed modulo m."""
import numpy as np

import fetch_truth as T

MOTIF = "GATTACAGCTTGCCAT"                                    # 16 letters, no border, not its own reverse complement
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
ORF_CODONS = 300                                             # codons between ATG and the stop of a planted reading frame
STOPS = ("TAA", "TAG", "TGA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


# ------------------------------------------------------------------ the rules
def tile_rows(rows3, R, m, ncoord, order=None):
    """The rows of B*R from the rows of B*3 (len(B) = m; a row's first ncoord fields are coordinates, the first of them its
    start; every field an integer) -> int64[n, fields].  order: the fields the pass orders its rows by, most significant
    first (None: by start, ties as in rows3)."""
    assert R >= 3 and ncoord >= 1
    rows3 = np.asarray(rows3, dtype=np.int64)
    if rows3.size == 0:
        return rows3.reshape(0, max(ncoord, rows3.shape[-1] if rows3.ndim == 2 else ncoord))
    co = rows3[:, :ncoord]
    assert (co.max(axis=1) - co.min(axis=1) < m).all(), "a row spans m letters or more: the tiling rule does not hold"
    assert (co.min(axis=1) == co[:, 0]).all() and (co[:, 0] >= 0).all() and (co.max(axis=1) <= 3 * m).all()
    start = rows3[:, 0]
    first, mid, last = rows3[start < m], rows3[(start >= m) & (start < 2 * m)], rows3[start >= 2 * m]
    shift = np.zeros(rows3.shape[1], dtype=np.int64)
    shift[:ncoord] = m
    inner = (mid[None, :, :] + np.arange(R - 2, dtype=np.int64)[:, None, None] * shift).reshape(-1, rows3.shape[1])
    out = np.concatenate([first, inner, last + (R - 3) * shift])
    keys = (0,) if order is None else tuple(order)
    return out[np.lexsort([out[:, c] for c in reversed(keys)])]          # lexsort is stable: ties stay as in rows3


def tile_counts(c1, c2, R):
    """Whatever is counted per window: c1 = the counts of B, c2 = those of B+B -> those of B^R."""
    c1, c2 = np.asarray(c1, dtype=np.int64), np.asarray(c2, dtype=np.int64)
    return R * c1 + (R - 1) * (c2 - 2 * c1)


def tile_table(t1, t2, R):
    """tile_counts for sparse tables (codes ascending, counts): the codes of B^R are those of B+B."""
    (u1, n1), (u2, n2) = t1, t2
    assert np.isin(u1, u2).all()
    c1 = np.zeros(u2.size, dtype=np.int64)
    c1[np.searchsorted(u2, u1)] = n1
    return u2.astype(np.int64), tile_counts(c1, n2, R)


_CLASS = np.full(256, 5, dtype=np.int64)                     # A C G T N other, as tests/annot_truth.py
for _j, _c in enumerate("ACGTN"):
    _CLASS[ord(_c)] = _CLASS[ord(_c.lower())] = _j


def class_prefix(B):
    """int64[m + 1, 7]: the counts A C G T N other masked of B[:x] for every x."""
    b = np.frombuffer(B.encode("latin-1"), dtype=np.uint8)
    one = np.zeros((b.size, 7), dtype=np.int64)
    one[np.arange(b.size), _CLASS[b]] = 1
    one[:, 6] = (b >= ord("a")) & (b <= ord("z"))
    return np.concatenate([np.zeros((1, 7), dtype=np.int64), np.cumsum(one, axis=0)])


def region_rule(P, a, b):
    """The seven counts of the letters [a, b) of B^R (a, b int64 arrays) from P = class_prefix(B)."""
    m = P.shape[0] - 1
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    upto = lambda x: (x // m)[:, None] * P[m][None, :] + P[x % m]
    return upto(b) - upto(a)


def letters_at(B, a, b):
    """The letters [a, b) of B^R as bytes."""
    src = np.frombuffer(B.encode("latin-1"), dtype=np.uint8)
    return src[np.arange(a, b, dtype=np.int64) % len(B)].tobytes()


def finds(s, q):
    """Every start of q in s, overlapping ones included."""
    out, j = [], s.find(q)
    while j >= 0:
        out.append(j)
        j = s.find(q, j + 1)
    return out


def search_rows(s, p):
    """(start, strand) of p on + (0) and of its reverse complement (1) in s, by (start, strand)."""
    return sorted([(j, 0) for j in finds(s, p)] + [(j, 1) for j in finds(s, revcomp(p))])


# ------------------------------------------------------------------ the block
def _mutate(word, at):
    return "".join("ACGT"[("ACGT".index(c) + 1) % 4] if j in at else c for j, c in enumerate(word))


def make_block(m, seed=20261020):
    """m >= 5700 letters, m % 3 == 0: random A C G T with, planted at fixed places,
      - CAG CAG CAG at both ends: three copies at either end of the record, six across every seam;
      - MOTIF at 52 (across the end of a line of 57 or 60) and at 1000, its reverse complement at 1500, copies at Hamming
        distance 1, 2 and 3 at 2000, 2100 and 2200;
      - tandem repeats: A x 20 at 2500, (TTG) x 8 at 2600, (AACCTG) x 5 at 2700;
      - N x 50 at 3030, N x 7 at 3100, lower case from 3200 to 3500;
      - a reading frame of ORF_CODONS codons from an ATG at 3600 to a TAA, one on the other strand from 4600."""
    assert m >= 5700 and m % 3 == 0
    rng = np.random.default_rng(seed)
    s = list("".join(np.array(list("ACGT"))[rng.integers(0, 4, m)]))

    def put(at, word):
        s[at:at + len(word)] = list(word)

    codons = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT" if a + b + c not in STOPS]
    body = lambda: "".join(codons[i] for i in rng.integers(0, len(codons), ORF_CODONS))
    put(0, "CAGCAGCAGT")
    put(m - 10, "TCAGCAGCAG")
    put(52, MOTIF)
    put(1000, MOTIF)
    put(1500, revcomp(MOTIF))
    put(2000, _mutate(MOTIF, (5,)))
    put(2100, _mutate(MOTIF, (6, 11)))
    put(2200, _mutate(MOTIF, (4, 8, 14)))
    put(2499, "C" + "A" * 20 + "G")
    put(2599, "A" + "TTG" * 8 + "C")
    put(2699, "G" + "AACCTG" * 5 + "T")
    put(3030, "N" * 50)
    put(3100, "N" * 7)
    put(3200, "".join(s[3200:3500]).lower())
    put(3597, "TAA" + "ATG" + body() + "TAA")
    put(4597, "TAA" + revcomp("ATG" + body() + "TAA") + "TTA")
    assert len(s) == m
    return "".join(s)


# ------------------------------------------------------------------ FASTA
def small_fasta(tag):
    """-> (bytes, [seq strings]): five records named <tag>0 .. <tag>4 with lines of 60, 17, none, 70 and 50 letters: A C G T
    with every 41st letter another one (IUPAC codes, lower case); a soft-masked stretch, an N run, MOTIF on both strands, a
    homopolymer, an empty record.  Every line is terminated."""
    rng = np.random.default_rng(41)
    odd = "NRYKMacgtnSWBDHVU"

    def letters(n):
        s = np.array(list("ACGT"))[rng.integers(0, 4, n)]
        s[7::41] = [odd[j % len(odd)] for j in range(len(s[7::41]))]
        return "".join(s)

    seqs = [letters(130), letters(200), "", letters(500), letters(120)]
    seqs[0] = seqs[0][:20] + MOTIF + seqs[0][36:70] + seqs[0][70:110].lower() + seqs[0][110:]
    seqs[1] = seqs[1][:50] + "N" * 30 + seqs[1][80:]
    seqs[3] = seqs[3][:100] + revcomp(MOTIF) + seqs[3][116:300] + "A" * 15 + "C" + seqs[3][316:]
    widths = (60, 17, 1, 70, 50)
    raw = b""
    for i, (s, w) in enumerate(zip(seqs, widths)):
        raw += b">%s%d record %d\n" % (tag.encode(), i, i)
        if s:
            raw += T.fold(s.encode("latin-1"), [w], b"\n")
    return raw, seqs


def copies_for(m, letters=(1 << 32) + (1 << 26)):
    """The smallest R that puts more than `letters` letters into the record."""
    return letters // m + 1


def block_lines(B, width, eol):
    assert len(B) % width == 0 and len(B) % 3 == 0
    nl = b"\r\n" if eol == 2 else b"\n"
    one = T.fold(B.encode("latin-1"), [width], nl)
    assert len(one) % 2 == 1, "an odd number of bytes per copy puts a copy at every phase of a 256-byte run"
    return one


def giant_fasta(device, head, B, width, eol, R, tail):
    """head + '>giant' + R copies of B in lines of `width` (eol 1: LF, 2: CR LF) + tail, the last terminator of the stream
    cut off -> (uint8 tensor on `device`, layout).  layout: the byte offset of every part, the record ids, and the table
    row of the giant record as the parts say it must be."""
    import torch
    one = block_lines(B, width, eol)
    hdr = b">giant copies of one block" + (b"\r\n" if eol == 2 else b"\n")
    assert head.endswith(b"\n") and tail.endswith(b"\n")
    tail = tail[:-1]
    n_head, n_tail = head.count(b">"), tail.count(b">")
    body_off = len(head) + len(hdr)
    tail_off = body_off + R * len(one)
    n = tail_off + len(tail)
    out = torch.empty(n, dtype=torch.uint8, device=device)
    put = lambda at, b: out[at:at + len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    put(0, head + hdr)
    out[body_off:tail_off].copy_(torch.frombuffer(bytearray(one), dtype=torch.uint8).to(device).repeat(R))
    put(tail_off, tail)
    layout = dict(n_bytes=n, head_off=0, giant_off=len(head), body_off=body_off, tail_off=tail_off, copy_bytes=len(one),
                  head_ids=list(range(n_head)), giant=n_head, tail_ids=list(range(n_head + 1, n_head + 1 + n_tail)),
                  row=dict(boff=body_off, blen=R * len(one), slen=R * len(B), llen=width + eol, elen=eol, norm=1))
    return out, layout


def expected_rows(head, tail, layout):
    """The table rows of the whole stream: those of head and tail by tests/fetch_truth.py, the giant's from the layout."""
    rows = T.fasta_rows(head)
    rows.append(dict(layout["row"]))
    for r in T.fasta_rows(tail):
        rows.append(dict(r, boff=r["boff"] + layout["tail_off"]))
    return rows


# ------------------------------------------------------------------ FASTQ
BARCODES = ("ACGTACGT", "TTGGCCAA", "GATCGATC")
ADAPTER = "AGATCGGAAGAGCACACGTC"


def fastq_block(n_reads=1000, seed=5):
    """-> (bytes of odd length, [(name, seq, qual)]).  Read i has (i * 37) % 301 letters: every length 0..300; names of
    several lengths, some with a comment that ends in a barcode (every other one with a letter changed); quality bytes run through 33..126; every 50th read repeats an earlier one, every
    50th is the reverse complement of one; every 10th begins with a barcode and ends in the adapter; a few N."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads):
        L = (i * 37) % 301
        s = "".join(np.array(list("ACGT"))[rng.integers(0, 4, L)])
        if i % 50 == 49:
            s = reads[i - 10][1]
        elif i % 50 == 48:
            s = revcomp(reads[i - 20][1])
        elif i % 10 == 3 and L >= 60:
            s = BARCODES[(i // 10) % 3] + s[8:L - 12] + ADAPTER[:12]
        elif i % 17 == 5 and L > 4:
            s = s[:L // 2] + "N" + s[L // 2 + 1:]
        L = len(s)
        q = bytes(33 + (i * 13 + 5 * j) % 94 for j in range(L)).decode()
        name = "r%d" % i + ("/1" if i % 3 == 0 else "") + (" %d:N:0:%s" % (1 + i % 2, BARCODES[i % 3] if i % 8 == 1 else _mutate(BARCODES[i % 3], (i % 8,))) if i % 4 == 1 else "")
        reads.append((name, s, q))
    raw = "".join("@%s\n%s\n+\n%s\n" % r for r in reads).encode("latin-1")
    if len(raw) % 2 == 0:
        name, s, q = reads[-1]
        reads[-1] = (name + "x", s, q)
        raw = "".join("@%s\n%s\n+\n%s\n" % r for r in reads).encode("latin-1")
    return raw, reads


def fastq_mate_block(reads, seed=6):
    """The mates of fastq_block's reads as a block of another (odd) length: 15 random letters, then the reverse complement of
    the read without its last 7 letters, every 9th with two letters changed -> (bytes, [(name, seq, qual)])."""
    rng = np.random.default_rng(seed)
    mates = []
    for i, (name, s, _) in enumerate(reads):
        t = "".join(np.array(list("ACGT"))[rng.integers(0, 4, 15)]) + revcomp(s.replace("N", "A"))[:max(len(s) - 7, 0)]
        if i % 9 == 4 and len(t) > 40:
            t = _mutate(t, (20, 33))
        q = bytes(33 + (i * 11 + 3 * j) % 94 for j in range(len(t))).decode()
        mates.append((name.replace("/1", "/2"), t, q))
    raw = "".join("@%s\n%s\n+\n%s\n" % r for r in mates).encode("latin-1")
    if len(raw) % 2 == 0:
        name, t, q = mates[-1]
        mates[-1] = (name + "y", t, q)
        raw = "".join("@%s\n%s\n+\n%s\n" % r for r in mates).encode("latin-1")
    return raw, mates


def periodic_fastq(device, block_bytes, R):
    """R copies of the block as one uint8 tensor on `device`."""
    import torch
    assert len(block_bytes) % 2 == 1
    return torch.frombuffer(bytearray(block_bytes), dtype=torch.uint8).to(device).repeat(R)
