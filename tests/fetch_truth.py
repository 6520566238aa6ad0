"""The fetch kernels' reference, written out plainly, and the inputs of the fetch sweep.

Nothing here imports the package or the oracle: tests/test_fetch_truth_host.py pins every function below to the oracle
(and the committed reference vectors) on the CPU, and tests/test_gpu_fetch_sweep.py then trusts the kernels to it."""
import random

import numpy as np

# ------------------------------------------------------------------ the operations
_SPACE = b"\n\r "                                    # jump_table: 10, 13 and 32 are dropped, nothing else
_LOWER, _UPPER = b"abcdefghijklmnopqrstuvwxyz", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
_TO_UPPER = bytes.maketrans(_LOWER, _UPPER)


def despace(b):
    return bytes(b).translate(None, _SPACE)


def comp_table():
    """IUPAC complement: A<->T C<->G M<->K R<->Y V<->B H<->D and U->A, case kept, every other byte itself."""
    src, dst = b"", b""
    for x, y in (b"AT", b"CG", b"MK", b"RY", b"VB", b"HD"):
        src += bytes([x, y, x + 32, y + 32])
        dst += bytes([y, x, y + 32, x + 32])
    return bytes.maketrans(src + b"Uu", dst + b"Aa")


_COMP = comp_table()


def apply_flags(s, flags):
    """upper (1), then complement (4), then reverse (2)."""
    s = bytes(s)
    if flags & 1:
        s = s.translate(_TO_UPPER)
    if flags & 4:
        s = s.translate(_COMP)
    if flags & 2:
        s = s[::-1]
    return s


def arith_range(row, a, b):
    """Byte range of bases [a, b) of a record whose every line but the last holds llen - elen bases."""
    bpl = row["llen"] - row["elen"]
    return row["boff"] + a + row["elen"] * (a // bpl), (b - a) + row["elen"] * (b // bpl - a // bpl)


def slice_by_id(raw, row, a, b, flags, regular):
    """Bases [a, b) of the record `row`.  regular: the bytes the line arithmetic names, despaced, cut to b - a; otherwise
    the despaced record, sliced.  The flags apply to what was obtained (a short answer is reversed as it is)."""
    if regular:
        off, blen = arith_range(row, a, b)
        s = despace(raw[off:off + blen])[:b - a]
    else:
        s = despace(raw[row["boff"]:row["boff"] + row["blen"]])[a:b]
    return apply_flags(s, flags)


def range_fetch(raw, off, blen, take, skip, flags):
    """fetch by byte range: despace [off, off + blen) (short at the end of the stream), drop `skip`, keep `take`."""
    return apply_flags(despace(raw[off:off + blen])[skip:skip + take], flags)


def fastq_read(raw, soff, qoff, n, phred, flags):
    """-> (seq, qual, quali): quali = byte - phred wrapped to int8; phred 0 means 33, as in the reference's getter."""
    qual = raw[qoff:qoff + n]
    q = (np.frombuffer(qual, dtype=np.uint8).astype(np.int16) - (phred or 33)).astype(np.int8)
    return apply_flags(raw[soff:soff + n], flags), qual, q


def fasta_rows(raw):
    """The index rows of a FASTA stream, line by line: boff, blen, slen, llen, elen, norm per header line.  blen counts a
    virtual newline behind a last line that has none; elen comes from the header line alone; slen counts every byte of a
    sequence line in front of its terminator."""
    rows, pos, cur = [], 0, None
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for s in lines:
        n = len(s)
        pos += n + 1
        if s[:1] == b">":
            if cur:
                cur["blen"] = pos - n - 1 - cur["boff"]
                rows.append(cur)
            cur = dict(boff=pos, blen=0, slen=0, llen=0, elen=2 if s.endswith(b"\r") else 1, bad=0)
            continue
        if cur is None:
            continue
        if cur["llen"] and cur["llen"] != n + 1:
            cur["bad"] += 1
        if not cur["llen"]:
            cur["llen"] = n + 1
        cur["slen"] += n - cur["elen"] + 1
    if cur:
        cur["blen"] = pos - cur["boff"]
        rows.append(cur)
    for r in rows:
        r["norm"] = 0 if r.pop("bad") > 1 else 1
    return rows


def fastq_rows(raw):
    """(soff, qoff, rlen) of every read of a four-line FASTQ stream; a CR in front of the newline is not a base."""
    rows, pos, lines = [], 0, raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for k, s in enumerate(lines):
        if k % 4 == 1:
            soff, rlen = pos, len(s) - (1 if s.endswith(b"\r") else 0)
        elif k % 4 == 3:
            rows.append((soff, pos, rlen))
        pos += len(s) + 1
    return rows


# ------------------------------------------------------------------ FASTA shapes
ALPHABET = b"ACGTNacgtnRYKMBDHVUryk"                 # upper and complement both change bytes of it
HEAD = b">swept record in a longer file"            # 30 bytes: at least 16 in front of the first base
TAIL_BASES = 40                                      # ... and a record behind it: more than 32 bytes behind the last base


def bases(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(ALPHABET) for _ in range(n))


def fold(seq, widths, nl, last_nl=True):
    """seq cut into lines of widths[0], widths[1], ... (the last width repeats), each ended by nl."""
    out, p, k = [], 0, 0
    while p < len(seq):
        w = widths[min(k, len(widths) - 1)]
        out.append(seq[p:p + w])
        p += w
        k += 1
    s = nl.join(out) + nl
    return s if last_nl else s[:-1]


class Shape:
    """One FASTA stream and the records of it that the sweep queries.  regular[id]: do slices of that record follow the
    line arithmetic?  force: records whose table row has to SAY line-regular although the stream disagrees.  kind: "inside"
    (16 bytes in front of the first base and 32 behind the last of every swept record), "front" or "back" (not so)."""

    def __init__(self, name, raw, ids, regular, kind="inside", force=(), clean=False):
        self.name, self.raw, self.ids, self.kind, self.force, self.clean = name, raw, list(ids), kind, tuple(force), clean
        self.regular = dict(zip(self.ids, regular))
        self.rows = fasta_rows(raw)

    def slen(self, rid):
        return self.rows[rid]["slen"]

    def margins(self, rid):
        """(bytes in front of the first base, bytes behind the last base) of a record."""
        r = self.rows[rid]
        body = self.raw[r["boff"]:r["boff"] + r["blen"]]
        last = max(k for k, c in enumerate(body) if c not in (10, 13))
        return r["boff"], len(self.raw) - (r["boff"] + last + 1)


def _tail(nl, seed=7):
    return b">tail record" + nl + fold(bases(TAIL_BASES, seed), [TAIL_BASES], nl)


def shape_lines(name, widths, slen, el, head=HEAD, kind="inside", regular=True, force=False, clean=False, edit=None, seed=None):
    """header, one record of slen bases in lines of `widths`, a tail record.  edit(seq) may change bytes of the bases."""
    nl = b"\r\n" if el == 2 else b"\n"
    seq = bases(slen, seed if seed is not None else 1000 * widths[0] + el)
    if edit:
        seq = edit(seq)
    raw = head + nl + fold(seq, widths, nl) + _tail(nl)
    return Shape(name, raw, [0], [regular], kind, force=[0] if force else (), clean=clean)


A_SMALL = (16, 17, 18, 31, 32, 33)                  # slen = 3 * bpl + 5
A_LARGE = (60, 70)                                   # slen = 2 * bpl + 40: answers of two and three steps of 64 bytes


def slen_a(bpl):
    return 3 * bpl + 5 if bpl in A_SMALL else 2 * bpl + 40


def shape_a(bpl, el):
    return shape_lines("bpl%d_el%d" % (bpl, el), [bpl], slen_a(bpl), el, clean=True)


def shapes_a():
    return [shape_a(bpl, el) for el in (1, 2) for bpl in A_SMALL + A_LARGE]


def _put(k, c):
    return lambda s: s[:k] + c + s[k + 1:]


def shape_start(el=1):
    """fewer than 16 bytes in front of the first base"""
    return shape_lines("start_el%d" % el, [20], 50, el, head=b">a", kind="front", clean=True)


def shape_end(el, final_nl):
    """the last record of the stream: fewer than 32 bytes behind its last base"""
    nl = b"\r\n" if el == 2 else b"\n"
    raw = b">first record of two" + nl + fold(bases(40, 3), [20], nl) + HEAD + nl + fold(bases(50, 50 + el), [20], nl)
    if not final_nl:
        raw = raw[:-1]
    return Shape("end_el%d_%s" % (el, "nl" if final_nl else "nonl"), raw, [1], [True], kind="back", clean=True)


def shape_odd_line(force):
    """lines of 20, 7, 20, 20 bases: norm = 1 (one line of another length) and not line-regular"""
    return shape_lines("odd_line" + (":forced" if force else ""), [20, 7, 20], 67, 1, regular=force, force=force)


def shape_space():
    """a space inside a line: the index counts it as a base, the fetch drops it; line-regular by its columns"""
    return shape_lines("space", [20], 50, 1, edit=_put(27, b" "))


def shape_empty_between():
    nl = b"\n"
    raw = (HEAD + nl + fold(bases(50, 11), [20], nl) + b">empty" + nl + b">third record, also swept" + nl +
           fold(bases(45, 12), [18], nl) + _tail(nl))
    return Shape("empty_between", raw, [0, 2], [True, True], clean=True)


def shapes_b():
    out = [shape_lines("bpl%d_el%d" % (bpl, el), [bpl], 50, el, clean=True) for bpl in (1, 2, 15) for el in (1, 2)]
    out += [shape_start(1), shape_start(2)]
    out += [shape_end(1, True), shape_end(1, False), shape_end(2, True), shape_end(2, False)]
    out += [shape_odd_line(False),
            shape_lines("two_odd_lines", [20, 7, 9, 20], 56, 1, regular=False),
            shape_space(),
            shape_lines("tab", [20], 50, 1, edit=_put(27, b"\t")),
            shape_lines("gt_inside", [20], 50, 1, edit=_put(27, b">"), clean=True),
            shape_lines("one_line", [50], 50, 1, clean=True),
            shape_lines("one_line_el2", [50], 50, 2, clean=True),
            shape_empty_between()]
    return out


def shapes_forced():
    return [shape_odd_line(True), shape_space()]


def shapes_guard():
    return [shape_a(bpl, el) for bpl in (16, 17, 60) for el in (1, 2)] + \
           [shape_start(1), shape_end(1, True), shape_end(1, False), shape_end(2, True), shape_end(2, False)]


COMPACT_BPL = (16, 17, 33, 60)


def shapes_compact():
    return [shape_a(bpl, el) for bpl in COMPACT_BPL for el in (1, 2)] + \
           [shape_start(1), shape_end(1, True), shape_end(1, False), shape_end(2, True), shape_end(2, False)] + shapes_forced()


# ------------------------------------------------------------------ queries
def n_pairs(slen):
    return slen * (slen + 1) // 2


def all_pairs(slen):
    """every (a, b) with 0 <= a < b <= slen"""
    a, b = np.triu_indices(slen + 1, 1)
    return a.astype(np.int64), b.astype(np.int64)


def queries(shape, flags="all"):
    """-> (ids, a, b, fl) over every swept record of a shape: all pairs with all eight flag values ("all"), or all pairs
    with the flags cycling 0..7 with the query index ("cycle")."""
    ids, aa, bb = [], [], []
    for rid in shape.ids:
        a, b = all_pairs(shape.slen(rid))
        ids.append(np.full(a.size, rid, dtype=np.int64))
        aa.append(a)
        bb.append(b)
    ids, a, b = np.concatenate(ids), np.concatenate(aa), np.concatenate(bb)
    if flags == "all":
        ids, a, b = np.repeat(ids, 8), np.repeat(a, 8), np.repeat(b, 8)
    fl = (np.arange(ids.size) % 8).astype(np.uint8)
    return ids, a, b, fl


def n_queries(shape, flags="all"):
    return sum(n_pairs(shape.slen(r)) for r in shape.ids) * (8 if flags == "all" else 1)


def _layout(take):
    offs = np.zeros(take.size + 1, dtype=np.int64)
    np.cumsum(take, out=offs[1:])
    return offs


def _pack(parts, take):
    """answers laid back to back at a stride of `take` bytes each (a short one padded with zeros) -> (buf, offs, lens)"""
    lens = np.array([len(s) for s in parts], dtype=np.int64)
    buf = np.frombuffer(b"".join(s + bytes(int(t) - len(s)) for s, t in zip(parts, take)), dtype=np.uint8)
    return buf, _layout(take), lens


def expected(shape, ids, a, b, fl, regular=None):
    """slice_by_id for every query -> (buf, offs, lens).  regular: override of shape.regular for all records."""
    base, parts = {}, []
    for i, x, y, f in zip(ids.tolist(), a.tolist(), b.tolist(), fl.tolist()):
        s = base.get((i, x, y))
        if s is None:
            s = base[(i, x, y)] = slice_by_id(shape.raw, shape.rows[i], x, y, 0, shape.regular[i] if regular is None else regular)
        parts.append(apply_flags(s, f))
    return _pack(parts, b - a)


def expected_fast(shape, ids, a, b, fl):
    """The same for the records of a `clean` shape (every slice is bases [a, b) of the despaced record), from the eight
    transformed copies of each record: a reversed answer is bytes [slen - b, slen - a) of the reversed copy."""
    assert shape.clean
    width = max(shape.slen(r) for r in shape.ids)
    src = np.zeros((len(shape.rows), 8, width), dtype=np.uint8)
    slen = np.zeros(len(shape.rows), dtype=np.int64)
    for r in shape.ids:
        row = shape.rows[r]
        t = despace(shape.raw[row["boff"]:row["boff"] + row["blen"]])[:row["slen"]]
        assert len(t) == row["slen"]
        slen[r] = len(t)
        for f in range(8):
            src[r, f, :len(t)] = np.frombuffer(apply_flags(t, f), dtype=np.uint8)
    take = b - a
    offs = _layout(take)
    first = (ids * 8 + fl) * width + np.where(fl & 2, slen[ids] - b, a)
    idx = np.arange(offs[-1]) + np.repeat(first - offs[:-1], take)
    return src.ravel()[idx], offs, take.copy()


def expected_ranges(raw, off, blen, take, skip, fl):
    return _pack([range_fetch(raw, o, n, t, s, f) for o, n, t, s, f in
                  zip(off.tolist(), blen.tolist(), take.tolist(), skip.tolist(), fl.tolist())], take)


def first_mismatch(buf, offs, out_len, exp, eoffs, elens):
    """None when every answer (its first elens[i] bytes at offs[i]) and every length is as expected, else a description."""
    if not np.array_equal(np.asarray(offs)[:elens.size], eoffs[:elens.size]):
        return "answer offsets differ"
    if out_len is not None and not np.array_equal(out_len, elens):
        i = int(np.nonzero(np.asarray(out_len) != elens)[0][0])
        return "query %d: out_len %d, expected %d" % (i, int(out_len[i]), int(elens[i]))
    take = np.diff(eoffs)
    total = int(eoffs[-1])
    buf = np.asarray(buf)[:total]
    if buf.size != total:
        return "answer buffer holds %d bytes, expected %d" % (buf.size, total)
    bad = buf != exp
    if not (elens == take).all():
        bad &= (np.arange(total) - np.repeat(eoffs[:-1], take)) < np.repeat(elens, take)
    if not bad.any():
        return None
    p = int(np.argmax(bad))
    i = int(np.searchsorted(eoffs, p, side="right")) - 1
    return "query %d byte %d: got %r, expected %r" % (i, p - int(eoffs[i]), buf[eoffs[i]:eoffs[i] + elens[i]].tobytes(),
                                                      exp[eoffs[i]:eoffs[i] + elens[i]].tobytes())


def guard_offsets(take):
    """answer i begins (i * 7) % 19 bytes behind the end of answer i - 1, the first at 3 -> (offsets, buffer size)"""
    gap = (np.arange(take.size) * 7) % 19
    gap[0] = 3
    off = np.cumsum(gap) + (_layout(take)[:-1])
    return off.astype(np.int64), int(off[-1] + take[-1]) + 32


def guard_image(size, off, parts):
    """what a buffer of 0xA5 holds after exactly the answers were written"""
    img = np.full(size, 0xA5, dtype=np.uint8)
    for o, s in zip(off.tolist(), parts):
        img[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return img


# ------------------------------------------------------------------ FASTQ streams
FQ_MAX = 300


def fastq_stream(crlf=False, final_nl=True, high=False):
    """Reads of every length 1 .. 300 once, in a fixed shuffled order; quality bytes run through 33 .. 126 (high: through
    33 .. 255, so bytes >= 128 occur in the short reads too).  The first read has fewer than 16 bytes in front
    of it, the last fewer than 16 behind."""
    nl = b"\r\n" if crlf else b"\n"
    order = list(range(1, FQ_MAX + 1))
    random.Random(5).shuffle(order)
    out, k = [], 0
    for n in order:
        if high:
            q = bytes(33 + (k + 3 * j) % 223 for j in range(n))
        else:
            q = bytes(33 + (k + j) % 94 for j in range(n))
        k += n
        out.append(b"@r%d" % n + nl + bases(n, n) + nl + b"+" + nl + q + nl)
    raw = b"".join(out)
    return raw if final_nl else raw[:-1]


def fastq_batches(n):
    """every read in order; then descending and repeated ids"""
    return [np.arange(n, dtype=np.int64),
            np.concatenate([np.arange(n - 1, -1, -1), [0, 0, n - 1, n - 1, 5, 5, 5]]).astype(np.int64)]


def revcomp_lengths():
    return list(range(131)) + [256, 4095, 4096, 4097, 65537]


def revcomp_input(n):
    """n bytes that run through all 256 values, starting at another one for every length"""
    return ((np.arange(n) * 3 + 5 * n) % 256).astype(np.uint8).tobytes()
