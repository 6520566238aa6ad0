"""Plain-Python truth for Fasta.records / write (test_fasta_write_host.py, test_gpu_fasta_write.py): the rules of
fx_fasta_format_alloc in include/fxgpu.h over Python strings.  No calls into the library.

Also a small FASTA writer and parser for the files the tests generate: bytes 10 / 13 / 32 dropped, records split at '>'."""

_COMP = {}
for _a, _b in ("AT", "TA", "CG", "GC", "MK", "KM", "RY", "YR", "VB", "BV", "HD", "DH", "UA"):
    _COMP[ord(_a)] = ord(_b)
    _COMP[ord(_a) + 32] = ord(_b) + 32
COMP = bytes(_COMP.get(c, c) for c in range(256))            # IUPAC complement, case kept, everything else itself
UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))
LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def _b(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def letters(seq, start, stop, minus, mask_rows, mask_mode, mask_char, uppercase):
    """S_k: seq (the despaced letters of the record) cut to [start, stop), then upper case, mask, complement, reverse.
    mask_rows: (start, stop) rows of this record on forward coordinates."""
    s = bytearray(_b(seq)[start:stop])
    if uppercase:
        s = bytearray(bytes(s).translate(UPPER))
    if mask_mode != "none":
        for a, b in mask_rows:
            lo, hi = max(a, start) - start, min(b, start + len(s)) - start
            if hi <= lo:
                continue
            if mask_mode == "soft":
                s[lo:hi] = bytes(s[lo:hi]).translate(LOWER)
            elif mask_mode == "upper":
                s[lo:hi] = bytes(s[lo:hi]).translate(UPPER)
            elif mask_mode == "hard":
                s[lo:hi] = _b(mask_char) * (hi - lo)
            else:
                raise ValueError(mask_mode)
    if minus:
        s = bytearray(bytes(s).translate(COMP)[::-1])
    return bytes(s)


def record(header, s, width):
    """'>' header '\\n', then s in lines of width (0: one line), each followed by '\\n'."""
    out = [b">", _b(header), b"\n"]
    w = width if width > 0 else max(len(s), 1)
    for i in range(0, len(s), w):
        out.append(s[i:i + w])
        out.append(b"\n")
    return b"".join(out)


def records(seqs, headers, queries, strand, width, mask_rows, mask_mode, mask_char, uppercase, min_len):
    """seqs: the despaced letters of every record; headers: one per QUERY; queries: (record, start, stop) with start = stop =
    None for the whole record; strand: one bool per query (True: minus); mask_rows: (record, start, stop) rows
    -> (bytes, offsets[n + 1])."""
    by_rec = {}
    for r, a, b in mask_rows or ():
        by_rec.setdefault(int(r), []).append((int(a), int(b)))
    out, offs = [], [0]
    for k, (r, a, b) in enumerate(queries):
        seq = _b(seqs[r])
        if a is None:
            a, b = 0, len(seq)
        s = letters(seq, int(a), int(b), bool(strand[k]), by_rec.get(int(r), ()), mask_mode, mask_char, uppercase)
        rec = record(headers[k], s, width) if len(s) >= min_len else b""
        out.append(rec)
        offs.append(offs[-1] + len(rec))
    return b"".join(out), offs


def write_fasta(recs, line_width, eol=b"\n", last="full"):
    """recs: (header, sequence) pairs -> the bytes of a FASTA file with lines of line_width letters.  last: "full" ends the
    file with its terminator, "unterminated" leaves it off the last line."""
    out = []
    for h, s in recs:
        s = _b(s)
        out.append(b">" + _b(h) + eol)
        for i in range(0, len(s), line_width):
            out.append(s[i:i + line_width] + eol)
    data = b"".join(out)
    if last == "unterminated" and data.endswith(eol):
        data = data[:-len(eol)]
    return data


def parse_fasta(data):
    """-> list of (header without '>' and terminator, letters with bytes 10 / 13 / 32 dropped)"""
    out = []
    for chunk in data.split(b">")[1:]:
        nl = chunk.find(b"\n")
        if nl < 0:
            nl = len(chunk)
        h = chunk[:nl]
        if h.endswith(b"\r"):
            h = h[:-1]
        body = chunk[nl + 1:]
        out.append((h, bytes(c for c in body if c not in (10, 13, 32))))
    return out
