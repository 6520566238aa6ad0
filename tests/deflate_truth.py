"""Host-side truth for the BGZF decoders: a plain walker over raw deflate streams (RFC 1951), a token-level encoder for the few
streams zlib cannot write, BGZF framing, and CORPUS -- members of valid deflate, by class, from fixed seeds.  Nothing here
imports the library: zlib decides what is valid, walk() says what shape a stream has.

The zlib classes are whatever the zlib behind Python's `zlib` module writes.  The figures in the tests (block counts, code
lengths, who decodes a class on the GPU) were taken with stock zlib 1.2 / 1.3; another implementation behind the same
interface (zlib-ng, for one) writes other, equally valid streams: the host tests then say which property a class has lost,
and that is a matter of the corpus, not of the decoders."""
import os
import struct
import zlib

import numpy as np

CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE, LEN_EXTRA, DIST_BASE, DIST_EXTRA = [], [], [], []          # RFC 1951 3.2.5
for _c in range(29):
    _e = 0 if _c < 8 or _c == 28 else (_c - 4) >> 2
    LEN_BASE.append(258 if _c == 28 else (3 + _c if _c < 8 else ((4 + (_c & 3)) << _e) + 3)); LEN_EXTRA.append(_e)
for _c in range(30):
    _e = 0 if _c < 4 else (_c >> 1) - 1
    DIST_BASE.append(1 + _c if _c < 4 else ((2 + (_c & 1)) << _e) + 1); DIST_EXTRA.append(_e)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 30


def canonical(lengths):
    """{symbol: code} of RFC 1951 3.2.2: codes of one length are consecutive in symbol order, shorter codes come first."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


def second_level(lengths, root):
    """Entries a two-level table needs behind a root of `root` bits: every root prefix (the first `root` bits of a code, in
    stream order) that has longer codes gets one sub-table, indexed by the bits that follow, as wide as the longest code
    under that prefix needs: 2 ** (longest - root)."""
    longest = {}
    for s, code in canonical(lengths).items():
        n = lengths[s]
        if n > root:
            p = code >> (n - root)
            longest[p] = max(longest.get(p, 0), n)
    return sum(1 << (n - root) for n in longest.values())


def _rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2)


def _table(lengths):
    """(list indexed by the next `width` bits of the stream, least significant first -> symbol << 4 | length, or 0; width)"""
    width = max(lengths) if lengths else 0
    t = [0] * (1 << width)
    for s, code in canonical(lengths).items():
        n = lengths[s]
        t[_rev(code, n)::1 << n] = [(s << 4) | n] * (1 << (width - n))
    return t, width


class _Bits:
    def __init__(self, data):
        self.d, self.p, self.buf, self.cnt = data, 0, 0, 0

    def need(self, n):
        while self.cnt < n:
            chunk = self.d[self.p:self.p + 8]
            if not chunk:
                chunk = b"\0"                              # zeros behind the end: a walk that used them fails the `pos` check
            self.buf |= int.from_bytes(chunk, "little") << self.cnt
            self.cnt += 8 * len(chunk)
            self.p += len(chunk)

    def take(self, n):
        self.need(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def sym(self, table, width):
        self.need(width)
        e = table[self.buf & ((1 << width) - 1)]
        if not e:
            raise ValueError("no such code")
        self.buf >>= e & 15
        self.cnt -= e & 15
        return e >> 4

    @property
    def pos(self):
        return self.p * 8 - self.cnt


def walk(cd):
    """One row (dict) per block of the raw deflate stream `cd`:
    type 0/1/2, final, nsym (literals + matches + the end-of-block code; 0 for a stored block), out (bytes the block makes),
    lit_max / dist_max (longest code of either tree), sub_wave / sub_serial ((literal, distance) second-level entries at root
    bits (10, 8) and (8, 6)), max_dist, max_len, last_tok ('lit', 'match' or None), ll / dl (the code lengths),
    hlit_cross (the repeat symbol, 16 .. 18, whose run begins in the literal/length lengths and ends in the distance lengths)."""
    b, rows, total = _Bits(cd), [], 0
    while True:
        final, typ = b.take(1), b.take(2)
        row = dict(type=typ, final=final, nsym=0, out=0, lit_max=0, dist_max=0, sub_wave=(0, 0), sub_serial=(0, 0),
                   max_dist=0, max_len=0, last_tok=None, ll=[], dl=[], hlit_cross=None)
        if typ == 0:
            b.take(b.cnt & 7)
            n, nn = b.take(16), b.take(16)
            if n ^ 0xFFFF != nn:
                raise ValueError("stored block: LEN / NLEN")
            for _ in range(n):
                b.take(8)
            row["out"] = n
        elif typ in (1, 2):
            if typ == 1:
                ll, dl = FIXED_LL, FIXED_DL
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORDER[i]] = b.take(3)
                ct, cw = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s, before = b.sym(ct, cw), len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    else:
                        lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
                    if before < hlit < len(lens):
                        row["hlit_cross"] = s                      # one repeat code spans both trees
                if len(lens) != hlit + hdist:
                    raise ValueError("a repeat runs past the code lengths")
                ll, dl = lens[:hlit], lens[hlit:]
            lt, lw = _table(ll)
            dt, dw = _table(dl)
            out = nsym = 0
            while True:
                s = b.sym(lt, lw)
                nsym += 1
                if s == 256:
                    break
                if s < 256:
                    out += 1
                    row["last_tok"] = "lit"
                    continue
                n = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                d = b.sym(dt, dw)
                d = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                if d > total + out:
                    raise ValueError("distance reaches in front of the stream")
                out += n
                row["last_tok"] = "match"
                row["max_dist"], row["max_len"] = max(row["max_dist"], d), max(row["max_len"], n)
            row.update(nsym=nsym, out=out, lit_max=max(ll), dist_max=max(dl), ll=list(ll), dl=list(dl),
                       sub_wave=(second_level(ll, 10), second_level(dl, 8)), sub_serial=(second_level(ll, 8), second_level(dl, 6)))
        else:
            raise ValueError("block type 3")
        total += row["out"]
        rows.append(row)
        if final:
            break
    if b.pos > 8 * len(cd) or b.pos <= 8 * len(cd) - 8:
        raise ValueError("the stream does not end in the last byte")
    return rows


# ---- encoder for the hand-built streams ---------------------------------------------------------------------------------
CL_LENGTHS = [4] * 13 + [5] * 6                                     # code-length code: all 19 symbols, complete (13/16 + 6/32)


class _Out:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits

    def code(self, codes, lengths, s):
        assert lengths[s], "symbol %d has no code" % s
        self.put(_rev(codes[s], lengths[s]), lengths[s])


def plain(lengths):
    """The code-length sequence that spells every length out (no repeat codes)."""
    return list(lengths)


def encode(blocks):
    """Raw deflate from a list of blocks, each a dict:
      kind 'stored': data (bytes);  kind 'fixed': tokens;  kind 'dynamic': ll, dl (code lengths, HLIT = len(ll), HDIST = len(dl)),
      tokens, and clseq -- the code-length sequence as the caller wants it written: an int 0..15 is that length, (16, n)
      repeats the length before n times (3..6), (17, n) / (18, n) are n zeros (3..10 / 11..138); default: plain(ll + dl).
      tokens: an int is a literal, (length, distance) a match.  final: BFINAL (default: the last block)."""
    o = _Out()
    for i, blk in enumerate(blocks):
        o.put(1 if blk.get("final", i == len(blocks) - 1) else 0, 1)
        if blk["kind"] == "stored":
            o.put(0, 2)
            o.put(0, -o.n % 8)
            o.put(len(blk["data"]), 16)
            o.put(len(blk["data"]) ^ 0xFFFF, 16)
            for c in blk["data"]:
                o.put(c, 8)
            continue
        if blk["kind"] == "fixed":
            o.put(1, 2)
            ll, dl = FIXED_LL, FIXED_DL
        else:
            o.put(2, 2)
            ll, dl = list(blk["ll"]), list(blk["dl"])
            seq, spelt = blk.get("clseq") or plain(ll + dl), []
            for item in seq:                                        # what the sequence says must be what the trees are
                if isinstance(item, int):
                    spelt.append(item)
                else:
                    s, n = item
                    assert (3 <= n <= 6) if s == 16 else (3 <= n <= 10) if s == 17 else (11 <= n <= 138)
                    spelt += [spelt[-1] if s == 16 else 0] * n
            assert spelt == ll + dl and 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30
            o.put(len(ll) - 257, 5)
            o.put(len(dl) - 1, 5)
            o.put(19 - 4, 4)
            for s in CLORDER:
                o.put(CL_LENGTHS[s], 3)
            cc = canonical(CL_LENGTHS)
            for item in seq:
                s, n = (item, 0) if isinstance(item, int) else item
                o.code(cc, CL_LENGTHS, s)
                if s >= 16:
                    o.put(n - (3 if s < 18 else 11), 2 if s == 16 else 3 if s == 17 else 7)
        lc, dc = canonical(ll), canonical(dl)
        for t in blk["tokens"]:
            if isinstance(t, int):
                o.code(lc, ll, t)
                continue
            n, d = t
            ls = max(c for c in range(29) if LEN_BASE[c] <= n and (c == 28 or n < 258))
            ds = max(c for c in range(30) if DIST_BASE[c] <= d)
            o.code(lc, ll, 257 + ls)
            o.put(n - LEN_BASE[ls], LEN_EXTRA[ls])
            o.code(dc, dl, ds)
            o.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
        o.code(lc, ll, 256)
    return o.v.to_bytes((o.n + 7) // 8, "little")


def member(cd, raw):
    """One BGZF member: the gzip header with the 'BC' extra field (BSIZE = size of the member - 1), deflate, CRC-32, ISIZE."""
    assert len(raw) <= 65536 and len(cd) <= 65510
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cd) + 25) + cd +
            struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw)))


# ---- the corpus ---------------------------------------------------------------------------------------------------------
def _deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, piece=None, flush=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if piece is None:
        return co.compress(raw) + co.flush()
    return b"".join(co.compress(raw[a:a + piece]) + co.flush(flush) for a in range(0, len(raw), piece)) + co.flush()


def zipf_text(n, seed=1, exponent=1.6):
    p = np.arange(1, 257, dtype=np.float64) ** -exponent
    return np.random.default_rng(seed).choice(256, n, p=p / p.sum()).astype(np.uint8).tobytes()


def genome_text(n, seed=2, n_run=True):
    """Soft-masked four-letter text in 60-column lines, with a run of N if asked."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, n, p=[.295, .205, .205, .295])]
    t = np.where(np.repeat(rng.random(n // 5000 + 1) < 0.4, 5000)[:n], t + 32, t).astype(np.uint8)
    if n_run:
        t[n // 3:n // 3 + 700] = ord("N")
    rows = t[:n - n % 60].reshape(-1, 60)
    return (b"\n".join(r.tobytes() for r in rows) + b"\n")[:n]


def quality_text(n, seed=3):
    """Quality lines of 150 columns, every Phred value 0 .. 40 equally likely."""
    q = (np.random.default_rng(seed).integers(0, 41, n) + 33).astype(np.uint8)
    rows = q[:n - n % 151].reshape(-1, 151)
    rows[:, 150] = 10
    return rows.tobytes()


def _ll(*specs):
    ll = [0] * 286
    for spec in specs:
        for s, n in spec.items():
            ll[s] = n
    return ll


def largest_demand(nsym=286, root=10):
    """The largest second-level demand at `root` bits of any complete code of at most nsym symbols and at most 15 bits, by
    dynamic programming over ALL such codes.  A canonical code is its counts per length; codes come in rising length, so a
    code of length L that begins at a (in units of 2 ** -15 of the code space) ends at a + 2 ** (15 - L), and the widest
    code under a root prefix is the one that covers the prefix's last unit: a prefix costs 2 ** (L - root) entries where
    that code has L > root bits.  f[a, s] = the most entries s symbols can cost that fill exactly [0, a), lengths taken in
    rising order (one more code of the same length at a time); the code is complete at a = 2 ** 15."""
    f = np.full((32769, nsym + 1), -1 << 20, dtype=np.int32)
    f[0, 0] = 0
    for n in range(1, 16):
        w = 1 << (15 - n)
        for a in range(0, 32768, w):
            cost = 1 << (n - root) if n > root and (a + w) % (1 << (15 - root)) == 0 else 0
            np.maximum(f[a + w, 1:], f[a, :-1] + cost, out=f[a + w, 1:])
    return int(f[32768].max())


def greedy_lengths():
    """A complete literal/length tree with the largest second-level demand at 10 root bits that 286 symbols allow (308,
    largest_demand(); the tree is one the search's trace-back gives, 285 symbols).  Codes of 1, 2 and 3 bits leave 128 root
    prefixes to the long codes: 233 codes of 11 bits fill 116 of them in pairs (232 entries) and begin the 117th, which ends
    in 12-bit codes (4); 45 codes of 12 bits, ten prefixes of four (40); the last prefix goes on with codes of 13, 14, 15 and
    15 bits (32).  Canonical codes come in rising length, so only the prefixes in which the length changes cost more entries
    than they hold symbols.  308 is below the wave kernel's P_LPOOL = 384: no valid stream can overflow its literal pool."""
    return [1, 2, 3] + [11] * 233 + [12] * 45 + [13, 14, 15, 15]


def _hand_built():
    rng = np.random.default_rng(11)
    out = {}
    # 32768 literals of 9 bits, end of block 2 bits, lengths 3 and 258 of 3 bits; distance codes 28 and 29 of 1 bit
    lits = rng.integers(0, 256, 32768).tolist()
    ll = _ll({s: 9 for s in range(256)}, {256: 2, 257: 3, 285: 3})
    out["dist_32768"] = [encode([dict(kind="dynamic", ll=ll, dl=[0] * 28 + [1, 1], tokens=lits + [(3, 32768), (258, 32768), (3, 32507)])])]
    # nine literals, end of block and lengths 3..6; sixteen distance codes of 4 bits; the (16, 6) begins at the length of
    # symbol 258 and ends at the length of distance code 2
    ll = _ll({s: 4 for s in range(97, 105)}, {10: 3, 256: 3, 257: 4, 258: 4, 259: 4, 260: 4})[:261]
    words = [97, 98, 99, 100, 10, 101, 102, (3, 3), 103, 104, (4, 7), (5, 1), 10, (6, 12), 97, (3, 2), (4, 16), 99, (5, 20), (6, 30), (3, 33), 10]
    tok = words * 5 + [(6, 60), (5, 97), 100, (4, 129), (3, 190), (6, 255), 10]
    out["repeat_across_hlit"] = [encode([dict(kind="dynamic", ll=ll, dl=[4] * 16, tokens=tok,
                                              clseq=ll[:258] + [(16, 6)] + [4] * 9 + [(16, 4)])])]
    # the same with a run of zeros: (18, 32) covers the lengths of symbols 258..285 and of distance codes 0..3
    ll = _ll({s: 4 for s in range(97, 105)}, {10: 2, 256: 3, 257: 3})
    tok = [97, 98, 99, 100, 101, 102, 103, 104, 10, 97, 98, 99, 100, 101, 102, 103, 104, (3, 5), (3, 8), 10, (3, 12), (3, 16), 97, (3, 7), (3, 13), 10]
    out["repeat_across_hlit"].append(encode([dict(kind="dynamic", ll=ll, dl=[0, 0, 0, 0, 2, 2, 2, 2], tokens=tok * 2,
                                                  clseq=ll[:258] + [(18, 32), 2, 2, 2, 2])]))
    # a distance tree of one code of one bit (incomplete, allowed); a block of literals with HDIST = 1 and no distance code
    ll = _ll({s: 3 for s in (65, 67, 71, 84)}, {10: 3, 256: 3, 257: 3, 264: 4, 285: 4})
    tok = [65, 67, 71, 84, (3, 1), 10, (10, 1), 71, (258, 1), 84, 65, (3, 1), (258, 1), 67, (10, 1), 10]
    out["one_dist_code"] = [encode([dict(kind="dynamic", ll=ll, dl=[1], tokens=tok * 20)]),
                            encode([dict(kind="dynamic", ll=ll, dl=[0], tokens=[65, 67, 71, 84, 10] * 300)])]
    # distance codes of 1, 2, ..., 14, 15, 15 bits, every one used
    dl = list(range(1, 16)) + [15]
    tok = [int(c) for c in rng.choice([65, 67, 71, 84, 10], 300)]
    for k in range(40):
        for ds in rng.permutation(16):
            tok += [(int(rng.choice([3, 10, 258])), DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds]))), int(rng.choice([65, 67, 71, 84]))]
    out["dist15"] = [encode([dict(kind="dynamic", ll=ll, dl=dl, tokens=tok)])]
    # the literal tree with the largest demand at 10 root bits: symbols in canonical order = rising length (the end-of-block
    # code and lengths 3, 4 have 12 bits; the codes of 13, 14, 15 and 15 bits are the lengths 115 .. 226): every literal
    # once, then matches through every level of the last sub-table, twice
    ll = greedy_lengths()
    tok = list(range(256)) + [(3, 16), (4, 7), (115, 1), (131, 16), (163, 9), (195, 13), (226, 16), 0, 255] * 2
    out["greedy_pool"] = [encode([dict(kind="dynamic", ll=ll, dl=[3] * 8, tokens=tok)])]
    # stored, dynamic, empty stored, final fixed block of three literals
    ll = _ll({s: 3 for s in (65, 67, 71, 84)}, {10: 3, 256: 3, 257: 3, 264: 4, 285: 4})
    out["stored_mix"] = [encode([dict(kind="stored", data=bytes(rng.integers(0, 256, 1000).tolist())),
                                 dict(kind="dynamic", ll=ll, dl=[2, 2] + [0] * 17 + [1], tokens=[65, 67, 71, 84, 10, (10, 2), (258, 1), (3, 1000)] * 30),   # 1000: into the stored block
                                 dict(kind="stored", data=b""),
                                 dict(kind="fixed", tokens=[69, 78, 68])])]
    return {k: [(cd, zlib.decompress(cd, -15)) for cd in v] for k, v in out.items()}


def _build():
    z, g = zipf_text(65280), genome_text(65280)
    c = {}
    c["zipf_default"] = [_deflate(z)]
    c["zipf_huffman_only"] = [_deflate(z, strategy=zlib.Z_HUFFMAN_ONLY)]
    c["zipf_filtered"] = [_deflate(z, strategy=zlib.Z_FILTERED)]
    rng = np.random.default_rng(4)
    fib = [1, 1]
    while sum(fib) < 65280:
        fib.append(fib[-1] + fib[-2])
    vals = rng.permutation(256)[:len(fib)]
    c["fib15"] = [_deflate(rng.permutation(np.repeat(vals, fib).astype(np.uint8)).tobytes()[:65280], strategy=zlib.Z_HUFFMAN_ONLY)]
    vocab = rng.integers(0, 256, (8000, 4), dtype=np.uint8)
    p = np.arange(1, 8001, dtype=np.float64) ** -1.15
    words = vocab[rng.choice(8000, 16320, p=p / p.sum())].tobytes()
    c["words_far"] = [_deflate(words, level) for level in (1, 6, 9)]
    c["memlevel1"] = [_deflate(z, mem=1)]
    for name, how in (("sync_flush", zlib.Z_SYNC_FLUSH), ("full_flush", zlib.Z_FULL_FLUSH), ("partial_flush", zlib.Z_PARTIAL_FLUSH),
                      ("z_block", zlib.Z_BLOCK)):
        c[name] = [_deflate(z[:60000], piece=7000, flush=how)]
    c["rle"] = [_deflate(g, strategy=zlib.Z_RLE)]
    c["fixed_big"] = [_deflate(g, strategy=zlib.Z_FIXED)]
    rep = genome_text(3000, seed=5) * 22
    c["isize_edge"] = [_deflate(rep[:65535]), _deflate(rep[:65535] + b"#"), _deflate(b"#" + rep[:65535])]
    c["dna"] = [_deflate(genome_text(65280, seed=seed, n_run=False)) for seed in (6, 7, 8)]
    c["qual"] = [_deflate(quality_text(65280))]
    # what the other BGZF tests feed the decoders, one member each: genome text with a run of N, the FASTQ fixture's records
    c["dna_n_run"] = [_deflate(g)]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "test.fq"), "rb") as fq:
        c["fastq_records"] = [_deflate(fq.read(65280))]
    out = {k: [(cd, zlib.decompress(cd, -15)) for cd in v] for k, v in c.items()}
    out.update(_hand_built())
    return out


NAMES = ("zipf_default", "zipf_huffman_only", "zipf_filtered", "fib15", "words_far", "memlevel1", "sync_flush", "full_flush",
         "partial_flush", "z_block", "rle", "fixed_big", "isize_edge", "dna", "qual", "dna_n_run", "fastq_records", "dist_32768",
         "repeat_across_hlit", "one_dist_code", "dist15", "greedy_pool", "stored_mix")


def __getattr__(name):
    """CORPUS is built when it is first asked for (collecting the tests needs NAMES only)."""
    if name == "CORPUS":
        globals()["CORPUS"] = _build()
        return globals()["CORPUS"]
    raise AttributeError(name)


def all_members():
    """(class, index in the class, deflate, raw) of every member, in the order of CORPUS."""
    corpus = globals().get("CORPUS") or __getattr__("CORPUS")
    return [(k, i, cd, raw) for k, v in corpus.items() for i, (cd, raw) in enumerate(v)]
