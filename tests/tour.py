"""One tour of every compute entry of the library on two sets of seeded inputs (not collected by pytest).

inputs(tmp_dir) writes the files and keeps their letters as Python strings; run(fx, inp, order) calls every entry once
through the Python API and the Blob methods and returns a flat dict name -> numpy array of integers or bytes;
expected_small() is the same dict, for the families that have a truth module under tests/, computed on the host.
tests/test_gpu_clean_memory.py runs the tour in child processes (tests/tour_child.py) and compares the dicts: the same
tour must give the same arrays in a fresh process, with every device block filled with 0xFF before it is handed out
(FX_DEBUG_FILL), and when the entries are called in another order or behind a wider call on the same handle.

small: a FASTA of about 20 KB in 8 records and 300 read pairs.  seam: the same construction sized to cross the seams of
the shared machinery once or twice -- a record of more than SRCH_CHUNK runs of SRCH_RUN bytes (two chunks of the
three-launch scan of csrc/fx_search.hpp, a carry from one to the next), and 4500 reads (more than one scan chunk of
reads, more than two radix tiles of RS_TILE pairs)."""
import os
import struct
import zlib

import numpy as np

SRCH_RUN, SRCH_CHUNK, RS_TILE = 256, 4096, 2048             # csrc/fx_search.hpp, csrc/fx_sort.hip

MOTIF = "GGATCCTTAGCA"                                       # 12 letters, planted with its reverse complement
LONG = "ACGGTCATTGCAAGCTTGACCGTAGGCTAACGTTGCATCG"           # 40 letters: longer than the 32 of one pattern word
EMOTIF = "TTGACAGCTAGCTCAG"                                  # 16 letters, planted exact, with a deletion and with an insertion
ADAPTER = "AGATCGGAAGAGC"                                    # 13 letters, in a third of the reads
BARCODES = {"s0": "ACGTACGT", "s1": "TTGGCCAA", "s2": "GATCGATC", "s3": "CCATGGTA"}
ORF = "ATG" + "GCTGAAAAGCTGCGTCCGGATATCGTTCAG" * 8 + "TAA"  # 1 + 80 codons without a stop, then a stop
PWM_INTS = [[8, -6, -6, -6], [-6, 8, -6, -6], [-6, -6, 8, -6], [-6, -6, -6, 8], [8, -6, -2, -6], [-6, 8, -6, -2], [5, 5, -9, -9], [-9, -9, 5, 5]]
PWM_SITE = "ACGTACAG"                                        # the best window of PWM_INTS

_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _letters(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


def _put(s, at, word):
    assert 0 <= at and at + len(word) <= len(s)
    return s[:at] + word + s[at + len(word):]


def _other(word, at):
    """word with the letter at `at` replaced by the next of A C G T."""
    return word[:at] + "ACGT"[("ACGT".index(word[at]) + 1) % 4] + word[at + 1:]


def _wrap(s, width, nl="\n", last_nl=True):
    lines = [s[k:k + width] for k in range(0, len(s), width)]
    return nl.join(lines) + (nl if last_nl and lines else "")


def _plant_all(s, tail_from=None):
    """The features every search family must report at least once, at known places of one long record."""
    s = _put(s, 57, MOTIF)                                   # across the first line end of a record wrapped at 60
    s = _put(s, 300, MOTIF)
    s = _put(s, 1200, revcomp(MOTIF))
    s = _put(s, 2000, "A" * 40)
    s = _put(s, 2500, ORF)
    s = _put(s, 3500, "CAG" * 15)
    s = _put(s, 4000, LONG)
    s = _put(s, 4500, _other(MOTIF, 3))                      # one mismatch outside the anchor
    s = _put(s, 4600, _other(_other(MOTIF, 0), 5))           # two
    s = _put(s, 4700, _other(MOTIF, 10))                     # one inside the anchor
    s = _put(s, 5000, EMOTIF[:7] + EMOTIF[8:])               # a deletion
    s = _put(s, 5100, EMOTIF[:9] + "G" + EMOTIF[9:])         # an insertion
    s = _put(s, 5200, EMOTIF)
    s = _put(s, 5500, PWM_SITE)
    s = _put(s, 5600, revcomp(PWM_SITE))
    if tail_from is not None:                                # around and behind the seam of the scan chunks
        for at in range(tail_from, len(s) - 100, 997):
            s = _put(s, at, MOTIF if (at // 997) % 2 else revcomp(MOTIF))
        s = _put(s, len(s) - 5000, LONG)
        s = _put(s, len(s) - 4000, EMOTIF)
        s = _put(s, len(s) - 3000, "CAG" * 15)
        s = _put(s, len(s) - 2000, ORF)
    return s


def fasta_text(big):
    """-> (file bytes, [(name, letters)]): eight records; `big` letters in the first one."""
    rng = np.random.default_rng(20 + big)
    r0 = _plant_all(_letters(rng, big), tail_from=1000000 if big > 1100000 else None)
    r1 = _put(_letters(rng, 1500), 700, MOTIF)
    low = _letters(rng, 2500, "acgt")
    for at, n in ((0, 7), (400, 1), (900, 130), (2400, 100)):
        low = _put(low, at, "n" * n)
    low = _put(low, 1500, "N" * 20)
    r4 = _put(_letters(rng, 1800), 610, revcomp(MOTIF))
    r5 = _letters(rng, 45)
    r6 = _put(_letters(rng, 3000, "ACGTACGTACGTACGTRYKMN"), 1000, "AT" * 14)
    r7 = _put(_put(_letters(rng, 2000), 100, LONG), 1985, MOTIF)
    odd = "\n".join([_wrap(r4[:600], 60, last_nl=False), r4[600:637], _wrap(r4[637:], 60, last_nl=False)]) + "\n"
    recs = [("chr_long the first record", r0, _wrap(r0, 60)),
            ("crlf", r1, _wrap(r1, 70, "\r\n")),
            ("lower_n soft masked", low, _wrap(low, 80)),
            ("empty", "", ""),
            ("odd_middle", r4, odd),
            ("short", r5, r5 + "\n"),
            ("mixed iupac", r6, _wrap(r6, 60)),
            ("last", r7, _wrap(r7, 60, last_nl=False))]
    text = "".join(">" + name + ("\r\n" if name == "crlf" else "\n") + body for name, _, body in recs)
    return text.encode("ascii"), [(name.split(" ")[0], seq) for name, seq, _ in recs]


def fastq_text(n):
    """-> (bytes of mate 1, bytes of mate 2, [(header, seq, qual)] of mate 1, the same of mate 2): n pairs cut from random
    fragments, lengths 1..150; a third of the fragments are shorter than the reads, which then run into the adapter; a tenth of
    the reads repeat an earlier one; the barcode stands behind the header's last ':'."""
    rng = np.random.default_rng(300 + n)
    codes = list(BARCODES.values())
    r1, r2 = [], []
    for i in range(n):
        if i % 10 == 9:                                      # an exact duplicate (of both mates) under a name of its own
            j = int(rng.integers(0, i))
            s1, q1, s2, q2 = r1[j][1], r1[j][2], r2[j][1], r2[j][2]
        else:
            short = i % 3 == 0                               # a fragment so short that the whole adapter is read behind it
            L = int(rng.integers(60, 151)) if short else int(rng.integers(1, 151))
            F = int(rng.integers(L // 2, L - len(ADAPTER))) if short else int(rng.integers(L, 2 * L + 40))
            frag = _letters(rng, F)
            if i % 17 == 0 and L > 3:
                frag = _put(frag, min(3, F - 1), "N")
            s1 = (frag + ADAPTER + _letters(rng, 150))[:L]
            s2 = (revcomp(frag) + revcomp(ADAPTER) + _letters(rng, 150))[:L]
            q1 = bytes(np.clip(rng.integers(2, 42, L) - np.arange(L) // 12, 0, 41).astype(np.uint8) + 33).decode()
            q2 = bytes(np.clip(rng.integers(2, 42, L) - np.arange(L) // 10, 0, 41).astype(np.uint8) + 33).decode()
        bc = codes[i % 4]
        if i % 5 == 1:
            bc = _other(bc, i % 8)                           # one mismatch
        elif i % 11 == 2:
            bc = _letters(rng, 8)
        r1.append(("r%d 1:N:0:%s" % (i, bc), s1, q1))
        r2.append(("r%d 2:N:0:%s" % (i, bc), s2, q2))
    text = lambda rs: "".join("@%s\n%s\n+\n%s\n" % r for r in rs).encode("ascii")
    return text(r1), text(r2), r1, r2


def bgzf(data, member=60000):
    """`data` framed as BGZF: members of at most `member` bytes with the 'BC' extra field, then the empty end member."""
    mem = []
    for k in range(0, max(len(data), 1), member):
        chunk = data[k:k + member]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        mem.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    mem.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(mem)


SIZES = {"small": (9000, 300), "seam": (1110000, 4500)}


def make(which):
    """The bytes and letters of one input set, nothing written."""
    big, n_reads = SIZES[which]
    fa, recs = fasta_text(big)
    q1, q2, r1, r2 = fastq_text(n_reads)
    return {"which": which, "fa": fa, "names": [n for n, _ in recs], "seqs": [s for _, s in recs], "fq1": q1, "fq2": q2, "reads1": r1, "reads2": r2}


def inputs(tmp_dir, which=("small", "seam")):
    """Writes the files of the sets under tmp_dir -> {set: make(set) + the paths}."""
    out = {}
    for w in which:
        inp = make(w)
        for key, ext in (("fa", ".fa"), ("fq1", "_1.fq"), ("fq2", "_2.fq")):
            inp[key + "_path"] = os.path.join(str(tmp_dir), w + ext)
            with open(inp[key + "_path"], "wb") as f:
                f.write(inp[key])
        if w == "small":
            inp["bgzf_path"] = os.path.join(str(tmp_dir), w + "_bgzf.fa.gz")
            with open(inp["bgzf_path"], "wb") as f:
                f.write(bgzf(inp["fa"], 6000))
        out[w] = inp
    return out


def load(tmp_dir, which):
    """The set `which` as inputs() wrote it (the files are there already: a child process)."""
    inp = make(which)
    for key, ext in (("fa", ".fa"), ("fq1", "_1.fq"), ("fq2", "_2.fq")):
        inp[key + "_path"] = os.path.join(str(tmp_dir), which + ext)
        assert open(inp[key + "_path"], "rb").read() == inp[key], key
    if which == "small":
        inp["bgzf_path"] = os.path.join(str(tmp_dir), which + "_bgzf.fa.gz")
    return inp


# ---------------------------------------------------------------------------------------------------- arguments of the calls
def queries(inp, n, seed):
    """n intervals on the records that have letters -> (ids, starts, stops, strands 0 / 1), int64 and uint8."""
    rng = np.random.default_rng(seed)
    slen = np.array([len(s) for s in inp["seqs"]], dtype=np.int64)
    ids = rng.choice(np.nonzero(slen > 0)[0], n).astype(np.int64)
    a = (rng.random(n) * slen[ids]).astype(np.int64)
    b = np.minimum(a + rng.integers(0, 400, n), slen[ids]).astype(np.int64)
    b[::7] = a[::7]                                          # empty intervals
    return ids, a, b, rng.integers(0, 2, n).astype(np.uint8)


def kmer_sets(inp):
    """(k, strings) of the two screening sets: under 4096 codes (the form kept in LDS) and over (the global form)."""
    return (11, [inp["seqs"][0][100:600], inp["reads1"][0][1]]), (13, [s[:30000] for s in inp["seqs"]] + [inp["reads1"][5][1]])


def _doubled(n):
    return np.concatenate([np.arange(n, dtype=np.int64), np.arange(n - 1, -1, -1, dtype=np.int64)])


class Ctx:
    """The open objects of one tour.  Every file gets an index file of this tour's own, so that each process builds its index
    on the device, whatever another tour left beside the inputs."""

    def __init__(self, fx, inp, scratch):
        from pyfastx_amd import _lib, kmer, pwm
        self.fx, self.L, self.inp = fx, _lib, inp
        ix = lambda name: os.path.join(scratch, name + ".fxi")
        self.fab = _lib.Blob.from_bytes(inp["fa"])
        self.fqb = _lib.Blob.from_bytes(inp["fq1"])
        self.fa = fx.Fasta(inp["fa_path"], index_file=ix("fa"))
        self.fq = fx.Fastq(inp["fq1_path"], index_file=ix("fq1"))
        self.fq2 = fx.Fastq(inp["fq2_path"], index_file=ix("fq2"))
        self.pair = fx.FastqPair(self.fq, self.fq2)
        self.scratch = scratch
        self.n_seq, self.n_reads = len(inp["seqs"]), len(inp["reads1"])
        self.pwm = pwm.Pwm.from_ints(np.array(PWM_INTS))
        (k1, s1), (k2, s2) = kmer_sets(inp)
        self.set_lds, self.set_global = kmer.KmerTable.from_strings(s1, k1), kmer.KmerTable.from_strings(s2, k2)
        assert len(self.set_lds) < 4096 < len(self.set_global)
        self.q_narrow, self.q_wide = queries(inp, 40, 1), queries(inp, 400, 2)


def _cols(obj, *names):
    return {n: getattr(obj, n) for n in names}


def _struct(s):
    return {n: np.int64(getattr(s, n)) for n, _ in s._fields_}


def _hits(h):
    return h._asdict()


def _sketch(sk):
    n = sk.n_sets
    return {"sizes": sk.sizes, "keys": np.concatenate([sk.hashes(i) for i in range(n)]) if n else np.zeros(0, np.uint64)}


def _table(t):
    return {"codes": t.codes, "counts": t.counts, "n_windows": np.int64(t.n_windows)}


def _sparse(a):
    nz = np.nonzero(a)[0]
    return {"size": np.int64(a.size), "at": nz.astype(np.int64), "count": np.asarray(a)[nz]}


def _strand_chars(sd):
    return ["-" if x else "+" for x in sd.tolist()]


# Every call: c the Ctx, w False for the call whose result is kept, True for the wider call of the same entry that "twice"
# puts in front of it on the same handle (more ids, a pattern with more hits, a larger k, more windows; an entry that has no
# width is called as it is).
def fa_build(c, w):
    s = c.fab.fasta_build()
    return dict(_struct(s), **c.fab.fasta_table(s.n_seq))


def fa_build_comp(c, w):
    s = c.fab.fasta_build(comp=True)
    return dict(_struct(s), comp=c.fab.fasta_comp(s.n_seq))


def fa_comp_dense(c, w):
    return {"comp": c.fab.fasta_comp(c.n_seq)}


def fa_comp_sparse(c, w):
    return dict(zip(("seqid", "abc", "num", "total"), c.fab.fasta_comp_sparse()))


def fa_line_regular(c, w):
    return {"regular": c.fab.fasta_line_regular(c.n_seq)}


def fa_len_stats(c, w):
    return _struct(c.fab.fasta_len_stats(count_min=1000, half=0.5 * sum(len(s) for s in c.inp["seqs"])))


def fa_names_sort(c, w):
    order, ndup = c.fab.names_sort(0, c.n_seq)
    return {"order": order, "n_dup": np.int64(ndup)}


def fa_names_lookup(c, w):
    c.fab.names_build(0)
    names = c.inp["names"] * (8 if w else 1)
    return {"ids": c.fab.names_lookup(names[::-1] + ["absent", ""])}


def fa_fetch(c, w):
    ids, a, b, sd = c.q_wide if w else c.q_narrow
    buf, offs, out_len = c.fab.fasta_fetch(ids, a, b, flags_per_query=(np.arange(ids.size) % 8).astype(np.uint8))
    return {"buf": buf[:int(offs[-1])] if offs.size else buf[:0], "offs": offs, "out_len": out_len}


def fa_search_short(c, w):
    return _hits(c.fa.search_all("ACG" if w else MOTIF))


def fa_search_long(c, w):
    return _hits(c.fa.search_all(MOTIF[:6] if w else LONG))


def fa_search_counts(c, w):
    return {"counts": c.fa.search_counts("ACG" if w else MOTIF), "counts_long": c.fa.search_counts(MOTIF[:6] if w else LONG)}


def fa_search_approx(c, w):
    return _hits(c.fa.search_approx(MOTIF, 3) if w else c.fa.search_approx(MOTIF, 2, anchor=slice(9, 12)))


def fa_search_edit_best(c, w):
    return _hits(c.fa.search_edit(EMOTIF[:10] if w else EMOTIF, 2, report="best"))


def fa_search_edit_all(c, w):
    return _hits(c.fa.search_edit(EMOTIF[:10] if w else EMOTIF, 2, report="all"))


def fa_pwm_scan(c, w):
    return _hits(c.fa.pwm_scan(c.pwm, min_score=10 if w else 40))


def fa_pwm_best(c, w):
    return _hits(c.fa.pwm_best(c.pwm, ids=list(range(c.n_seq)) * 4 if w else [7, 0, 3, 2]))


def fa_minimizers(c, w):
    return _hits(c.fa.minimizers(7, 3) if w else c.fa.minimizers(15, 10))


def fa_sketch_scaled(c, w):
    sk = c.fa.sketch(k=21, scaled=1 if w else 8)
    shared, total = sk.compare()
    return dict(_sketch(sk), shared=shared, total=total)


def fa_sketch_size(c, w):
    sk = c.fa.sketch(k=21, size=512 if w else 64)
    shared, total = sk.compare(limit=sk.size)
    return dict(_sketch(sk), shared=shared, total=total)


def fa_sketch_pooled(c, w):
    return _sketch(c.fa.sketch(k=21, scaled=1 if w else 8, pooled=True))


def fa_kmer_counts4(c, w):
    return {"counts": c.fa.kmer_counts(5) if w else c.fa.kmer_counts(4, canonical=True, ids=[0, 2, 7])}


def fa_kmer_counts11(c, w):
    return _sparse(c.fa.kmer_counts(12 if w else 11))


def fa_kmer_table21(c, w):
    return _table(c.fa.kmer_table(25) if w else c.fa.kmer_table(21, canonical=True))


def fa_kmer_hits_lds(c, w):
    nw, nh = c.fa.kmer_hits(c.set_lds, ids=None if w else [0, 6, 2])
    return {"n_windows": nw, "n_hits": nh}


def fa_kmer_hits_global(c, w):
    nw, nh = c.fa.kmer_hits(c.set_global, ids=list(range(c.n_seq)) * 3 if w else None)
    return {"n_windows": nw, "n_hits": nh}


def fa_region_stats(c, w):
    ids, a, b, _ = c.q_wide if w else c.q_narrow
    return _cols(c.fa.region_stats(ids, a, b), "ids", "starts", "stops", "counts")


def fa_window_stats(c, w):
    return _cols(c.fa.window_stats(100, 50) if w else c.fa.window_stats(500, 200), "ids", "starts", "stops", "counts")


def fa_class_runs(c, w):
    return _cols(c.fa.class_runs(letters="AC", min_len=2) if w else c.fa.class_runs("N"), "ids", "starts", "stops")


def fa_tandem_repeats(c, w):
    r = c.fa.tandem_repeats(min_copies=(6, 3, 2, 2, 2, 2)) if w else c.fa.tandem_repeats()
    return _cols(r, "ids", "starts", "stops", "periods", "motif_codes")


def fa_orfs_start(c, w):
    return _cols(c.fa.orfs(min_len=30 if w else 75, mode="start"), "ids", "starts", "stops", "frames", "flags")


def fa_orfs_stop(c, w):
    return _cols(c.fa.orfs(min_len=30 if w else 75, mode="stop"), "ids", "starts", "stops", "frames", "flags")


def fa_translate_many(c, w):
    ids, a, b, sd = c.q_wide if w else c.q_narrow
    buf, offs = c.fa.translate_many(ids, a, b, strand=sd)
    return {"buf": buf, "offs": offs}


def fq_build(c, w):
    s = c.fqb.fastq_build()
    return dict(_struct(s), **c.fqb.fastq_table(s.n_reads))


def fq_build_comp(c, w):
    s = c.fqb.fastq_build(comp=True)
    base, meta = c.fqb.fastq_comp()
    return dict(_struct(s), base=base, meta=meta)


def fq_fetch(c, w):
    ids = _doubled(c.n_reads) if w else np.arange(0, c.n_reads, 3, dtype=np.int64)
    rlen = np.array([len(c.inp["reads1"][i][1]) for i in ids.tolist()], dtype=np.int64)
    seq, qual, qi, offs = c.fqb.fastq_fetch(ids, rlen, phred=33)
    return {"seq": seq, "qual": qual, "quali": qi, "offs": offs}


def _ids(c, w):
    return _doubled(c.n_reads) if w else None


def fq_read_stats(c, w):
    return c.fq.read_stats(ids=_ids(c, w))


def fq_cycle_profile(c, w):
    return _cols(c.fq.cycle_profile(300 if w else None), "qual", "base", "depth")


def fq_select(c, w):
    return {"ids": c.fq.select(min_len=1) if w else c.fq.select(min_len=50, min_mean_qual=18, max_other=0)}


TRIM = dict(adapter=ADAPTER, min_overlap=3, max_error_rate=0.1, tail_qual=12, clip_front=1)


def fq_trim(c, w):
    return c.fq.trim(ids=_ids(c, w), **TRIM)


def fq_records(c, w):
    t = c.fq.trim(ids=_ids(c, w), **TRIM)
    buf, offs = c.fq.records(ids=_ids(c, w), start=t["start"], end=t["end"], min_len=20)
    return {"buf": buf, "offs": offs}


def fq_kmer_counts(c, w):
    return {"counts": c.fq.kmer_counts(6 if w else 4, ids=_ids(c, w))}


def fq_kmer_table(c, w):
    return _table(c.fq.kmer_table(25 if w else 21, ids=_ids(c, w)))


def fq_kmer_hits(c, w):
    nw, nh = c.fq.kmer_hits(c.set_global if w else c.set_lds, ids=_ids(c, w))
    return {"n_windows": nw, "n_hits": nh}


def fq_screen(c, w):
    return {"ids": c.fq.screen(c.set_global, min_hits=1 if w else 2, ids=_ids(c, w))}


def fq_duplicates(c, w):
    return {"first": c.fq.duplicates(ids=_ids(c, w))}


def fq_dedup(c, w):
    pos, copies = c.fq.dedup(ids=_ids(c, w), return_counts=True)
    return {"pos": pos, "copies": copies}


def fq_demux(c, w):
    dm = c.fq.demux(BARCODES, where="header", mismatches=1, ids=_ids(c, w))
    return _cols(dm, "sample", "dist", "second", "counts", "order", "bin_off")


def fq_sketch(c, w):
    return _sketch(c.fq.sketch(k=21, scaled=1 if w else 4, ids=_ids(c, w)))


def pair_overlap(c, w):
    return c.pair.overlap(ids=_ids(c, w))


def pair_merge(c, w):
    buf, offs = c.pair.merge(ids=_ids(c, w), min_len=20)
    return {"buf": buf, "offs": offs}


def pair_trim(c, w):
    return c.pair.trim(ids=_ids(c, w), **TRIM)


def _tuples(it):
    rows = list(it)
    width = len(rows[0]) if rows else 0
    return {"col%d" % k: np.frombuffer("\n".join(str(r[k]) for r in rows).encode("latin-1"), dtype=np.uint8) for k in range(width)}


def fastx_fasta(c, w):
    return _tuples(c.fx.Fastx(c.inp["fa_path"], uppercase=True, comment=True))


def fastx_fastq(c, w):
    return _tuples(c.fx.Fastx(c.inp["fq1_path"]))


def bgzf_fasta(c, w):
    """The open is the entry: it inflates the members and builds the index on a handle of its own, so the wider call cannot share
    the handle.  It gets an index file of its own instead -- the kept call then builds on the device too, in the blocks the wider
    one gave back to the pool -- and a wider batch of intervals."""
    fa = c.fx.Fasta(c.inp["bgzf_path"], index_file=os.path.join(c.scratch, "bgzf_wide.fxi" if w else "bgzf.fxi"))
    t = fa._table()
    ids, a, b, _ = c.q_wide if w else c.q_narrow
    buf, offs = fa.fetch_many(ids, a, b)
    return dict({k: np.asarray(t[k]) for k in ("boff", "blen", "slen", "llen", "elen", "norm")}, buf=buf, offs=offs)


BUILDS = [fa_build, fq_build]                                # first in every order: the other calls on these handles need the tables
CALLS = [fa_build_comp, fa_comp_dense, fa_comp_sparse, fa_line_regular, fa_len_stats, fa_names_sort, fa_names_lookup, fa_fetch,
         fa_search_short, fa_search_long, fa_search_counts, fa_search_approx, fa_search_edit_best, fa_search_edit_all, fa_pwm_scan,
         fa_pwm_best, fa_minimizers, fa_sketch_scaled, fa_sketch_size, fa_sketch_pooled, fa_kmer_counts4, fa_kmer_counts11,
         fa_kmer_table21, fa_kmer_hits_lds, fa_kmer_hits_global, fa_region_stats, fa_window_stats, fa_class_runs, fa_tandem_repeats,
         fa_orfs_start, fa_orfs_stop, fa_translate_many,
         fq_build_comp, fq_fetch, fq_read_stats, fq_cycle_profile, fq_select, fq_trim, fq_records, fq_kmer_counts, fq_kmer_table,
         fq_kmer_hits, fq_screen, fq_duplicates, fq_dedup, fq_demux, fq_sketch,
         pair_overlap, pair_merge, pair_trim, fastx_fasta, fastx_fastq, bgzf_fasta]
SMALL_ONLY = ("bgzf_fasta",)                                 # the BGZF file is the small FASTA
ORDERS = ("forward", "reverse", "twice")


def call_names(which):
    return [f.__name__ for f in BUILDS + CALLS if which == "small" or f.__name__ not in SMALL_ONLY]


def _flat(name, res):
    out = {}
    for k, v in res.items():
        a = np.array(v)                                      # a copy: the pinned block under a result goes back to its pool
        assert a.dtype.kind in "iub", (name, k, a.dtype)
        out[name + "." + k] = a
    return out


def run(fx, inp, order="forward", scratch=None, probe=None, log=None):
    """Every call once -> {call.column: array}.  scratch: a directory of this tour's own for its index files.  probe: a
    function without arguments, called before and after every call; log gets (call, probe before, probe after)."""
    assert order in ORDERS, order
    c = Ctx(fx, inp, scratch or os.path.dirname(inp["fa_path"]))
    names = call_names(inp["which"])
    calls = [f for f in BUILDS + CALLS if f.__name__ in names]
    if order == "reverse":
        calls = calls[:len(BUILDS)] + calls[len(BUILDS):][::-1]
    out = {}
    for f in calls:
        before = probe() if probe else None
        if order == "twice":
            f(c, True)
        out.update(_flat(f.__name__, f(c, False)))
        if log is not None:
            log.append((f.__name__, before, probe() if probe else None))
    return out


# ---------------------------------------------------------------------------------------------------- the truth of the small set
_EXPECTED = None


def _rows(rows, *cols):
    """[(a, b, ...)] -> {col: int64 array}; a strand column given as '+' / '-' becomes its byte."""
    out = {}
    for j, c in enumerate(cols):
        v = [ord(r[j]) if isinstance(r[j], str) else r[j] for r in rows]
        out[c] = np.array(v, dtype=np.uint64 if c in ("codes", "keys") else np.int64).reshape(len(rows))
    return out


def _counts_of(rows, n):
    c = np.zeros((n, 2), dtype=np.int64)
    for r in rows:
        c[r[0], 1 if r[3] == "-" else 0] += 1
    return c


def _pack(parts):
    offs = np.zeros(len(parts) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), offs


def expected_small():
    """{call.column: array} of the small set for every family with a truth module under tests/ or a function of the oracle,
    computed once on the host from the letters make() kept."""
    global _EXPECTED
    if _EXPECTED is not None:
        return _EXPECTED
    import fxoracle
    import annot_truth
    import dedup_truth
    import demux_truth
    import fetch_truth
    import kmer_screen_truth
    import kmer_table_truth
    import kmer_truth
    import minimizer_truth
    import orf_truth
    import pair_truth
    import pwm_truth
    import search_approx_truth
    import search_edit_truth
    import sketch_truth
    import tandem_truth
    import trim_truth
    from pyfastx_amd import demux as _demux, kmer, pair as _pair, sketch as _sk, trim as _trim

    inp = make("small")
    seqs, n = inp["seqs"], len(inp["seqs"])
    E = {}

    def put(call, cols):
        for k, v in cols.items():
            E[call + "." + k] = np.asarray(v)

    # index rows and composition: the oracle
    recs, total = fxoracle.fasta_index(inp["fa"])
    assert [len(s) for s in seqs] == recs["slen"].tolist()
    table = {c: recs[c] for c in ("boff", "blen", "slen", "llen", "elen", "norm", "dlen", "name_len")}
    put("fa_build", dict(table, n_seq=n, seq_len=total, n_bytes=len(inp["fa"])))
    comp = fxoracle.fasta_comp(inp["fa"], n)
    put("fa_build_comp", {"n_seq": n, "seq_len": total, "comp": comp})
    put("fa_comp_dense", {"comp": comp})
    at = np.nonzero(comp)
    put("fa_comp_sparse", {"seqid": at[0] + 1, "abc": at[1], "num": comp[at], "total": comp.sum(axis=0)})
    put("bgzf_fasta", {c: table[c] for c in ("boff", "blen", "slen", "llen", "elen", "norm")})
    rq, size, _ = fxoracle.fastq_index(inp["fq1"])
    put("fq_build", dict({c: rq[c] for c in ("rlen", "soff", "qoff", "dlen", "name_len")}, n_reads=len(rq), size=size, n_bytes=len(inp["fq1"])))
    put("fq_build_comp", {"n_reads": len(rq), "size": size})

    # fetch: the letters, sliced, with the flags of fetch_truth
    ids, a, b, sd = queries(inp, 40, 1)
    parts = [fetch_truth.apply_flags(seqs[i][x:y].encode(), q % 8) for q, (i, x, y) in enumerate(zip(ids.tolist(), a.tolist(), b.tolist()))]
    buf, offs = _pack(parts)
    put("fa_fetch", {"buf": buf, "offs": offs, "out_len": np.diff(offs)})
    buf, offs = _pack([seqs[i][x:y].encode() for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())])
    put("bgzf_fasta", {"buf": buf, "offs": offs})

    # exact search: the approximate truth at d = 0
    hit_cols = ("ids", "starts", "stops", "strands")
    rows = search_approx_truth.truth(seqs, MOTIF, 0, rev=revcomp(MOTIF))
    put("fa_search_short", _rows(rows, *hit_cols))
    rows_long = search_approx_truth.truth(seqs, LONG, 0, rev=revcomp(LONG))
    put("fa_search_long", _rows(rows_long, *hit_cols))
    put("fa_search_counts", {"counts": _counts_of(rows, n), "counts_long": _counts_of(rows_long, n)})
    put("fa_search_approx", _rows(search_approx_truth.truth(seqs, MOTIF, 2, anchor=slice(9, 12), rev=revcomp(MOTIF)), *hit_cols, "mismatches"))
    put("fa_search_edit_best", _rows(search_edit_truth.truth(seqs, EMOTIF, 2, report="best", rev=revcomp(EMOTIF)), *hit_cols, "edits"))
    put("fa_search_edit_all", _rows(search_edit_truth.truth(seqs, EMOTIF, 2, report="all", rev=revcomp(EMOTIF)), *hit_cols, "edits"))

    ints = np.array(PWM_INTS)
    rows, _, _ = pwm_truth.truth(seqs, ints, 40)
    put("fa_pwm_scan", _rows(rows, *hit_cols, "scores"))
    _, bs, bp = pwm_truth.truth(seqs, ints, 40, ids=[7, 0, 3, 2])
    put("fa_pwm_best", {"scores": bs, "starts": bp})

    rows, _ = minimizer_truth.truth(seqs, 15, 10)
    put("fa_minimizers", dict(_rows([(i, s, s + 15, sd_, c) for i, s, sd_, c in rows], *hit_cols, "codes")))

    def sets(per):
        return {"sizes": np.array([len(s) for s in per], dtype=np.int64), "keys": np.array([x for s in per for x in s], dtype=np.uint64)}

    def pairs(per, limit=0):
        m = [[sketch_truth.compare_model(x, y, limit) for y in per] for x in per]
        return {"shared": np.array([[c[0] for c in r] for r in m], dtype=np.int64), "total": np.array([[c[1] for c in r] for r in m], dtype=np.int64)}

    mk8 = _sk.check_args(21, 8, None)[3]
    per = sketch_truth.fasta_sets(seqs, 21, True, mk8, form=sketch_truth.key_set_np)
    put("fa_sketch_scaled", dict(sets(per), **pairs(per)))
    per = sketch_truth.fasta_sets(seqs, 21, True, _sk.check_args(21, None, 64)[3], 64, form=sketch_truth.key_set_np)
    put("fa_sketch_size", dict(sets(per), **pairs(per, 64)))
    put("fa_sketch_pooled", sets(sketch_truth.fasta_sets(seqs, 21, True, mk8, pooled=True, form=sketch_truth.key_set_np)))

    put("fa_kmer_counts4", {"counts": kmer_truth.kmer_counts_truth([seqs[i] for i in (0, 2, 7)], 4, canonical=True)})
    put("fa_kmer_counts11", _sparse(kmer_truth.kmer_counts_truth(seqs, 11)))
    codes, counts = kmer_table_truth.table_truth(seqs, 21, canonical=True)
    put("fa_kmer_table21", {"codes": codes, "counts": counts, "n_windows": counts.sum()})
    (k1, s1), (k2, s2) = kmer_sets(inp)
    lds, glob = kmer.KmerTable.from_strings(s1, k1), kmer.KmerTable.from_strings(s2, k2)
    assert np.array_equal(lds.codes, kmer_table_truth.table_truth(s1, k1)[0]) and np.array_equal(glob.codes, kmer_table_truth.table_truth(s2, k2)[0])
    nw, nh = kmer_screen_truth.hits_truth([seqs[i] for i in (0, 6, 2)], k1, lds.codes)
    put("fa_kmer_hits_lds", {"n_windows": nw, "n_hits": nh})
    nw, nh = kmer_screen_truth.hits_truth(seqs, k2, glob.codes)
    put("fa_kmer_hits_global", {"n_windows": nw, "n_hits": nh})

    put("fa_region_stats", {"ids": ids, "starts": a, "stops": b,
                            "counts": np.array([annot_truth.region_counts(seqs[i], x, y) for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())], dtype=np.int64)})
    rows = [(i, x, y) for i in range(n) for x, y in annot_truth.windows(len(seqs[i]), 500, 200, True)]
    put("fa_window_stats", dict(_rows(rows, "ids", "starts", "stops"), counts=np.array([annot_truth.region_counts(seqs[i], x, y) for i, x, y in rows], dtype=np.int64)))
    put("fa_class_runs", _rows([(i, x, y) for i in range(n) for x, y in annot_truth.class_runs(seqs[i], "Nn")], "ids", "starts", "stops"))
    put("fa_tandem_repeats", _rows([(i,) + r for i in range(n) for r in tandem_truth.repeats(seqs[i])], "ids", "starts", "stops", "periods", "motif_codes"))
    for mode in ("start", "stop"):
        put("fa_orfs_" + mode, _rows([(i,) + r for i in range(n) for r in orf_truth.orfs(seqs[i], mode=mode, min_len=75)], "ids", "starts", "stops", "frames", "flags"))
    buf, offs = _pack([orf_truth.translate(seqs[i][x:y], "-" if s else "+").encode() for i, x, y, s in zip(ids.tolist(), a.tolist(), b.tolist(), sd.tolist())])
    put("fa_translate_many", {"buf": buf, "offs": offs})

    # FASTQ
    r1, r2 = inp["reads1"], inp["reads2"]
    u8 = lambda s: np.frombuffer(s.encode(), dtype=np.uint8)
    args = _trim.trim_args(TRIM["clip_front"], 0, TRIM["adapter"], TRIM["min_overlap"], TRIM["max_error_rate"], None, None, TRIM["tail_qual"])
    kw = trim_truth.truth_kwargs(args)
    t1 = np.array([trim_truth.trim_truth(u8(s), u8(q), 33, **kw) for _, s, q in r1], dtype=np.int64).reshape(-1, 2)
    t2 = np.array([trim_truth.trim_truth(u8(s), u8(q), 33, **kw) for _, s, q in r2], dtype=np.int64).reshape(-1, 2)
    put("fq_trim", {"start": t1[:, 0], "end": t1[:, 1]})
    buf, offs = _pack([trim_truth.record(("@" + h).encode(), u8(s), u8(q), x, y) if y - x >= 20 else b"" for (h, s, q), (x, y) in zip(r1, t1.tolist())])
    put("fq_records", {"buf": buf, "offs": offs})
    got = [fetch_truth.fastq_read(inp["fq1"], int(rq["soff"][i]), int(rq["qoff"][i]), int(rq["rlen"][i]), 33, 0) for i in range(0, len(r1), 3)]
    buf, offs = _pack([g[0] for g in got])
    put("fq_fetch", {"seq": buf, "qual": _pack([g[1] for g in got])[0], "quali": np.concatenate([g[2] for g in got]), "offs": offs})
    for call, data, fmt, kw in (("fastx_fasta", inp["fa"], "fasta", dict(uppercase=True, comment=True)), ("fastx_fastq", inp["fq1"], "fastq", {})):
        rows = fxoracle.fastx_tuples(data, fmt, **kw)
        put(call, {"col%d" % k: np.frombuffer("\n".join(str(r[k]) for r in rows).encode("latin-1"), dtype=np.uint8) for k in range(len(rows[0]))})
    reads = [s for _, s, _ in r1]
    put("fq_kmer_counts", {"counts": kmer_truth.kmer_counts_truth(reads, 4)})
    codes, counts = kmer_table_truth.table_truth(reads, 21)
    put("fq_kmer_table", {"codes": codes, "counts": counts, "n_windows": counts.sum()})
    nw, nh = kmer_screen_truth.hits_truth(reads, k1, lds.codes)
    put("fq_kmer_hits", {"n_windows": nw, "n_hits": nh})
    nw, nh = kmer_screen_truth.hits_truth(reads, k2, glob.codes)
    put("fq_screen", {"ids": kmer_screen_truth.screen_truth(nw, nh, min_hits=2)})
    put("fq_sketch", sets([sketch_truth.fastq_set(reads, 21, True, _sk.check_args(21, 4, None)[3], form=sketch_truth.key_set_np)]))
    put("fq_duplicates", {"first": dedup_truth.first_truth(reads)})
    pos, copies = dedup_truth.dedup_truth(reads)
    put("fq_dedup", {"pos": pos, "copies": copies})
    dargs = _demux.demux_args(BARCODES, "header", 0, 1, 1, False)
    segs, sheet = demux_truth.segments(dargs)
    sample, dist, second = demux_truth.demux_truth([(("@" + h).encode(), s.encode()) for h, s, _ in r1], segs, sheet, 1)
    order, bin_off, counts = demux_truth.bins_of(sample, len(BARCODES))
    put("fq_demux", {"sample": sample, "dist": dist, "second": second, "counts": counts, "order": order, "bin_off": bin_off})

    # pairs
    oargs = _pair.overlap_args(30, 5, 0.2)
    ov = [pair_truth.overlap_truth(x[1].encode(), y[1].encode(), oargs["min_overlap"], oargs["max_diff"], oargs["err"]) for x, y in zip(r1, r2)]
    put("pair_overlap", {k: np.array([o[k] for o in ov], dtype=np.int64) for k in ("diag", "overlap", "mismatches", "end1", "end2", "insert")})
    buf, offs = _pack([pair_truth.merged_truth(("@" + x[0]).encode(), x[1].encode(), x[2].encode(), y[1].encode(), y[2].encode(), o["diag"], 20)
                       for x, y, o in zip(r1, r2, ov)])
    put("pair_merge", {"buf": buf, "offs": offs})
    e1 = np.minimum(t1[:, 1], [o["end1"] for o in ov])
    e2 = np.minimum(t2[:, 1], [o["end2"] for o in ov])
    put("pair_trim", {"start1": np.minimum(t1[:, 0], e1), "end1": e1, "start2": np.minimum(t2[:, 0], e2), "end2": e2,
                      "diag": np.array([o["diag"] for o in ov], dtype=np.int64)})
    _EXPECTED = E
    return E


# the calls of the tour for which no module under tests/ holds a truth: their results are compared between the situations only
NO_TRUTH = ["fa_line_regular", "fa_len_stats", "fa_names_sort", "fa_names_lookup", "fq_read_stats", "fq_cycle_profile", "fq_select"]
