"""-m gpu: the passes at stream offsets past 2^32 bytes, in-record coordinates past 2^31 and 2^32 letters and more than 2^23
runs of 256 bytes, on periodic streams built in device memory (tests/periodic.py).  A record of R copies of one block B, a
FASTQ of R copies of one block of reads: the exact answer follows from the CPU truth of two or three copies by the rules
that tests/test_periodic_host.py pins.  Every comparison is exact.  One giant stream is alive at a time; the only skip is
a device with under 24 GiB free."""
import numpy as np
import pytest

import annot_truth
import fetch_truth as T
import kmer_table_truth
import kmer_truth
import minimizer_truth
import orf_truth
import periodic as P
import pwm_truth
import search_approx_truth
import sketch_truth
import tandem_truth

pytestmark = pytest.mark.gpu

NEED_FREE = 24 << 30
PWM = np.array([[9 if "ACGT"[c] == ch else -9 for c in range(4)] for ch in P.MOTIF], dtype=np.int32)
PWM_MIN = 9 * 16 - 18 * 3                                    # MOTIF with up to three letters changed
_alive = []                                                  # the giant stream that is open: [close function]


def _close_alive():
    while _alive:
        _alive.pop()()


def _room():
    import torch
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    _close_alive()
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip("torch.cuda.mem_get_info() reports %.1f GiB free, under 24 GiB" % (free / 2**30))


class Giant:
    """One giant FASTA stream, built and indexed: the blob, the layout, the block and its copies, the small records."""

    def __init__(self, width, eol):
        import torch
        from pyfastx_amd import _lib
        self.m = m = 1001 * width
        self.R = R = P.copies_for(m)
        self.B = P.make_block(m)
        self.B2, self.B3 = self.B * 2, self.B * 3
        self.head, self.seqs = P.small_fasta("h")
        self.tail, _ = P.small_fasta("t")
        self.width, self.eol = width, eol
        t, self.lay = P.giant_fasta(torch.device("cuda:0"), self.head, self.B, width, eol, R, self.tail)
        torch.cuda.synchronize()
        self.blob = _lib.Blob.from_device(t.data_ptr(), self.lay["n_bytes"], device=0, keepalive=t)
        self.summary = self.blob.fasta_build()
        self.n = int(self.summary.n_seq)
        self.g = self.lay["giant"]
        self.gid = np.array([self.g], dtype=np.int64)
        self.hid = np.array(self.lay["head_ids"], dtype=np.int64)
        self.tid = np.array(self.lay["tail_ids"], dtype=np.int64)
        self.slen = R * m
        del t

    def close(self):
        import torch
        self.blob.close()
        self.blob = None
        torch.cuda.empty_cache()


def _giant(width, eol):
    _room()
    g = Giant(width, eol)
    _alive.append(g.close)
    return g


@pytest.fixture(scope="module")
def lf():
    g = _giant(60, 1)
    yield g
    if g.blob is not None:
        _close_alive()


@pytest.fixture(scope="module")
def crlf():
    g = _giant(57, 2)
    yield g
    if g.blob is not None:
        _close_alive()


def strand01(strands):
    return (np.asarray(strands) == ord("-")).astype(np.int64)


def per_strand(rows, col):
    """How many rows have 0 and how many 1 in field `col`."""
    return np.bincount([r[col] for r in rows], minlength=2).astype(np.int64)


# ------------------------------------------------------------------ what every shape is asked
def check_build(G, oracle):
    import torch
    lay, R, m = G.lay, G.R, G.m
    assert G.slen > (1 << 32) + (1 << 26) and lay["tail_off"] > 1 << 32 and lay["row"]["blen"] // 256 > 1 << 23
    assert G.n == 11 and G.summary.seq_len == G.slen + 2 * sum(len(s) for s in G.seqs)
    t = G.blob.fasta_table(G.n)
    rows = P.expected_rows(G.head, G.tail, lay)
    for c in ("boff", "blen", "slen", "llen", "elen", "norm"):
        assert t[c].tolist() == [r[c] for r in rows], c
    assert G.blob.fasta_line_regular(G.n)[G.g] == 1
    # composition: per byte value, nothing crosses a seam; what is counted is read off the oracle on three and four copies
    small = [P.giant_fasta(torch.device("cpu"), G.head, G.B, G.width, G.eol, r, G.tail)[0].numpy().tobytes() for r in (3, 4)]
    c3, c4 = (oracle.fasta_comp(s, G.n) for s in small)
    want = c3.copy()
    want[G.g] = c3[G.g] + (R - 3) * (c4[G.g] - c3[G.g])
    assert want[G.g].sum() >= G.slen and np.array_equal(c3[G.tid], c3[G.hid])
    assert np.array_equal(G.blob.fasta_comp(G.n), want)
    names = [b"h%d" % i for i in range(5)] + [b"giant"] + [b"t%d" % i for i in range(5)]
    order, ndup = G.blob.names_sort(0, G.n)
    assert ndup == 0 and order.tolist() == sorted(range(G.n), key=lambda i: names[i])


def fetch_queries(G):
    """About 2000 queries on the giant record around 2^31, 2^32 and its end, all eight flag values, lengths 1..5000; some in
    the tail records."""
    rng = np.random.default_rng(31)
    a, b = [], []
    for centre in (1 << 31, 1 << 32, G.slen):
        s = centre + rng.integers(-5000, 5001, 640)
        n = rng.integers(1, 5001, 640)
        s[:8] = centre - np.array([1, 2, 64, 65, 5000, 4999, 1, 300])      # ends on, one past and across the centre
        n[:8] = [1, 2, 64, 130, 5000, 5000, 2, 600]
        s = np.clip(s, 0, G.slen - 1)
        a.append(s)
        b.append(np.minimum(s + n, G.slen))
    a, b = np.concatenate(a), np.concatenate(b)
    ids = np.full(a.size, G.g, dtype=np.int64)
    for k, i in enumerate(G.tid.tolist()):
        L = len(G.seqs[k])
        if L:
            s = rng.integers(0, L, 16)
            ids, a, b = np.concatenate([ids, np.full(16, i)]), np.concatenate([a, s]), np.concatenate([b, np.minimum(s + rng.integers(1, L + 1, 16), L)])
    fl = (np.arange(ids.size) % 8).astype(np.uint8)
    return ids.astype(np.int64), a.astype(np.int64), b.astype(np.int64), fl


def check_fetch(G):
    ids, a, b, fl = fetch_queries(G)
    on_giant = ids == G.g
    assert ids.size >= 1984 and (b > a).all() and (b - a).max() == 5000 and (b - a).min() == 1
    low = on_giant & (b < 1 << 31)                           # a + take < 2^31: the line arithmetic of k_fetch_lines
    assert low.sum() > 100 and (on_giant & ~low).sum() > 1000 and (on_giant & (a < 1 << 31) & (b >= 1 << 31)).sum() > 100
    assert (on_giant & (a >= 1 << 32)).sum() > 600 and (on_giant & (b == G.slen)).sum() > 100
    parts = []
    for i, x, y, f in zip(ids.tolist(), a.tolist(), b.tolist(), fl.tolist()):
        s = P.letters_at(G.B, x, y) if i == G.g else G.seqs[i - G.g - 1][x:y].encode("latin-1")
        parts.append(T.apply_flags(s, f))
    exp = T._pack(parts, b - a)
    assert (exp[2] == b - a).all()
    for flags in (0, 16):                                    # 16: FX_LONG, the general kernel in place of the line arithmetic
        buf, offs, out_len = G.blob.fasta_fetch(ids, a, b, flags=flags, flags_per_query=fl)
        bad = T.first_mismatch(buf, offs, out_len, *exp)
        assert bad is None, (flags, bad)
    buf, offs = G.blob.fasta_fetch_alloc(ids, a, b, flags_per_query=fl)
    bad = T.first_mismatch(buf, offs, None, *exp)
    assert bad is None, bad


def check_search(G):
    from pyfastx_amd import search
    seam = G.B[-12:] + G.B[:12]
    for p in (P.MOTIF, seam):
        want = P.tile_rows(P.search_rows(G.B3, p), G.R, G.m, 1, order=(0, 1))
        assert want.shape[0] >= G.R - 1 and want[-1, 0] > 1 << 32
        h = search.search_blob(G.blob, p, ids=G.gid)
        assert (h.ids == G.g).all()
        assert np.array_equal(h.starts, want[:, 0]) and np.array_equal(strand01(h.strands), want[:, 1]) and np.array_equal(h.stops, h.starts + len(p))
        c = search.count_blob(G.blob, p)
        assert c[G.g].tolist() == np.bincount(want[:, 1], minlength=2).tolist() and np.array_equal(c[G.tid], c[G.hid])
    # every letter of the record is one of N's: a count per strand past 2^32
    c = search.count_blob(G.blob, "N", degenerate=True)
    assert c[G.g].tolist() == [G.slen, G.slen] and G.slen > 1 << 32
    assert c[G.hid].tolist() == [[len(s)] * 2 for s in G.seqs] and np.array_equal(c[G.tid], c[G.hid])
    # the records behind offset 2^32 answer as their twins in front
    for p in (P.MOTIF, "AC"):
        hh, ht = (search.search_blob(G.blob, p, ids=i) for i in (G.hid, G.tid))
        want = [(i, j, sd) for i, s in enumerate(G.seqs) for j, sd in P.search_rows(s, p)]
        assert len(want) >= 2 and list(zip(hh.ids.tolist(), hh.starts.tolist(), strand01(hh.strands).tolist())) == want
        assert np.array_equal(ht.ids, hh.ids + G.g + 1) and np.array_equal(ht.starts, hh.starts) and np.array_equal(ht.strands, hh.strands)


def check_kmers(G, ks=(4, 6, 7, 13)):
    from pyfastx_amd import kmer
    one = lambda s, k: kmer_truth.flat_counts(s, [0], [len(s)], k)
    idx = {}
    for k in ks:
        want = P.tile_counts(one(G.B, k), one(G.B2, k), G.R)
        assert want.sum() > 1 << 32
        got = kmer.fasta_counts_blob(G.blob, k, ids=G.gid)
        assert got.dtype == np.int64 and np.array_equal(got, want), k
        i = np.arange(4 ** k, dtype=np.int64)
        canon = np.bincount(np.minimum(i, kmer_truth.revcomp_code(i, k)), weights=want, minlength=4 ** k).astype(np.int64)   # exact below 2^53
        assert np.array_equal(kmer.fasta_counts_blob(G.blob, k, canonical=True, ids=G.gid), canon), k
    # all records: the twins add theirs
    small = kmer_truth.kmer_counts_truth(G.seqs, 4)
    want = P.tile_counts(one(G.B, 4), one(G.B2, 4), G.R) + 2 * small
    assert np.array_equal(kmer.fasta_counts_blob(G.blob, 4), want)
    assert np.array_equal(kmer.fasta_counts_blob(G.blob, 4, ids=G.tid), small)


def check_regions(G):
    from pyfastx_amd import annot
    pre = P.class_prefix(G.B)
    rng = np.random.default_rng(17)
    n = 10_000
    a = rng.integers(0, G.slen, n)
    span = np.where(np.arange(n) % 2 == 0, rng.integers(1, 5000, n), rng.integers(1, G.slen, n))
    b = np.minimum(a + span, G.slen)
    a[0], b[0] = 0, G.slen                                   # the whole record
    a[1], b[1] = (1 << 32) - 1, (1 << 32) + 1
    a[2], b[2] = 5, (1 << 32) + 7
    assert (b - a).min() == 1 and ((b - a) > 1 << 32).sum() > 2 and (a > 1 << 32).sum() > 50
    got = annot.region_blob(G.blob, np.full(n, G.g), a, b).counts
    want = P.region_rule(pre, a, b)
    assert want[0, :6].sum() == G.slen and want[0, 4] == 57 * G.R and want[0, 6] == 300 * G.R
    assert np.array_equal(got, want)
    # the twin behind 2^32
    s = G.seqs[0]
    got = annot.region_blob(G.blob, [G.hid[0], G.tid[0]], [3, 3], [len(s), len(s)]).counts
    assert got[0].tolist() == got[1].tolist() == annot_truth.region_counts(s, 3, len(s))
    return pre


# ------------------------------------------------------------------ FASTA, lines of 60 and LF
def test_lf_build(lf, oracle):
    check_build(lf, oracle)


def test_lf_fetch(lf):
    check_fetch(lf)


def test_lf_exact_search(lf):
    check_search(lf)


def test_lf_search_with_mismatches(lf):
    from pyfastx_amd import search
    G = lf
    code = {"+": 0, "-": 1}
    rows3 = [(a, b, code[sd], mm) for _, a, b, sd, mm in
             search_approx_truth.truth([G.B3], P.MOTIF, 3, anchor=range(0, 4), rev=P.revcomp(P.MOTIF))]
    want = P.tile_rows(rows3, G.R, G.m, 2, order=(0, 2))
    assert sorted(set(want[:, 3].tolist())) == [0, 1, 2, 3] and want.shape[0] >= 6 * G.R
    h = search.approx_blob(G.blob, P.MOTIF, 3, anchor=range(0, 4), ids=G.gid)
    assert (h.ids == G.g).all() and np.array_equal(h.starts, want[:, 0]) and np.array_equal(h.stops, want[:, 1])
    assert np.array_equal(strand01(h.strands), want[:, 2]) and np.array_equal(h.mismatches.astype(np.int64), want[:, 3])
    c = search.approx_count_blob(G.blob, P.MOTIF, 3, anchor=range(0, 4))
    assert c[G.g].tolist() == np.bincount(want[:, 2], minlength=2).tolist() and np.array_equal(c[G.tid], c[G.hid]) and c[G.hid].sum() >= 2


def test_lf_pwm(lf):
    from pyfastx_amd import pwm
    G = lf
    mode = pwm.strand_mode("both")
    code = {"+": 0, "-": 1}
    rows3, bs3, bp3 = pwm_truth.truth([G.B3], PWM, PWM_MIN)
    want = P.tile_rows([(a, b, code[sd], sc) for _, a, b, sd, sc in rows3], G.R, G.m, 2, order=(0, 2))
    assert want.shape[0] >= 6 * G.R
    n, hits, cnt = G.blob.fasta_pwm_scan(PWM, mode, PWM_MIN, ids=G.gid, cap=10**7, counts=True)
    rec, starts, strands, scores = hits
    assert n == want.shape[0] and (rec == G.g).all() and np.array_equal(starts, want[:, 0])
    assert np.array_equal(strand01(strands), want[:, 2]) and np.array_equal(scores.astype(np.int64), want[:, 3])
    assert cnt[0].tolist() == np.bincount(want[:, 2], minlength=2).tolist()
    # the best window: the first of the maxima, which the first copy holds
    sel = np.array([G.g, G.tid[0], G.tid[3]], dtype=np.int64)
    _, bs, bp = pwm_truth.truth([G.B3, G.seqs[0], G.seqs[3]], PWM, PWM_MIN)
    assert bs[0].tolist() == [144, 144] and bp[0].tolist() == [52, 1500]
    scores, starts = G.blob.fasta_pwm_best(PWM, mode, ids=sel)
    assert np.array_equal(scores.astype(np.int64), bs) and np.array_equal(starts, bp)


@pytest.mark.parametrize("k,w", [(15, 10), (31, 32)])
def test_lf_minimizers(lf, k, w):
    from pyfastx_amd import _lib, minimizer
    G = lf
    rows = lambda s: [(a, "+-".index(sd), c) for a, sd, c in minimizer_truth.record_rows(s, k, w)]
    want = P.tile_counts(per_strand(rows(G.B), 1), per_strand(rows(G.B2), 1), G.R)
    c = minimizer.count_blob(G.blob, k, w)
    assert want.sum() > 10**8 and c[G.g].tolist() == want.tolist()
    small = [rows(s) for s in G.seqs]
    assert c[G.hid].tolist() == [per_strand(r, 1).tolist() for r in small] and np.array_equal(c[G.tid], c[G.hid])
    hh, ht = (minimizer.minimizers_blob(G.blob, k, w, ids=i) for i in (G.hid, G.tid))
    flat = [(i,) + r for i, rs in enumerate(small) for r in rs]
    assert len(flat) > 20 and list(zip(hh.ids.tolist(), hh.starts.tolist(), strand01(hh.strands).tolist(), hh.codes.tolist())) == flat
    assert np.array_equal(ht.ids, hh.ids + G.g + 1) and np.array_equal(ht.starts, hh.starts) and np.array_equal(ht.codes, hh.codes)
    # the giant's rows are more than max_hits allows: refused with the count
    with pytest.raises(_lib.FxError) as e:
        G.blob.fasta_minimizers(k, w, _lib.FX_MZ_CANONICAL, ids=G.gid, cap=10**8)
    assert e.value.code == _lib.FX_ERANGE and e.value.n_hits == want.sum()


def test_lf_tandem_repeats(lf):
    from pyfastx_amd import tandem
    G = lf
    want = P.tile_rows(tandem_truth.repeats(G.B3), G.R, G.m, 2, order=(1, 2))
    assert {1, 3, 6} <= set(want[:, 2].tolist()) and want.shape[0] == 4 * G.R - 1 and want[-1, 1] > 1 << 32   # three per copy, one per seam
    t = tandem.repeats_blob(G.blob, ids=G.gid)
    assert (t.ids == G.g).all() and np.array_equal(t.starts, want[:, 0]) and np.array_equal(t.stops, want[:, 1])
    assert np.array_equal(t.periods.astype(np.int64), want[:, 2]) and np.array_equal(t.motif_codes.astype(np.int64), want[:, 3])
    th, tt = (tandem.repeats_blob(G.blob, ids=i) for i in (G.hid, G.tid))
    assert len(th) >= 1 and np.array_equal(tt.ids, th.ids + G.g + 1) and np.array_equal(tt.starts, th.starts) and np.array_equal(tt.stops, th.stops)


@pytest.mark.parametrize("mode", ["start", "stop"])
def test_lf_orfs(lf, mode):
    from pyfastx_amd import orf
    G = lf
    rows3 = [(a, b, orf_truth.close_coordinate(G.B3, (a, b, fr, fl)), fr, fl) for a, b, fr, fl in orf_truth.orfs(G.B3, mode=mode, min_len=600)]
    want = P.tile_rows(rows3, G.R, G.m, 3, order=(2,))
    want = want[np.lexsort([want[:, 3] < 0, want[:, 2]])]     # at one closing coordinate forward before reverse
    assert want.shape[0] >= 2 * G.R and (want[:, 3] > 0).any() and (want[:, 3] < 0).any()
    o = orf.orfs_blob(G.blob, min_len=600, mode=mode, ids=G.gid)
    assert (o.ids == G.g).all() and np.array_equal(o.starts, want[:, 0]) and np.array_equal(o.stops, want[:, 1])
    assert np.array_equal(o.frames.astype(np.int64), want[:, 3]) and np.array_equal(o.flags.astype(np.int64), want[:, 4])


def test_lf_class_runs(lf):
    from pyfastx_amd import annot
    G = lf
    for kind, letters, min_len in (("N", "Nn", 1), ("N", "Nn", 10), ("masked", "abcdefghijklmnopqrstuvwxyz", 1)):
        want = P.tile_rows(annot_truth.class_runs(G.B3, letters, min_len), G.R, G.m, 2)
        assert want.shape[0] in (G.R, 2 * G.R)
        r = annot.runs_blob(G.blob, kind, min_len=min_len, ids=G.gid)
        assert (r.ids == G.g).all() and np.array_equal(r.starts, want[:, 0]) and np.array_equal(r.stops, want[:, 1]), (kind, min_len)
    rh, rt = (annot.runs_blob(G.blob, "masked", ids=i) for i in (G.hid, G.tid))
    assert len(rh.ids) >= 2 and np.array_equal(rt.ids, rh.ids + G.g + 1) and np.array_equal(rt.starts, rh.starts) and np.array_equal(rt.stops, rh.stops)


def test_lf_translate(lf):
    from pyfastx_amd import orf
    G = lf
    rng = np.random.default_rng(23)
    n = 400
    a = np.concatenate([(1 << 32) + rng.integers(-2000, 2000, n // 2), (1 << 31) + rng.integers(-2000, 2000, n // 4), G.slen - rng.integers(1500, 4000, n // 4)])
    b = a + rng.integers(0, 1500, n)
    a[0], b[0] = (1 << 32) - 1, (1 << 32) + 2                # one codon across 2^32
    sd = (np.arange(n) % 2).astype(np.uint8)
    assert (a >= 1 << 32).sum() > 50 and ((a < 1 << 32) & (b > 1 << 32)).sum() > 20
    buf, offs = orf.translate_blob(G.blob, np.full(n, G.g), a, b, strand=sd)
    assert np.array_equal(np.diff(offs), (b - a) // 3)
    data = bytes(buf)
    for j in range(n):
        want = orf_truth.translate(P.letters_at(G.B, int(a[j]), int(b[j])).decode(), "-" if sd[j] else "+")
        assert data[offs[j]:offs[j + 1]].decode() == want, j


def test_lf_regions_and_windows(lf):
    from pyfastx_amd import annot
    G = lf
    pre = check_regions(G)
    slen = np.array([len(s) for s in G.seqs] + [G.slen] + [len(s) for s in G.seqs], dtype=np.int64)
    w = annot.window_blob(G.blob, slen, 10**6, 10**6, ids=G.gid)
    a = np.arange(0, G.slen, 10**6, dtype=np.int64)
    b = np.minimum(a + 10**6, G.slen)
    assert b[-1] - a[-1] < 10**6 and a.size > 4000               # a partial window at the end
    assert (w.ids == G.g).all() and np.array_equal(w.starts, a) and np.array_equal(w.stops, b)
    assert np.array_equal(w.counts, P.region_rule(pre, a, b))
    full = annot.window_blob(G.blob, slen, 10**6, 10**6, ids=G.gid, partial=False)
    assert np.array_equal(full.starts, a[:-1]) and np.array_equal(full.counts, P.region_rule(pre, a[:-1], b[:-1]))


def test_lf_kmer_counts(lf):
    check_kmers(lf)


@pytest.mark.parametrize("k,canonical,max_bytes", [(21, False, 16 << 30), (31, True, 16 << 30)])
def test_lf_kmer_table(lf, k, canonical, max_bytes):
    from pyfastx_amd import kmer
    G = lf
    t = lambda s: kmer_table_truth.table_truth([s], k, canonical)
    u, n = P.tile_table(t(G.B), t(G.B2), G.R)
    got = kmer.fasta_table_blob(G.blob, k, canonical=canonical, ids=G.gid, max_bytes=max_bytes)
    assert got.n_parts > 1 and got.n_windows == n.sum() > 1 << 32
    assert np.array_equal(got.codes, u) and np.array_equal(got.counts, n)


def test_lf_kmer_hits_and_sketch(lf):
    from pyfastx_amd import kmer, sketch
    from kmer_screen_truth import hits_truth
    G = lf
    k = 21
    table = kmer.KmerTable.from_strings(G.seqs, k, canonical=True)
    assert len(table) > 300
    nw, nh = kmer.fasta_hits_blob(G.blob, 0, table)
    got = np.stack([np.asarray(nw, dtype=np.int64), np.asarray(nh, dtype=np.int64)], axis=1)
    c = lambda s: np.array([x[0] for x in hits_truth([s], k, table.codes, canonical=True)], dtype=np.int64)
    assert got[G.g].tolist() == P.tile_counts(c(G.B), c(G.B2), G.R).tolist() and np.array_equal(got[G.tid], got[G.hid])
    snw, snh = hits_truth(G.seqs, k, table.codes, canonical=True)
    assert got[G.hid, 0].tolist() == snw.tolist() and got[G.hid, 1].tolist() == snh.tolist() and snh.sum() > 300
    table.release()
    sel = np.concatenate([G.hid[[0, 3]], G.gid, G.tid[[0, 3]]])
    for kw in (dict(scaled=20), dict(size=1000)):
        sk = sketch.fasta_sketch_blob(G.blob, k, ids=sel, **kw)
        cut = lambda s: sketch_truth.cut(sketch_truth.key_set_np(s, k, True).tolist(), sk.max_key, sk.size)
        want = cut(G.B2)                                       # the distinct k-mers of B^R are those of B+B
        assert len(want) > 500 and sk.hashes(2).tolist() == want
        for j, i in ((0, 0), (1, 3)):
            assert sk.hashes(j).tolist() == sk.hashes(j + 3).tolist() == cut(G.seqs[i])
        assert sk.hashes(0).size + sk.hashes(1).size > 10
        sk.release()


# ------------------------------------------------------------------ FASTA, lines of 57 and CR LF
def test_crlf_build(crlf, oracle):
    check_build(crlf, oracle)


def test_crlf_fetch(crlf):
    check_fetch(crlf)


def test_crlf_exact_search(crlf):
    check_search(crlf)


def test_crlf_kmer_counts(crlf):
    check_kmers(crlf, ks=(6, 13))


def test_crlf_regions(crlf):
    check_regions(crlf)


# ------------------------------------------------------------------ the launch split of the FASTQ forms at a small size
def _split_stream(where):
    """10^5 reads of 5..35 letters and one of 65 536: fq_maxlen = 65 536, so a launch takes 2^31 / 65 536 = 32 768 queries
    and the whole selection four launches."""
    rng = np.random.default_rng(7 + ("first", "middle", "last").index(where))
    n = 100_000
    lens = rng.integers(5, 36, n + 1)
    at = {"first": 0, "middle": 50_001, "last": n}[where]
    lens[at] = 65_536
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, int(lens.sum()), p=[.2475, .2475, .2475, .2475, .01])]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    parts = []
    for i in range(n + 1):
        s = letters[starts[i]:starts[i] + lens[i]].tobytes()
        parts.append(b"@q%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    return b"".join(parts), letters, starts, lens


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_fastq_launch_split_small(where):
    from pyfastx_amd import _lib, kmer
    _close_alive()
    raw, letters, starts, lens = _split_stream(where)
    n = lens.size
    b = _lib.Blob.from_bytes(raw, device=0)
    assert b.fastq_build().n_reads == n and n > 3 * ((1 << 31) // 65_536)
    for k in (4, 11):
        want = kmer_truth.flat_counts(letters, starts, lens, k)
        assert np.array_equal(kmer.fastq_counts_blob(b, n, k), want), k
        assert np.array_equal(kmer.fastq_counts_blob(b, n, k, canonical=True), kmer_truth.fold_canonical(want, k)), k
    # a selection with intervals: every third read, in descending order, cut at both ends
    ids = np.arange(n - 1, -1, -3, dtype=np.int64)
    if int(np.argmax(lens)) not in ids:
        ids[ids.size // 2] = int(np.argmax(lens))               # the long read is one of them
    a = np.minimum(lens[ids], 2)
    e = np.maximum(lens[ids] - 1, a)
    cut = e - a
    pos = np.concatenate([[0], np.cumsum(cut)[:-1]])
    flat = letters[np.repeat(starts[ids] + a - pos, cut) + np.arange(int(cut.sum()))]
    assert ids.size > (1 << 31) // 65_536 and cut.max() > 60_000
    for k in (4, 11):
        assert np.array_equal(kmer.fastq_counts_blob(b, n, k, ids=ids, start=a, end=e), kmer_truth.flat_counts(flat, pos, cut, k)), k
    u, c = kmer_table_truth.table_of_codes(kmer_table_truth.flat_codes(letters, starts, 21))
    t = kmer.fastq_table_blob(b, n, 21)
    assert np.array_equal(t.codes, u) and np.array_equal(t.counts, c)
    u, c = kmer_table_truth.table_of_codes(kmer_table_truth.flat_codes(flat, pos, 21, canonical=True))
    t = kmer.fastq_table_blob(b, n, 21, canonical=True, ids=ids, start=a, end=e)
    assert np.array_equal(t.codes, u) and np.array_equal(t.counts, c)
    b.close()


# ------------------------------------------------------------------ FASTQ: R copies of a block of 1000 reads, and its mates
class GiantFastq:
    """The read stream and the mate stream (a block of another length), built and indexed, and the block's reads as arrays."""

    def __init__(self):
        import torch
        from pyfastx_amd import _lib
        raw1, self.reads = P.fastq_block()
        raw2, self.mates = P.fastq_mate_block(self.reads)
        self.block, self.block2, self.nb = len(raw1), len(raw2), len(self.reads)
        self.R = R = ((1 << 32) + (1 << 26)) // min(self.block, self.block2) + 1
        self.n = R * self.nb
        self.rows = [(np.frombuffer(s.encode(), dtype=np.uint8), np.frombuffer(q.encode(), dtype=np.uint8)) for _, s, q in self.reads]
        self.rows2 = [(np.frombuffer(s.encode(), dtype=np.uint8), np.frombuffer(q.encode(), dtype=np.uint8)) for _, s, q in self.mates]
        self.seqs = [s for _, s, _ in self.reads]
        self.blobs = []
        for raw in (raw1, raw2):
            t = P.periodic_fastq(torch.device("cuda:0"), raw, R)
            torch.cuda.synchronize()
            b = _lib.Blob.from_device(t.data_ptr(), R * len(raw), device=0, keepalive=t)
            assert b.fastq_build().n_reads == self.n
            self.blobs.append(b)
            del t
        self.blob, self.mate = self.blobs
        self.across = (1 << 32) // self.block                  # the copy that lies across offset 2^32
        ids = np.concatenate([c * self.nb + np.arange(self.nb, dtype=np.int64) for c in (0, self.across, R - 1)])
        np.random.default_rng(2).shuffle(ids)
        self.ids, self.of = ids, ids % self.nb

    def close(self):
        import torch
        for b in self.blobs:
            b.close()
        self.blobs, self.blob, self.mate = [], None, None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def fq():
    _room()
    g = GiantFastq()
    _alive.append(g.close)
    yield g
    if g.blob is not None:
        _close_alive()


def test_fq_build(fq):
    assert fq.R * fq.block > (1 << 32) + (1 << 26) and fq.R * fq.block2 > (1 << 32) + (1 << 26) and fq.block != fq.block2
    for blob, raw_rows, block, reads in ((fq.blob, T.fastq_rows(P.fastq_block()[0]), fq.block, fq.reads),
                                         (fq.mate, T.fastq_rows(P.fastq_mate_block(fq.reads)[0]), fq.block2, fq.mates)):
        t = blob.fastq_table(fq.n)
        first = np.array(raw_rows, dtype=np.int64)              # soff, qoff, rlen of the block
        shift = (np.arange(fq.R, dtype=np.int64) * block)[:, None]
        assert np.array_equal(t["soff"].reshape(fq.R, fq.nb), first[None, :, 0] + shift)
        assert np.array_equal(t["qoff"].reshape(fq.R, fq.nb), first[None, :, 1] + shift)
        assert np.array_equal(t["rlen"].reshape(fq.R, fq.nb), np.broadcast_to(first[:, 2], (fq.R, fq.nb)))
        assert t["soff"][-1] > 1 << 32 and t["soff"][-fq.nb] == first[0, 0] + (fq.R - 1) * block      # the last copy
        name_len = np.array([len(n.split(" ")[0]) for n, _, _ in reads], dtype=np.int64)
        assert np.array_equal(t["name_len"].reshape(fq.R, fq.nb), np.broadcast_to(name_len, (fq.R, fq.nb)))
        assert np.array_equal(t["name_off"].reshape(fq.R, fq.nb)[:, 0], shift[:, 0] + 1)
    lo, hi = fq.across * fq.block, (fq.across + 1) * fq.block
    assert lo < 1 << 32 < hi and 0 < fq.across < fq.R - 1


def test_fq_read_stats_trim_records(fq):
    from pyfastx_amd import qc, trim
    from test_gpu_fastq_qc import stats_truth
    from trim_truth import record, trim_truth_fast, truth_kwargs
    st = qc.read_stats_blob(fq.blob, fq.n, fq.ids, 33, 20)
    want = stats_truth(33, fq.rows, 20, fq.of)
    assert sorted(st) == sorted(want)
    for k in want:
        assert st[k].dtype == want[k].dtype and np.array_equal(st[k], want[k]), k
    args = trim.trim_args(adapter=P.ADAPTER, min_overlap=5, max_error_rate=0.1, front_qual=10, window=(2, 3), tail_qual=20)
    iv = trim.trim_blob(fq.blob, fq.n, fq.ids, 33, args)
    one = [trim_truth_fast(s, q, 33, **truth_kwargs(args)) for s, q in fq.rows]
    a = np.array([one[i][0] for i in fq.of], dtype=np.int64)
    b = np.array([one[i][1] for i in fq.of], dtype=np.int64)
    lens = np.array([len(s) for s, _ in fq.rows], dtype=np.int64)
    assert (b[lens[fq.of] >= 60] < lens[fq.of][lens[fq.of] >= 60]).any() and (a > 0).any()
    assert np.array_equal(iv["start"], a) and np.array_equal(iv["end"], b)
    buf, offs, kept = trim.records_blob(fq.blob, fq.n, fq.ids, a, b, 20)
    parts = [record(b"@" + fq.reads[i][0].encode(), *fq.rows[i], x, y) if y - x >= 20 else b"" for i, x, y in zip(fq.of.tolist(), a.tolist(), b.tolist())]
    assert kept == sum(1 for x in parts if x) and 0 < kept < fq.ids.size
    assert np.array_equal(np.diff(offs), [len(x) for x in parts]) and buf.tobytes() == b"".join(parts)


def test_fq_screen_and_demux(fq):
    from pyfastx_amd import demux, kmer
    from demux_truth import bins_of, demux_truth_fast, segments
    from kmer_screen_truth import hits_truth, screen_truth
    table = kmer.KmerTable.from_strings([P.ADAPTER] + list(P.BARCODES), 8, canonical=False)
    nw, nh = kmer.fastq_hits_blob(fq.blob, 0, fq.n, table, ids=fq.ids)
    wnw, wnh = hits_truth(fq.seqs, 8, table.codes)
    assert wnh.sum() > 100 and np.array_equal(np.asarray(nw, dtype=np.int64), wnw[fq.of]) and np.array_equal(np.asarray(nh, dtype=np.int64), wnh[fq.of])
    got = kmer.fastq_screen_blob(fq.blob, 0, fq.n, table, min_hits=2, ids=fq.ids)
    assert np.array_equal(got, screen_truth(wnw[fq.of], wnh[fq.of], 2)) and 0 < got.size < fq.ids.size
    table.release()
    rlen = np.tile(np.array([len(s) for s in fq.seqs], dtype=np.int64), fq.R)
    samples = {"s%d" % k: bc for k, bc in enumerate(P.BARCODES)}
    heads = [(b"@" + n.encode(), s.encode()) for n, s, _ in fq.reads]
    for where in ("5p", "header"):
        args = demux.demux_args(samples, where=where, mismatches=1)
        segs, sheet = segments(args)
        want = demux_truth_fast(heads, segs, sheet, args["margin"])
        dm = demux.demux_blob(fq.blob, rlen, fq.ids, args)
        assert (want[0] >= 0).sum() > 50 and (want[1] == 1).any()
        for got, w in zip((dm.sample, dm.dist, dm.second), want):
            assert np.array_equal(got, w[fq.of]), where
        order, bin_off, counts = bins_of(want[0][fq.of], len(sheet))
        assert np.array_equal(dm.counts, counts) and np.array_equal(dm.bin_off, bin_off) and np.array_equal(dm.order, order)


def test_fq_pairs(fq):
    from pyfastx_amd import pair
    from pair_truth import NONE, merged_truth, overlap_truth
    args = pair.overlap_args()
    cols = pair.overlap_blob(fq.blob, fq.mate, fq.n, fq.ids, args)
    one = [overlap_truth(r1[0], r2[0], **args) for r1, r2 in zip(fq.rows, fq.rows2)]
    assert sum(r["diag"] != NONE for r in one) > 500 and any(r["mismatches"] > 0 for r in one)
    for k in ("diag", "overlap", "mismatches", "end1", "end2"):
        assert np.array_equal(np.asarray(cols[k], dtype=np.int64), np.array([one[i][k] for i in fq.of], dtype=np.int64)), k
    buf, offs, merged = pair.merge_blob(fq.blob, fq.mate, fq.n, fq.ids, cols["diag"], 30)
    memo = {}
    parts = []
    for i in fq.of.tolist():
        if i not in memo:
            memo[i] = merged_truth(b"@" + fq.reads[i][0].encode(), *fq.rows[i], *fq.rows2[i], one[i]["diag"], 30)
        parts.append(memo[i])
    assert merged == sum(1 for x in parts if x) and 0 < merged < fq.ids.size
    assert np.array_equal(np.diff(offs), [len(x) for x in parts]) and buf.tobytes() == b"".join(parts)


def test_fq_whole_stream_counts(fq):
    from pyfastx_amd import kmer, qc, sketch
    from test_gpu_fastq_qc import cycle_truth
    prof = qc.cycle_profile_blob(fq.blob, 300, 33)
    qual, base, depth = cycle_truth(fq.rows, 300)
    assert depth[0] * fq.R == fq.n - 4 * fq.R                  # four reads of the block are empty
    assert np.array_equal(prof.qual, qual * fq.R) and np.array_equal(prof.base, base * fq.R) and np.array_equal(prof.depth, depth * fq.R)
    for k in (4, 11):
        want = kmer_truth.kmer_counts_truth(fq.seqs, k) * fq.R
        assert want.sum() > 1 << 30 and np.array_equal(kmer.fastq_counts_blob(fq.blob, fq.n, k), want), k
    u, c = kmer_table_truth.table_truth(fq.seqs, 21)
    t = kmer.fastq_table_blob(fq.blob, fq.n, 21)
    assert np.array_equal(t.codes, u) and np.array_equal(t.counts, c * fq.R) and t.n_windows == c.sum() * fq.R
    sk = sketch.fastq_sketch_blob(fq.blob, fq.n, 21, scaled=50)
    want = sketch_truth.fastq_set(fq.seqs, 21, True, sk.max_key, form=sketch_truth.key_set_np)
    assert len(want) > 500 and sk.hashes(0).tolist() == want
    sk.release()


def test_fq_duplicates(fq):
    from pyfastx_amd import dedup
    import dedup_truth
    for revcomp in (False, True):
        bf = dedup_truth.first_truth(fq.seqs, revcomp)          # the first occurrence of read i is the block's of i % nb
        assert (bf != np.arange(fq.nb)).sum() >= (40 if revcomp else 20)
        first, n_groups, _ = dedup.duplicates_blob(fq.blob, fq.n, revcomp=revcomp)
        assert n_groups == np.unique(bf).size and np.array_equal(first.reshape(fq.R, fq.nb), np.broadcast_to(bf, (fq.R, fq.nb)))
        pos, copies, n_groups, _ = dedup.dedup_blob(fq.blob, fq.n, revcomp=revcomp, return_counts=True)
        wpos, wcopies = dedup_truth.dedup_truth(fq.seqs, revcomp)
        assert n_groups == wpos.size and np.array_equal(pos, wpos) and np.array_equal(copies, wcopies * fq.R)
