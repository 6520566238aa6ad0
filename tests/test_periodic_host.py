"""The reference of tests/test_gpu_big_offsets.py alone, no GPU: the rules of tests/periodic.py against the truth modules on
five copies of a small block, and the builders (on the CPU device) against the oracle's parse.  This is where "no row spans
m letters" is shown for the block and the parameters the GPU test uses: tile_rows asserts it."""
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

M, R = 6060, 5                                               # 101 lines of 60: 6161 bytes per copy, odd
PWM = np.array([[9 if "ACGT"[c] == ch else -9 for c in range(4)] for ch in P.MOTIF], dtype=np.int32)


@pytest.fixture(scope="module")
def blocks():
    B = P.make_block(M)
    return B, B * 2, B * 3, B * R


def orf_rows(seq, mode, min_len):
    """(start, stop, frame, flags, close): the truth's rows with the coordinate their order goes by."""
    return [r + (orf_truth.close_coordinate(seq, r),) for r in orf_truth.orfs(seq, mode=mode, min_len=min_len)]


def test_block_holds_what_was_planted(blocks):
    B, _, B3, _ = blocks
    assert len(B) == M and set(B) <= set("ACGTNacgt")
    assert [r[0] for r in P.search_rows(B, P.MOTIF)] == [52, 1000, 1500] and P.search_rows(B, P.MOTIF)[2][1] == 1
    rep = tandem_truth.repeats(B3)
    assert {1, 3, 6} <= {r[2] for r in rep}
    assert any(r[0] < M <= r[1] - 1 for r in rep) and any(r[0] < 2 * M <= r[1] - 1 for r in rep)       # one across each seam
    assert [b - a for a, b in annot_truth.class_runs(B, "Nn")] == [50, 7]
    assert annot_truth.class_runs(B, "acgtn") == [(3200, 3500)]
    rows = orf_truth.orfs(B, min_len=600)
    assert sorted(r[2] > 0 for r in rows) == [False, True] and all(r[1] - r[0] == 3 * P.ORF_CODONS + 3 for r in rows)   # ATG and the codons, not the stop


@pytest.mark.parametrize("width,eol", [(60, 1), (57, 2)])
def test_copy_layout(width, eol):
    m = 101 * width
    one = P.block_lines(P.make_block(m), width, eol)
    assert len(one) == 101 * (width + eol) and len(one) % 2 == 1 and m % 3 == 0
    assert len({(j * len(one)) % 256 for j in range(256)}) == 256          # a copy begins at every phase of a 256-byte run
    assert P.copies_for(1001 * width) * 1001 * width > (1 << 32) + (1 << 26) >= (P.copies_for(1001 * width) - 1) * 1001 * width


def test_tile_rows_search(blocks):
    B, _, B3, BR = blocks
    seam = B[-12:] + B[:12]
    for p in (P.MOTIF, seam):
        want = np.array(P.search_rows(BR, p), dtype=np.int64)
        assert want.shape[0] >= R - 1
        assert np.array_equal(P.tile_rows(P.search_rows(B3, p), R, M, 1, order=(0, 1)), want)


def test_tile_rows_approx_and_pwm(blocks):
    B, _, B3, BR = blocks
    code = {"+": 0, "-": 1}
    f = lambda s: [(a, b, code[sd], mm) for _, a, b, sd, mm in
                   search_approx_truth.truth([s], P.MOTIF, 3, anchor=range(0, 4), rev=P.revcomp(P.MOTIF))]
    want = np.array(f(BR), dtype=np.int64)
    assert sorted(set(want[:, 3].tolist())) == [0, 1, 2, 3]
    assert np.array_equal(P.tile_rows(f(B3), R, M, 2, order=(0, 2)), want)
    g = lambda s: [(a, b, code[sd], sc) for _, a, b, sd, sc in pwm_truth.truth([s], PWM, 9 * 16 - 18 * 3)[0]]
    want = np.array(g(BR), dtype=np.int64)
    assert want.shape[0] >= 6 * R
    assert np.array_equal(P.tile_rows(g(B3), R, M, 2, order=(0, 2)), want)


def test_tile_rows_tandem_orfs_runs(blocks):
    B, _, B3, BR = blocks
    assert np.array_equal(P.tile_rows(tandem_truth.repeats(B3), R, M, 2, order=(1, 2)), np.array(tandem_truth.repeats(BR), dtype=np.int64))
    for mode, min_len in (("start", 600), ("stop", 600)):
        want = np.array(orf_rows(BR, mode, min_len), dtype=np.int64)
        got = P.tile_rows([(a, b, c, fr, fl) for a, b, fr, fl, c in orf_rows(B3, mode, min_len)], R, M, 3, order=(2, 3))
        assert want.shape[0] >= 2 * R
        # forward before reverse at one closing coordinate: frames 1..3 before -1..-3
        key = np.lexsort([-np.sign(got[:, 3]), got[:, 2]])
        assert np.array_equal(got[key][:, [0, 1, 3, 4, 2]], want), mode
    for letters, min_len in (("Nn", 1), ("Nn", 10), ("acgtn", 1)):
        want = np.array(annot_truth.class_runs(BR, letters, min_len), dtype=np.int64)
        assert np.array_equal(P.tile_rows(annot_truth.class_runs(B3, letters, min_len), R, M, 2), want)


@pytest.mark.parametrize("k,w", [(15, 10), (31, 32)])
def test_minimizer_rules(blocks, k, w):
    B, B2, B3, BR = blocks
    f = lambda s: [(a, "+-".index(sd), code) for a, sd, code in minimizer_truth.record_rows(s, k, w)]
    want = f(BR)
    got = P.tile_rows(np.array([r[:2] for r in f(B3)], dtype=np.int64), R, M, 1)
    assert np.array_equal(got, np.array([r[:2] for r in want], dtype=np.int64))
    per_strand = lambda rows: np.bincount([r[1] for r in rows], minlength=2)
    assert np.array_equal(P.tile_counts(per_strand(f(B)), per_strand(f(B2)), R), per_strand(want))


@pytest.mark.parametrize("canonical", [False, True])
def test_kmer_rules(blocks, canonical):
    B, B2, _, BR = blocks
    for k in (4, 6, 7):
        c = lambda s: kmer_truth.kmer_counts_truth([s], k, canonical)
        assert np.array_equal(P.tile_counts(c(B), c(B2), R), c(BR)), k
    for k in (21, 31):
        t = lambda s: kmer_table_truth.table_truth([s], k, canonical)
        u, n = P.tile_table(t(B), t(B2), R)
        wu, wn = t(BR)
        assert np.array_equal(u, wu) and np.array_equal(n, wn), k
        assert np.array_equal(sketch_truth.key_set_np(B2, k, canonical), sketch_truth.key_set_np(BR, k, canonical))


def test_region_and_letters(blocks):
    B, _, _, BR = blocks
    pre = P.class_prefix(B)
    rng = np.random.default_rng(1)
    a = rng.integers(0, R * M, 300)
    b = np.minimum(a + rng.integers(1, R * M, 300), R * M)
    a[0], b[0] = 0, R * M
    got = P.region_rule(pre, a, b)
    for j in range(a.size):
        assert got[j].tolist() == annot_truth.region_counts(BR, int(a[j]), int(b[j])), j
        assert P.letters_at(B, int(a[j]), int(b[j])) == BR[a[j]:b[j]].encode()


@pytest.mark.parametrize("width,eol", [(60, 1), (57, 2)])
def test_giant_fasta_parses_as_laid_out(oracle, width, eol):
    import torch
    m = 101 * width
    B = P.make_block(m)
    head, hseqs = P.small_fasta("h")
    tail, tseqs = P.small_fasta("t")
    assert hseqs == tseqs and len(head) == len(tail)
    t, lay = P.giant_fasta(torch.device("cpu"), head, B, width, eol, R, tail)
    raw = t.numpy().tobytes()
    assert len(raw) == lay["n_bytes"] and not raw.endswith(b"\n")
    assert raw[lay["body_off"]:lay["tail_off"]] == P.block_lines(B, width, eol) * R and raw[lay["tail_off"]:] == tail[:-1]
    recs, total = oracle.fasta_index(raw)
    rows = P.expected_rows(head, tail, lay)
    assert len(recs) == len(rows) == 11 and lay["giant"] == 5 and lay["tail_ids"] == [6, 7, 8, 9, 10]
    for r, mine in zip(recs, rows):
        assert [int(r[c]) for c in ("boff", "blen", "slen", "llen", "elen", "norm")] == [mine[c] for c in ("boff", "blen", "slen", "llen", "elen", "norm")]
    g = rows[lay["giant"]]
    assert T.despace(raw[g["boff"]:g["boff"] + g["blen"]]).decode() == B * R
    for i, s in enumerate(hseqs):                            # the tail's rows are the head's, moved
        h, tl = rows[i], rows[lay["tail_ids"][i]]
        assert T.despace(raw[h["boff"]:h["boff"] + h["blen"]]).decode("latin-1") == s
        assert dict(tl, boff=0) == dict(h, boff=0) and tl["boff"] - lay["tail_off"] == h["boff"]


def test_periodic_fastq_parses_as_laid_out(oracle):
    import torch
    raw1, reads = P.fastq_block()
    assert len(raw1) % 2 == 1 and len(reads) == 1000
    lens = [len(s) for _, s, _ in reads]
    assert set(lens) == set(range(301)) and len({len(n) for n, _, _ in reads}) >= 6
    assert {ord(c) for _, _, q in reads for c in q} == set(range(33, 127))
    seqs = [s for _, s, _ in reads]
    assert sum(seqs[i] == seqs[i - 10] for i in range(49, 1000, 50)) == 20 and P.revcomp(seqs[28]) == seqs[48]
    assert any(s.startswith(P.BARCODES[0]) and s.endswith(P.ADAPTER[:12]) for s in seqs)
    raw = P.periodic_fastq(torch.device("cpu"), raw1, 3).numpy().tobytes()
    assert raw == raw1 * 3
    recs, size, _ = oracle.fastq_index(raw)
    assert len(recs) == 3000 and size == 3 * sum(lens)
    rows = T.fastq_rows(raw1)
    for c in range(3):
        part = recs[c * 1000:(c + 1) * 1000]
        assert [(int(r["soff"]) - c * len(raw1), int(r["qoff"]) - c * len(raw1), int(r["rlen"])) for r in part] == rows
        assert [int(r["rlen"]) for r in part] == lens
