"""CPU: the inputs and the truth of the tour (tests/tour.py) that tests/test_gpu_clean_memory.py runs on the device.

The seam inputs must stay over the seams they were sized for -- two chunks of the three-launch scan over the runs of one
record, more than one scan chunk and more than two radix tiles of reads -- and no larger; the small inputs must hold the record
shapes and the planted features, and the truth of the small tour must report each of them: a tour whose results were all empty
arrays would pass every comparison."""
import numpy as np
import pytest

import tour


@pytest.fixture(scope="module")
def sets():
    return {w: tour.make(w) for w in ("small", "seam")}


def _runs(recs):
    """Runs of SRCH_RUN bytes a record's body touches (srch_nruns of csrc/fx_search.hpp)."""
    b, e = recs["boff"].astype(np.int64), (recs["boff"] + recs["blen"]).astype(np.int64)
    return np.where(e > b, (e - 1) // tour.SRCH_RUN - b // tour.SRCH_RUN + 1, 0)


def test_the_constants_are_the_kernels():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "pyfastx_amd", "csrc", "fx_search.hpp")).read()
    assert int(re.search(r"constexpr int SRCH_RUN = (\d+);", src).group(1)) == tour.SRCH_RUN
    per = int(re.search(r"constexpr int SRCH_PER = (\d+);", src).group(1))
    block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(ROOT, "pyfastx_amd", "csrc", "fx_kernels.hpp")).read()).group(1))
    assert re.search(r"constexpr int SRCH_CHUNK = BLOCK \* SRCH_PER;", src) and block * per == tour.SRCH_CHUNK
    sort = open(os.path.join(ROOT, "pyfastx_amd", "csrc", "fx_sort.hip")).read()
    assert re.search(r"RS_BLOCK = 256, RS_ROUNDS = FX_RS_ROUNDS, RS_TILE = RS_BLOCK \* RS_ROUNDS", sort)
    assert 256 * int(re.search(r"#define FX_RS_ROUNDS (\d+)", sort).group(1)) == tour.RS_TILE


def test_seam_inputs_cross_each_seam_and_no_more(oracle, sets):
    inp = sets["seam"]
    recs, _ = oracle.fasta_index(inp["fa"])
    runs = _runs(recs)
    assert runs.max() > tour.SRCH_CHUNK and runs.sum() <= 2 * tour.SRCH_CHUNK           # two chunks of runs, the largest record alone over one
    assert 1.1e6 < len(inp["fa"]) < 1.4e6
    n = len(inp["reads1"])
    assert n == len(inp["reads2"]) == 4500 and tour.SRCH_CHUNK < n <= 2 * tour.SRCH_CHUNK and 2 * tour.RS_TILE < n <= 3 * tour.RS_TILE
    rq, _, _ = oracle.fastq_index(inp["fq1"])
    assert len(rq) == n and rq["rlen"].tolist() == [len(r[1]) for r in inp["reads1"]]
    # the small set stays under every one of them
    small = sets["small"]
    recs, _ = oracle.fasta_index(small["fa"])
    assert _runs(recs).sum() < tour.SRCH_CHUNK and len(small["reads1"]) == 300 < tour.RS_TILE


@pytest.mark.parametrize("which", ["small", "seam"])
def test_the_records_have_their_shapes(oracle, sets, which):
    inp = sets[which]
    recs, total = oracle.fasta_index(inp["fa"])
    assert len(recs) == 8 and recs["slen"].tolist() == [len(s) for s in inp["seqs"]] and total == sum(len(s) for s in inp["seqs"])
    if which == "small":
        assert 19000 < len(inp["fa"]) < 21000 and recs["slen"][0] > 5000
    assert (recs["llen"][0], recs["elen"][0]) == (61, 1)                                 # wrapped at 60
    assert recs["elen"][1] == 2                                                         # CRLF
    low = inp["seqs"][2]                                                                # lower case but for one run of N
    assert low.replace("N", "n") == low.lower() and low.startswith("nnnnnnn") and "n" * 130 in low and "N" * 20 in low
    assert recs["slen"][3] == 0                                                         # empty
    assert recs["norm"][4] == 0 and recs["norm"][[0, 1, 2, 5, 6, 7]].all()               # an odd middle line
    assert not inp["fa"].endswith(b"\n")                                                # the last line unterminated
    # reads: lengths 1..150, a tenth exact duplicates, the adapter in about a third, the barcode behind the last ':'
    r1 = inp["reads1"]
    lens = [len(r[1]) for r in r1]
    assert min(lens) >= 1 and max(lens) <= 150 and max(lens) > 140 and min(lens) < 5
    seen, dup = set(), 0
    for _, s, _ in r1:
        dup += s in seen
        seen.add(s)
    assert dup >= len(r1) // 10
    assert len(r1) * 28 // 100 <= sum(tour.ADAPTER in s for _, s, _ in r1) <= len(r1) * 40 // 100     # a third, give or take the duplicates
    assert all(len(h.rsplit(":", 1)[1]) == 8 for h, _, _ in r1)
    assert [h.split(" ")[0] for h, _, _ in r1] == [h.split(" ")[0] for h, _, _ in inp["reads2"]]


def test_the_truth_covers_the_tour_and_every_planted_feature_gives_rows(sets):
    E = tour.expected_small()
    calls = tour.call_names("small")
    assert len(calls) == len(set(calls)) == 55
    assert {k.split(".")[0] for k in E} | set(tour.NO_TRUTH) == set(calls) and not {k.split(".")[0] for k in E} & set(tour.NO_TRUTH)
    rows = lambda call: set(zip(*(E[call + "." + c].tolist() for c in ("ids", "starts", "stops", "strands"))))
    P, M = ord("+"), ord("-")
    # the motif (one across a line end, one in the CRLF record, one that ends the unterminated last line) and its reverse complement
    assert {(0, 57, 69, P), (0, 300, 312, P), (0, 1200, 1212, M), (1, 700, 712, P), (4, 610, 622, M), (7, 1985, 1997, P)} <= rows("fa_search_short")
    assert rows("fa_search_long") == {(0, 4000, 4040, P), (7, 100, 140, P)}
    assert E["fa_search_counts.counts"].sum() == len(rows("fa_search_short")) and E["fa_search_counts.counts_long"].sum() == 2
    # mismatches: one and two outside the anchor are hits, one inside it is not
    approx = dict(zip(zip(E["fa_search_approx.ids"].tolist(), E["fa_search_approx.starts"].tolist()), E["fa_search_approx.mismatches"].tolist()))
    assert approx[(0, 4500)] == 1 and approx[(0, 4600)] == 2 and (0, 4700) not in approx and approx[(0, 300)] == 0
    # edits: the deletion, the insertion and the exact copy are the three best rows
    best = set(zip(E["fa_search_edit_best.starts"].tolist(), E["fa_search_edit_best.stops"].tolist(), E["fa_search_edit_best.edits"].tolist()))
    assert {(5000, 5015, 1), (5100, 5117, 1), (5200, 5216, 0)} <= best and E["fa_search_edit_all.ids"].size > len(best)
    top = int(np.array(tour.PWM_INTS).max(axis=1).sum())
    scan = dict(zip(zip(E["fa_pwm_scan.starts"].tolist(), E["fa_pwm_scan.strands"].tolist()), E["fa_pwm_scan.scores"].tolist()))
    assert scan[(5500, P)] == top and scan[(5600, M)] == top and E["fa_pwm_best.scores"][1].tolist() == [top, top]
    assert E["fa_pwm_best.starts"][2].tolist() == [-1, -1]                               # the empty record
    # the poly-A stretch and the tandem repeat of period 3; the N runs; the ORF
    tr = set(zip(E["fa_tandem_repeats.ids"].tolist(), E["fa_tandem_repeats.starts"].tolist(), E["fa_tandem_repeats.periods"].tolist()))
    assert (0, 2000, 1) in tr and any(i == 0 and 3498 <= a <= 3500 and p == 3 for i, a, p in tr)
    runs = set(zip(E["fa_class_runs.ids"].tolist(), E["fa_class_runs.starts"].tolist(), E["fa_class_runs.stops"].tolist()))
    assert {(2, 0, 7), (2, 400, 401), (2, 900, 1030), (2, 1500, 1520), (2, 2400, 2500)} <= runs
    for mode in ("start", "stop"):
        orfs = zip(E["fa_orfs_%s.ids" % mode].tolist(), E["fa_orfs_%s.starts" % mode].tolist(), E["fa_orfs_%s.stops" % mode].tolist())
        assert any(i == 0 and a <= 2500 and b == 2500 + len(tour.ORF) - 3 for i, a, b in orfs), mode
    # no family is empty
    for k, v in E.items():
        assert v.size > 0, k
    assert E["fa_minimizers.ids"].size > 1000 and E["fa_kmer_table21.codes"].size > 10000 and (E["fa_kmer_hits_lds.n_hits"] > 0).any()
    assert E["fa_window_stats.ids"].size > 90 and (E["fa_region_stats.counts"].sum(axis=1) > 0).any() and E["fa_translate_many.buf"].size > 1000
    assert (E["fa_sketch_scaled.shared"].diagonal() == E["fa_sketch_scaled.sizes"]).all() and E["fa_sketch_size.sizes"].max() == 64
    # reads: the adapter is cut, duplicates are found, every sample and the unassigned bin get reads, mates overlap and merge
    n = len(sets["small"]["reads1"])
    lens = np.array([len(r[1]) for r in sets["small"]["reads1"]])
    assert (E["fq_trim.end"] < lens - 5).sum() > n // 5 and (E["fq_trim.start"] <= E["fq_trim.end"]).all()
    assert (np.diff(E["fq_records.offs"]) > 0).sum() > n // 2
    assert (E["fq_duplicates.first"] != np.arange(n)).sum() >= n // 10 and E["fq_dedup.copies"].max() >= 2
    assert (E["fq_demux.counts"][:5] > 0).all() and (E["fq_demux.dist"] == 1).sum() > n // 10
    assert (E["pair_overlap.insert"] > 0).sum() > n // 4 and (E["pair_overlap.end1"] < lens).sum() > n // 10
    assert (np.diff(E["pair_merge.offs"]) > 0).sum() > n // 4
    assert (E["fq_kmer_hits.n_hits"] > 0).any() and E["fq_screen.ids"].size > 0 and E["fq_sketch.sizes"][0] > 1000


def test_the_bgzf_framing_is_read_by_zlib(sets):
    import zlib
    raw, framed = sets["small"]["fa"], tour.bgzf(sets["small"]["fa"], 6000)
    out, rest, members = b"", framed, 0
    while rest:
        d = zlib.decompressobj(31)
        out += d.decompress(rest)
        rest = d.unused_data
        members += 1
    assert out == raw and members == (len(raw) + 5999) // 6000 + 1
