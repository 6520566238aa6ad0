"""-m gpu: no result depends on what device memory held before a call.

The tour of tests/tour.py -- every compute entry once, on the small inputs and on inputs that cross the seams of the shared
scan and sort -- runs in child processes (tests/tour_child.py), one at a time, and must give the same arrays (a) as the truth
modules say, in a fresh process, (b) with every block the allocation routes hand out filled with 0xFF first
(FX_DEBUG_FILL=255), (c) with the calls in reverse order, and with every call behind a wider call of the same entry on the same
handle, which is what reaches the grow-only arrays of a handle, and (d) with (b) and the second form of (c) at once.  Every
compared value is an integer or a byte: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tour

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# Ends a child that hangs, nothing else: ten times the wall time of the plain forward tour on the seam inputs, and at least 60 s.
# Measured on the MI355X at this commit: the tour 0.3 s, the whole child with its imports 2.7 s (5.5 s for the plain and the
# filled one together), so the floor of 60 s holds.
TIMEOUT = 60

# Every call of the tour, by name (tour.call_names): the builds, then the order "forward" takes.
CALLS = [
    "fa_build", "fq_build",
    "fa_build_comp", "fa_comp_dense", "fa_comp_sparse", "fa_line_regular", "fa_len_stats", "fa_names_sort", "fa_names_lookup", "fa_fetch",
    "fa_search_short", "fa_search_long", "fa_search_counts", "fa_search_approx", "fa_search_edit_best", "fa_search_edit_all",
    "fa_pwm_scan", "fa_pwm_best", "fa_minimizers", "fa_sketch_scaled", "fa_sketch_size", "fa_sketch_pooled",
    "fa_kmer_counts4", "fa_kmer_counts11", "fa_kmer_table21", "fa_kmer_hits_lds", "fa_kmer_hits_global",
    "fa_region_stats", "fa_window_stats", "fa_class_runs", "fa_tandem_repeats", "fa_orfs_start", "fa_orfs_stop", "fa_translate_many",
    "fq_build_comp", "fq_fetch", "fq_read_stats", "fq_cycle_profile", "fq_select", "fq_trim", "fq_records",
    "fq_kmer_counts", "fq_kmer_table", "fq_kmer_hits", "fq_screen", "fq_duplicates", "fq_dedup", "fq_demux", "fq_sketch",
    "pair_overlap", "pair_merge", "pair_trim", "fastx_fasta", "fastx_fastq", "bgzf_fasta",
]

# The calls that take no block from plain allocation or the scratch pool, read off the host code (csrc/fxgpu.hip): every other
# call must have received at least one filled block, or the filled run did not reach it.
ALLOCATES_NOTHING = {
    "fa_line_regular": "fx_fasta_line_regular copies the handle's fa_reg column, which the build wrote, straight into the caller's array",
}

# The columns of the small tour that no truth module covers (tour.expected_small): compared between the situations only.  A
# literal list, so that it can only shrink on purpose.
NO_TRUTH_KEYS = [
    "fa_build.hoff", "fa_build.n_lines", "fa_build_comp.n_bytes", "fa_build_comp.n_lines",
    "fa_len_stats.count_ge", "fa_len_stats.longest_id", "fa_len_stats.longest_len", "fa_len_stats.med_hi", "fa_len_stats.med_lo",
    "fa_len_stats.n_seq", "fa_len_stats.nx_count", "fa_len_stats.nx_len", "fa_len_stats.shortest_id", "fa_len_stats.shortest_len",
    "fa_len_stats.sum_len", "fa_line_regular.regular", "fa_names_lookup.ids", "fa_names_sort.n_dup", "fa_names_sort.order",
    "fq_build.first_id", "fq_build.n_lines", "fq_build.name_off",
    "fq_build_comp.base", "fq_build_comp.first_id", "fq_build_comp.meta", "fq_build_comp.n_bytes", "fq_build_comp.n_lines",
    "fq_cycle_profile.base", "fq_cycle_profile.depth", "fq_cycle_profile.qual",
    "fq_read_stats.length", "fq_read_stats.n_gc", "fq_read_stats.n_low", "fq_read_stats.n_other", "fq_read_stats.qmax",
    "fq_read_stats.qmin", "fq_read_stats.qsum", "fq_select.ids",
]

_state = {"dead": None, "inputs": None, "runs": {}}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("tour")
    if _state["inputs"] is None:
        _state["inputs"] = tour.inputs(d)
    return str(d)


def child(work, which, order, fill=None):
    """The arrays of one tour in a process of its own (each situation once per module).  A child that ends with a status, a
    signal or the timeout fails the test and every later one of the module, which then starts nothing more."""
    if _state["dead"]:
        pytest.fail("no further process is started: " + _state["dead"], pytrace=False)
    key = (which, order, fill)
    if key in _state["runs"]:
        return _state["runs"][key]
    out = os.path.join(work, "%s_%s_%s.npz" % (which, order, "plain" if fill is None else fill))
    env = {k: v for k, v in os.environ.items() if k != "FX_DEBUG_FILL"}
    if fill is not None:
        env["FX_DEBUG_FILL"] = str(fill)
    what = "tour %s %s%s" % (which, order, "" if fill is None else " FX_DEBUG_FILL=%d" % fill)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "tour_child.py"), work, which, order, out], env=env, capture_output=True,
                           text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _state["dead"] = "%s did not end within %d s" % (what, TIMEOUT)
        pytest.fail(_state["dead"] + "\n" + str(e.stdout or "")[-2000:] + str(e.stderr or "")[-2000:], pytrace=False)
    if r.returncode != 0:
        _state["dead"] = "%s ended with status %d" % (what, r.returncode)
        pytest.fail(_state["dead"] + "\n" + r.stdout[-2000:] + r.stderr[-3000:], pytrace=False)
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    os.remove(out)
    _state["runs"][key] = res
    return res


def arrays(res):
    return {k: v for k, v in res.items() if not k.startswith("__")}


def assert_same(got, want, what):
    """The same keys, dtypes and shapes, every array equal -> the number of arrays compared."""
    got, want = arrays(got), arrays(want)
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    bad = [k for k in want if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]
    for k in bad[:5]:
        at = np.nonzero(np.ravel(got[k] != want[k]))[0][:5] if got[k].shape == want[k].shape else []
        print("%s: %s differs: %s %s against %s %s, first at %s: %s against %s" % (
            what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape, list(at), np.ravel(got[k])[at].tolist(), np.ravel(want[k])[at].tolist()))
    assert not bad, "%s: %d of %d arrays differ: %s" % (what, len(bad), len(want), bad)
    return len(want)


def calls_of(res, which):
    """The calls a child made, checked against the literal list -> {call: blocks it received}."""
    names = [str(c) for c in res["__calls"]]
    want = [c for c in CALLS if which == "small" or c not in tour.SMALL_ONLY]
    assert sorted(names) == sorted(want) and names[:2] == want[:2], sorted(set(names) ^ set(want))
    assert {k.split(".")[0] for k in arrays(res)} == set(names)
    return dict(zip(names, (res["__blocks"][:, 1] - res["__blocks"][:, 0]).tolist()))


def test_the_list_of_calls_is_the_tour():
    assert CALLS == tour.call_names("small") and len(CALLS) == 55
    assert set(ALLOCATES_NOTHING) <= set(CALLS)


def test_plain_tour_equals_the_truth(work):
    got = child(work, "small", "forward")
    calls_of(got, "small")
    assert int(got["__byte"]) == -1 and not got["__blocks"].any() and not got["__bytes"].any()
    want = tour.expected_small()
    have = arrays(got)
    assert set(want) <= set(have), sorted(set(want) - set(have))
    bad = [k for k in want if have[k].shape != want[k].shape or not np.array_equal(have[k], want[k])]
    assert not bad, bad
    assert sorted(set(have) - set(want)) == sorted(NO_TRUTH_KEYS)
    print("plain tour: %d arrays of %d calls equal the truth, %d more have none" % (len(want), len(CALLS), len(NO_TRUTH_KEYS)))


@pytest.mark.parametrize("which", ["small", "seam"])
def test_filled_memory_changes_nothing(work, which):
    plain = child(work, which, "forward")
    filled = child(work, which, "forward", fill=255)
    assert int(filled["__byte"]) == 255 and int(plain["__byte"]) == -1
    n = assert_same(filled, plain, "filled " + which)
    got = calls_of(filled, which)
    dry = sorted(c for c, blocks in got.items() if blocks <= 0)
    assert dry == sorted(c for c in ALLOCATES_NOTHING if c in got), dry
    assert filled["__blocks"][-1, 1] > 0 and filled["__bytes"][-1, 1] > 0 and not plain["__blocks"].any()
    print("filled %s: %d arrays of %d calls equal, %d blocks and %d bytes filled" % (
        which, n, len(got), filled["__blocks"][-1, 1], filled["__bytes"][-1, 1]))


@pytest.mark.parametrize("order", ["reverse", "twice"])
@pytest.mark.parametrize("which", ["small", "seam"])
def test_call_order_changes_nothing(work, which, order):
    plain = child(work, which, "forward")
    other = child(work, which, order)
    n = assert_same(other, plain, "%s %s" % (order, which))
    print("%s %s: %d arrays of %d calls equal" % (order, which, n, len(calls_of(other, which))))


def test_filled_and_twice_together(work):
    plain = child(work, "seam", "forward")
    both = child(work, "seam", "twice", fill=255)
    assert int(both["__byte"]) == 255
    n = assert_same(both, plain, "filled twice seam")
    got = calls_of(both, "seam")
    assert sorted(c for c, blocks in got.items() if blocks <= 0) == sorted(c for c in ALLOCATES_NOTHING if c in got)
    print("filled twice seam: %d arrays of %d calls equal, %d blocks filled" % (n, len(got), both["__blocks"][-1, 1]))
