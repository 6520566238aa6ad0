"""-m gpu: the host choreography of the passes over the 256-byte runs of the resident FASTA stream -- the window-hit entries
(fx_fasta_search, fx_fasta_search_approx, fx_fasta_pwm_scan, fx_fasta_pwm_best) and the interval entries (fx_fasta_class_runs,
fx_fasta_tandem_repeats, fx_fasta_orfs).  What is pinned here is what the entries share and no result test looks at: which
kernels a call launches and under which timing id (prof_read), and the early exits -- a selection of empty records, no hit
under a cap, a cap of 0 -- with the totals and the messages they leave.

The launch counts are read off the host code: a scan (sscan) is three launches under its id (chunk sums, top, apply); the run
plan is one scan; the hit entries add the kept scan, the fix at slen and the three-component hit scan (10, and one more for
the per-record counts); the interval entries add the carry scan, the list and the closes scan (10; the class runs time their
close under the scan id as well: 11)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MOTIF, RMOTIF = b"GATTAC", b"GTAATC"
ORF = "ATG" + "GCT" * 10 + "TAA"
SET_A = bytes(2 if i == ord("A") >> 3 else 0 for i in range(32))       # the byte set {A}
STOPS = (1 << 48) | (1 << 50) | (1 << 56)                              # TAA TAG TGA by codon index 16 c0 + 4 c1 + c2
ATG = 1 << 14
EMPTY = np.array([1], dtype=np.int64)


def _fasta():
    """-> (bytes of the file, the text of the first record).  The background has no A, so nothing but what is planted is a
    poly-A stretch, a START, a stop on either strand or a copy of the motif."""
    rng = np.random.default_rng(20)
    t = list("".join(rng.choice(list("CGT"), 700)))
    for at, word in ((100, "A" * 12), (250, ORF), (400, MOTIF.decode()), (600, RMOTIF.decode())):
        t[at:at + len(word)] = word
    t = "".join(t)
    out = ">big\n" + "".join(t[k:k + 60] + "\n" for k in range(0, 700, 60))
    out += ">empty\n" + ">five\nCGTAC\n" + ">lower\n" + "cgtgcttgc" * 5 + "\n"
    return out.encode(), t


@pytest.fixture(scope="module")
def lib():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def blob(lib):
    raw, _ = _fasta()
    b = lib.Blob.from_bytes(raw, device=0)
    assert b.fasta_build().n_seq == 4
    b.fasta_rank_build()
    b.prof_enable(1)
    return b


def _launches(b, call):
    b.prof_reset()
    out = call()
    return out, {k: n for k, (_, n) in b.prof_read().items()}


def _pwm():
    """10 for the motif's letter, -10 for every other: 60 is the motif alone"""
    mat = np.full((6, 4), -10, dtype=np.int32)
    for j, c in enumerate(MOTIF.decode()):
        mat[j, "ACGT".index(c)] = 10
    return mat


def _count(t, w):
    return sum(t.startswith(w, k) for k in range(len(t)))


def test_text_is_what_the_cases_need():
    raw, t = _fasta()
    assert (raw.index(b">empty") - 1) // 256 - (raw.index(b"\n") + 1) // 256 + 1 >= 3       # the 256-byte runs of the first record
    assert _count(t, MOTIF.decode()) == 1 and _count(t, RMOTIF.decode()) == 1 and "A" * 12 in t and "A" * 13 not in t


# ------------------------------------------------------------------ the launches of every call
def test_search_launches(lib, blob):
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    (n, hits, cnt), k = _launches(blob, lambda: blob.fasta_search(MOTIF, RMOTIF, both, cap=100))
    assert k == {"k_search_count": 1, "k_search_scan": 10, "k_search_emit": 1}
    assert n == 2 and cnt is None and [h.dtype for h in hits] == [np.int64, np.int64, np.uint8]
    assert sorted(zip(*[h.tolist() for h in hits])) == [(0, 400, ord("+")), (0, 600, ord("-"))]
    (n, hits, cnt), k = _launches(blob, lambda: blob.fasta_search(MOTIF, RMOTIF, both, cap=0, counts=True))
    assert k == {"k_search_count": 1, "k_search_scan": 11}
    assert n == 2 and hits is None and cnt.tolist() == [[1, 1], [0, 0], [0, 0], [0, 0]]


def test_search_approx_launches(lib, blob):
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    (n, hits, _), k = _launches(blob, lambda: blob.fasta_search_approx(MOTIF, RMOTIF, both, 1, cap=1000))
    assert k == {"k_asearch_count": 1, "k_search_scan": 10, "k_asearch_emit": 1}
    assert n >= 2 and [h.dtype for h in hits] == [np.int64, np.int64, np.uint8, np.uint8] and all(h.size == n for h in hits)
    rows = list(zip(*[h.tolist() for h in hits]))
    assert (0, 400, ord("+"), 0) in rows and (0, 600, ord("-"), 0) in rows


def test_pwm_launches(lib, blob):
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    (n, hits, _), k = _launches(blob, lambda: blob.fasta_pwm_scan(_pwm(), both, 60, cap=100))
    assert k == {"k_pwm_count": 1, "k_search_scan": 10, "k_pwm_emit": 1}
    assert n == 2 and [h.dtype for h in hits] == [np.int64, np.int64, np.uint8, np.int32]
    assert sorted(zip(*[h.tolist() for h in hits])) == [(0, 400, ord("+"), 60), (0, 600, ord("-"), 60)]
    (scores, starts), k = _launches(blob, lambda: blob.fasta_pwm_best(_pwm(), both))
    assert k == {"k_pwm_count": 1, "k_search_scan": 6, "k_pwm_best": 1}
    assert scores[0].tolist() == [60, 60] and starts[0].tolist() == [400, 600]
    assert scores[1].tolist() == [np.iinfo(np.int32).min] * 2 and starts[1].tolist() == [-1, -1]


def test_interval_launches(blob):
    (rec, a, z), k = _launches(blob, lambda: blob.fasta_class_runs(SET_A, min_len=12))
    assert k == {"k_an_runs_count": 1, "k_an_runs_scan": 11, "k_an_runs_emit": 1}
    assert (rec.tolist(), a.tolist(), z.tolist()) == ([0], [100], [112])
    out, k = _launches(blob, lambda: blob.fasta_tandem_repeats([12]))
    assert k == {"k_td_count": 1, "k_td_scan": 10, "k_td_close": 1, "k_td_emit": 1}
    assert [c.tolist() for c in out[:4]] == [[0], [100], [112], [1]] and [c.dtype for c in out] == [np.int64] * 3 + [np.uint8, np.uint32]
    out, k = _launches(blob, lambda: blob.fasta_orfs(STOPS, ATG, mode=1, strands=3, min_len=30))
    assert k == {"k_orf_count": 1, "k_orf_scan": 10, "k_orf_close": 1, "k_orf_emit": 1}
    assert [c.tolist() for c in out[:3]] == [[0], [250], [250 + len(ORF) - 3]] and [c.dtype for c in out] == [np.int64] * 3 + [np.int8, np.uint8]


# ------------------------------------------------------------------ the exits
def test_only_empty_records(lib, blob):
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    for call in (lambda: blob.fasta_search(MOTIF, RMOTIF, both, ids=EMPTY, cap=5, counts=True),
                 lambda: blob.fasta_search_approx(MOTIF, RMOTIF, both, 1, ids=EMPTY, cap=5, counts=True),
                 lambda: blob.fasta_pwm_scan(_pwm(), both, 60, ids=EMPTY, cap=5, counts=True)):
        n, hits, cnt = call()
        assert n == 0 and hits is None and cnt.dtype == np.int64 and cnt.tolist() == [[0, 0]]
    for call, dtypes in ((lambda: blob.fasta_class_runs(SET_A, ids=EMPTY), [np.int64] * 3),
                         (lambda: blob.fasta_tandem_repeats([12], ids=EMPTY), [np.int64] * 3 + [np.uint8, np.uint32]),
                         (lambda: blob.fasta_orfs(STOPS, ATG, ids=EMPTY), [np.int64] * 3 + [np.int8, np.uint8])):
        out = call()
        assert [c.dtype for c in out] == dtypes and all(c.size == 0 for c in out)


def test_no_hit_under_a_cap(lib, blob):
    for call, width in ((lambda: blob.fasta_search(b"ACACAC", None, lib.FX_SEARCH_PLUS, cap=5), 3),
                        (lambda: blob.fasta_search_approx(b"ACACACACAC", None, lib.FX_SEARCH_PLUS, 1, cap=5), 4),
                        (lambda: blob.fasta_pwm_scan(_pwm(), lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS, 61, cap=5), 4)):
        n, hits, cnt = call()
        assert n == 0 and cnt is None and hits is not None and len(hits) == width and all(h.size == 0 for h in hits)


def test_cap_of_zero(lib, blob):
    both = lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS
    n_approx = blob.fasta_search_approx(MOTIF, RMOTIF, both, 1, cap=1000)[0]
    for call, total in ((lambda: blob.fasta_search(MOTIF, RMOTIF, both, cap=0), 2),
                        (lambda: blob.fasta_search_approx(MOTIF, RMOTIF, both, 1, cap=0), n_approx),
                        (lambda: blob.fasta_pwm_scan(_pwm(), both, 60, cap=0), 2)):
        with pytest.raises(lib.FxError) as e:
            call()
        assert e.value.code == lib.FX_ERANGE and e.value.n_hits == total
        assert str(e.value) == lib.lib().fx_last_error().decode() == "%d hits, more than the 0 asked for" % total
    for call, noun in ((lambda: blob.fasta_class_runs(SET_A, min_len=12, cap=0), "runs"),
                       (lambda: blob.fasta_tandem_repeats([12], cap=0), "repeats"),
                       (lambda: blob.fasta_orfs(STOPS, ATG, mode=1, strands=3, min_len=30, cap=0), "open reading frames")):
        with pytest.raises(lib.FxError) as e:
            call()
        assert e.value.code == lib.FX_ERANGE and e.value.n_rows == 1
        assert str(e.value) == lib.lib().fx_last_error().decode() == "1 %s, more than the 0 asked for" % noun
