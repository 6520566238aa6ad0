"""-m gpu: the host choreography of fx_fasta_minimizers, in the manner of test_gpu_run_drivers.py: the entry is a fourth user
of the driver of the window-hit entries, so a call launches what fx_fasta_pwm_scan launches -- one count kernel, the scans
under k_search_scan (the run plan, the kept scan, the fix at slen, the three-component hit scan: 10, and one more for the
per-record counts), one emit kernel -- and counts-only launches no emit.  The exits it shares with them: a selection of empty
records, no row under a cap, a cap of 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, W = 5, 4
EMPTY = np.array([1], dtype=np.int64)


def _fasta():
    rng = np.random.default_rng(20)
    t = "".join(rng.choice(list("ACGT"), 700))
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
    b.prof_enable(1)
    return b


def _launches(b, call):
    b.prof_reset()
    out = call()
    return out, {k: n for k, (_, n) in b.prof_read().items()}


def _pwm_scan_launches(lib, b):
    mat = np.full((6, 4), -10, dtype=np.int32)
    _, k = _launches(b, lambda: b.fasta_pwm_scan(mat, lib.FX_SEARCH_PLUS | lib.FX_SEARCH_MINUS, -60, cap=10000))
    return k["k_search_scan"]


def test_minimizer_launches(lib, blob):
    from minimizer_truth import truth
    raw, t = _fasta()
    seqs = [t, "", "CGTAC", "cgtgcttgc" * 5]
    assert (raw.index(b">empty") - 1) // 256 - (raw.index(b"\n") + 1) // 256 + 1 >= 3       # the 256-byte runs of the first record
    scans = _pwm_scan_launches(lib, blob)
    for flags, canonical, order in ((lib.FX_MZ_CANONICAL, True, "hash"), (lib.FX_MZ_LEX, False, "lex")):
        rows, counts = truth(seqs, K, W, canonical, order)
        (n, hits, cnt), k = _launches(blob, lambda: blob.fasta_minimizers(K, W, flags, cap=10000))
        assert k == {"k_mz_count": 1, "k_search_scan": scans, "k_mz_emit": 1} and scans == 10
        assert n == len(rows) > 100 and cnt is None and [h.dtype for h in hits] == [np.int64, np.int64, np.uint8, np.uint64]
        assert list(zip(hits[0].tolist(), hits[1].tolist(), [chr(c) for c in hits[2].tolist()], hits[3].tolist())) == rows
        (n, hits, cnt), k = _launches(blob, lambda: blob.fasta_minimizers(K, W, flags, cap=0, counts=True))
        assert k == {"k_mz_count": 1, "k_search_scan": scans + 1}
        assert n == len(rows) and hits is None and (cnt == counts).all() and cnt[1].tolist() == [0, 0]


def test_exits(lib, blob):
    n, hits, cnt = blob.fasta_minimizers(K, W, lib.FX_MZ_CANONICAL, ids=EMPTY, cap=5, counts=True)
    assert n == 0 and hits is None and cnt.dtype == np.int64 and cnt.tolist() == [[0, 0]]
    n, hits, cnt = blob.fasta_minimizers(K, W, lib.FX_MZ_CANONICAL, ids=np.array([2], dtype=np.int64), cap=5)      # five letters: no window
    assert n == 0 and cnt is None and hits is not None and len(hits) == 4 and all(h.size == 0 for h in hits)
    total = blob.fasta_minimizers(K, W, lib.FX_MZ_CANONICAL, cap=10000)[0]
    with pytest.raises(lib.FxError) as e:
        blob.fasta_minimizers(K, W, lib.FX_MZ_CANONICAL, cap=0)
    assert e.value.code == lib.FX_ERANGE and e.value.n_hits == total
    assert str(e.value) == lib.lib().fx_last_error().decode() == "%d hits, more than the 0 asked for" % total
