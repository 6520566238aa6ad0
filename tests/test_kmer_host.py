"""CPU: the definition tests/kmer_truth.py on hand-written sequences and against an independent brute force, the argument
rules of pyfastx_amd/kmer.py, and the two C entries of the k-mer extension (declared, exported, no CPU fallback)."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT
from kmer_truth import fold_canonical, flat_counts, kmer_counts_truth, kmer_profile_truth, revcomp_code


def idx(kmer):
    return sum("ACGT".index(c) * 4 ** (len(kmer) - 1 - j) for j, c in enumerate(kmer))


def spectrum(k, **named):
    out = np.zeros(4 ** k, dtype=np.int64)
    for name, n in named.items():
        out[idx(name)] = n
    return out


# ------------------------------------------------------------------ the definition, by hand
def test_worked_example():
    assert (idx("AC"), idx("CG"), idx("GT")) == (1, 6, 11)
    assert kmer_counts_truth(["ACGTNACG"], 2).tolist() == spectrum(2, AC=2, CG=2, GT=1).tolist()
    c = kmer_counts_truth(["ACGTNACG"], 2, canonical=True)
    assert c[1] == 3 and c[6] == 2 and c[11] == 0 and c.sum() == 5        # AC, AC and GT under AC; CG is its own reverse complement


def test_by_hand():
    # a palindrome at even k counts once
    assert kmer_counts_truth(["ACGT"], 4, canonical=True).tolist() == spectrum(4, ACGT=1).tolist()
    assert kmer_counts_truth(["AATT", "AATT"], 4, canonical=True)[idx("AATT")] == 2
    # a record shorter than k, an empty record
    assert kmer_counts_truth(["ACG", "", "AC"], 4).sum() == 0
    # lower case counts as upper case
    assert kmer_counts_truth(["acGt"], 2).tolist() == spectrum(2, AC=1, CG=1, GT=1).tolist()
    # an invalid byte at the first and at the last position
    assert kmer_counts_truth(["NACGT"], 3).tolist() == spectrum(3, ACG=1, CGT=1).tolist()
    assert kmer_counts_truth(["ACGTN"], 3).tolist() == spectrum(3, ACG=1, CGT=1).tolist()
    assert kmer_counts_truth(["ACG-", "*ACG", "AC1G", "ACU"], 3).tolist() == spectrum(3, ACG=2).tolist()
    # k = 1 is a letter count
    s = "ACGTTTGGGGnnNacgtRY-"
    assert kmer_counts_truth([s], 1).tolist() == [s.upper().count(c) for c in "ACGT"]
    assert kmer_counts_truth([s], 1, canonical=True).tolist() == [s.upper().count("A") + s.upper().count("T"),
                                                                  s.upper().count("C") + s.upper().count("G"), 0, 0]
    # windows never span two sequences; the rows of the profile add up to the whole
    assert kmer_counts_truth(["AC", "GT"], 2).tolist() == spectrum(2, AC=1, GT=1).tolist()
    p = kmer_profile_truth(["ACGT", "", "TTTT"], 2)
    assert p.shape == (3, 16) and p[1].sum() == 0 and p[2][idx("TT")] == 3
    assert (p.sum(axis=0) == kmer_counts_truth(["ACGT", "", "TTTT"], 2)).all()
    # the first base is the most significant digit
    assert idx("CAAA") == 64 and kmer_counts_truth(["CAAA"], 4)[64] == 1
    assert revcomp_code(idx("AACG"), 4) == idx("CGTT")


def _brute(seqs, k, canonical):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    d = Counter()
    for s in seqs:
        s = s.upper()
        for j in range(len(s) - k + 1):
            w = s[j:j + k]
            if set(w) <= set("ACGT"):
                if canonical:
                    w = min(w, "".join(comp[c] for c in reversed(w)))
                d[w] += 1
    out = np.zeros(4 ** k, dtype=np.int64)
    for w, n in d.items():
        out[idx(w)] = n
    return out


@pytest.mark.parametrize("k", range(1, 9))
def test_truth_against_brute_force(k):
    rng = np.random.default_rng(100 + k)
    letters = np.array(list("ACGTNacgtn-"))
    seqs = ["".join(rng.choice(letters, int(n), p=[.2, .2, .2, .2, .02, .04, .04, .04, .04, .01, .01])) for n in rng.integers(0, 400, 12)]
    for canonical in (False, True):
        want = _brute(seqs, k, canonical)
        assert (kmer_counts_truth(seqs, k, canonical) == want).all()
        assert (kmer_profile_truth(seqs, k, canonical).sum(axis=0) == want).all()
    plain = kmer_counts_truth(seqs, k)
    assert (fold_canonical(plain, k) == kmer_counts_truth(seqs, k, True)).all()
    # the chunked form the GPU tests use on large inputs
    flat = "".join(seqs)
    starts = np.cumsum([0] + [len(s) for s in seqs[:-1]])
    lens = np.array([len(s) for s in seqs])
    for canonical in (False, True):
        assert (flat_counts(flat, starts, lens, k, canonical, chunk=97) == kmer_counts_truth(seqs, k, canonical)).all()


# ------------------------------------------------------------------ argument rules
def test_check_k():
    from pyfastx_amd import kmer
    assert kmer.check_k(1) == 1 and kmer.check_k(13) == 13 and kmer.check_k(np.int64(7)) == 7
    for bad in (0, 14, -1, True, False, 4.0, "4", None, [4]):
        with pytest.raises(ValueError):
            kmer.check_k(bad)
    assert kmer.check_k(6, kmer.MAX_PROFILE_K) == 6
    with pytest.raises(ValueError):
        kmer.check_k(7, kmer.MAX_PROFILE_K)
    assert kmer.kmer_string(idx("GATTACA"), 7) == "GATTACA"
    assert kmer.revcomp_code(np.array([idx("AACG")]), 4).tolist() == [idx("CGTT")]


def test_profile_max_bytes():
    from pyfastx_amd import kmer
    assert kmer.check_profile(4, 10, 10 * 256 * 8) == 4
    with pytest.raises(ValueError, match=str(10 * 256 * 8)):
        kmer.check_profile(4, 10, 10 * 256 * 8 - 1)
    with pytest.raises(ValueError):
        kmer.check_profile(7, 1, 1 << 30)
    with pytest.raises(ValueError):
        kmer.check_profile(True, 1, 1 << 30)
    with pytest.raises(ValueError):
        kmer.check_profile(4, 1, -1)
    assert kmer.check_profile(6, 0, 0) == 6                               # an empty selection takes no bytes


class _NoBlob:
    """Stands where the resident blob would: the argument rules must have raised before it is touched."""
    def __getattr__(self, name):
        raise AssertionError("the blob was reached")


def test_fastq_argument_rules():
    from pyfastx_amd import kmer
    nb = _NoBlob()
    for bad in (0, 14, 2.0, True):
        with pytest.raises(ValueError):
            kmer.fastq_counts_blob(nb, 5, bad)
    for bad in ([5], [-1], [0, 9]):
        with pytest.raises(IndexError, match="index out of range"):
            kmer.fastq_counts_blob(nb, 5, 4, ids=bad)
    with pytest.raises(ValueError):
        kmer.fastq_counts_blob(nb, 5, 4, ids=[[0, 1]])
    for s, e in ((None, [1] * 5), ([0] * 5, None), ([0, 0], [1, 1])):
        with pytest.raises(ValueError):
            kmer.fastq_counts_blob(nb, 5, 4, start=s, end=e)
    with pytest.raises(ValueError):
        kmer.fastq_counts_blob(nb, 5, 4, ids=[1, 2], start=[0] * 5, end=[1] * 5)
    for bad in (0, 14, 2.0, True):
        with pytest.raises(ValueError):
            kmer.fasta_counts_blob(nb, bad)
    with pytest.raises(ValueError):
        kmer.fasta_profile_blob(nb, 7, False, None, 3, 1 << 30)
    with pytest.raises(ValueError):
        kmer.fasta_profile_blob(nb, 6, False, None, 3, 100)


# ------------------------------------------------------------------ the C entries
def _declared():
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", hdr))


def test_declared_and_exported():
    from pyfastx_amd import _lib
    L = _lib.lib()
    for name in ("fx_fasta_kmers", "fx_fastq_kmers"):
        assert name in _declared() and name in _lib.SYMBOLS and hasattr(L, name)
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_kmer_fasta", "k_kmer_scan", "k_kmer_fix", "k_kmer_fastq"):
        assert names.count(k) == 1, k
    assert _lib.FX_KMER_CANONICAL == 1 and "FX_KMER_CANONICAL = 1" in open(os.path.join(ROOT, "include", "fxgpu.h")).read()


def test_null_arguments():
    """A null handle or output pointer: FX_EINVAL and nothing touched, with or without a device."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    p, rows, bad = C.c_void_p(), C.c_int64(7), C.c_int64(-5)
    assert L.fx_fasta_kmers(None, 4, 0, None, 0, 0, C.byref(p), C.byref(rows), C.byref(bad)) == _lib.FX_EINVAL
    assert p.value is None and rows.value == 7 and bad.value == -5
    assert L.fx_fastq_kmers(None, 4, 0, None, 0, None, None, C.byref(p), C.byref(bad)) == _lib.FX_EINVAL
    assert p.value is None and bad.value == -5


def test_no_cpu_fallback_without_gpu():
    """Without a device there is no handle to count on: Blob.from_bytes already fails with FX_EDEVICE, so the two entries are
    never reached -- all this shows is that the wrappers offer no way round the handle.  What covers the entries themselves
    on the host is test_null_arguments and test_declared_and_exported."""
    from pyfastx_amd import _lib
    if _lib.lib().fx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.FxError) as e:
        _lib.Blob.from_bytes(b">a\nACGT\n").fasta_kmers(2)
    assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(_lib.FxError) as e:
        _lib.Blob.from_bytes(b"@r\nACGT\n+\nIIII\n").fastq_kmers(2)
    assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
