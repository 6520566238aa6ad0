"""-m "not gpu": the argument rules of Fastq.kmer_hits / screen and Fasta.kmer_hits, KmerTable.from_strings against the
definition, the ratio conversion, the C entries on null pointers and without a device, and the self-check of
tests/kmer_screen_truth.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kmer_screen_truth
from conftest import ROOT
from kmer_table_truth import table_truth
from pyfastx_amd import kmer


def test_truth_self_check():
    kmer_screen_truth.self_check()


def test_argument_rules():
    t = kmer.KmerTable(3, False, np.array([6], dtype=np.int64), np.array([1], dtype=np.int64))
    assert kmer.check_screen_table(t) is t
    for bad in (None, [6], np.array([6]), "ACG", 6, {6}):
        with pytest.raises(TypeError):
            kmer.check_screen_table(bad)
    assert kmer.check_screen() == (1, (0, 0), False)
    assert kmer.check_screen(0, None, True) == (0, (0, 0), True)
    assert kmer.check_screen(np.int64(5), 0.5) == (5, (1, 2), False)
    for m in (True, False, 1.0, -1, "1", None):
        with pytest.raises(ValueError):
            kmer.check_screen(min_hits=m)
    for f in (-0.1, 1.001, 2, float("nan"), float("inf"), "half"):
        with pytest.raises(ValueError):
            kmer.check_screen(min_frac=f)


def test_ratio_conversion():
    """min_frac becomes the closest fraction with a denominator <= 1000, as qc.as_ratio makes it for select."""
    from pyfastx_amd import qc
    for x, want in ((0, (0, 1)), (1, (1, 1)), (0.5, (1, 2)), (0.25, (1, 4)), (1 / 3, (1, 3)), (0.1, (1, 10)), (0.999, (999, 1000)),
                    (np.float32(0.75), (3, 4)), (0.12345, qc.as_ratio(0.12345))):
        assert kmer.check_screen(1, x)[1] == want == qc.as_ratio(x), x
    num, den = kmer.check_screen(1, 0.7071)[1]
    assert 0 < num <= den <= qc.MAX_DENOMINATOR


def test_from_strings():
    seqs = ["ACGTACGTTTGACA", "acgtnACGTACCAGT", "AC", "", "NNNNNNNN", "GATTACAGATTACAGATTACAGATTACAGATTACA", b"TTGACAGG", "ACGT\x80ACGTA"]
    for k in (1, 3, 4, 8, 31):
        for canonical in (False, True):
            t = kmer.KmerTable.from_strings(seqs, k, canonical)
            codes, counts = table_truth(seqs, k, canonical)
            assert t.k == k and t.canonical == canonical and t.codes.dtype == np.int64 and t.counts.dtype == np.int64
            assert np.array_equal(t.codes, codes) and np.array_equal(t.counts, counts), (k, canonical)
            assert t.n_windows == counts.sum()
    # an even-k palindrome counts once per occurrence; its reverse-complement strand folds onto it
    t = kmer.KmerTable.from_strings(["ACGT", "TTACGTAA"], 4, canonical=True)
    assert t.count("ACGT") == 2 and np.array_equal(t.codes, table_truth(["ACGT", "TTACGTAA"], 4, True)[0])
    assert len(kmer.KmerTable.from_strings(["ACG"], 4)) == 0 and len(kmer.KmerTable.from_strings([], 4)) == 0
    one = kmer.KmerTable.from_strings("ACGTT", 4)
    assert one.strings() == ["ACGT", "CGTT"]
    for bad in (0, 32, 4.0, True):
        with pytest.raises(ValueError):
            kmer.KmerTable.from_strings(["ACGT"], bad)


def test_lds_key_limit_matches_the_kernels():
    src = open(os.path.join(ROOT, "pyfastx_amd", "csrc", "fx_kmer_screen.hpp")).read()
    log2 = int(re.search(r"KS_LDS_LOG2\s*=\s*(\d+)", src).group(1))
    assert kmer.SCREEN_LDS_KEYS == (1 << log2) // 2 == 4096       # load 0.5 of an image of 64 KiB


def test_declared_exported_bound():
    from pyfastx_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    for name, nargs in (("fx_kmer_set_create", 6), ("fx_kmer_set_free", 1), ("fx_kmer_set_contains", 4), ("fx_fastq_kmer_hits", 10),
                        ("fx_fastq_kmer_screen", 13), ("fx_fasta_kmer_hits", 8)):
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == nargs
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_ks_insert", "k_ks_contains", "k_ks_fastq", "k_ks_fasta", "k_ks_screen"):
        assert names.count(k) == 1, k
    for m in ("kmer_set", "fastq_kmer_hits", "fastq_kmer_screen", "fasta_kmer_hits"):
        assert callable(getattr(_lib.Blob, m))
    import pyfastx_amd
    for cls, ms in ((pyfastx_amd.Fastq, ("kmer_hits", "screen")), (pyfastx_amd.Fasta, ("kmer_hits",))):
        for m in ms:
            assert callable(getattr(cls, m))


def test_null_arguments():
    """A null handle, set or output pointer: FX_EINVAL and nothing touched, with or without a device."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)        # handle- or set-shaped: refused before it is looked at
    s = C.c_void_p(7)
    assert L.fx_kmer_set_create(None, 21, 0, None, 0, C.byref(s)) == _lib.FX_EINVAL and s.value == 7
    assert L.fx_kmer_set_create(fake, 21, 0, None, 0, None) == _lib.FX_EINVAL
    assert L.fx_kmer_set_free(None) == _lib.FX_OK
    out = np.zeros(1, dtype=np.uint8)
    assert L.fx_kmer_set_contains(None, None, 0, None) == _lib.FX_EINVAL
    assert L.fx_kmer_set_contains(None, np.zeros(1, dtype=np.int64).ctypes.data, 1, out.ctypes.data) == _lib.FX_EINVAL and out[0] == 0

    def hits(call, h, st, null=None, head=()):
        o = [C.c_void_p(7), C.c_void_p(7), C.c_int64(-5), C.c_int64(-5)]
        refs = [None if i == null else C.byref(x) for i, x in enumerate(o)]
        return call(h, st, None, 0, *head, *refs), [x.value for x in o]

    for call, head in ((L.fx_fastq_kmer_hits, (None, None)), (L.fx_fasta_kmer_hits, ())):
        assert hits(call, None, fake, head=head) == (_lib.FX_EINVAL, [7, 7, -5, -5])
        assert hits(call, fake, None, head=head) == (_lib.FX_EINVAL, [7, 7, -5, -5])
        for i in range(4):
            rc, vals = hits(call, fake, fake, null=i, head=head)
            assert rc == _lib.FX_EINVAL and all(v in (7, -5) for v in vals)
    p, n, bad = C.c_void_p(7), C.c_int64(-5), C.c_int64(-5)
    tail = (1, 0, 0, 0)
    assert L.fx_fastq_kmer_screen(None, fake, None, 0, None, None, *tail, C.byref(p), C.byref(n), C.byref(bad)) == _lib.FX_EINVAL
    assert L.fx_fastq_kmer_screen(fake, None, None, 0, None, None, *tail, C.byref(p), C.byref(n), C.byref(bad)) == _lib.FX_EINVAL
    assert L.fx_fastq_kmer_screen(fake, fake, None, 0, None, None, *tail, None, C.byref(n), C.byref(bad)) == _lib.FX_EINVAL
    assert L.fx_fastq_kmer_screen(fake, fake, None, 0, None, None, *tail, C.byref(p), None, C.byref(bad)) == _lib.FX_EINVAL
    assert L.fx_fastq_kmer_screen(fake, fake, None, 0, None, None, *tail, C.byref(p), C.byref(n), None) == _lib.FX_EINVAL
    assert (p.value, n.value, bad.value) == (7, -5, -5)


def test_no_cpu_fallback_without_gpu():
    """Without a device there is no handle to build a set through or to screen on: FX_EDEVICE, as tests/test_cabi.py sees it for
    the other entries.  With a device the entries are the subject of tests/test_gpu_kmer_screen.py."""
    from pyfastx_amd import _lib
    if _lib.lib().fx_device_count() > 0:
        return
    t = kmer.KmerTable.from_strings(["ACGTACGT"], 4)
    for raw, call in ((b"@r\nACGT\n+\nIIII\n", lambda b: kmer.fastq_hits_blob(b, 0, 1, t)),
                      (b"@r\nACGT\n+\nIIII\n", lambda b: kmer.fastq_screen_blob(b, 0, 1, t)),
                      (b">a\nACGT\n", lambda b: kmer.fasta_hits_blob(b, 0, t)),
                      (b">a\nACGT\n", lambda b: b.kmer_set(4, False, t.codes))):
        with pytest.raises(_lib.FxError) as e:
            call(_lib.Blob.from_bytes(raw))
        assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
    assert not t._sets
