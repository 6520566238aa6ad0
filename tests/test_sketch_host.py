"""CPU: the argument rules of the sketch entries, max_key = ceil(4^k / scaled), the two forms of the model against each other,
compare_model against plain set arithmetic, the formulas that follow from (shared, total), and the entries without a device."""
import ctypes as C

import numpy as np
import pytest

from sketch_truth import compare_model, cut, fasta_sets, fastq_set, key_set, key_set_np


def _rand(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


def test_check_args():
    from pyfastx_amd import sketch
    assert sketch.check_args(21, 1000, None) == (21, 1000, 0, -(-4 ** 21 // 1000))
    assert sketch.check_args(21, None, 500) == (21, None, 500, 4 ** 21)
    assert sketch.check_args(np.int64(4), np.int64(3), np.int64(7)) == (4, 3, 7, 86)
    assert sketch.check_args(1, None, 0) == (1, None, 0, 4)
    for bad in ((21, None, None), (0, 10, None), (32, 10, None), (21, 0, None), (21, -5, 10), (21, None, -1), (21, 10, -1), (21.0, 10, None), ("21", 10, None),
                (21, 10.5, None), (21, None, 3.0), (True, 10, None)):
        with pytest.raises(ValueError):
            sketch.check_args(*bad)


@pytest.mark.parametrize("k", [1, 16, 31])
@pytest.mark.parametrize("scaled", [1, 3, 10 ** 9])
def test_max_key_is_the_scaled_rule(k, scaled):
    """key < max_key exactly when key * scaled < 4^k, in Python ints: at the threshold, around it and at the ends of the range."""
    from pyfastx_amd import sketch
    m = sketch.max_key_of(k, scaled)
    assert 1 <= m <= 4 ** k and m == sketch.check_args(k, scaled)[3]
    rng = np.random.default_rng(k * scaled % 1000)
    probes = {0, 4 ** k - 1, m - 1, m, max(m - 2, 0), min(m + 1, 4 ** k - 1)} | {int(x) for x in rng.integers(0, 4 ** k, 200, dtype=np.uint64)}
    for key in probes:
        if 0 <= key < 4 ** k:
            assert (key < m) == (key * scaled < 4 ** k), (k, scaled, key)
    assert sketch.max_key_of(k, None) == 4 ** k


def test_model_forms_agree():
    rng = np.random.default_rng(5)
    texts = [_rand(rng, 300), _rand(rng, 257, "ACGTacgt"), _rand(rng, 400, "ACGTNRYKM-*."), "ACGT" * 20, "A" * 40, "ACG", "", "N" * 50,
             _rand(rng, 120) + "N" + _rand(rng, 120), "U" + _rand(rng, 60)]
    for k in (1, 2, 4, 15, 16, 21, 31):
        for canonical in (True, False):
            for t in texts:
                assert sorted(key_set(t, k, canonical)) == key_set_np(t, k, canonical).tolist(), (k, canonical, t[:20])
    sets = fasta_sets(texts, 4, True, 4 ** 4, 0)
    assert fasta_sets(texts, 4, True, 4 ** 4, 0, form=key_set_np) == sets and sets[5] == [] and sets[6] == [] and sets[7] == []
    assert fasta_sets(texts, 4, True, 100, 5, ids=[3, 0, 3], pooled=True) == [cut(set(sets[0]) | set(sets[3]), 100, 5)]
    reads = texts[:4]
    assert fastq_set(reads, 4, False, 4 ** 4, 0) == sorted(set().union(*[key_set(r, 4, False) for r in reads]))
    assert fastq_set(reads, 4, False, 200, 3, ids=[1, 1, 0], start=[0, 5, 10], end=[50, 5, 14]) == \
        cut(key_set(reads[1][:50], 4, False) | key_set(reads[0][10:14], 4, False), 200, 3)


def test_compare_model_against_set_arithmetic():
    rng = np.random.default_rng(9)
    for _ in range(200):
        na, nb, top = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(1, 80))
        A = sorted(set(rng.integers(0, top, na).tolist()))
        B = sorted(set(rng.integers(0, top, nb).tolist()))
        for limit in (0, 1, 5, 1000):
            for max_key in (0, top // 2 + 1):
                a = [x for x in A if not max_key or x < max_key]
                b = [x for x in B if not max_key or x < max_key]
                U = sorted(set(a) | set(b))
                UL = U[:limit] if limit else U
                assert compare_model(A, B, limit, max_key) == (len([x for x in UL if x in set(a) and x in set(b)]), len(UL))
    assert compare_model([], [], 0) == (0, 0) and compare_model([1, 2], [], 1) == (0, 1) and compare_model([3], [3], 5) == (1, 1)


def test_formulas():
    from pyfastx_amd import sketch
    shared = np.array([[0, 5, 10], [3, 0, 0]], dtype=np.int64)
    total = np.array([[10, 10, 10], [4, 0, 7]], dtype=np.int64)
    j = sketch.jaccard_of(shared, total)
    assert j.tolist() == [[0.0, 0.5, 1.0], [0.75, 0.0, 0.0]]
    c = sketch.containment_of(shared, [10, 0])
    assert c.tolist() == [[0.0, 0.5, 1.0], [0.0, 0.0, 0.0]]
    d = sketch.mash_distance_of(j, 21)
    assert d[0, 0] == 1.0 and d[0, 2] == 0.0 and d[1, 1] == 1.0
    assert d[0, 1] == pytest.approx(-np.log(2 * 0.5 / 1.5) / 21) and d[1, 0] == pytest.approx(-np.log(1.5 / 1.75) / 21)
    assert sketch.mash_distance_of(np.array([1e-30]), 1).tolist() == [1.0]                # clipped
    a = sketch.ani_of(c, 21)
    assert a[0, 2] == 1.0 and a[0, 0] == 0.0 and a[0, 1] == pytest.approx(0.5 ** (1 / 21))


def test_entries_without_a_device_and_null_arguments():
    """What the numbers alone decide is refused first, with or without a device; fx_sketch_from_host, the one entry that takes no
    handle and no sketch, answers FX_EDEVICE without one (a handle or a sketch cannot exist there: Blob.from_bytes fails)."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    s, nr, bad = C.c_void_p(), C.c_int(7), C.c_int64(3)
    mk = 4 ** 21
    for args in ((0, 1, mk, 0, 0), (32, 1, mk, 0, 0), (21, 4, mk, 0, 0), (21, 1, 0, 0, 0), (21, 1, 4 ** 21 + 1, 0, 0), (21, 1, mk, -1, 0), (21, 1, mk, 0, 65),
                 (21, 1, mk, 0, -1)):
        k, fl, m, size, over = args
        assert L.fx_fasta_sketch(None, k, fl, None, 0, m, size, over, C.byref(s), C.byref(nr)) == _lib.FX_EINVAL, args
        assert L.fx_fastq_sketch(None, k, fl, None, 0, None, None, m, size, over, C.byref(s), C.byref(nr), C.byref(bad)) == _lib.FX_EINVAL, args
    assert L.fx_fasta_sketch(None, 21, 1, None, 0, mk, 0, 0, C.byref(s), C.byref(nr)) == _lib.FX_EINVAL and s.value is None and nr.value == 0
    assert L.fx_sketch_info(None, None, None, None, None, None, None) == _lib.FX_EINVAL
    assert L.fx_sketch_read(None, C.byref(s), C.byref(s)) == _lib.FX_EINVAL
    assert L.fx_sketch_compare(None, None, None, 0, None, 0, 0, 0, 10, C.byref(s), C.byref(s)) == _lib.FX_EINVAL
    assert L.fx_sketch_free(None) == _lib.FX_OK
    off = np.zeros(2, dtype=np.int64)
    assert L.fx_sketch_from_host(0, 0, 1, 4, 0, 1, off.ctypes.data, None, C.byref(s)) == _lib.FX_EINVAL
    assert L.fx_sketch_from_host(0, 21, 1, mk, 0, 1, None, None, C.byref(s)) == _lib.FX_EINVAL
    if L.fx_device_count() > 0:
        return
    assert L.fx_sketch_from_host(0, 21, 1, mk, 0, 1, off.ctypes.data, None, C.byref(s)) == _lib.FX_EDEVICE and s.value is None
    from pyfastx_amd import sketch
    with pytest.raises(_lib.FxError) as e:
        sketch.Sketch.from_hashes([[1, 2, 3]], 21, scaled=1)
    assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(_lib.FxError) as e:
        _lib.Blob.from_bytes(b">a\nACGT\n").fasta_sketch(2, 1, max_key=16)
    assert e.value.code == _lib.FX_EDEVICE
