"""CPU: the truth of the tandem-repeat tests pinned on hand-written cases and checked against the definition on random
texts, the argument rules of pyfastx_amd/tandem.py, the TandemRepeats object, and the new entry's declaration -- nothing
here needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tandem_truth as T
from conftest import ROOT

TWO = (2,) * 8


def _code(word):
    v = 0
    for ch in word:
        v = v * 4 + "ACGT".index(ch)
    return v


# ------------------------------------------------------------------ the truth, on hand-written cases
def test_truth_smallest_period_only():
    assert T.repeats("ATATAT", TWO) == [(0, 6, 2, _code("AT"))]                # not period 4 (ATAT twice is too short anyway), not 6
    assert T.repeats("ATATATAT", TWO) == [(0, 8, 2, _code("AT"))]              # period 4 fits twice, its motif ATAT is AT twice
    assert T.repeats("AAAAAA", TWO) == [(0, 6, 1, 0)]                          # periods 2 and 3 fit, their motifs are A written over
    assert T.repeats("AAAAAAAA", TWO) == [(0, 8, 1, 0)]


def test_truth_partial_copy_and_invalid_letters():
    assert T.repeats("ACGACGACGAC", TWO) == [(0, 11, 3, _code("ACG"))]         # the trailing AC belongs to it
    assert T.repeats("ACACNACAC", TWO) == [(0, 4, 2, _code("AC")), (5, 9, 2, _code("AC"))]
    assert T.repeats("NNNNNN", TWO) == [] and T.repeats("RRRRYYYY--**", TWO) == []   # an invalid letter does not match itself
    assert T.repeats("", TWO) == [] and T.repeats("A", TWO) == []


def test_truth_folds_case():
    assert T.repeats("acACac", TWO) == [(0, 6, 2, _code("AC"))]
    assert T.repeats("gGgG", TWO) == [(0, 4, 1, 2)]


def test_truth_overlapping_periods():
    # ACACACA and AGAGAG share the A at 6: [0, 7) of AC and [6, 12) of AG
    assert T.repeats("ACACACAGAGAG", TWO) == [(0, 7, 2, _code("AC")), (6, 12, 2, _code("AG"))]
    # a period-1 stretch inside a period-3 one: both are reported
    assert T.repeats("CAACAACAAC", TWO) == [(1, 3, 1, 0), (4, 6, 1, 0), (7, 9, 1, 0), (0, 10, 3, _code("CAA"))]


def test_truth_thresholds():
    s = "G" + "ACT" * 5 + "G"                                                  # 15 letters of period 3 at [1, 16)
    assert T.repeats(s, (0, 0, 5)) == [(1, 16, 3, _code("ACT"))]
    assert T.repeats(s[:15] + "G", (0, 0, 5)) == []                            # one letter less: 14 < 3 * 5
    assert T.repeats(s, (0, 0, 6)) == []
    assert T.repeats(s, (0, 0, 2), min_len=15) == [(1, 16, 3, _code("ACT"))]
    assert T.repeats(s, (0, 0, 2), min_len=16) == []
    assert T.repeats(s, {3: 5}) == T.repeats(s, (0, 0, 5))
    assert T.repeats("ATATATAT", (0, 0, 0, 2)) == []                           # period 4 alone asked for: ATAT is not primitive
    assert T.repeats("ACGT" * 2, (0, 0, 0, 2)) == [(0, 8, 4, _code("ACGT"))]


def _periodic(c, a, b, p):
    return all(x is not None for x in c[a:b]) and all(c[j] == c[j - p] for j in range(a + p, b))


def _definition(seq, mc, min_len):
    """Every interval of the definition, by trying all (a, b, p) -- cubic, for short texts."""
    c, rows = T.codes(seq), []
    n = len(c)
    for p in range(1, 9):
        if not mc[p - 1]:
            continue
        for a in range(n):
            for b in range(a + max(2 * p, p * mc[p - 1], min_len, 1), n + 1):
                if not _periodic(c, a, b, p):
                    break
                if (a > 0 and _periodic(c, a - 1, b, p)) or (b < n and _periodic(c, a, b + 1, p)):
                    continue
                if any(p % q == 0 and _periodic(c, a, b, q) for q in range(1, p)):
                    continue
                m = 0
                for x in c[a:a + p]:
                    m = m * 4 + x
                rows.append((a, b, p, m))
    return sorted(rows, key=lambda r: (r[1], r[2]))


def test_truth_is_the_definition_on_random_texts():
    rng = np.random.default_rng(5)
    n_rows = 0
    for it in range(300):
        alphabet = ["AC", "ACGT", "ACN", "ACGTacgtNRY"][it % 4]
        s = "".join(rng.choice(list(alphabet), int(rng.integers(0, 70))))
        mc = T.min_copies_list([TWO, T.DEFAULT, (0, 0, 0, 2), (3, 0, 2, 0, 0, 2)][(it // 4) % 4])
        min_len = (0, 0, 6, 13)[(it // 16) % 4]
        got = T.repeats(s, mc, min_len)
        assert got == _definition(s, mc, min_len), (s, mc, min_len)
        n_rows += len(got)
    assert n_rows > 300                                                       # (not a vacuous comparison)


def test_canonical_against_brute_force():
    from pyfastx_amd import tandem
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for p in range(1, 5):
        table = tandem.canonical_table(p)
        assert table.dtype == np.uint32 and table.shape == (4 ** p,)
        for code in range(4 ** p):
            w = tandem.motif_string(code, p)
            assert _code(w) == code
            rc = "".join(comp[ch] for ch in reversed(w))
            want = min(_code(x[r:] + x[:r]) for x in (w, rc) for r in range(p))
            assert int(table[code]) == want == T.canonical(code, p), (w, p)
    assert tandem.motif_string(int(tandem.canonical_table(2)[_code("TG")]), 2) == "AC"
    assert tandem.motif_string(int(tandem.canonical_table(8)[_code("TTAGGGTT")]), 8) == "AAAACCCT"         # (TTTTAGGG read on the other strand)


# ------------------------------------------------------------------ argument rules
def test_min_copies_rules():
    from pyfastx_amd import tandem
    assert tandem.check_min_copies((12, 7, 5, 4, 4, 4)).tolist() == [12, 7, 5, 4, 4, 4]
    assert tandem.check_min_copies([0, 0, 0, 5]).tolist() == [0, 0, 0, 5]
    assert tandem.check_min_copies({2: 6, 5: 3}).tolist() == [0, 6, 0, 0, 3]
    assert tandem.check_min_copies((2,) * 8).tolist() == [2] * 8
    assert tandem.check_min_copies([3, 0, 0]).tolist() == [3]
    assert tandem.check_min_copies(np.array([2, 2])).dtype == np.int32
    for bad in ((), (2,) * 9, (1,), (5, 1), (-2,), (0, 0), {}, {0: 3}, {9: 3}, {2: 1}, {2: 0}, (2.5,), (True,), "12", 12, None, (1 << 31,)):
        with pytest.raises(ValueError):
            tandem.check_min_copies(bad)
    assert tandem.check_limits(0, 0) == (0, 0)
    for kw in (dict(min_len=-1), dict(min_len=1.5), dict(max_repeats=-1), dict(max_repeats=None)):
        with pytest.raises(ValueError):
            tandem.check_limits(**kw)


# ------------------------------------------------------------------ the result object
def _object():
    from pyfastx_amd import tandem
    #       record 2: (AC)5 at 3, (GT)3 at 1 closing earlier; record 0: (A)12 at 7, (AAG)4+1 at 0
    rows = [(2, 1, 7, 2, _code("GT")), (2, 3, 13, 2, _code("AC")), (0, 0, 13, 3, _code("AAG")), (0, 7, 19, 1, 0)]
    cols = list(zip(*rows))
    return tandem.TandemRepeats(np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.int64), np.array(cols[2], dtype=np.int64),
                                np.array(cols[3], dtype=np.uint8), np.array(cols[4], dtype=np.uint32), names=lambda i: "chr%d" % i)


def test_tandem_repeats_object(tmp_path):
    r = _object()
    assert len(r) == 4
    assert r.lengths.tolist() == [6, 10, 13, 12] and r.copies.tolist() == [3, 5, 4, 12]
    assert r.motifs == ["GT", "AC", "AAG", "A"]
    assert r.canonical_motifs.dtype == np.uint32
    assert [T.motif_string(c, p) for c, p in zip(r.canonical_motifs.tolist(), r.periods.tolist())] == ["AC", "AC", "AAG", "A"]
    assert r.counts_by_motif() == {"AC": 2, "AAG": 1, "A": 1}
    assert r.counts_by_motif(canonical=False) == {"GT": 1, "AC": 1, "AAG": 1, "A": 1}
    p = str(tmp_path / "ssr.bed")
    r.write_bed(p)
    assert open(p).read() == "chr2\t1\t7\t(GT)3\nchr2\t3\t13\t(AC)5\nchr0\t0\t13\t(AAG)4\nchr0\t7\t19\t(A)12\n"


def test_sorted_by_start():
    from pyfastx_amd import tandem
    # ordered by stop: the long period-3 stretch closes last although it starts first
    rows = [(5, 4, 6, 1, 0), (5, 7, 9, 1, 0), (5, 0, 10, 3, _code("CAA")), (1, 2, 9, 2, 1), (1, 2, 9, 4, 7)]
    cols = [np.array(c) for c in zip(*rows)]
    r = tandem.TandemRepeats(cols[0].astype(np.int64), cols[1].astype(np.int64), cols[2].astype(np.int64), cols[3].astype(np.uint8),
                             cols[4].astype(np.uint32))
    s = r.sorted_by_start()
    assert isinstance(s, tandem.TandemRepeats)
    got = list(zip(s.ids.tolist(), s.starts.tolist(), s.stops.tolist(), s.periods.tolist(), s.motif_codes.tolist()))
    assert got == [rows[2], rows[0], rows[1], rows[3], rows[4]]                # record 5 stays in front of record 1
    assert s.periods.dtype == np.uint8 and s.motif_codes.dtype == np.uint32
    e = tandem.TandemRepeats(*(np.zeros(0, dtype=d) for d in (np.int64, np.int64, np.int64, np.uint8, np.uint32)))
    assert len(e.sorted_by_start()) == 0 and e.counts_by_motif() == {} and e.motifs == [] and e.canonical_motifs.size == 0


# ------------------------------------------------------------------ the C entry
def test_entry_declared_exported_bound():
    from pyfastx_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxgpu.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bint\s+fx_fasta_tandem_repeats\s*\(", hdr)
    assert "fx_fasta_tandem_repeats" in _lib.SYMBOLS
    assert len(L.fx_fasta_tandem_repeats.argtypes) == 14
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_td_count", "k_td_scan", "k_td_close", "k_td_emit"):
        assert k in names


def test_entry_without_a_device_or_a_handle():
    """Without a device the entry answers FX_EDEVICE before it looks at an argument; with one, a null handle is FX_EINVAL."""
    from pyfastx_amd import _lib
    L = _lib.lib()
    want = _lib.FX_EDEVICE if L.fx_device_count() <= 0 else _lib.FX_EINVAL
    out = [C.c_void_p() for _ in range(5)]
    n, m = C.c_int64(0), C.c_int64(0)
    mc = (C.c_int32 * 8)(*TWO)
    assert L.fx_fasta_tandem_repeats(None, mc, 8, 0, None, 0, 10, *[C.byref(p) for p in out], C.byref(n), C.byref(m)) == want
    assert L.fx_fasta_tandem_repeats(None, None, 99, -1, None, -1, -1, None, None, None, None, None, None, None) == want
