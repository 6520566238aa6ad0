"""-m gpu: Fasta.low_complexity and Fastq.complexity (fx_fasta_low_complexity, fx_fastq_complexity, csrc/fx_dust.hpp) against
the plain Python truth of dust_truth.py over fa[i].seq / fq[i].seq: one set of records with planted repeats in every line
layout and on many phases of the 256-byte block, the seams of the carry, the selections, the cap, the window tuple, the soft
mask; reads of every length class; and the two calls in fresh processes on clean, filled and used device memory.  Every
comparison is exact integer equality."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import dust_truth as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOWS, THRESHOLDS, MIN_LENS = (4, 5, 8, 33, 63, 64), (1, 20, 65), (1, 50)
TIMEOUT = 60                                                # ends a child that hangs, nothing else (test_gpu_clean_memory.py's floor)


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _rows(r):
    return list(zip(r.ids.tolist(), r.starts.tolist(), r.stops.tolist()))


_truth = {}


def truth(seq, window, threshold, min_len=1):
    """The truth's rows of one text, computed once per (text, window, threshold): min_len only filters them."""
    key = (seq, window, threshold)
    if key not in _truth:
        _truth[key] = T.mask(seq, window, threshold, 1)
    return [(a, b) for a, b in _truth[key] if b - a >= min_len]


def truth_rows(seqs, window, threshold, min_len=1, ids=None):
    return [(i, a, b) for i in (range(len(seqs)) if ids is None else ids) for a, b in truth(seqs[i], window, threshold, min_len)]


def build(records, width, eol="\n", first_header=0, space_in_line=False):
    """records: [(name, seq)], width 0: unwrapped -> (bytes, [raw offset of every letter of every record]).  first_header: the
    letters the first record's name is padded with, which moves every record through the phases of the 256-byte block."""
    out, where = bytearray(), []
    for i, (name, s) in enumerate(records):
        hdr = ">" + name
        if i == 0:
            hdr += "d" * first_header
        out += hdr.encode() + eol.encode()
        at = []
        lines = [s[k:k + width] for k in range(0, len(s), width)] if width else ([s] if s else [])
        for j, ln in enumerate(lines):
            for k, ch in enumerate(ln):
                if space_in_line and j % 3 == 1 and k == 3 and len(ln) > 4:
                    out += b" "
                at.append(len(out))
                out += ch.encode()
            out += eol.encode()
        where.append(at)
    return bytes(out), where


# ------------------------------------------------------------------ a. one set of records, every layout
PLANTS = ("A", "T", "g", "AC", "ACG", "GATTACA", "ca", "TTTTTTC")


def _planted_records():
    """Four records of about 6 kB: random stretches of 140..320 letters (a few N and lower-case letters among them) between
    planted repeats of 7..1000 letters; the first begins with a repeat, the last ends with one."""
    rng = np.random.default_rng(20260)
    lens = [7, 8, 9, 12, 16, 20, 23, 30, 40, 64, 65, 100, 130, 300, 520, 1000]
    recs = []
    for r in range(4):
        parts = []
        if r == 0:
            parts.append("A" * 31)
        for k in range(15):
            parts.append(_rand(rng, int(rng.integers(140, 321)), "ACGT" * 12 + "Nacgt"))
            unit = PLANTS[int(rng.integers(0, len(PLANTS)))]
            n = lens[(5 * r + 3 * k) % len(lens)]
            parts.append((unit * (n // len(unit) + 1))[:n])
        parts.append(_rand(rng, 200) if r != 3 else "T" * 40)
        recs.append(("rec%d" % r, "".join(parts)))
    return recs


RECORDS = _planted_records()
SEQS = [s for _, s in RECORDS]
LAYOUTS = [("w1", 1, "\n", 0, False), ("w7", 7, "\n", 1, False), ("w60", 60, "\n", 15, False), ("w255", 255, "\n", 16, False),
           ("w256", 256, "\n", 255, False), ("w257", 257, "\n", 37, False), ("unwrapped", 0, "\n", 100, False),
           ("w1crlf", 1, "\r\n", 64, False), ("w7crlf", 7, "\r\n", 128, False), ("w60crlf", 60, "\r\n", 200, False),
           ("w255crlf", 255, "\r\n", 240, False), ("w256crlf", 256, "\r\n", 17, False), ("w257crlf", 257, "\r\n", 31, False),
           ("unwrappedcrlf", 0, "\r\n", 63, False), ("w60blank", 60, "\n", 254, True), ("w60gz", 60, "\n", 129, False)]


def test_the_phases_cover_the_block():
    assert {0, 1, 15, 16, 255} <= {c[3] for c in LAYOUTS} and len({c[3] for c in LAYOUTS}) == len(LAYOUTS)
    assert 20000 <= sum(map(len, SEQS)) <= 25000             # files of 20..50 kB (one letter per line: up to three bytes a letter)


@pytest.mark.parametrize("name", [c[0] for c in LAYOUTS])
def test_planted_layouts(fx, tmp_path, name):
    _, width, eol, pad, space = next(c for c in LAYOUTS if c[0] == name)
    raw, where = build(RECORDS, width, eol, pad, space)
    path = str(tmp_path / (name + ".fa"))
    if name.endswith("gz"):
        path += ".gz"
        with gzip.open(path, "wb") as f:
            f.write(raw)
    else:
        with open(path, "wb") as f:
            f.write(raw)
    fa = fx.Fasta(path)
    assert [fa[i].seq for i in range(len(fa))] == SEQS
    # what the file must hold for the case to mean something, from the truth and the raw offsets of the letters
    for window in (64, 33):
        rows = truth_rows(SEQS, window, 20)
        blocks = [(where[i][a] // 256, where[i][b - 1] // 256) for i, a, b in rows]
        assert len(rows) >= 20, (window, len(rows))
        assert any(y > x for x, y in blocks), "no row crosses a 256-byte boundary"
        assert any(y - x >= 2 for x, y in blocks), "no row spans more than two runs"
        assert any(a == 0 for _, a, _ in rows), "no row starts at 0"
        assert any(b == len(SEQS[i]) for i, _, b in rows), "no row ends at slen"
    for window in WINDOWS:
        for threshold in THRESHOLDS:
            for min_len in MIN_LENS:
                got = _rows(fa.low_complexity(window, threshold, min_len))
                assert got == truth_rows(SEQS, window, threshold, min_len), (window, threshold, min_len)


# ------------------------------------------------------------------ b. the seams
def _touching():
    """Two homopolymers g letters apart whose masked intervals are one row at g and two rows at g + 1, found with the truth."""
    rng = np.random.default_rng(5)
    filler = _rand(rng, 400)
    for g in range(60, 300):
        one, two = "A" * 30 + filler[:g] + "C" * 30, "A" * 30 + filler[:g + 1] + "C" * 30
        r1, r2 = T.mask(one, 64, 20), T.mask(two, 64, 20)
        if len(r1) == 1 and len(r2) == 2 and r2[1][0] - r2[0][1] == 1:
            # alone, the two stretches give intervals that touch exactly: [.., x) and [x, ..)
            left, right = T.mask(one[:30 + g] + "N" * 30, 64, 20), T.mask("N" * 30 + one[30:], 64, 20)
            assert len(left) == len(right) == 1 and left[0][1] == right[0][0], (g, left, right)
            return one, two
    raise AssertionError("no touching pair found")


def _trap_record():
    """One unwrapped record behind a header that puts its first letter at raw offset 256 - 56: homopolymers of 7..12 letters
    that start exactly 2 W - 2 = 126 letters in front of a 256-byte boundary, and again exactly W - 1 = 63 in front of one."""
    rng = np.random.default_rng(99)
    body0 = 200
    s = list(_rand(rng, 256 * 14))
    spots = []
    for k, n in enumerate(range(7, 13)):
        for j, back in enumerate((126, 63)):
            edge = 256 * (2 * k + j + 2)                      # raw offset of a block boundary
            at = edge - back - body0
            s[at:at + n] = "ACGT"[k % 4] * n
            spots.append((at, n, edge))
    return "".join(s), body0, spots


def _seam_records():
    rng = np.random.default_rng(314)
    trap, body0, spots = _trap_record()
    one, two = _touching()
    x = "AC" * 40 + _rand(rng, 150) + "T" * 25 + _rand(rng, 90, "ACGTN") + "ACG" * 20
    recs = [("trap", trap), ("touch1", one), ("touch2", two),
            ("endsA", _rand(rng, 300) + "AAAA"), ("beginsA", "AAAA" + _rand(rng, 300)), ("fourA1", "AAAA"), ("fourA2", "AAAA"), ("threeA", "AAA")]
    recs += [("len%d" % n, "A" * n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 32, 33, 34, 62, 63, 64, 65)]
    recs += [("rnd%d" % n, _rand(rng, n)) for n in (3, 4, 5, 63, 64, 65)]
    recs += [("n_inside", "AC" * 100 + "N" * 300 + "AC" * 100), ("only_n", "N" * 500), ("upper", x.upper()), ("lower", x.lower()),
             ("tail", _rand(rng, 100) + "G" * 40)]
    return recs, body0, spots


def test_seams(fx, tmp_path):
    recs, body0, spots = _seam_records()
    raw, where = build(recs, 0, "\n", body0 - len(">trap\n"))
    assert where[0][0] == body0 and all(where[0][at] + back == edge for (at, n, edge), back in zip(spots, (126, 63) * 6)) and len(spots) == 12
    path = str(tmp_path / "seams.fa")
    with open(path, "wb") as f:
        f.write(raw)
    fa = fx.Fasta(path)
    seqs = [s for _, s in recs]
    names = [n for n, _ in recs]
    assert [fa[i].seq for i in range(len(fa))] == seqs
    at = {n: i for i, n in enumerate(names)}
    # what the truth says about the seams themselves
    assert truth(seqs[at["trap"]], 64, 20) == []             # the warm-up trap: no row at W = 64
    assert len(truth(seqs[at["touch1"]], 64, 20)) == 1 and len(truth(seqs[at["touch2"]], 64, 20)) == 2
    for n in ("endsA", "beginsA", "fourA1", "fourA2", "threeA", "only_n", "len0", "len1", "len2", "len3", "len6"):
        assert truth(seqs[at[n]], 64, 20) == [], n
    assert truth(seqs[at["len7"]], 64, 20) == [(0, 7)] and truth(seqs[at["len65"]], 64, 20) == [(0, 65)]
    inside = truth(seqs[at["n_inside"]], 64, 20)             # the repeat on both sides, nothing in the middle of the 300 N
    assert len(inside) == 2 and inside[0][0] == 0 and inside[0][1] < 300 and inside[1][0] > 400 and inside[1][1] == 700
    assert truth(seqs[at["upper"]], 64, 20) == truth(seqs[at["lower"]], 64, 20) != []
    for window in WINDOWS:
        for threshold in THRESHOLDS:
            for min_len in MIN_LENS:
                got = _rows(fa.low_complexity(window, threshold, min_len))
                assert got == truth_rows(seqs, window, threshold, min_len), (window, threshold, min_len)
    got = _rows(fa.low_complexity())
    assert [(a, b) for i, a, b in got if i == at["upper"]] == [(a, b) for i, a, b in got if i == at["lower"]] != []


# ------------------------------------------------------------------ c. selections, the cap, the window tuple, the soft mask
@pytest.fixture(scope="module")
def planted(fx, tmp_path_factory):
    raw, _ = build(RECORDS, 60)
    path = str(tmp_path_factory.mktemp("dust") / "planted.fa")
    with open(path, "wb") as f:
        f.write(raw)
    return fx.Fasta(path)


def test_ids(planted):
    fa = planted
    want = truth_rows(SEQS, 64, 20)
    assert _rows(fa.low_complexity(ids=[1, 3])) == [r for r in want if r[0] in (1, 3)]
    assert _rows(fa.low_complexity(ids=[3, 2, 0])) == [r for r in want if r[0] != 1]        # class_runs' rule: ascending, distinct
    assert _rows(fa.low_complexity(ids=["rec2", "rec0", "rec2"])) == [r for r in want if r[0] in (0, 2)]
    assert _rows(fa.low_complexity(33, 20, 50, ids=[2])) == truth_rows(SEQS, 33, 20, 50, ids=[2])
    assert len(fa.low_complexity(ids=[])) == 0
    with pytest.raises(KeyError):
        fa.low_complexity(ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.low_complexity(ids=[len(fa)])
    r = fa.low_complexity()
    assert r.lengths.tolist() == [b - a for _, a, b in want] and r.ids.dtype == r.starts.dtype == r.stops.dtype == np.int64


def test_cap(planted):
    from pyfastx_amd import _lib
    fa = planted
    total = len(truth_rows(SEQS, 64, 20))
    assert len(fa.low_complexity(max_rows=total)) == total
    with pytest.raises(ValueError, match="%d intervals, more than max_rows=%d" % (total, total - 1)):
        fa.low_complexity(max_rows=total - 1)
    both = len([r for s in SEQS for r in T.mask_multi(s, (8, 64), 20)])
    assert len(fa.low_complexity((8, 64), max_rows=both)) == both
    with pytest.raises(ValueError, match="more than max_rows=%d" % (both - 1)):
        fa.low_complexity((8, 64), max_rows=both - 1)
    with pytest.raises(_lib.FxError) as e:
        fa._search_blob().fasta_low_complexity(64, 20, 1, None, cap=total - 1)
    assert e.value.code == _lib.FX_ERANGE and e.value.n_rows == total
    for bad in (dict(window=3), dict(window=65), dict(threshold=0), dict(threshold=1001), dict(min_len=0)):
        with pytest.raises(_lib.FxError) as e:
            fa._search_blob().fasta_low_complexity(**{**dict(window=64, threshold=20, min_len=1), **bad})
        assert e.value.code == _lib.FX_EINVAL, bad


def test_window_tuple(planted):
    fa = planted
    for windows, min_len in (((8, 64), 1), ((4, 33, 63), 50), ((64,), 1), ((5, 8, 33, 64), 1)):
        want = [(i, a, b) for i, s in enumerate(SEQS) for a, b in T.mask_multi(s, windows, 20, min_len)]
        assert _rows(fa.low_complexity(windows, 20, min_len)) == want, (windows, min_len)
    assert _rows(fa.low_complexity((8, 64))) != _rows(fa.low_complexity(64))


def test_soft_mask(fx, tmp_path):
    recs = [(n, s.upper()) for n, s in RECORDS]
    raw, _ = build(recs, 60)
    path = str(tmp_path / "upper.fa")
    with open(path, "wb") as f:
        f.write(raw)
    fa = fx.Fasta(path)
    buf, offs = fa.records(mask=fa.low_complexity(), mask_mode="soft", width=0)
    buf = bytes(buf)
    for i, (_, s) in enumerate(recs):
        body = buf[offs[i]:offs[i + 1]].split(b"\n")[1].decode()
        want = list(s)
        for a, b in truth(s, 64, 20):
            want[a:b] = s[a:b].lower()
        assert body == "".join(want) and body != s, i


# ------------------------------------------------------------------ d. FASTQ
def _reads():
    rng = np.random.default_rng(8)
    lens = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 150, 151, 1000]
    seqs = []
    for rep in range(20):
        for L in lens:
            kind = (rep + L) % 5
            if kind == 0:
                s = _rand(rng, L)
            elif kind == 1:
                s = "ACGTNacgt"[rep % 9] * L
            elif kind == 2:
                s = ("AC" * (L // 2 + 1))[:L]
            elif kind == 3:
                s = _rand(rng, L, "ACGT" * 5 + "Nacgt")
            else:
                s = (_rand(rng, L // 2) + "a" * L)[:L]
            seqs.append(s)
    seqs.insert(100, "A" * 70000)                            # above 65 535 letters, dust_sum above 2^31
    seqs.append(_rand(rng, 70000, "ACGTN"))
    return seqs


@pytest.fixture(scope="module")
def reads(fx, tmp_path_factory):
    seqs = _reads()
    p = tmp_path_factory.mktemp("dustq") / "reads.fq"
    p.write_bytes(b"".join(b"@r%d\n" % i + s.encode() + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs)))
    fq = fx.Fastq(str(p))
    assert len(fq) == len(seqs) and all(fq[i].seq == seqs[i] for i in range(0, len(seqs), 7))
    return fq, seqs, [T.read_columns(s) for s in seqs]


def _check_columns(c, want):
    assert list(c) == ["length", "n_triplets", "dust_sum", "n_diff", "dust", "complexity"]
    assert (c["length"].dtype, c["n_triplets"].dtype, c["dust_sum"].dtype, c["n_diff"].dtype) == (np.int64, np.int32, np.int64, np.int32)
    for j, k in enumerate(("length", "n_triplets", "dust_sum", "n_diff")):
        assert c[k].tolist() == [w[j] for w in want], k
    assert c["dust"].tolist() == [T.dust(w[2], w[1]) for w in want]
    assert c["complexity"].tolist() == [T.complexity(w[3], w[0]) for w in want]


def test_fastq_columns(reads):
    fq, seqs, want = reads
    c = fq.complexity()
    _check_columns(c, want)
    assert want[100] == (70000, 69998, 69998 * 69997 // 2, 0) and c["dust_sum"][100] > 2 ** 31
    # the filter the columns are for.  Over a whole read random letters score about 10 * (n / 2) / 64 = 0.08 n (12 at 150
    # letters), a read of one or two letters 10 * (n / 2) / 2 = 2.5 n or more: a cut at 50 parts the reads of 150
    low = set(np.nonzero(c["dust"] > 50)[0].tolist())
    longest = lambda s: max(len(r) for ch in "ACGT" for r in s.upper().split(ch))          # (the longest stretch without one of the letters)
    plain = [i for i, s in enumerate(seqs) if len(s) == 150 and len(set(s.upper())) <= 2 and "N" not in s.upper()]
    mixed = [i for i, s in enumerate(seqs) if len(s) == 150 and len(set(s.upper())) >= 4 and longest(s) < 40]
    assert 100 in low and len(plain) >= 8 and len(mixed) >= 8 and set(plain) <= low and not set(mixed) & low


def test_fastq_ids_and_intervals(reads):
    fq, seqs, want = reads
    rng = np.random.default_rng(4)
    ids = np.concatenate([rng.integers(0, len(seqs), 300), [100, 100, 0, len(seqs) - 1]]).astype(np.int64)
    _check_columns(fq.complexity(ids=ids), [want[i] for i in ids])
    iv = fq.trim(clip_front=3, clip_tail=2)
    a, b = np.asarray(iv["start"]), np.asarray(iv["end"])
    _check_columns(fq.complexity(start=a, end=b), [T.read_columns(s[x:y]) for s, x, y in zip(seqs, a.tolist(), b.tolist())])
    iv = fq.trim(ids=ids, clip_front=17, clip_tail=16)
    a, b = np.asarray(iv["start"]), np.asarray(iv["end"])
    _check_columns(fq.complexity(ids=ids, start=a, end=b), [T.read_columns(seqs[i][x:y]) for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())])
    a = np.array([int(rng.integers(0, len(seqs[i]) + 1)) for i in ids], dtype=np.int64)
    b = np.array([int(rng.integers(x, len(seqs[i]) + 1)) for i, x in zip(ids, a)], dtype=np.int64)
    _check_columns(fq.complexity(ids=ids, start=a, end=b), [T.read_columns(seqs[i][x:y]) for i, x, y in zip(ids.tolist(), a.tolist(), b.tolist())])
    assert all(len(v) == 0 for v in fq.complexity(ids=[]).values())
    n = len(seqs)
    for s, e in (([0] * (n - 1) + [5], [0] * (n - 1) + [4]), ([0] * n, [0] * 10 + [151] + [0] * (n - 11)), ([-1] + [0] * (n - 1), [0] * n)):
        with pytest.raises(IndexError, match="lies outside its read"):
            fq.complexity(start=s, end=e)
    with pytest.raises(IndexError):
        fq.complexity(ids=[n])
    with pytest.raises(ValueError):
        fq.complexity(start=[0] * n)


def test_fastq_against_the_kmer_counts(reads):
    """n_triplets and dust_sum are sum c and sum c (c - 1) / 2 of the 3-mer spectrum of the read: nothing of dust_truth here."""
    fq, seqs, _ = reads
    c = fq.complexity()
    for i in list(range(0, len(seqs), 9)) + [100, len(seqs) - 1]:
        k = np.asarray(fq.kmer_counts(3, ids=[i])).astype(np.int64)
        assert int(k.sum()) == int(c["n_triplets"][i]) and int((k * (k - 1) // 2).sum()) == int(c["dust_sum"][i]), i


# ------------------------------------------------------------------ e. clean, filled and used device memory
def _child(work, mode, fill=None):
    out = os.path.join(work, "%s_%s.npz" % (mode, "plain" if fill is None else fill))
    env = {k: v for k, v in os.environ.items() if k != "FX_DEBUG_FILL"}
    if fill is not None:
        env["FX_DEBUG_FILL"] = str(fill)
    r = subprocess.run([sys.executable, os.path.join(HERE, "dust_child.py"), work, mode, out], env=env, capture_output=True, text=True,
                       timeout=TIMEOUT)
    assert r.returncode == 0, (mode, fill, r.stdout[-2000:], r.stderr[-3000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_memory_hygiene(tmp_path):
    import dust_child
    work = str(tmp_path)
    seqs, reads_ = dust_child.write_inputs(work)
    plain, filled, behind = _child(work, "plain"), _child(work, "plain", fill=255), _child(work, "behind")
    assert int(plain["fill_byte"]) == -1 and int(filled["fill_byte"]) == 255 and int(filled["fill_blocks"]) > 0
    rows = truth_rows(seqs, 64, 20)
    want = {"ids": [r[0] for r in rows], "starts": [r[1] for r in rows], "stops": [r[2] for r in rows]}
    cols = [T.read_columns(s) for s in reads_]
    for j, k in enumerate(("length", "n_triplets", "dust_sum", "n_diff")):
        want[k] = [c[j] for c in cols]
    assert len(rows) >= 5
    for res in (plain, filled, behind):
        for k, v in want.items():
            assert res[k].tolist() == v, k
