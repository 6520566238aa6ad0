"""-m gpu: Fasta.search_all / search_counts (fx_fasta_search, csrc/fx_search.hpp) against a plain Python oracle over
fa[i].seq -- str.find from every position for exact patterns, character classes of the IUPAC subset rule for degenerate
ones -- on the fixtures, on generated files with every line layout the index accepts, and on a synthetic genome."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

BASES = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
         "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
        "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _revcomp_exact(p):
    from pyfastx_amd import _lib
    return _lib.revcomp_bytes(p.encode("latin-1")).decode("latin-1")


def _finds(s, q):
    out, j = [], s.find(q)
    while j >= 0:
        out.append(j)
        j = s.find(q, j + 1)
    return out


def _degenerate_regex(p):
    cls = []
    for c in p.upper():
        S = set(BASES[c])
        ok = "".join(t + t.lower() for t, ts in BASES.items() if set(ts) <= S)
        cls.append("[" + ok + "]")
    return re.compile("(?=" + "".join(cls) + ")")


def oracle(seqs, p, strand="both", degenerate=False):
    """[(record, start, stop, '+'/'-')] by (record, start), '+' first."""
    L = len(p)
    if degenerate:
        rp = "".join(COMP[c] for c in reversed(p.upper()))
        fwd, rev = _degenerate_regex(p), _degenerate_regex(rp)
        find = lambda s, rx: [m.start() for m in rx.finditer(s)]
    else:
        fwd, rev = p, _revcomp_exact(p)
        find = _finds
    rows = []
    for i, s in enumerate(seqs):
        if strand in ("+", "both"):
            rows += [(i, j, j + L, 0) for j in find(s, fwd)]
        if strand in ("-", "both"):
            rows += [(i, j, j + L, 1) for j in find(s, rev)]
    rows.sort()
    return [(i, a, b, "+-"[k]) for i, a, b, k in rows]


def got(h):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()]))


def check(fa, seqs, p, strand="both", degenerate=False):
    h = fa.search_all(p, strand=strand, degenerate=degenerate)
    assert h.ids.dtype == np.int64 and h.starts.dtype == np.int64 and h.stops.dtype == np.int64 and h.strands.dtype == np.uint8
    want = oracle(seqs, p, strand, degenerate)
    assert got(h) == want, (p, strand, degenerate)
    c = fa.search_counts(p, strand=strand, degenerate=degenerate)
    assert c.shape == (len(seqs), 2) and c.dtype == np.int64
    bc = np.zeros((len(seqs), 2), dtype=np.int64)
    np.add.at(bc, (h.ids, (h.strands == ord("-")).astype(np.int64)), 1)
    assert (c == bc).all()
    return h


@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


def _patterns_of(seqs, rng):
    """patterns cut from inside records: some inside a line, some across line ends (60-column fixture lines)."""
    ps = []
    for i in rng.choice(len(seqs), min(6, len(seqs)), replace=False):
        s = seqs[i]
        for L in (5, 12, 31, 40):
            if len(s) > L + 2:
                a = int(rng.integers(0, len(s) - L))
                ps.append(s[a:a + L])
        if len(s) > 80:
            ps.append(s[55:67])                          # the bases on both sides of the first line end
    return ps


@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
@pytest.mark.parametrize("upper", [False, True])
def test_fixture(fx, fixture_files, fn, upper):
    fa = fx.Fasta(fixture_files[fn], uppercase=upper)
    seqs = [fa[i].seq for i in range(len(fa))]
    rng = np.random.default_rng(5)
    for p in ["GAATTC", "gaattc", "A", "AT"] + _patterns_of(seqs, rng):
        check(fa, seqs, p)
    for p in ("GANTC", "RGATCY", "NNNNNNNNNNNN", "garyn"):
        check(fa, seqs, p, degenerate=True)
    check(fa, seqs, "GAATTC", strand="+")
    check(fa, seqs, "GANTC", strand="-", degenerate=True)
    # the same answers from an index reopened from its .fxi (the table installed from the file)
    del fa
    fa2 = fx.Fasta(fixture_files[fn], uppercase=upper)
    check(fa2, seqs, "GAATTC")
    check(fa2, seqs, "RGATCY", degenerate=True)


def test_sequence_search_agrees(fx, fixture_files):
    fa = fx.Fasta(fixture_files["test.fa"])
    seqs = [fa[i].seq for i in range(len(fa))]
    rng = np.random.default_rng(11)
    for p in ["GAATTC", "ACGT", "TTTT", "CAGCTG"] + _patterns_of(seqs, rng)[:8]:
        h = fa.search_all(p)
        for i in range(len(fa)):
            sel = h.ids == i
            plus = h.starts[sel & (h.strands == ord("+"))]
            minus = h.stops[sel & (h.strands == ord("-"))]
            assert fa[i].search(p) == (int(plus[0]) + 1 if plus.size else None), (p, i)
            assert fa[i].search(p, "-") == (int(minus[0]) if minus.size else None), (p, i)


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def _generated(tmp_path):
    rng = np.random.default_rng(2026)
    files = {}
    # irregular line lengths and blank lines inside records (norm = 0)
    recs = []
    for i in range(8):
        s = _rand(rng, int(rng.integers(50, 900)))
        lines, a = [], 0
        while a < len(s):
            k = int(rng.integers(1, 90))
            lines.append(s[a:a + k])
            a += k
            if rng.random() < 0.15:
                lines.append("")
        recs.append(">irr%d\n" % i + "\n".join(lines) + "\n")
    files["irregular"] = _write(tmp_path / "irregular.fa", "".join(recs))
    # CRLF, spaces inside sequence lines, soft-masked lower case
    recs = []
    for i in range(6):
        s = _rand(rng, int(rng.integers(100, 700)), "ACGTacgt")
        lines = [s[a:a + 60] for a in range(0, len(s), 60)]
        lines = [ln[:10] + " " + ln[10:] if j % 3 == 1 else ln for j, ln in enumerate(lines)]
        recs.append(">crlf%d desc\r\n" % i + "\r\n".join(lines) + "\r\n")
    files["crlf"] = _write(tmp_path / "crlf.fa", "".join(recs))
    # N runs, bytes that are no IUPAC letter, empty records, a record shorter than the pattern, an unterminated last line
    recs = [">n0\n" + "ACGTN" * 20 + "NNNNNNNNNNNNNNNNNNNN\n" + "GAA-TTC*GAATTC12RYKM\n", ">empty\n", ">short\nGA\n",
            ">mixed\n" + _rand(rng, 300, "ACGTNRYKM-*.") + "\n", ">empty2\n\n", ">last\nGAATTCAAAAGAATTC"]
    files["odd"] = _write(tmp_path / "odd.fa", "".join(recs))
    # a record far longer than one lane's run, patterns at the first and the last base of records, record junctions
    long = _rand(rng, 50_000)
    recs = [">long\n" + "\n".join(long[a:a + 70] for a in range(0, len(long), 70)) + "\n",
            ">edge1\nGAATTCACGTACGTACGATTTTGAATTC\n", ">edge2\nTTCGGGAAAAAAAAACCCGA\n", ">poly\nAAAA\n",
            ">edge3\n" + "C" * 300 + "\n"]
    files["long"] = _write(tmp_path / "long.fa", "".join(recs))
    return files


@pytest.mark.parametrize("upper", [False, True])
def test_generated_layouts(fx, tmp_path, upper):
    for name, path in _generated(tmp_path).items():
        fa = fx.Fasta(path, uppercase=upper)
        seqs = [fa[i].seq for i in range(len(fa))]
        rng = np.random.default_rng(len(name))
        pats = ["GAATTC", "gaattc", "A", "AA", "acg", "N", "-", "GA"] + _patterns_of(seqs, rng)
        long_recs = [s for s in seqs if len(s) >= 64]
        if long_recs:
            pats += [long_recs[0][:64], long_recs[-1][-64:], long_recs[0][100:164] if len(long_recs[0]) > 200 else long_recs[0][:33]]
        for p in pats:
            check(fa, seqs, p)
        for p in ("GANTC", "RGATCY", "N", "ACGTRYKMSWBDHVNU", "n" * 64):
            check(fa, seqs, p, degenerate=True)


def test_edges_junctions_overlaps(fx, tmp_path):
    fa = fx.Fasta(_generated(tmp_path)["long"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    # tail of edge1 + head of edge2: in the stream they are only a newline and a header apart -- no hit
    p = seqs[1][-4:] + seqs[2][:4]
    assert got(fa.search_all(p, strand="+")) == []
    h = fa.search_all("GAATTC", strand="+", ids=[names.index("edge1")])
    assert got(h) == [(1, 0, 6, "+"), (1, len(seqs[1]) - 6, len(seqs[1]), "+")]      # first and last base of the record
    h = fa.search_all("GAATTC", ids=[names.index("edge1")])                          # a palindrome: two rows per site
    assert [r[3] for r in got(h)] == ["+", "-", "+", "-"]
    h = fa.search_all("AA", strand="+", ids=["poly"])
    assert got(h) == [(3, 0, 2, "+"), (3, 1, 3, "+"), (3, 2, 4, "+")]                # AA in AAAA: 3 overlapping hits
    assert fa.search_counts("C" * 64, strand="+")[4].tolist() == [300 - 63, 0]


def test_limits(fx, fixture_files):
    fa = fx.Fasta(fixture_files["test.fa"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    full = fa.search_all("GAATTC")
    sel = [5, 0, 17, 5]
    h = fa.search_all("GAATTC", ids=sel)
    keep = np.isin(full.ids, [0, 5, 17])
    assert got(h) == got(type(full)(*(a[keep] for a in full)))
    assert got(fa.search_all("GAATTC", ids=[names[i] for i in sel])) == got(h)
    with pytest.raises(KeyError):
        fa.search_all("GAATTC", ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.search_all("GAATTC", ids=[len(fa)])
    n = full.ids.size
    assert n > 10
    assert got(fa.search_all("GAATTC", max_hits=n)) == got(full)
    with pytest.raises(ValueError, match=str(n)):
        fa.search_all("GAATTC", max_hits=n - 1)
    for bad in ("", "A" * 65, "GA TC"):
        with pytest.raises(ValueError):
            fa.search_all(bad)
    with pytest.raises(ValueError):
        fa.search_all("GAXTC", degenerate=True)
    with pytest.raises(ValueError):
        fa.search_counts("GAATTC", strand="x")
    assert fa.search_counts("A").sum() == sum(s.count("A") + s.count("T") for s in seqs)


def test_sharded_raises(fx, fixture_files, monkeypatch):
    """Byte-range shards (devices=[...]) and windows (out of core) carry no halo for a hit across a cut: refused.  The
    object is made to report itself sharded, as a multi-device or windowed Fasta does (Fasta._sharded)."""
    fa = fx.Fasta(fixture_files["test.fa"])
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa.search_all("GAATTC")
    with pytest.raises(NotImplementedError):
        fa.search_counts("GAATTC")


def _np_hits(flat, starts_of_rec, slen, p, degenerate):
    """(record, start) of every window of the flat sequence that matches p and lies inside one record."""
    L = len(p)
    N = flat.size - L + 1
    m = np.ones(N, dtype=bool)
    codes = {c: 0 for c in range(256)}
    bits = {"A": 1, "C": 2, "G": 4, "T": 8}
    for k, v in BASES.items():
        codes[ord(k)] = codes[ord(k.lower())] = sum(bits[b] for b in v)
    code = np.array([codes[c] for c in range(256)], dtype=np.uint8)
    for j, ch in enumerate(p):
        w = flat[j:j + N]
        if degenerate:
            S = code[ord(ch)]
            cw = code[w]
            m &= (cw != 0) & ((cw & ~S) == 0)
        else:
            m &= w == ord(ch)
    pos = np.nonzero(m)[0]
    rec = np.searchsorted(starts_of_rec, pos, side="right") - 1
    inside = pos - starts_of_rec[rec] + L <= slen[rec]
    return rec[inside], (pos - starts_of_rec[rec])[inside]


def test_synthetic_genome_200mbp(fx):
    import torch
    from pyfastx_amd import _lib, search, synth
    dev = torch.device("cuda:0")
    plan = synth.fasta_plan(total_bp=200_000_000)
    blob_t, flat_t, flat_start = synth.fasta_generate(plan, dev, keep_flat=True)
    b = _lib.Blob.from_device(blob_t.data_ptr(), int(plan["n_bytes"]), device=0, keepalive=blob_t)
    s = b.fasta_build()
    assert s.n_seq == len(plan["slen"])
    flat = flat_t.cpu().numpy()
    slen = plan["slen"]
    for p, deg in (("GAATTC", False), ("GANTC", True), ("ACGTRYNNNNRYACGT", True)):
        rp = search.iupac_revcomp(p) if deg else _revcomp_exact(p)
        fr, fs = _np_hits(flat, flat_start, slen, p, deg)
        rr, rs = _np_hits(flat, flat_start, slen, rp, deg)
        key = np.concatenate([fr * (1 << 40) + fs * 2, rr * (1 << 40) + rs * 2 + 1])
        key.sort()
        h = search.search_blob(b, p, "both", deg)
        mine = h.ids * (1 << 40) + h.starts * 2 + (h.strands == ord("-"))
        assert h.ids.size == key.size and (mine == key).all(), p
        assert (h.stops == h.starts + len(p)).all()
        c = search.count_blob(b, p, "both", deg)
        assert c[:, 0].tolist() == np.bincount(fr, minlength=len(slen)).tolist()
        assert c[:, 1].tolist() == np.bincount(rr, minlength=len(slen)).tolist()
    c = search.count_blob(b, "a", "+", False)                       # soft-masked bases, exact: lower case only
    assert c[:, 0].sum() == int((flat == ord("a")).sum())
    del b, blob_t, flat_t
