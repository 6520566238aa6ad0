"""-m gpu: Fasta.search_edit / search_edit_counts (fx_fasta_search_edit, csrc/fx_search_edit.hpp) against the dynamic
programme of search_edit_truth.py over fa[i].seq: edits = 0 against search_all, the rows of search_approx among the ends,
every line layout the index accepts, both word widths, sites across the edges of the 256-byte runs (the L + k warm-up), the
start pass at its limits, runs full of ends, the cut at slen, row offsets across a scan chunk, selections, counts, limits and
the binding.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest

from conftest import DATA
from search_edit_truth import strand_rows, truth

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 12, 31, 32, 33, 40, 63, 64)
BUDGETS = (0, 1, 2, 3, 8)
REPORTS = ("all", "best")


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1") if isinstance(text, str) else text)
    return str(path)


def _rand(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes().decode()


def _revcomp(p):
    return p[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def _edit(rng, p, n_sub, n_ins, n_del):
    """p with n_sub letters replaced by another base, n_del letters taken out and n_ins letters put in (inside, never at an end)."""
    q = list(p)
    for j in rng.choice(len(q), min(n_sub, len(q)), replace=False):
        q[j] = str(rng.choice([b for b in "ACGT" if b != q[j].upper()]))
    for _ in range(n_del):
        if len(q) > 2:
            del q[int(rng.integers(1, len(q) - 1))]
    for _ in range(n_ins):
        j = int(rng.integers(1, len(q))) if len(q) > 1 else 0
        q.insert(j, str(rng.choice([b for b in "ACGT" if b not in (q[j - 1].upper(), q[min(j, len(q) - 1)].upper())])))
    return "".join(q)


def _planted(rng, n, sites, alphabet="ACGT"):
    """A random text of n letters with the given (position, string) sites written over it."""
    t = list(_rand(rng, n, alphabet))
    for a, s in sites:
        assert 0 <= a and a + len(s) <= n
        t[a:a + len(s)] = s
    return "".join(t)


def got(h):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], h.edits.tolist()))


def check(fa, seqs, p, k, strand="both", degenerate=False, reports=REPORTS, seen=None, rev=None):
    """search_edit against the truth and search_edit_counts against the rows, for every report; seen[k] collects the edits met.
    -> the rows of the last report."""
    for report in reports:
        h = fa.search_edit(p, k, strand=strand, degenerate=degenerate, report=report)
        assert h.ids.dtype == np.int64 and h.starts.dtype == np.int64 and h.stops.dtype == np.int64
        assert h.strands.dtype == np.uint8 and h.edits.dtype == np.uint8
        want = truth(seqs, p, k, strand, degenerate, report, rev=rev)
        assert got(h) == want, (p, k, strand, degenerate, report)
        c = fa.search_edit_counts(p, k, strand=strand, degenerate=degenerate, report=report)
        assert c.shape == (len(seqs), 2) and c.dtype == np.int64
        bc = np.zeros((len(seqs), 2), dtype=np.int64)
        np.add.at(bc, (h.ids, (h.strands == ord("-")).astype(np.int64)), 1)
        assert (c == bc).all(), (p, k, report)
        if seen is not None:
            seen.setdefault(k, set()).update(h.edits.tolist())
    return want


@pytest.fixture()
def fixture_files(tmp_path):
    out = {}
    for fn in ("test.fa", "test.fa.gz"):
        shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
        out[fn] = str(tmp_path / fn)
    return out


# ------------------------------------------------------------------ edits = 0 is search_all
@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
@pytest.mark.parametrize("upper", [False, True])
def test_no_edits_equals_search_all(fx, fixture_files, fn, upper):
    fa = fx.Fasta(fixture_files[fn], uppercase=upper)
    s = fa[3].seq
    cases = [(p, False) for p in ("GAATTC", "gaattc", "A", "AT", s[55:67], s[10:41], s[20:60], s[5:69])]
    cases += [(p, True) for p in ("GANTC", "RGATCY", "NNNNNNNNNNNN", "garyn")]
    for p, deg in cases:
        a, e = fa.search_edit(p, 0, degenerate=deg, report="all"), fa.search_all(p, degenerate=deg)
        assert got(a) == [r + (0,) for r in zip(e.ids.tolist(), e.starts.tolist(), e.stops.tolist(), [chr(c) for c in e.strands.tolist()])], p
        assert (fa.search_edit_counts(p, 0, degenerate=deg, report="all") == fa.search_counts(p, degenerate=deg)).all()
    assert fa.search_edit("GAATTC", 0, report="all").ids.size > 10
    for strand in "+-":
        a, e = fa.search_edit("GANTC", 0, strand=strand, degenerate=True, report="all"), fa.search_all("GANTC", strand=strand, degenerate=True)
        assert (a.ids == e.ids).all() and (a.starts == e.starts).all() and (a.strands == e.strands).all() and not a.edits.any()


# ------------------------------------------------------------------ every substitution hit is an end
def test_substitution_hits_are_ends(fx, fixture_files):
    fa = fx.Fasta(fixture_files["test.fa"])
    s = fa[3].seq
    rng = np.random.default_rng(8)
    n = 0
    for p, d, deg in (("GAATTC", 1, False), (_edit(rng, s[100:131], 2, 0, 0), 3, False), (_edit(rng, s[40:80], 3, 0, 0), 4, False),
                      ("RGATCY", 2, True), (s[7:19], 2, False)):
        a, e = fa.search_approx(p, d, degenerate=deg), fa.search_edit(p, d, degenerate=deg, report="all")
        ends = dict(zip(zip(e.ids.tolist(), e.stops.tolist(), e.strands.tolist()), e.edits.tolist()))
        for key, mis in zip(zip(a.ids.tolist(), a.stops.tolist(), a.strands.tolist()), a.mismatches.tolist()):
            assert key in ends and ends[key] <= mis, (p, key)
        n += a.ids.size
    assert n > 50


# ------------------------------------------------------------------ line layouts
def _layout(name):
    rng = np.random.default_rng(2027)
    if name == "irregular":                   # irregular line lengths and blank lines inside records; records start mid-block
        recs = []
        for i in range(8):
            s = _rand(rng, int(rng.integers(70, 900)))
            lines, a = [], 0
            while a < len(s):
                k = int(rng.integers(1, 90))
                lines.append(s[a:a + k])
                a += k
                if rng.random() < 0.15:
                    lines.append("")
            recs.append(">irr%d\n" % i + "\n".join(lines) + "\n")
        return "".join(recs)
    if name == "crlf":                        # CRLF, spaces inside sequence lines, soft-masked lower case
        recs = []
        for i in range(6):
            s = _rand(rng, int(rng.integers(100, 700)), "ACGTacgt")
            lines = [s[a:a + 60] for a in range(0, len(s), 60)]
            lines = [ln[:10] + " " + ln[10:] if j % 3 == 1 else ln for j, ln in enumerate(lines)]
            recs.append(">crlf%d desc\r\n" % i + "\r\n".join(lines) + "\r\n")
        return "".join(recs)
    if name == "odd":                         # N runs, bytes that are no IUPAC letter, empty records, records shorter than L - k and of
        #                                       exactly L - k, L and L + k letters, an unterminated last line
        sizes = sorted({n for L in LENGTHS for k in BUDGETS if k <= L - 1 for n in (L - k - 1, L - k, L, L + k) if n >= 1})
        return "".join([">n0\n" + "ACGTN" * 20 + "NNNNNNNNNNNNNNNNNNNN\n" + "GAA-TTC*GAATTC12RYKM\n", ">empty\n", ">short\nGA\n",
                        ">mixed\n" + _rand(rng, 300, "ACGTNRYKM-*.") + "\n", ">empty2\n\n"] +
                       [">size%d\n%s\n" % (n, _rand(rng, n)) for n in sizes] + [">last\nGAATTCAAAAGAATTC"])
    assert name == "long"                     # a record far longer than one lane's run: sites straddle many block edges
    long = _rand(rng, 50_000)
    return "".join([">long\n" + "\n".join(long[a:a + 70] for a in range(0, len(long), 70)) + "\n", ">edge1\nGAATTCACGTACGTACGATTTTGAATTC\n",
                    ">poly\nAAAA\n", ">edge3\n" + "C" * 300 + "\n"])


def _split(rng, k):
    """k edits as (substitutions, insertions, deletions), at random"""
    cut = np.sort(rng.integers(0, k + 1, 2))
    return int(cut[0]), int(cut[1] - cut[0]), int(k - cut[1])


@pytest.mark.parametrize("name,upper", [("irregular", False), ("crlf", False), ("crlf", True), ("odd", False), ("long", False)])
def test_layouts(fx, tmp_path, name, upper):
    fa = fx.Fasta(_write(tmp_path / (name + ".fa"), _layout(name)), uppercase=upper)
    seqs = [fa[i].seq for i in range(len(fa))]
    rng = np.random.default_rng(len(name))
    from pyfastx_amd import _lib
    seen, turn, strands = {}, 0, ("both", "+", "-")
    fewer = {}
    for L in LENGTHS:
        src = [s for s in seqs if len(s) >= L + 8]
        for k in (k for k in BUDGETS if k <= L - 1):
            # two patterns cut from a record: one k edits away from its site, one fewer (0, 1, .. in turn; an exact site shows
            # every distance up to k under report = "all": the ends beside it cost one more each)
            fewer[k] = fewer.get(k, -1) + 1
            for m in sorted({k, fewer[k] % (k + 1)}):
                s = src[int(rng.integers(0, len(src)))]
                a = int(rng.integers(0, len(s) - L - 8 + 1))
                n_sub, n_ins, n_del = _split(rng, m)
                # L letters again: n_del more are cut than the pattern keeps, n_ins fewer
                p = _edit(rng, s[a:a + L + n_del - n_ins], n_sub, n_ins, n_del)
                if len(p) != L:                # (too short to take a letter out of)
                    p = s[a:a + L]
                strand = strands[turn % 3]
                turn += 1
                if strand == "-":              # (the library's complement: the odd layout holds more than A C G T)
                    p = _lib.revcomp_bytes(p.encode("latin-1")).decode("latin-1")
                want = check(fa, seqs, p, k, strand=strand, seen=seen)
                assert len(want) >= 1
    # short records searched with themselves: the single stretch, both edges of the record
    for i, s in enumerate(seqs):
        if 2 <= len(s) <= 64 and set(s) <= set("ACGT"):
            k = min(2, len(s) - 1)
            assert (i, 0, len(s), "+", 0) in check(fa, seqs, s, k, strand="+", seen=seen)
    for p, k in (("GANTC", 1), ("RGATCY", 2), ("ACGTRYKMSWBDHVNU", 3), ("n" * 33, 8)):
        check(fa, seqs, p, k, degenerate=True, seen=seen)
    for k in BUDGETS:                          # a set that only ever meets distance 0 would hide the score
        assert seen[k] >= set(range(k + 1)), (k, seen[k])


# ------------------------------------------------------------------ the edges of the 256-byte runs
def _letter_offsets(data):
    """File offset of every kept letter of the one record in `data`."""
    body = data.index(b"\n") + 1
    a = np.frombuffer(data, dtype=np.uint8)[body:]
    return body + np.nonzero((a != 10) & (a != 13) & (a != 32))[0]


def _edge_file(rng, p, k, lines):
    """One record laid out by `lines` (letters per line), random letters, and sites of p written over them so that, wherever the
    16-byte alignment of the stream puts the 256-byte blocks (mis = 0..15), a site of every kind -- k substitutions, k inserted
    letters, k deleted letters -- ends on the last kept byte of a block and another on the first kept byte of the next.
    -> (file bytes, text, [(kind, index of the end letter)])."""
    L, n = len(p), int(sum(lines))
    shell = b">edges\n" + b"".join(b"A" * int(w) + b"\n" for w in lines)
    off = _letter_offsets(shell)
    assert off.size == n
    kinds = {"sub": (k, 0, 0), "ins": (0, k, 0), "del": (0, 0, k)}
    sites, ends, blk = [], [], 2
    for mis in range(16):
        block = (off + mis) // 256
        for kind, (n_sub, n_ins, n_del) in kinds.items():
            for first in (False, True):
                idx = np.nonzero(block == blk + (1 if first else 0))[0]
                e = int(idx[0] if first else idx[-1])
                s = _edit(rng, p, n_sub, n_ins, n_del)
                sites.append((e + 1 - len(s), s))
                ends.append((kind, e))
                blk += 2                       # a pair of blocks per site (127 letters or more each): no two sites overlap
    assert int(((off[-1] + 15) // 256)) > blk, "the record is too short for its sites"
    # within L + k letters of the record's first letter (the warm-up and the start pass stop at boff), and ending at its last
    sites += [(0, _edit(rng, p, 0, 0, 1)), (n - L - 1, _edit(rng, p, 0, 1, 0))]
    ends += [("del", L - 2), ("ins", n - 1)]
    text = _planted(rng, n, sites)
    data, a = bytearray(shell), np.frombuffer(text.encode(), dtype=np.uint8)
    np.frombuffer(data, dtype=np.uint8)[off] = a
    return bytes(data), text, ends, off


@pytest.mark.parametrize("L,k", [(20, 2), (40, 3)])
@pytest.mark.parametrize("layout", ["single", "255-256"])
def test_run_edges(fx, tmp_path, layout, L, k):
    """A site that holds k inserted letters spans L + k letters.  Where it ends on the first kept byte of a block, the lane of
    that block has to have walked L + k - 1 letters before its own: with the L - 1 of the exact search it would score the
    site's last L letters alone, which are about 2k edits away -- that "ins" site, on the first byte, is the one a shorter
    warm-up loses (the "del" and "sub" sites need L - 1 or fewer)."""
    rng = np.random.default_rng(L + len(layout))
    p = _rand(rng, L)
    blocks = 16 * 3 * 2 * 2 + 8
    if layout == "single":
        lines = np.ones(blocks * 128, dtype=np.int64)                      # a letter and a newline: 128 kept bytes per block
    else:
        lines = np.array([255, 256] * (blocks // 2 + 1), dtype=np.int64)   # the newline walks through the blocks
    data, text, ends, off = _edge_file(rng, p, k, lines)
    fa = fx.Fasta(_write(tmp_path / "edges.fa", data))
    seqs = [fa[0].seq]
    assert seqs[0] == text
    for strand, q in (("+", p), ("-", _revcomp(p))):
        want = check(fa, seqs, q, k, strand=strand)
        every = {(r[2], r[4]) for r in truth(seqs, q, k, strand, report="all")}
        for kind, e in ends:
            assert any(stop == e + 1 and d <= k for stop, d in every), (kind, e)
        assert len(want) >= len(ends)
    # the planted ends do lie on both sides of a block edge for every alignment of the stream
    for mis in range(16):
        block = (off + mis) // 256
        last = {int(np.nonzero(block == b)[0][-1]) for b in np.unique(block)}
        first = {int(np.nonzero(block == b)[0][0]) for b in np.unique(block)}
        for kind in ("sub", "ins", "del"):
            assert any(kd == kind and e in last for kd, e in ends) and any(kd == kind and e in first for kd, e in ends), (mis, kind)


# ------------------------------------------------------------------ the start pass at its limits
def test_start_pass_limits(fx, tmp_path):
    rng = np.random.default_rng(41)
    p = _rand(rng, 24)
    ins, dele = _edit(rng, p, 0, 2, 0), _edit(rng, p, 0, 0, 2)
    p64 = _rand(rng, 64)
    parts = [p64[a:a + 7] for a in range(0, 64, 7)]                       # eight letters put in, seven apart, none near an end
    s72 = "".join(x + str(rng.choice([b for b in "ACGT" if b not in (x[-1], y[0])])) for x, y in zip(parts[:8], parts[1:9])) + "".join(parts[8:])
    assert len(s72) == 72
    recs = [
        # the end letter directly behind a blank line / a CRLF: the walk back starts on a letter and skips the rest
        ">blank\n" + _rand(rng, 50) + ins[:-1] + "\n\n" + ins[-1] + _rand(rng, 40) + "\n",
        ">crlf\r\n" + _rand(rng, 33) + dele[:-1] + "\r\n" + dele[-1] + " " + _rand(rng, 30) + "\r\n",
        # the record begins with the site less its first letters: the walk stops at boff before it has L + k letters
        ">head\n" + p[3:] + _rand(rng, 20) + "\n",
        ">head2\n\n \n" + ins[1:13] + "\n" + ins[13:] + "\n",
        # L = 64, k = 8: the longest span there is, 72 letters, across lines of 7
        ">span72\n" + "\n".join((_rand(rng, 9) + s72 + _rand(rng, 9))[a:a + 7] for a in range(0, 90, 7)) + "\n",
    ]
    fa = fx.Fasta(_write(tmp_path / "starts.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    for q, k in ((p, 2), (p, 3), (p, 8), (ins, 2), (dele, 3)):
        check(fa, seqs, q, k)
        check(fa, seqs, q, k, strand="-", rev=None)
    ends = {(r[0], r[2], r[4]) for r in check(fa, seqs, p, 3, strand="+")}      # (the starts are the truth's: the shortest span)
    assert (0, 50 + len(ins), 2) in ends and (1, 33 + len(dele), 2) in ends
    assert (2, 21, 3) in ends                                            # three letters short of the pattern, from the record's first letter
    rows = check(fa, seqs, p64, 8)
    assert (4, 9, 81, "+", 8) in rows
    assert got(fa.search_edit(_revcomp(p64), 8, strand="-", ids=[4])) == [(4, 9, 81, "-", 8)]


# ------------------------------------------------------------------ runs full of ends, plateaus
def test_dense_ends(fx, tmp_path):
    ac = "AC" * 600
    fa = fx.Fasta(_write(tmp_path / "dense.fa", ">polyA\n" + "A" * 1000 + "\n>polyC\n" + "C" * 300 + "\n>ac\n" + ac + "\n>at\n" +
                         "AT" * 600 + "\n"))
    seqs = [fa[i].seq for i in range(len(fa))]
    for L in (1, 4, 32, 33, 64):
        p = "A" * L
        for k in sorted({0, min(2, L - 1), min(8, L - 1)}):
            # every letter of polyA from L - k on ends a stretch of A within k edits; polyC has none (k < L)
            h = fa.search_edit(p, k, strand="+", report="all")
            assert [r for r in got(h) if r[0] == 0] == [(0, max(e + 1 - L, 0), e + 1, "+", max(L - e - 1, 0)) for e in range(L - k - 1, 1000)]
            assert not (h.ids == 1).any()
            # best: one dip from k down to 0, then a plateau of 0 to the record's end: its leftmost end alone
            assert [r for r in got(fa.search_edit(p, k, strand="+", ids=[0]))] == [(0, 0, L, "+", 0)]
            check(fa, seqs, p, k)
    h = fa.search_edit("T", 0, report="all", ids=[0])                     # 'A' on '-': 256 ends on one strand in every full run
    assert got(h) == [(0, e, e + 1, "-", 0) for e in range(1000)]
    for L in (8, 33):
        # a repeat searched in itself at k = 2: an end at every letter, on '+' in the AC record (GT.. is nowhere), on both strands
        # in the AT record (AT.. is its own reverse complement): 256 + 256 ends in every full run
        for rec, unit, strands in ((2, "AC", 1), (3, "AT", 2)):
            p = (unit * 40)[:L]
            rows = check(fa, seqs, p, 2)
            every = fa.search_edit(p, 2, report="all", ids=[rec])
            assert every.ids.size == strands * (len(ac) - (L - 2) + 1)
            assert len({chr(c) for c in every.strands.tolist()}) == strands
            assert 1 <= len([r for r in rows if r[0] == rec]) < every.ids.size


# ------------------------------------------------------------------ the cut at slen
def test_cut_at_slen(fx, tmp_path):
    """A record whose first line ends in CR LF and whose later lines end in LF alone: the index counts two bytes off every
    line, so slen is smaller than the number of kept bytes and `seq` stops there -- no end may lie past that cut.  The letters
    around the cut are searched for: a site that ends exactly at slen is a row, the same site one letter further is not."""
    rng = np.random.default_rng(55)
    recs, kept = [], []
    for i, n_lines in enumerate((3, 12, 40, 1, 200)):
        lines = [_rand(rng, 60) for _ in range(n_lines)]
        kept.append("".join(lines))
        recs.append(">m%d\r\n" % i + lines[0] + "\r\n" + "".join(ln + "\n" for ln in lines[1:]))
    fa = fx.Fasta(_write(tmp_path / "mixed.fa", "".join(recs)))
    seqs = [fa[i].seq for i in range(len(fa))]
    assert [len(s) for s in seqs] == [len(fa[i]) for i in range(len(fa))]
    cut = [i for i, (s, t) in enumerate(zip(seqs, kept)) if len(s) < len(t)]
    assert cut, "no record is cut: the case is not exercised"
    for i in cut:
        s, t = seqs[i], kept[i]
        assert t.startswith(s)
        n = len(s)
        at, past = t[n - 14:n], t[n - 13:n + 1]                          # ends exactly at slen; ends one letter past it
        for q, k in ((at, 0), (_edit(rng, at, 1, 0, 1), 2), (past, 0), (_edit(rng, past, 1, 1, 0), 2)):
            for report in REPORTS:
                h = fa.search_edit(q, k, report=report)
                assert (h.stops <= np.array([len(x) for x in seqs])[h.ids]).all(), q
                assert got(h) == truth(seqs, q, k, report=report)
        assert (i, n - 14, n, "+", 0) in got(fa.search_edit(at, 0))
        assert not [r for r in got(fa.search_edit(past, 0, strand="+", report="all")) if r[0] == i]
        c = fa.search_edit_counts(past, 2, report="all")
        h = fa.search_edit(past, 2, report="all")
        assert c[i].tolist() == [int(((h.ids == i) & (h.strands == ord(s_))).sum()) for s_ in "+-"]


# ------------------------------------------------------------------ row offsets across a chunk of the scans
def test_scan_chunk(fx, tmp_path):
    """One record of more than SRCH_CHUNK = 4096 runs: the offsets of the rows behind run 4096 carry the sum of a whole scan
    chunk.  The background is a letter the pattern lacks: an end needs a matching letter (k < L), so ends lie within L + k of a
    site, and the truth is taken on those neighbourhoods -- the total is asserted against the whole answer."""
    rng = np.random.default_rng(77)
    n, L, k = 1_100_000, 16, 3
    p = _rand(rng, L, "ACG")
    edge = 4096 * 256 * 80 // 81                                          # the letter at the chunk boundary, lines of 80
    at = [1000, edge - 3000, edge - 300, edge - 10, edge + 200, edge + 2500, n - 60]
    sites = [(a, _edit(rng, p, j % 3, (j + 1) % 2, j % 2)) for j, a in enumerate(at)]
    text = list("T" * n)
    for a, s in sites:
        text[a:a + len(s)] = s
    text = "".join(text)
    fa = fx.Fasta(_write(tmp_path / "big.fa", ">big\n" + "\n".join(text[i:i + 80] for i in range(0, n, 80)) + "\n"))
    for report in REPORTS:
        h = fa.search_edit(p, k, strand="+", report=report)
        want = []
        for a, s in sites:                                                # T...T site T...T: the neighbourhood holds every end near it
            lo, hi = a - 2 * (L + k), a + len(s) + 2 * (L + k)
            want += [(0, lo + x, lo + y, "+", d) for x, y, d in strand_rows(text[lo:hi], p, k, False, report) if x >= 0]
        assert got(h) == want and len(want) >= 4
        assert int((h.stops > edge + 100).sum()) >= 2 and int((h.stops < edge - 100).sum()) >= 2
        assert fa.search_edit_counts(p, k, strand="+", report=report).tolist() == [[len(want), 0]]


# ------------------------------------------------------------------ counts, ids, limits, arguments
def test_counts_ids_limits(fx, fixture_files, monkeypatch):
    fa = fx.Fasta(fixture_files["test.fa"])
    seqs = [fa[i].seq for i in range(len(fa))]
    names = list(fa.keys())
    p = seqs[3][100:112]
    for report in REPORTS:
        full = fa.search_edit(p, 2, report=report)
        assert got(full) == truth(seqs, p, 2, report=report)
        sel = [5, 0, 17, 5, 3]
        keep = np.isin(full.ids, [0, 3, 5, 17])
        want = got(type(full)(*(a[keep] for a in full)))
        assert len(want) >= 1
        assert got(fa.search_edit(p, 2, report=report, ids=sel)) == want                # unsorted and repeated: as search_all treats them
        assert got(fa.search_edit(p, 2, report=report, ids=[names[i] for i in sel])) == want
        c = fa.search_edit_counts(p, 2, report=report)
        bc = np.zeros((len(seqs), 2), dtype=np.int64)
        np.add.at(bc, (full.ids, (full.strands == ord("-")).astype(np.int64)), 1)
        assert (c == bc).all()
    e = fa.search_all("GAATTC", ids=sel)
    assert [r[:4] for r in got(fa.search_edit("GAATTC", 0, report="all", ids=sel))] == list(zip(e.ids.tolist(), e.starts.tolist(), e.stops.tolist(),
                                                                                              [chr(c) for c in e.strands.tolist()]))
    with pytest.raises(KeyError):
        fa.search_edit(p, 1, ids=["no_such_record"])
    with pytest.raises(IndexError):
        fa.search_edit(p, 1, ids=[len(fa)])
    # max_hits bounds the ends, not the rows
    n_ends, n_best = fa.search_edit(p, 2, report="all").ids.size, fa.search_edit(p, 2).ids.size
    assert n_best < n_ends
    assert got(fa.search_edit(p, 2, max_hits=n_ends)) == got(fa.search_edit(p, 2))
    for report in REPORTS:
        with pytest.raises(ValueError, match="%d ends" % n_ends):
            fa.search_edit(p, 2, report=report, max_hits=n_ends - 1)
    assert n_best <= n_ends - 1
    for q, k, kw, exc in (("GAATTC", -1, {}, ValueError), ("GAATTC", 9, {}, ValueError), ("GAATTC", 6, {}, ValueError), ("A", 1, {}, ValueError),
                          ("GAATTC", 1.5, {}, TypeError), ("GAATTC", 1, {"report": "x"}, ValueError), ("GAATTC", 1, {"strand": "x"}, ValueError),
                          ("", 0, {}, ValueError), ("A" * 65, 1, {}, ValueError), ("GA TC", 1, {}, ValueError),
                          ("GAXTC", 1, {"degenerate": True}, ValueError)):
        with pytest.raises(exc):
            fa.search_edit(q, k, **kw)
        with pytest.raises(exc):
            fa.search_edit_counts(q, k, **kw)
    # byte-range shards and windows carry no halo for a site across a cut: refused, as search_all refuses them
    monkeypatch.setattr(type(fa), "_sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError):
        fa.search_edit(p, 1)
    with pytest.raises(NotImplementedError):
        fa.search_edit_counts(p, 1)


# ------------------------------------------------------------------ the binding
def test_binding():
    from pyfastx_amd import _lib as lib
    i64, u8 = np.int64, np.uint8
    two = ("ACGTACGTAAAAAAAAAAAA", "ATGGCTGCTGCTGCTTAACG")
    fasta = lib.Blob.from_bytes((">two\n%s\n%s\n>one\nACGTTTTTTTTTTTTACGT\n>none\n" % two).encode(), device=0)
    assert fasta.fasta_build().n_seq == 3
    plus = lib.FX_SEARCH_PLUS
    for report in (lib.FX_EDIT_ALL, lib.FX_EDIT_BEST):
        call = lambda ids, cap, counts: fasta.fasta_search_edit(b"ACGT", None, plus, 1, report, ids, cap, counts)
        n, n_ends, rows, cnt = call(None, 1000, True)
        assert n_ends >= n >= 4 and (n == n_ends) == (report == lib.FX_EDIT_ALL)
        assert cnt.dtype == i64 and cnt.shape == (3, 2) and int(cnt.sum()) == n and cnt[2].tolist() == [0, 0]
        assert len(rows) == 5
        for a, dt in zip(rows, (i64, i64, i64, u8, u8)):
            assert isinstance(a, np.ndarray) and a.dtype == dt and a.shape == (n,)
            assert lib.lib().fx_pinned_holds(a.ctypes.data, max(a.nbytes, 1)) == 1
        assert set(rows[3].tolist()) == {ord("+")} and set(rows[4].tolist()) <= {0, 1}
        n_c, ends_c, rows_c, cnt_c = call(None, 0, True)                  # counts only: no row comes home
        assert (n_c, ends_c, rows_c) == (n, n_ends, None) and (cnt_c == cnt).all()
        for empty in ([], np.arange(4, dtype=i64)[2:2]):                  # n = 0
            n0, e0, rows0, cnt0 = call(empty, 1000, True)
            assert (n0, e0) == (0, 0) and cnt0.shape == (0, 2) and (rows0 is None or all(a.size == 0 for a in rows0))
        n1, e1, rows1, _ = fasta.fasta_search_edit(b"GGGGGGGG", None, plus, 0, report, None, 10, False)      # no end at all
        assert (n1, e1) == (0, 0) and all(a.size == 0 for a in rows1)
        with pytest.raises(lib.FxError) as e:
            call(None, n_ends - 1, False)
        assert e.value.code == lib.FX_ERANGE and e.value.n_ends == n_ends and str(e.value) == lib.lib().fx_last_error().decode()
        n2, e2, _, _ = call(None, n_ends, False)                          # exactly the ends: accepted
        assert (n2, e2) == (n, n_ends)
    for bad in (dict(max_edits=4), dict(max_edits=-1), dict(report=2), dict(pattern=b"A" * 65), dict(mode=0)):
        kw = dict(pattern=b"ACGT", rpattern=None, mode=plus, max_edits=1, report=0, ids=None, cap=10)
        kw.update(bad)
        with pytest.raises(lib.FxError) as e:
            fasta.fasta_search_edit(**kw)
        assert e.value.code == lib.FX_EINVAL, bad
