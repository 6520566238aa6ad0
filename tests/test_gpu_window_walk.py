"""-m gpu: every kernel that looks at windows of the resident streams, asked about ONE small FASTA and ONE small FASTQ that hold
the cases a shared walk can get wrong -- run boundaries of the 256-byte blocks with and without bytes to warm up on, white
space in front of a run, runs off the 16-byte grid, read lengths and interval starts around the 16-byte pieces.  Each family's
own suite checks its own layouts; here a slip in what the families share shows in all of them at once.  Truth is brute force
in plain Python over the strings the files were written from.  Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUN = 256                                                      # bytes of the stream per lane of the FASTA walks
DIGIT = {"A": 0, "C": 1, "G": 2, "T": 3}
LUT = np.full(256, 4, dtype=np.int64)
for _c, _d in DIGIT.items():
    LUT[ord(_c)] = _d


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode("latin-1"))
    return str(path)


def _rand(rng, n, letters="ACGT"):
    return "".join(letters[int(j)] for j in rng.integers(0, len(letters), n))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


# ------------------------------------------------------------------ brute force
def codes_of(s, k, canonical=False):
    """The code every valid window of s is counted under, in order of the windows: each window from its own k letters."""
    d = LUT[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)]
    n = d.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    f, r, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for j in range(k):
        w = d[j:j + n]
        bad |= w > 3
        f = f * 4 + (w & 3)
        r = r + (3 - (w & 3)) * 4 ** j                         # the reverse complement: the last letter's complement leads
    return (np.minimum(f, r) if canonical else f)[~bad]


def table_of(seqs, k, canonical=False):
    """(codes ascending, counts) of all the windows of seqs."""
    codes, counts = np.unique(np.concatenate([codes_of(s, k, canonical) for s in seqs]), return_counts=True)
    return codes, counts.astype(np.int64)


def hits_of(seqs, k, canonical, set_codes):
    per = [codes_of(s, k, canonical) for s in seqs]
    return np.array([p.size for p in per]), np.array([int(np.isin(p, set_codes).sum()) for p in per])


def same_table(t, want):
    return t.codes.dtype == np.int64 and np.array_equal(t.codes, want[0]) and np.array_equal(t.counts, want[1])


def same_dense(got, want):
    """A dense spectrum against (codes, counts): the same entries, every other one zero."""
    nz = np.flatnonzero(got)
    return got.dtype == np.int64 and np.array_equal(nz, want[0]) and np.array_equal(got[nz], want[1])


def hamming_rows(seqs, p, d):
    """[(record, start, stop, strand, distance)] of the windows within d substitutions of p ('+') or of its reverse complement
    ('-'), by (record, start), '+' first."""
    L, rows = len(p), []
    for r, s in enumerate(seqs):
        for a in range(len(s) - L + 1):
            for strand, q in (("+", p), ("-", _rc(p))):
                m = sum(x != y for x, y in zip(s[a:a + L], q)) if d else int(s[a:a + L] != q)
                if m <= d:
                    rows.append((r, a, a + L, strand, m))
    return rows


def pwm_rows(seqs, ints, t):
    """[(record, start, stop, strand, score)] of the windows of valid letters whose score reaches t."""
    W, rows = len(ints), []
    for r, s in enumerate(seqs):
        for a in range(len(s) - W + 1):
            w = s[a:a + W]
            if not all(c in DIGIT for c in w):
                continue
            sf = sum(int(ints[j][DIGIT[c]]) for j, c in enumerate(w))
            sr = sum(int(ints[W - 1 - j][3 - DIGIT[c]]) for j, c in enumerate(w))
            rows += [(r, a, a + W, "+", sf)] if sf >= t else []
            rows += [(r, a, a + W, "-", sr)] if sr >= t else []
    return rows


# ------------------------------------------------------------------ the FASTA
def _lines(s, width):
    return "".join(s[a:a + width] + "\n" for a in range(0, len(s), width))


class _Text:
    """A FASTA under construction: the file, the letters of every record and the offset of every record's first sequence byte."""

    def __init__(self):
        self.text, self.seqs, self.boff = "", [], []

    def add(self, at, body, letters, eol="\n"):
        """One more record whose bytes begin at offset `at` inside a 256-byte block: its header is padded for that."""
        head = ">r%d_" % len(self.seqs)
        pad = (at - (len(self.text) + len(head) + len(eol))) % RUN
        self.text += head + "x" * pad + eol
        assert len(self.text) % RUN == at
        self.boff.append(len(self.text))
        self.seqs.append(letters)
        self.text += body


def _build_fasta(rng):
    """-> (text, seqs, boff): the file, the letters of every record and the offset of every record's first sequence byte.
    A header is padded so that the record's bytes begin at the wanted offset inside a 256-byte block."""
    t = _Text()
    add = t.add

    s = _rand(rng, 300)
    add(37, _lines(s, 60), s)                                  # begins and ends off the 16-byte grid, crosses one boundary
    s = list(_rand(rng, 700))                                  # begins exactly on a boundary: its first run has no warm-up
    for byte in (RUN - 1, 2 * RUN + 1):                        # N: the last letter in front of one boundary, the second behind another
        assert byte % 71 != 70
        s[byte - byte // 71] = "N"
    s = "".join(s)
    add(0, _lines(s, 70), s)
    s = _rand(rng, 200)
    add(RUN - 1, _lines(s, 60), s)                             # one byte in front of a boundary
    s = _rand(rng, 200)
    add(RUN - 15, _lines(s, 60), s)                            # 15 bytes: the record begins inside the 16 bytes in front of its second run
    # white space in front of a run: the 16 bytes in front of the boundary hold 5 letters, the 32 bytes 16
    a, b, c = _rand(rng, 135), _rand(rng, 5), _rand(rng, 230)
    body = a + "\n" + "\n" * 4 + "\n" * 3 + b[:3] + "\r\n" + "\n" * 6 + b[3:] + c[:58] + "\n" + _lines(c[58:], 60)
    add(100, body, a + b + c)
    assert (t.boff[-1] + body.index(c[:58])) % RUN == 0 and body[body.index(c[:58]) - 16:body.index(c[:58])].count("\n") == 10
    s = _rand(rng, 50)
    add(37, s + "\n", s)                                       # one short run: a masked first and last chunk and nothing between
    s = _rand(rng, 41, "ACGTN")
    add(70, s + "\n", s)
    s = _rand(rng, 310)
    add(250, _lines(s, 80)[:-1], s)                            # the last record has no final newline
    return t.text, t.seqs, t.boff


@pytest.fixture(scope="module")
def fasta(fx, tmp_path_factory):
    text, seqs, boff = _build_fasta(np.random.default_rng(20))
    assert 2500 < len(text) < 4500 and not text.endswith("\n")
    assert [b % RUN for b in boff[:4]] == [37, 0, RUN - 1, RUN - 15]
    fa = fx.Fasta(_write(tmp_path_factory.mktemp("ww") / "w.fa", text))
    assert [fa[i].seq for i in range(len(fa))] == seqs
    return fa, seqs, text, boff


@pytest.fixture(scope="module")
def fasta_tables(fasta):
    """(k, canonical) -> (codes, counts) of the whole file, computed once."""
    seqs = fasta[1]
    return {(k, c): table_of(seqs, k, c) for k in (1, 2, 12, 13, 14, 17, 31) for c in (False, True)}


def _across_boundaries(seqs, text, boff, L):
    """Patterns of L letters cut from the records so that they lie across a block boundary of the stream."""
    out = []
    for s, b in zip(seqs, boff):
        if "N" in s:
            continue
        body = text[b:].split(">")[0]
        for edge in range((b // RUN + 1) * RUN, b + len(body), RUN):
            at = max(sum(1 for ch in body[:edge - b] if ch not in "\r\n") - L // 2, 0)      # letters in front of the boundary
            if 0 <= at and at + L <= len(s):
                out.append(s[at:at + L])
    assert len(out) >= 5
    return out


@pytest.fixture(scope="module")
def dense13(fasta):
    """canonical -> the non-zero entries of the dense spectrum at k = 13 (4^13 counters come back per call: asked once)."""
    out = {}
    for canonical in (False, True):
        got = fasta[0].kmer_counts(13, canonical=canonical)
        assert got.dtype == np.int64 and got.shape == (4 ** 13,)
        nz = np.flatnonzero(got)
        out[canonical] = (nz, np.asarray(got[nz]))
    return out


@pytest.mark.parametrize("k", [1, 2, 12])
def test_fasta_dense(fasta, fasta_tables, k):
    fa = fasta[0]
    for canonical in (False, True):
        assert same_dense(fa.kmer_counts(k, canonical=canonical), fasta_tables[k, canonical]), (k, canonical)


def test_fasta_dense_13(fasta_tables, dense13):
    for canonical in (False, True):
        assert np.array_equal(dense13[canonical][0], fasta_tables[13, canonical][0]), canonical
        assert np.array_equal(dense13[canonical][1], fasta_tables[13, canonical][1]), canonical


@pytest.mark.parametrize("k", [13, 14, 17, 31])
def test_fasta_table_and_hits(fasta, fasta_tables, dense13, k):
    from pyfastx_amd import kmer
    fa, seqs = fasta[:2]
    for canonical in (False, True):
        t = fa.kmer_table(k, canonical=canonical)
        assert same_table(t, fasta_tables[k, canonical]), (k, canonical)
        nw, nh = fa.kmer_hits(t)                               # the table of the file itself: every window hits
        want = np.array([codes_of(s, k).size for s in seqs])
        assert nw.dtype == nh.dtype == np.int64 and np.array_equal(nw, want) and np.array_equal(nh, want), (k, canonical)
        if k == 13:                                            # the dense form and the table, entry by entry
            assert np.array_equal(dense13[canonical][0], t.codes) and np.array_equal(dense13[canonical][1], t.counts), canonical
        if k != 17:                                            # the table of one record
            codes, counts = table_of([seqs[0]], k, canonical)
            nw, nh = fa.kmer_hits(kmer.KmerTable(k, canonical, codes, counts))
            ww, wh = hits_of(seqs, k, canonical, codes)
            assert np.array_equal(nw, ww) and np.array_equal(nh, wh) and wh[0] == ww[0] and wh.sum() < ww.sum(), (k, canonical)


@pytest.mark.parametrize("L", [1, 17, 33, 64])
def test_fasta_search(fasta, L):
    fa, seqs, text, boff = fasta
    for p in _across_boundaries(seqs, text, boff, L):
        h = fa.search_all(p)
        got = list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()]))
        want = [row[:4] for row in hamming_rows(seqs, p, 0)]
        assert want and got == want, p


@pytest.mark.parametrize("L", [17, 33])
def test_fasta_search_approx(fasta, L):
    fa, seqs, text, boff = fasta
    for j, p in enumerate(_across_boundaries(seqs, text, boff, L)):
        at = (5 * j) % L
        q = p[:at] + "ACGT"[(DIGIT[p[at]] + 1) % 4] + p[at + 1:]                    # one letter off, at another place each time
        h = fa.search_approx(q, 1)
        got = list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], h.mismatches.tolist()))
        want = hamming_rows(seqs, q, 1)
        assert any(row[4] == 1 for row in want) and got == want, q


@pytest.mark.parametrize("W", [4, 40])
def test_fasta_pwm(fasta, W):
    from pyfastx_amd.pwm import Pwm
    fa, seqs = fasta[:2]
    rng = np.random.default_rng(W)
    ints = rng.integers(-50, 51, (W, 4)).astype(np.int32)
    t = 100 if W == 4 else 300                                 # random weights: a minority of the windows reaches it
    h = fa.pwm_scan(Pwm.from_ints(ints), min_score=t)
    got = list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], h.scores.tolist()))
    want = pwm_rows(seqs, ints, t)
    assert len(want) > 10 and len(set(row[0] for row in want)) > 3 and got == want


# ------------------------------------------------------------------ the cut at slen
# One count, fix and emit kernel runs under every window-hit form, and one helper places the cut for them, for the spectra and for
# the sketches.  A record whose first line ends in CR LF and whose later lines end in LF alone has more kept bytes than slen (one
# per later line) and `seq` stops at slen: no row may come from behind that cut.  Four records: A with whole runs behind the cut,
# B with the cut on a 256-byte boundary of the stream, C inside one block, D without a cut.
CUT_LINES = dict(A=(700, 60), B=(320, 60), C=(8, 20))          # record -> (lines, letters per line)


def _mixed(s, width):
    """The first line CR LF, the later ones LF."""
    return s[:width] + "\r\n" + _lines(s[width:], width)


def _cut_of(n_lines, width):
    """(slen, raw offset of kept byte number slen from the record's first byte) of _mixed(): the index takes two bytes off every line."""
    slen = n_lines * width - (n_lines - 1)
    line, col = divmod(slen, width)
    return slen, (width + 2) + (line - 1) * (width + 1) + col


def _build_cut_fasta(rng):
    """-> (text, kept): the file and the kept letters of every record (seq is kept[i][:slen])."""
    t = _Text()
    for name, at in (("A", -5), ("B", 0), ("C", None)):         # A, B: where in its block the first byte behind the cut lies
        n, width = CUT_LINES[name]
        s = _rand(rng, n * width)
        t.add(60 if at is None else (at - _cut_of(n, width)[1]) % RUN, _mixed(s, width), s, eol="\r\n")      # (the header's line end is what the index goes by)
    s = _rand(rng, 90)
    t.add(200, s + "\n", s)                                    # D
    return t.text, t.seqs


def _cut_patterns(kept, slens, L):
    """Per cut record: the site that ends exactly at slen, the same site one letter later, the last kept letters."""
    return [(i, kept[i][n - L:n], kept[i][n - L + 1:n + 1], kept[i][-L:]) for i, n in enumerate(slens[:3])]


@pytest.fixture(scope="module")
def cut_text():
    text, kept = _build_cut_fasta(np.random.default_rng(22))
    assert 20_000 < len(text) < 80_000
    slens = [_cut_of(*CUT_LINES[name])[0] for name in "ABC"] + [len(kept[3])]
    return text, kept, slens, [s[:n] for s, n in zip(kept, slens)]


def test_cut_text_is_what_the_cases_need(cut_text, oracle):
    """No device: the conditions that keep test_cut_at_slen from passing vacuously, from the bytes and the CPU oracle's index."""
    text, kept, slens, seqs = cut_text
    raw = text.encode("latin-1")
    recs, _ = oracle.fasta_index(raw)
    assert recs["slen"].tolist() == slens
    body = [raw[int(r["boff"]):int(r["boff"] + r["blen"])] for r in recs]
    at = [np.flatnonzero(~np.isin(np.frombuffer(b, dtype=np.uint8), (10, 13, 32))) for b in body]      # raw offsets of the kept bytes
    assert [bytes(np.frombuffer(b, dtype=np.uint8)[a]).decode() for b, a in zip(body, at)] == kept
    cut = [int(r["boff"]) + int(a[n]) if n < a.size else None for r, a, n in zip(recs, at, slens)]      # stream address of kept byte number slen
    end = [int(r["boff"] + r["blen"]) for r in recs]
    assert end[0] // RUN - -(-cut[0] // RUN) >= 2                                   # A: two whole runs behind the cut
    assert cut[1] % RUN == 0 and end[1] - cut[1] >= RUN and cut[1] - int(recs["boff"][1]) >= RUN      # B: a whole run on either side
    assert int(recs["boff"][2]) // RUN == (end[2] - 1) // RUN and cut[2] is not None and len(kept[2]) - slens[2] >= 5      # C
    assert cut[3] is None and len(kept[3]) == slens[3]                              # D
    for L in (12, 40):
        for i, q_at, q_past, q_tail in _cut_patterns(kept, slens, L):
            n = slens[i]
            assert (i, n - L, n, "+") in [row[:4] for row in hamming_rows(seqs, q_at, 0)]
            assert not [row for row in hamming_rows(seqs, q_past, 0) + hamming_rows(seqs, q_tail, 0) if row[0] == i]
            assert kept[i].find(q_past) == n - L + 1 and kept[i].find(q_tail) == len(kept[i]) - L      # they are there, behind the cut


@pytest.fixture(scope="module")
def cut_fasta(fx, cut_text, tmp_path_factory):
    text, kept, slens, seqs = cut_text
    fa = fx.Fasta(_write(tmp_path_factory.mktemp("wc") / "cut.fa", text))
    assert [fa[i].seq for i in range(len(fa))] == seqs
    return fa, seqs, kept, slens


def _counts_of(rows, n):
    c = np.zeros((n, 2), dtype=np.int64)
    for row in rows:
        c[row[0], int(row[3] == "-")] += 1
    return c


def _hits(h, *cols):
    return list(zip(h.ids.tolist(), h.starts.tolist(), h.stops.tolist(), [chr(c) for c in h.strands.tolist()], *[getattr(h, c).tolist() for c in cols]))


def _match_ints(q):
    """The matrix that scores a letter of q 10 and any other -10."""
    return np.array([[10 if DIGIT[c] == j else -10 for j in range(4)] for c in q], dtype=np.int32)


@pytest.mark.parametrize("form", ["exact", "approx", "edit", "pwm-A", "pwm-B", "pwm-C", "minimizers", "kmers", "sketch"])
def test_cut_at_slen(cut_fasta, form):
    """Every form that shares the cut, asked for rows and for counts about the three sites of A, B and C (the matrix, whose brute
    force is the slowest, one record's sites per case)."""
    fa, seqs, kept, slens = cut_fasta
    n_rec = len(seqs)
    if form == "exact":
        for L in (12, 40):                                     # both register widths
            for i, q_at, q_past, q_tail in _cut_patterns(kept, slens, L):
                for q in (q_at, q_past, q_tail):
                    want = [row[:4] for row in hamming_rows(seqs, q, 0)]
                    assert _hits(fa.search_all(q)) == want, (i, q)
                    assert np.array_equal(fa.search_counts(q), _counts_of(want, n_rec)), (i, q)
                assert (i, slens[i] - L, slens[i], "+") in _hits(fa.search_all(q_at))
    elif form == "approx":
        for i, q_at, q_past, q_tail in _cut_patterns(kept, slens, 12):
            for q in (q_at, q_past, q_tail):
                q = q[:3] + "ACGT"[(DIGIT[q[3]] + 1) % 4] + q[4:]                  # one letter off
                want = hamming_rows(seqs, q, 2)
                assert _hits(fa.search_approx(q, 2), "mismatches") == want, (i, q)
                assert np.array_equal(fa.search_approx_counts(q, 2), _counts_of(want, n_rec)), (i, q)
            assert (i, slens[i] - 12, slens[i], "+", 0) in _hits(fa.search_approx(q_at, 2), "mismatches")
    elif form == "edit":
        from search_edit_truth import truth
        for i, q_at, q_past, q_tail in _cut_patterns(kept, slens, 12):
            for q in (q_at, q_past, q_tail):
                for report in ("all", "best"):
                    want = truth(seqs, q, 1, report=report, rev=_rc(q))
                    assert _hits(fa.search_edit(q, 1, report=report), "edits") == want, (i, q, report)
                    assert np.array_equal(fa.search_edit_counts(q, 1, report=report), _counts_of(want, n_rec)), (i, q, report)
            assert (i, slens[i] - 12, slens[i], "+", 0) in _hits(fa.search_edit(q_at, 1, report="best"), "edits")
    elif form.startswith("pwm"):
        from pyfastx_amd.pwm import Pwm
        for i, q_at, q_past, q_tail in _cut_patterns(kept, slens, 12)["ABC".index(form[-1]):][:1]:
            for q in (q_at, q_past, q_tail):
                ints = _match_ints(q)
                every = pwm_rows(seqs, ints, -10 ** 9)
                want = [row for row in every if row[4] >= 80]                       # two letters off at the most
                assert _hits(fa.pwm_scan(Pwm.from_ints(ints), min_score=80), "scores") == want, (i, q)
                assert np.array_equal(fa.pwm_counts(Pwm.from_ints(ints), min_score=80), _counts_of(want, n_rec)), (i, q)
                top = {}
                for r, a, _, strand, score in every:           # the larger score, then the smaller start
                    if (r, strand) not in top or score > top[r, strand][0]:
                        top[r, strand] = (score, a)
                b = fa.pwm_best(Pwm.from_ints(ints))
                got = {(r, strand): (int(b.scores[r, col]), int(b.starts[r, col])) for r in range(n_rec) for col, strand in enumerate("+-")}
                assert got == top, (i, q)
                assert (got[i, "+"][0] == 120) == (q is q_at), (i, q)               # the whole site: in front of the cut only
    elif form == "minimizers":
        from minimizer_truth import truth
        for k, w, canonical in ((5, 4, True), (7, 3, False)):
            rows, counts = truth(seqs, k, w, canonical, "hash")
            m = fa.minimizers(k, w, canonical=canonical)
            assert list(zip(m.ids.tolist(), m.starts.tolist(), [chr(c) for c in m.strands.tolist()], m.codes.tolist())) == rows, (k, w, canonical)
            assert np.array_equal(fa.minimizer_counts(k, w, canonical=canonical), counts), (k, w, canonical)
            assert all((m.starts[m.ids == i] + k <= slens[i]).all() for i in range(n_rec))
    elif form == "kmers":
        for k, canonical in ((6, False), (3, True)):
            per = [np.bincount(codes_of(s, k, canonical), minlength=4 ** k) for s in seqs]
            got = fa.kmer_profile(k, canonical=canonical)
            assert got.dtype == np.int64 and np.array_equal(got, np.array(per)), (k, canonical)
            for i in range(n_rec):
                assert np.array_equal(fa.kmer_counts(k, canonical=canonical, ids=[i]), per[i]), (k, canonical, i)
            assert np.array_equal(fa.kmer_counts(k, canonical=canonical), sum(per)), (k, canonical)
    else:
        from sketch_truth import key_set_np
        for k, canonical in ((15, True), (9, False)):
            per = [key_set_np(s, k, canonical) for s in seqs]
            sk = fa.sketch(k, scaled=1, canonical=canonical)
            assert sk.sizes.tolist() == [p.size for p in per], (k, canonical)
            assert all(np.array_equal(sk.hashes(i), per[i]) for i in range(n_rec)), (k, canonical)
            pooled = fa.sketch(k, scaled=1, canonical=canonical, pooled=True)
            assert np.array_equal(pooled.hashes(0), np.unique(np.concatenate(per))), (k, canonical)
            behind = [np.setdiff1d(key_set_np(kept[i], k, canonical), per[i]).size for i in range(3)]
            assert min(behind) > 0                             # keys that only the letters behind the cut hold: none came back


# ------------------------------------------------------------------ the FASTQ
N_READS, LPR = 40, 4                                           # lpr = ceil(mean read length / 16) lanes per read
FIXED = (0, 1, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49, 16 * LPR - 1, 16 * LPR + 1)


@pytest.fixture(scope="module")
def fastq(fx, tmp_path_factory):
    rng = np.random.default_rng(21)
    lens = list(FIXED) + rng.integers(20, 110, N_READS - len(FIXED) - 1).tolist()
    lens.append(56 * N_READS - sum(lens))                      # a mean of 56 bases: lpr = 4, and the reads above 64 take a second step
    assert 64 < lens[-1] and max(lens) > 100
    pool = _rand(rng, 600)                                     # slices of one pool, so that reads share k-mers
    reads = []
    for j, n in enumerate(lens):
        a = int(rng.integers(0, len(pool) - n + 1))
        s = list(pool[a:a + n])
        if j >= len(FIXED) and j % 3 == 0:
            for at in rng.integers(0, n, 2):
                s[int(at)] = "N"
        reads.append("".join(s))
    fq = fx.Fastq(_write(tmp_path_factory.mktemp("wq") / "w.fq", "".join("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads))))
    assert len(fq) == N_READS and (-(-sum(lens) // N_READS) + 15) // 16 == LPR
    ids, start, end = [], [], []
    for i, s in enumerate(reads):                              # every interval the read has room for
        for a in (0, 1, 15, 16, 17):
            for b in (len(s), len(s) - 1):
                if a <= b:
                    ids.append(i); start.append(a); end.append(b)
    cuts = [reads[i][a:b] for i, a, b in zip(ids, start, end)]
    return fq, reads, dict(ids=ids, start=start, end=end), cuts


def test_fastq_dense(fastq):
    fq, reads, iv, cuts = fastq
    for k in (1, 13):
        for canonical in (False, True):
            assert same_dense(fq.kmer_counts(k, canonical=canonical), table_of(reads, k, canonical)), (k, canonical)
            assert same_dense(fq.kmer_counts(k, canonical=canonical, **iv), table_of(cuts, k, canonical)), (k, canonical)


@pytest.mark.parametrize("k", [13, 17, 18, 31])
def test_fastq_table_and_hits(fastq, k):
    from pyfastx_amd import kmer
    fq, reads, iv, cuts = fastq
    rng = np.random.default_rng(k)
    for canonical in (False, True):
        whole, cut = table_of(reads, k, canonical), table_of(cuts, k, canonical)
        assert whole[0].size > 200
        assert same_table(fq.kmer_table(k, canonical=canonical), whole), (k, canonical)
        assert same_table(fq.kmer_table(k, canonical=canonical, **iv), cut), (k, canonical)
        # a set of the windows of every fourth read: in LDS; with codes no read has it passes 4096 and lies in global memory
        small = table_of(reads[::4], k, canonical)[0]
        extra = np.setdiff1d(table_of([_rand(rng, 3 * kmer.SCREEN_LDS_KEYS)], k, canonical)[0], whole[0])
        large = np.union1d(small, extra)
        assert small.size <= kmer.SCREEN_LDS_KEYS < large.size
        tables = [kmer.KmerTable(k, canonical, codes, np.ones(codes.size, dtype=np.int64)) for codes in (small, large)]
        for kw, seqs in ((dict(), reads), (iv, cuts)):
            ww, wh = hits_of(seqs, k, canonical, small)
            assert 0 < wh.sum() < ww.sum()
            for t in tables:
                nw, nh = fq.kmer_hits(t, **kw)
                assert nw.dtype == nh.dtype == np.int32 and np.array_equal(nw, ww) and np.array_equal(nh, wh), (k, canonical, len(t))
        for t in tables:
            t.release()
