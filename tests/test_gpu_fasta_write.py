"""-m gpu: Fasta.records / write and fx_fasta_format_alloc (csrc/fx_fasta_format.hpp) against the plain-Python truth of
fasta_write_truth.py: byte-for-byte equality of the buffer and of the offsets -- over every line shape of the source, every
output width, both strands, the three mask modes, the edges of the emit kernel's chunks and tiles, irregular records, the
fixtures, the round trips through a file, and the errors."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import fasta_write_truth as T
from conftest import DATA

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b"ACGTacgtNnRYKMrykm", dtype=np.uint8)
WIDTHS = (0, 1, 2, 7, 16, 59, 60, 61, 64, 100, 10**6)


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return pyfastx_amd


@pytest.fixture(scope="module")
def tile(fx):
    from pyfastx_amd import fasta_out
    return fasta_out.tile()


def rand_seq(rng, n, alphabet=ALPHABET):
    return alphabet[rng.integers(0, alphabet.size, n)].tobytes()


def built(data):
    """The resident stream of `data` with its table built -> (blob, [(header, letters)] as the parser reads them)."""
    from pyfastx_amd import _lib
    b = _lib.Blob.from_bytes(data)
    s = b.fasta_build()
    recs = T.parse_fasta(data)
    assert s.n_seq == len(recs)
    return b, recs


def same(got, want, what=""):
    buf, offs = got[0], got[1]
    wbuf, woffs = want
    assert offs.dtype == np.int64 and offs.tolist() == woffs, what
    if buf.tobytes() != wbuf:
        g = buf.tobytes()
        k = next(i for i in range(min(len(g), len(wbuf))) if g[i] != wbuf[i])
        raise AssertionError("%s: first difference at byte %d: %r != %r" % (what, k, g[max(k - 20, 0):k + 20], wbuf[max(k - 20, 0):k + 20]))


def run(blob, recs, queries, minus=None, width=60, headers=None, mask=None, mode="none", char="N", upper=False, min_len=0):
    """One call of the C entry through the binding, and the truth for it.  queries: (record, start, stop), start = stop = None for
    whole records (then every query must be whole); headers None: the records' own."""
    from pyfastx_amd import fasta_out
    n = len(queries)
    minus = [False] * n if minus is None else list(minus)
    whole = n == 0 or queries[0][1] is None
    ids = np.array([q[0] for q in queries], dtype=np.int64)
    a = None if whole else np.array([q[1] for q in queries], dtype=np.int64)
    b = None if whole else np.array([q[2] for q in queries], dtype=np.int64)
    fpq = np.array([(6 if m else 0) | (1 if upper else 0) for m in minus], dtype=np.uint8)
    hdr = hdr_off = None
    if headers is not None:
        hdr, hdr_off = fasta_out.pack_headers(headers, n)
    got = blob.fasta_format_alloc(n, ids, a, b, flags=1 if upper else 0, flags_per_query=fpq if any(minus) else None, width=width, hdr=hdr,
                                  hdr_off=hdr_off, mask=mask, mask_mode=fasta_out.MASK_MODES[mode], mask_byte=ord(char), min_len=min_len)
    rows = [] if mask is None else list(zip(*(np.asarray(c).tolist() for c in mask)))
    want = T.records([s for _, s in recs], [recs[q[0]][0] for q in queries] if headers is None else headers, queries, minus, width, rows, mode,
                     char, upper, min_len)
    same(got, want, "width %d" % width)
    kept = sum(1 for x, y in zip(want[1], want[1][1:]) if y > x)
    assert got[2] == kept
    return got


# ------------------------------------------------------------------ line shapes
@pytest.mark.parametrize("lw", [1, 15, 16, 17, 60, 64, 255, 256, 257])
def test_line_shapes(fx, lw):
    """Input lines of lw letters, ended by \\n or \\r\\n, the file's last line terminated or not; records of length 0, 1, lw - 1, lw,
    lw + 1 and a few lines with a full or a short last line; whole records at every output width, own headers."""
    rng = np.random.default_rng(lw)
    lens = [0, 1, max(lw - 1, 1), lw, lw + 1, 3 * lw, 3 * lw + lw // 2 + 1, 1000 + lw]
    for eol in (b"\n", b"\r\n"):
        for last in ("full", "unterminated"):
            order = rng.permutation(len(lens))
            recs = [("r%d len %d" % (k, lens[j]), rand_seq(rng, lens[j])) for k, j in enumerate(order)]
            if last == "unterminated" and not recs[-1][1]:
                recs.append(("tail", rand_seq(rng, 2 * lw + 1)))
            blob, parsed = built(T.write_fasta(recs, lw, eol, last))
            assert [s for _, s in parsed] == [s for _, s in recs]
            if eol == b"\r\n" and last == "unterminated":
                # The letters of a record are what the fetch path returns (flags 0), and the table -- as the reference's index does
                # -- counts the unterminated last line of a \r\n file one letter short: the last record is held against that.
                k = len(recs) - 1
                t = blob.fasta_table(len(recs))
                fb, fo, fl = blob.fasta_fetch([k], [0], [int(t["slen"][k])])
                tail = fb[:int(fl[0])].tobytes()
                assert tail in (parsed[k][1], parsed[k][1][:-1])
                parsed[k] = (parsed[k][0], tail)
            q = [(k, None, None) for k in range(len(recs))]
            for w in WIDTHS:
                run(blob, parsed, q, width=w)
            run(blob, parsed, q, minus=[k % 2 == 1 for k in range(len(q))], width=lw + 1, upper=True)
            # seq_id = NULL: the records 0..n-1
            got = blob.fasta_format_alloc(len(recs), None, None, None, width=7)
            same(got, T.records([s for _, s in parsed], [h for h, _ in parsed], q, [False] * len(q), 7, [], "none", "N", False, 0))


# ------------------------------------------------------------------ intervals
@pytest.mark.parametrize("lw, eol", [(16, b"\n"), (17, b"\r\n"), (60, b"\n"), (61, b"\r\n")])
def test_interval_phases(fx, lw, eol):
    """Start and stop at every phase of a source line, both strands and upper case mixed per row in one call."""
    rng = np.random.default_rng(100 + lw)
    recs = [("a", rand_seq(rng, 5 * lw + 3)), ("b", rand_seq(rng, 2 * lw)), ("c", rand_seq(rng, lw - 1))]
    blob, parsed = built(T.write_fasta(recs, lw, eol))
    q, minus = [], []
    for a in range(0, 2 * lw + 2):
        for ln in (0, 1, 2, lw - 1, lw, lw + 1, 2 * lw + 5):
            q.append((0, a, min(a + ln, len(recs[0][1]))))
            minus.append((a + ln) % 3 == 0)
    for a in range(0, lw):
        q.append((1, a, 2 * lw - a // 2))
        minus.append(a % 2 == 0)
        q.append((2, a // 2, lw - 1))
        minus.append(a % 2 == 1)
    hdrs = ["q%d" % k for k in range(len(q))]
    for w in (0, 1, 16, lw, 100):
        run(blob, parsed, q, minus=minus, width=w, headers=hdrs)
    # the upper-case bit differs per row too
    from pyfastx_amd import fasta_out
    fpq = np.array([(6 if m else 0) | (k & 1) for k, m in enumerate(minus)], dtype=np.uint8)
    hdr, hdr_off = fasta_out.pack_headers(hdrs, len(q))
    got = blob.fasta_format_alloc(len(q), [x[0] for x in q], [x[1] for x in q], [x[2] for x in q], flags_per_query=fpq, width=19, hdr=hdr, hdr_off=hdr_off)
    want, offs = [], [0]
    for k, (r, a, b) in enumerate(q):
        want.append(T.record(hdrs[k], T.letters(parsed[r][1], a, b, minus[k], (), "none", "N", bool(k & 1)), 19))
        offs.append(offs[-1] + len(want[-1]))
    same(got, (b"".join(want), offs))


# ------------------------------------------------------------------ chunk and tile edges
@pytest.fixture(scope="module")
def long_blob(fx, tile):
    rng = np.random.default_rng(7)
    recs = [("long one", rand_seq(rng, 40 * tile + 123)), ("second", rand_seq(rng, tile + 50)), ("third", rand_seq(rng, 3 * tile))]
    return built(T.write_fasta(recs, 60))


def test_records_across_tile_edges(fx, tile, long_blob):
    """Records whose size runs over T - 20 .. T + 20 at header lengths 0 .. 17: the records begin at every offset mod 16, and the
    tile edges fall on every part of a record."""
    blob, parsed = long_blob
    q, hdrs = [], []
    for hl in range(18):
        for size in range(tile - 20, tile + 21):
            q.append((1, 3, 3 + size - hl - 3))                 # width 0: size = header + 2 + L + 1
            hdrs.append("h" * hl)
    got = run(blob, parsed, q, width=0, headers=hdrs)
    assert set((got[1][:-1] % 16).tolist()) == set(range(16))
    assert set((np.diff(got[1]) - tile).tolist()) == set(range(-20, 21))


def test_many_short_records_per_chunk(fx, tile):
    """2 000 records of 0 .. 40 letters: several whole records in one 16-byte chunk; lines shorter than 16 letters take the
    despaced path, the others the line arithmetic, in one call."""
    rng = np.random.default_rng(11)
    recs = [("r%d" % k, rand_seq(rng, int(rng.integers(0, 41)))) for k in range(2000)]
    blob, parsed = built(T.write_fasta(recs, 60))
    q = [(k, None, None) for k in range(2000)]
    for w in (0, 7, 16):
        run(blob, parsed, q, width=w)
    run(blob, parsed, q, minus=[k % 2 == 0 for k in range(2000)], width=5, min_len=3)
    run(blob, parsed, [(k, 1, len(parsed[k][1])) for k in range(2000) if parsed[k][1]], width=9, headers=["" for k in range(2000) if parsed[k][1]])


def test_one_record_of_forty_tiles(fx, tile, long_blob):
    blob, parsed = long_blob
    for w, minus in ((60, False), (80, True), (0, False), (61, True)):
        run(blob, parsed, [(0, None, None)], minus=[minus], width=w)
    run(blob, parsed, [(0, 17, 40 * tile + 100)], minus=[True], width=100, headers=["x"])


def test_custom_headers_of_0_and_300_bytes(fx, long_blob):
    blob, parsed = long_blob
    q = [(1, 0, 10), (1, 5, 70), (0, 100, 100), (2, 0, 1), (1, 0, 200)]
    hdrs = ["", "H" * 300, "", "y" * 300, "z"]
    for w in (0, 16, 60):
        run(blob, parsed, q, minus=[False, True, False, True, False], width=w, headers=hdrs)


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("mode", ["soft", "hard", "upper"])
def test_masks(fx, tile, mode):
    """Rows that begin or end at line ends, chunk ends and tile ends, three rows inside one 16-byte chunk, empty rows, a row over
    a whole record, a record without rows between two with rows, rows outside the queried interval, the minus strand."""
    rng = np.random.default_rng(13)
    L0 = 2 * tile + 777
    recs = [("m0", rand_seq(rng, L0)), ("m1 no rows", rand_seq(rng, 500)), ("m2", rand_seq(rng, 400)), ("m3 all", rand_seq(rng, 333))]
    blob, parsed = built(T.write_fasta(recs, 60))
    rows = [(0, 0, 1), (0, 5, 5), (0, 16, 18), (0, 20, 21), (0, 23, 30),            # an empty row; three rows in one chunk
            (0, 60, 120), (0, 180, 181), (0, 239, 241), (0, 300, 300), (0, 320, 336),  # source line ends (60 letters per line)
            (0, tile - 64, tile - 32), (0, tile - 16, tile), (0, tile, tile + 16), (0, tile + 48, tile + 61),
            (0, 2 * tile - 3, 2 * tile + 3), (0, L0 - 1, L0),
            (2, 0, 0), (2, 10, 50), (2, 50, 50), (2, 399, 400),
            (3, 0, 333)]
    mask = tuple(np.array(c, dtype=np.int64) for c in zip(*rows))
    q = [(k, None, None) for k in range(4)]
    for w in (0, 16, 60, 61, 80):
        # output widths put the same rows on output line ends, chunk ends and tile ends of the written bytes
        run(blob, parsed, q, width=w, mask=mask, mode=mode, char="x")
    run(blob, parsed, q, minus=[True, True, True, True], width=60, mask=mask, mode=mode)
    run(blob, parsed, q, minus=[False, True, False, True], width=64, mask=mask, mode=mode, upper=True)
    # intervals: rows before, across and behind them
    iq = [(0, 17, 29), (0, 21, 23), (0, 30, 60), (0, 100, 200), (0, tile - 20, tile + 20), (2, 50, 399), (2, 0, 10), (1, 3, 400), (3, 100, 200),
          (0, 19, 19)]
    for minus in (False, True):
        run(blob, parsed, iq, minus=[minus] * len(iq), width=7, headers=["i%d" % k for k in range(len(iq))], mask=mask, mode=mode, char="-")
    # the same rows with mask_mode none change nothing
    run(blob, parsed, q, width=60, mask=mask, mode="none")


# ------------------------------------------------------------------ irregular records
def test_irregular_records_mixed_with_regular_ones(fx):
    rng = np.random.default_rng(17)
    s = [rand_seq(rng, n) for n in (70, 73, 59, 45, 38, 100)]
    lines = lambda x, w: b"".join(x[i:i + w] + b"\n" for i in range(0, len(x), w))
    data = (b">reg0 first\n" + lines(s[0], 20) +
            b">odd line in the middle\n" + s[1][:20] + b"\n" + s[1][20:33] + b"\n" + lines(s[1][33:], 20) +
            b">space inside a line\n" + s[2][:20] + b"\n" + s[2][20:27] + b" " + s[2][27:39] + b"\n" + lines(s[2][39:], 20) +
            b">blank line\n" + s[3][:20] + b"\n\n" + lines(s[3][20:], 20) +
            b">short lines\n" + lines(s[4], 10) +
            b">reg5 last\n" + lines(s[5], 20))
    blob, parsed = built(data)
    assert [x for _, x in parsed] == s
    q = [(k, None, None) for k in range(6)]
    for w in (0, 1, 16, 20, 60):
        run(blob, parsed, q, width=w)
    run(blob, parsed, q + q[::-1], minus=[k % 2 == 0 for k in range(12)], width=13, upper=True)
    mask = tuple(np.array(c, dtype=np.int64) for c in zip((1, 15, 40), (3, 0, 21), (4, 9, 11), (5, 0, 100)))
    for mode in ("soft", "hard", "upper"):
        run(blob, parsed, q, minus=[False, True, False, True, False, True], width=20, mask=mask, mode=mode)
    # Intervals.  Of a record that is not line-regular (1, 3) and of one whose lines are short (4) they are cut from the despaced
    # letters; records 0 and 5 go by the line arithmetic in the same call.
    iq = [(r, a, b) for r in (0, 1, 3, 4, 5) for a, b in ((0, 5), (3, 30), (19, 21), (20, 38), (11, 11), (0, len(s[r])), (len(s[r]) - 1, len(s[r])))]
    for minus in (False, True):
        run(blob, parsed, iq, minus=[minus] * len(iq), width=8, headers=["%d" % k for k in range(len(iq))])
    # An interval of the record with a space inside a line: its letters are what the fetch path returns for it (flags 0)
    sq = [(2, a, b) for a, b in ((0, 59), (0, 60), (5, 25), (20, 30), (26, 28), (27, 60), (30, 41))]
    ids, a, b = (np.array(c, dtype=np.int64) for c in zip(*sq))
    fb, fo, fl = blob.fasta_fetch(ids, a, b)
    pieces = [fb[fo[k]:fo[k] + fl[k]].tobytes() for k in range(len(sq))]
    for minus in (False, True):
        got = blob.fasta_format_alloc(len(sq), ids, a, b, flags=6 if minus else 0, width=9)
        want = T.records(pieces, [parsed[2][0]] * len(sq), [(k, None, None) for k in range(len(sq))], [minus] * len(sq), 9, [], "none", "N", False, 0)
        same(got, want, "space record")
        assert got[3] == sum(len(p) for p in pieces)


# ------------------------------------------------------------------ the Fasta methods: round trips
def letters_only(rng, n):
    return rand_seq(rng, n, np.frombuffer(b"ACGTacgtNnRYKMrykm", dtype=np.uint8))


@pytest.fixture()
def gen_file(tmp_path):
    rng = np.random.default_rng(23)
    lens = [500, 0, 60, 61, 59, 1, 12345, 120, 7]
    recs = [("seq%d description %d" % (k, n), letters_only(rng, n)) for k, n in enumerate(lens)]
    data = T.write_fasta(recs, 60)
    p = tmp_path / "gen.fa"
    p.write_bytes(data)
    return str(p), data, recs


def test_round_trip_same_width_is_the_file(fx, gen_file):
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    buf, offs = fa.records(width=60)
    assert buf.tobytes() == data and offs[-1] == len(data) and offs.size == len(recs) + 1
    again = fx.Fasta(path)                                    # the index file exists now: the table comes from its rows
    buf2, offs2 = again.records(width=60)
    assert buf2.tobytes() == data and offs2.tolist() == offs.tolist()
    names = [h.split()[0] for h, _ in recs]
    buf3, _ = again.records(names[2:5], width=60)
    assert buf3.tobytes() == data[offs[2]:offs[5]]


def test_write_reopen_gives_the_same_sequences(fx, gen_file, tmp_path):
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    out = str(tmp_path / "w37.fa")
    r = fa.write(out, width=37)
    assert r == {"records": len(recs), "bases": sum(len(s) for _, s in recs), "dropped": 0}
    back = fx.Fasta(out)
    assert len(back) == len(recs)
    for k, (h, s) in enumerate(recs):
        assert back[k].seq == s.decode() and back[k].description == h
    assert max(len(l) for l in open(out, "rb").read().split(b"\n") if not l.startswith(b">")) == 37


def test_uppercase_then_soft_mask_restores_the_file(fx, gen_file):
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    up = fx.Fasta(path, uppercase=True)
    plain = fa.records()
    assert up.records()[0].tobytes() == T.records([s for _, s in recs], [h for h, _ in recs], [(k, None, None) for k in range(len(recs))],
                                                   [False] * len(recs), 60, [], "none", "N", True, 0)[0]
    masked = up.records(mask=fa.class_runs("masked"))
    assert masked[0].tobytes() == plain[0].tobytes() and masked[1].tolist() == plain[1].tolist()
    hard = fa.records(mask=fa.class_runs("masked"), mask_mode="hard", mask_char="N", width=0)
    want = T.records([bytes(78 if 97 <= c <= 122 else c for c in s) for _, s in recs], [h for h, _ in recs],
                     [(k, None, None) for k in range(len(recs))], [False] * len(recs), 0, [], "none", "N", False, 0)
    same(hard, want)


def test_intervals_at_width_0_are_subseq_records(fx, gen_file):
    from pyfastx_amd import cli
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    rng = np.random.default_rng(29)
    pick = [k for k, (_, s) in enumerate(recs) if len(s) > 0]
    ids = rng.choice(pick, 300)
    L = np.array([len(recs[i][1]) for i in ids])
    starts = (rng.random(300) * L).astype(np.int64) + 1      # 1-based, inclusive
    ends = np.minimum(starts + rng.integers(0, 200, 300), L)
    chroms = ["seq%d" % i for i in ids]
    buf, offs = fa.records(chroms, starts - 1, ends, width=0)
    assert buf.tobytes() == cli.subseq_records(fa, chroms, starts, ends)
    byid, _ = fa.records(ids, starts - 1, ends, width=0)     # ids instead of names: the same auto headers
    assert byid.tobytes() == buf.tobytes()
    neg, _ = fa.records(chroms[:3], (starts - 1)[:3], ends[:3], strand=["-", "+", "-"], width=0)
    assert neg.tobytes().split(b"\n")[0] == (">%s:%d-%d(-)" % (chroms[0], starts[0], ends[0])).encode()
    assert neg.tobytes().split(b"\n")[2] == (">%s:%d-%d" % (chroms[1], starts[1], ends[1])).encode()


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("fn", ["test.fa", "test.fa.gz"])
def test_fixtures(fx, tmp_path, fn):
    shutil.copy(os.path.join(DATA, fn), tmp_path / fn)
    fa = fx.Fasta(str(tmp_path / fn))
    n = len(fa)
    seqs = [fa[i].seq.encode("latin-1") for i in range(n)]
    hdrs = [fa[i].description for i in range(n)]
    whole = [(k, None, None) for k in range(n)]
    same(fa.records(width=60), T.records(seqs, hdrs, whole, [False] * n, 60, [], "none", "N", False, 0), fn)
    same(fa.records(strand="-", width=80, uppercase=True), T.records(seqs, hdrs, whole, [True] * n, 80, [], "none", "N", True, 0), fn)
    rng = np.random.default_rng(31)
    ids = rng.integers(0, n, 2000)
    L = np.array([len(seqs[i]) for i in ids])
    a = (rng.random(2000) * L).astype(np.int64)
    b = np.minimum(a + rng.integers(0, 300, 2000), L)
    minus = rng.random(2000) < 0.5
    names = [fa[int(i)].name for i in ids]
    from pyfastx_amd import fasta_out
    want_h = [h.decode() for h in fasta_out.auto_headers(names, a, b, minus)]
    runs = fa.class_runs(letters="Gg")
    rows = list(zip(*(np.asarray(c).tolist() for c in fasta_out.merge_intervals(runs.ids, runs.starts, runs.stops))))
    got = fa.records(ids, a, b, strand=["-" if m else "+" for m in minus], width=50, mask=runs, mask_mode="hard", mask_char="n")
    same(got, T.records(seqs, want_h, list(zip(ids.tolist(), a.tolist(), b.tolist())), minus.tolist(), 50, rows, "hard", "n", False, 0), fn)


# ------------------------------------------------------------------ write in batches
def test_write_batches_counts_and_dropped(fx, gen_file, tmp_path):
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    n = len(recs)
    out = str(tmp_path / "b.fa")
    r = fa.write(out, width=60, batch_bytes=700)              # record 6 (12 345 letters) is larger than a batch and goes alone
    assert open(out, "rb").read() == data and r == {"records": n, "bases": sum(len(s) for _, s in recs), "dropped": 0}
    r = fa.write(out, width=10, min_len=60, batch_bytes=100)
    keep = [k for k, (_, s) in enumerate(recs) if len(s) >= 60]
    want = T.records([s for _, s in recs], [h for h, _ in recs], [(k, None, None) for k in range(n)], [False] * n, 10, [], "none", "N", False, 60)
    assert open(out, "rb").read() == want[0]
    assert r == {"records": len(keep), "bases": sum(len(recs[k][1]) for k in keep), "dropped": n - len(keep)}
    # intervals, custom headers and a mask through the batches
    ids = [0, 6, 6, 3, 0, 2]
    a, b = [10, 0, 5000, 0, 499, 1], [300, 12345, 5100, 61, 500, 60]
    hdrs = ["c%d" % k for k in range(6)]
    mask = ([0, 6], [0, 100], [250, 6000])
    r = fa.write(out, ids, a, b, strand=["+", "-", "+", "-", "+", "-"], width=70, mask=mask, mask_mode="upper", headers=hdrs, batch_bytes=400)
    want = T.records([s for _, s in recs], hdrs, list(zip(ids, a, b)), [False, True] * 3, 70, list(zip(*mask)), "upper", "N", False, 0)
    assert open(out, "rb").read() == want[0] and r["records"] == 6 and r["bases"] == sum(y - x for x, y in zip(a, b))
    with pytest.raises(ValueError):
        fa.write(out, batch_bytes=0)


# ------------------------------------------------------------------ errors
def test_errors_name_the_row_and_allocate_nothing(fx, gen_file):
    from pyfastx_amd import _lib
    path, data, recs = gen_file
    fa = fx.Fasta(path)
    n = len(recs)
    with pytest.raises(KeyError, match="nope does not exist in fasta file"):
        fa.records(["seq0", "nope"])
    with pytest.raises(IndexError, match="query 2") as e:
        fa.records([0, 1, n, -1])
    assert e.value.first_bad == 2
    with pytest.raises(IndexError, match="query 1"):
        fa.records([0, n], [0, 0], [1, 1])
    with pytest.raises(ValueError, match="query 3") as e:
        fa.records([0, 0, 2, 2, 0], [0, 5, 0, 0, 7], [500, 5, 60, 61, 3])
    assert e.value.first_bad == 3
    with pytest.raises(ValueError, match="query 4"):
        fa.records([0, 0, 2, 2, 0], [0, 5, 0, 0, 7], [500, 5, 60, 60, 3])
    with pytest.raises(ValueError, match="query 0"):
        fa.records([0], [-1], [3])
    for kw in (dict(width=-1), dict(width=2.5), dict(mask_mode="lower"), dict(mask_char="NN"), dict(min_len=-1), dict(strand="x"),
               dict(headers=["just one"]), dict(mask=([0], [1]))):
        with pytest.raises(ValueError):
            fa.records(**kw)
    with pytest.raises(ValueError):
        fa.records([0, 1], [0, 0], None)
    # the C entry itself: what it rejects leaves both output pointers NULL
    blob, _ = built(data)
    L = _lib.lib()
    i64 = lambda x: np.array(x, dtype=np.int64)

    def call(h, nq, ids=None, a=None, b=None, width=60, mask=None, mode=0):
        dst, offs, kept, bases, bad = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
        m = [None] * 3 if mask is None else [i64(c) for c in mask]
        p = lambda x: None if x is None else x.ctypes.data
        rc = L.fx_fasta_format_alloc(h, nq, p(ids), p(a), p(b), 0, None, width, None, None, 0 if mask is None else m[0].size, p(m[0]), p(m[1]), p(m[2]),
                                     mode, 78, 0, C.byref(dst), C.byref(offs), C.byref(kept), C.byref(bases), C.byref(bad))
        assert rc == 0 or (dst.value is None and offs.value is None)
        if rc == 0:
            L.fx_pinned_free(dst); L.fx_pinned_free(offs)
        return rc, bad.value

    live = fa.records()                                       # a block that is out while the calls below fail: it stays as it is
    assert L.fx_pinned_holds(live[0].ctypes.data, live[0].nbytes) == 1
    assert call(blob._h, n) == (0, -1)
    assert call(blob._h, 3, i64([0, n, -1])) == (_lib.FX_ERANGE, 1)
    assert call(blob._h, 3, i64([0, 2, 2]), i64([0, 0, 61]), i64([500, 60, 60])) == (_lib.FX_ERANGE, 2)
    assert call(blob._h, n, width=-1)[0] == _lib.FX_EINVAL
    assert call(blob._h, 2, None, i64([0, 0]), i64([1, 1]))[0] == _lib.FX_EINVAL      # intervals need ids
    assert call(blob._h, n, mask=([0, 0], [10, 5], [12, 8]), mode=1) == (_lib.FX_EINVAL, 1)        # unsorted
    assert call(blob._h, n, mask=([0, 0], [5, 9], [10, 12]), mode=1) == (_lib.FX_EINVAL, 1)        # overlapping
    assert call(blob._h, n, mask=([2, 0], [0, 0], [5, 5]), mode=2) == (_lib.FX_EINVAL, 1)          # records out of order
    assert call(blob._h, n, mask=([0, 2], [0, 50], [5, 61]), mode=3) == (_lib.FX_EINVAL, 1)        # past the record's end
    assert call(blob._h, n, mask=([0, n], [0, 0], [5, 0]), mode=3) == (_lib.FX_EINVAL, 1)          # an unknown record
    assert call(blob._h, n, mask=([0, 0], [10, 5], [12, 8]), mode=0) == (0, -1)                    # FX_MASK_NONE ignores the rows
    assert call(blob._h, n, mask=([0, 0, 0], [5, 10, 10], [10, 10, 12]), mode=1) == (0, -1)        # touching and empty rows are fine
    assert call(blob._h, n, mode=4)[0] == _lib.FX_EINVAL
    fresh = _lib.Blob.from_bytes(data)
    assert call(fresh._h, 1)[0] == _lib.FX_ESTATE                                                  # before the build
    shard = _lib.Blob.from_bytes(data)
    shard.set_shard(4096, ord("\n"), True)
    shard.fasta_build()
    assert call(shard._h, 1)[0] == _lib.FX_EINVAL
    # a table installed from index rows holds no header lines: the own-header path says so, custom headers work
    t = blob.fasta_table(n)
    bare = _lib.Blob.from_bytes(data)
    bare.fasta_set_table(t["boff"], t["blen"], t["slen"], t["llen"], t["elen"], t["norm"])
    assert call(bare._h, n)[0] == _lib.FX_ESTATE
    from pyfastx_amd import fasta_out
    hdr, hdr_off = fasta_out.pack_headers([h for h, _ in recs], n)
    got = bare.fasta_format_alloc(n, None, None, None, width=60, hdr=hdr, hdr_off=hdr_off)
    assert got[0].tobytes() == data
    assert L.fx_pinned_holds(live[0].ctypes.data, live[0].nbytes) == 1 and live[0].tobytes() == data
