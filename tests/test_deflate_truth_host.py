"""-m "not gpu": the deflate corpus of deflate_truth.py is valid -- zlib inflates every member to the bytes kept with it -- and
every class has the shape it is named for, by walk() alone; walk() and encode() are checked against zlib.  What the figures
were when this was written stands next to the assertion; the assertions are the properties."""
import gzip
import zlib

import numpy as np
import pytest

import deflate_truth as D


class _Rows(dict):
    """(class, member) -> walk() of it; every member is walked once, when the first test asks."""
    def __missing__(self, key):
        self.update({(k, i): D.walk(cd) for k, i, cd, raw in D.all_members()})
        return self[key]

    def values(self):
        self[D.NAMES[0], 0]
        return dict.values(self)


ROWS = _Rows()


def _rows(name):
    return [r for i in range(len(D.CORPUS[name])) for r in ROWS[name, i]]


def test_second_level_rule_on_trees_worked_by_hand():
    """The fixed literal/length tree (RFC 1951 3.2.6) has 112 codes of 9 bits, 110010000 .. 111111111: at 8 root bits they pair
    up under 56 prefixes of two entries each, at 9 and 10 root bits nothing is left over.  Lengths 1, 2, 3, 3 + ... : one
    prefix, as wide as its LONGEST code, not one table per code; two prefixes of different depth do not share."""
    assert D.second_level(D.FIXED_LL, 8) == 112 and D.second_level(D.FIXED_LL, 9) == 0 and D.second_level(D.FIXED_LL, 10) == 0
    assert D.second_level(D.FIXED_DL, 6) == 0 and D.second_level(D.FIXED_DL, 4) == 30      # thirty codes of 5 bits: 15 pairs
    # codes 0, 10, 110, 1110, 11110, 11111: at 2 root bits only the prefix 11 has longer codes, the longest of 5 bits: 8 entries
    assert D.second_level([1, 2, 3, 4, 5, 5], 2) == 8 and D.second_level([1, 2, 3, 4, 5, 5], 3) == 4 and D.second_level([1, 2, 3, 4, 5, 5], 5) == 0
    # 00, 01, 100, 101, 1100, 1101, 1110, 1111 at 2 root bits: prefix 10 needs 2 entries, prefix 11 needs 4
    assert D.second_level([2, 2, 3, 3, 4, 4, 4, 4], 2) == 6
    # an incomplete tree (one code of one bit) and an empty one need nothing
    assert D.second_level([1], 6) == 0 and D.second_level([0, 0], 6) == 0
    # symbols take their codes in symbol order within a length (3.2.2): B = 0, A = 10, C = 110, D = 111
    assert D.canonical([2, 1, 3, 3]) == {1: 0, 0: 2, 2: 6, 3: 7}


def test_every_member_inflates_to_its_bytes_with_zlib():
    n = 0
    for k, i, cd, raw in D.all_members():
        assert zlib.decompress(cd, -15) == raw, (k, i)
        assert len(raw) <= 65536 and len(cd) <= 65510, (k, i)
        assert sum(r["out"] for r in ROWS[k, i]) == len(raw), (k, i)
        assert [r["final"] for r in ROWS[k, i]] == [0] * (len(ROWS[k, i]) - 1) + [1]
        n += 1
    assert n == 31 and tuple(D.CORPUS) == D.NAMES and len(D.NAMES) == 23


@pytest.mark.parametrize("name", D.NAMES)
def test_a_class_is_a_valid_gzip_file(name):
    members = D.CORPUS[name]
    assert gzip.decompress(b"".join(D.member(cd, raw) for cd, raw in members)) == b"".join(raw for _, raw in members)


@pytest.mark.parametrize("name", ["zipf_default", "zipf_huffman_only", "zipf_filtered"])
def test_zipf_trees_need_large_second_level_tables(name):
    """Measured: literal codes of 14 bits; 172 / 198 / 186 entries at 10 root bits in the largest block; 238 .. 268 at 8 root
    bits, every block over the serial decoder's POOL = 96 by the literal tree alone; distance codes of 10 bits (default)."""
    rows = _rows(name)
    assert all(r["type"] == 2 for r in rows)
    assert max(r["lit_max"] for r in rows) >= 13
    assert max(r["sub_wave"][0] for r in rows) > 128 and max(r["sub_wave"][0] for r in rows) < 384
    assert all(r["sub_serial"][0] > 96 for r in rows)
    if name == "zipf_default":
        assert max(r["dist_max"] for r in rows) > 8 and max(r["sub_wave"][1] for r in rows) > 0
    if name == "zipf_huffman_only":
        assert all(r["max_len"] == 0 for r in rows)


def test_fifteen_bit_codes():
    """fib15: 65280 bytes of 23 values with Fibonacci frequencies; a 15-bit literal code (measured: in the first block).
    dist15: distance codes of 1 .. 15 bits, the two 15-bit ones (distances 129 .. 256) used; 128 entries at 8 root bits."""
    assert max(r["lit_max"] for r in _rows("fib15")) == 15
    (r,) = _rows("dist15")
    assert r["dist_max"] == 15 and r["dl"] == list(range(1, 16)) + [15] and r["max_dist"] > 192 and r["sub_wave"][1] == 128
    assert r["sub_serial"][1] > 96                         # and the serial decoder's pool cannot hold it (512)


def test_words_far_has_matches_up_to_the_limit_of_zlib():
    """Measured: largest distances 32468, 32468, 32492 at levels 1, 6, 9 (zlib's limit: 32768 - 262 = 32506); literal codes of 14, 14, 13 bits."""
    for i in range(3):
        rows = ROWS["words_far", i]
        assert 32000 < max(r["max_dist"] for r in rows) <= 32506 and max(r["lit_max"] for r in rows) >= 13
    assert len(D.CORPUS["words_far"]) == 3


def test_memlevel1_is_many_short_blocks():
    """Measured: 198 blocks of 128 symbols (127 and the end-of-block code), the last of 47; under 1500 bits each."""
    rows = _rows("memlevel1")
    assert len(D.CORPUS["memlevel1"]) == 1 and len(rows) > 100
    assert all(r["nsym"] <= 128 for r in rows) and sum(r["nsym"] == 128 for r in rows) >= len(rows) - 1


@pytest.mark.parametrize("name,between", [("sync_flush", [0]), ("full_flush", [0]), ("partial_flush", [1]), ("z_block", [])])
def test_flush_classes_have_empty_blocks_in_the_middle(name, between):
    """Nine dynamic blocks, each followed by an empty stored block (sync, full) or an empty fixed block of ten bits (partial) or
    by nothing (Z_BLOCK); every stream ends in an empty final fixed block."""
    rows = _rows(name)
    assert [r["type"] for r in rows] == ([2] + between) * 9 + [1]
    for r in rows:
        if r["type"] != 2:
            assert r["out"] == 0 and r["nsym"] == (1 if r["type"] == 1 else 0)
        else:
            assert r["out"] in (7000, 4000)
    assert rows[-1]["final"] == 1 and sum(r["out"] for r in rows) == 60000


def test_rle_fixed_and_stored_mix():
    assert all(r["type"] == 2 and r["max_dist"] <= 1 for r in _rows("rle")) and max(r["max_len"] for r in _rows("rle")) > 3
    assert [r["type"] for r in _rows("fixed_big")] == [1] and _rows("fixed_big")[0]["max_len"] == 258
    rows = _rows("stored_mix")
    assert [(r["type"], r["final"]) for r in rows] == [(0, 0), (2, 0), (0, 0), (1, 1)]
    assert rows[0]["out"] == 1000 and rows[2]["out"] == 0 and (rows[3]["out"], rows[3]["nsym"]) == (3, 4)
    assert rows[1]["max_dist"] == 1000                     # the dynamic block copies from the stored one


def test_isize_edge():
    sizes = [len(raw) for _, raw in D.CORPUS["isize_edge"]]
    ends = [ROWS["isize_edge", i][-1]["last_tok"] for i in range(len(sizes))]
    assert sizes[:2] == [65535, 65536] and ends[:2] == ["match", "lit"]
    assert (65536, "match") in zip(sizes, ends)            # a match that ends at the last bit of a full match map


def test_streams_zlib_does_not_write():
    (r,) = _rows("dist_32768")
    assert (r["max_dist"], r["max_len"], r["last_tok"]) == (32768, 258, "match") and r["out"] == 32768 + 3 + 258 + 3
    assert r["sub_serial"][0] > 96                         # 256 literal codes of 9 bits: the serial decoder's canonical walk again
    a, b = _rows("repeat_across_hlit")
    assert a["hlit_cross"] == 16 and b["hlit_cross"] == 18
    assert a["ll"][-3:] == [4, 4, 4] and a["dl"][:3] == [4, 4, 4] and b["ll"][-28:] == [0] * 28 and b["dl"][:5] == [0, 0, 0, 0, 2]
    assert all(r["hlit_cross"] is None for k in D.CORPUS if k != "repeat_across_hlit" for r in _rows(k))     # zlib never does
    a, b = _rows("one_dist_code")
    assert a["dl"] == [1] and a["max_dist"] == 1 and a["max_len"] == 258 and b["dl"] == [0] and b["max_len"] == 0


def _all_complete_codes(nsym, maxbits):
    """Every complete canonical code of at most nsym symbols and maxbits bits, as its lengths in rising order."""
    def go(n, space, syms, lens):                          # space: what is left of the code space, in units of 2 ** -maxbits
        if space == 0:
            yield lens
        w = 1 << (maxbits - min(n, maxbits))
        if n > maxbits or space == 0 or space > syms * w:  # (what is left cannot be filled by codes this long or longer)
            return
        for c in range(0, min(syms, space // w) + 1):
            yield from go(n + 1, space - c * w, syms - c, lens + [n] * c)
    return go(1, 1 << maxbits, nsym, [])


def test_the_search_for_the_largest_demand_is_exhaustive():
    """largest_demand() against plain enumeration where that is possible: every complete code of at most 16 symbols (3 700
    of them, up to 15 bits deep), each one's demand by second_level(), at 3 and at 10 root bits."""
    codes = list(_all_complete_codes(16, 15))
    assert len(codes) > 3000 and all(sum(2.0 ** -n for n in c) == 1.0 for c in codes) and max(map(max, codes)) == 15
    for root in (3, 10):
        assert D.largest_demand(16, root) == max(D.second_level(c, root) for c in codes), root
    assert D.largest_demand(2, 10) == 0 and D.largest_demand(1, 10) < 0        # 0, 1: the only code of two symbols; none of one


def test_greedy_pool_is_the_largest_literal_demand_and_fits():
    """308 second-level entries at 10 root bits: no complete tree of at most 286 symbols needs more (largest_demand(), which
    tries all of them), and greedy_pool's tree needs exactly that.  It is under P_LPOOL = 384, so the wave decoder's hand-over
    reason 1 cannot be produced by a valid stream.  At the serial decoder's 8 root bits the same tree needs 392 of at most 404."""
    (r,) = _rows("greedy_pool")
    assert r["ll"] == D.greedy_lengths() and len(r["ll"]) <= 286 and r["lit_max"] == 15 and r["max_len"] == 226
    assert r["sub_wave"][0] == D.largest_demand(286, 10) == 308 < 384
    assert r["sub_serial"][0] == 392 and D.largest_demand(286, 8) == 404
    assert all(rr["sub_wave"][0] <= 308 for rows in ROWS.values() for rr in rows)
    assert D.largest_demand(30, 8) == 144 < 256            # and the distance pool of the wave decoder (P_DPOOL) holds any distance tree


@pytest.mark.parametrize("name", ["dna", "qual"])
def test_controls_have_no_literal_sub_table(name):
    """Genome text between its runs of N, and quality strings without rare values: every literal/length code fits the wave
    decoder's root table.  Measured: literal codes of 10 bits (dna) and 9 (qual), distance codes of 11 .. 13 bits."""
    rows = _rows(name)
    assert all(r["type"] == 2 and r["sub_wave"][0] == 0 for r in rows)
    print(name, [(r["lit_max"], r["dist_max"], r["sub_wave"]) for r in rows])


@pytest.mark.parametrize("name", ["dna_n_run", "fastq_records"])
def test_controls_from_the_other_bgzf_tests(name):
    """What test_gpu_bgzf.py feeds the decoders, as one member: genome text with a run of N (the rare literal gets a code of 12
    bits: 8 literal sub-table entries), the first 65280 bytes of the FASTQ fixture (13 bits, 18 entries).  Ordinary streams:
    a few sub-table entries, far from the Zipf classes."""
    rows = _rows(name)
    assert len(rows) == 1 and rows[0]["type"] == 2 and rows[0]["out"] == 65280
    assert 0 < rows[0]["sub_wave"][0] <= 32 and rows[0]["sub_wave"][1] <= 32


def test_walk_agrees_with_zlib_on_random_inputs():
    """200 inputs of mixed alphabet, length, level, strategy, memLevel and flushes: walk() parses each to its last byte, its
    blocks make as many bytes as zlib gives back, and no block has more symbols than bytes + 1 or fewer than bytes / 258."""
    rng = np.random.default_rng(200)
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
    types = set()
    for case in range(200):
        n = int(rng.integers(0, 3000))
        alphabet = int(rng.choice([1, 2, 4, 20, 256]))
        raw = rng.integers(0, alphabet, n).astype(np.uint8).tobytes()
        if case % 5 == 0:
            raw = raw[:200] * 9
        level, strategy, mem = int(rng.integers(0, 10)), strategies[int(rng.integers(0, 5))], int(rng.integers(1, 10))
        if case % 3 == 0:
            cd = D._deflate(raw, level, strategy, mem, piece=int(rng.integers(1, 900)), flush=int(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_PARTIAL_FLUSH, zlib.Z_BLOCK])))
        else:
            cd = D._deflate(raw, level, strategy, mem)
        rows = D.walk(cd)
        assert sum(r["out"] for r in rows) == len(raw) == len(zlib.decompress(cd, -15)), case
        assert [r["final"] for r in rows] == [0] * (len(rows) - 1) + [1], case
        for r in rows:
            types.add(r["type"])
            if r["type"]:
                assert r["out"] / 258 <= r["nsym"] - 1 <= r["out"] and r["max_len"] <= 258 and r["max_dist"] <= 32768, case
                assert r["lit_max"] <= 15 and r["dist_max"] <= 15
            if r["type"] == 2:                             # Kraft: zlib's trees are complete, or have a single distance code
                assert sum(2.0 ** -n for n in r["ll"] if n) == 1.0, case
                assert sum(2.0 ** -n for n in r["dl"] if n) in (0.0, 0.5, 1.0), case
    assert types == {0, 1, 2}
    with pytest.raises(ValueError):
        D.walk(D._deflate(b"hello hello hello")[:-1])      # a stream cut short does not parse


def _expand(blocks):
    out = bytearray()
    for blk in blocks:
        if blk["kind"] == "stored":
            out += blk["data"]
            continue
        for t in blk["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                for _ in range(t[0]):
                    out.append(out[-t[1]])
    return bytes(out)


def test_encode_round_trips_through_zlib():
    """Every length 3 .. 258 and a distance from every distance code, in a fixed and in a dynamic block behind a stored one:
    zlib gives back what the tokens say, and walk() reads back the trees and the block structure that went in."""
    rng = np.random.default_rng(9)
    head = bytes(rng.integers(0, 256, 33000).tolist())
    tok = [int(c) for c in rng.integers(0, 256, 50)]
    for n in range(3, 259):
        ds = n % 30
        tok += [(n, D.DIST_BASE[ds] + int(rng.integers(0, 1 << D.DIST_EXTRA[ds]))), int(rng.integers(0, 256))]
    ll = [9] * 256 + [3] + [7] * 16 + [6] * 10 + [5, 5, 5]  # 1/2 + 1/8 + 1/8 + 10/64 + 3/32 = 1
    dl = [5] * 28 + [4, 4]                                  # 28/32 + 2/16 = 1
    for kind in ("fixed", "dynamic"):
        blocks = [dict(kind="stored", data=head), dict(kind=kind, ll=ll, dl=dl, tokens=tok), dict(kind="stored", data=b""),
                  dict(kind=kind, ll=ll, dl=dl, tokens=[1, 2, 3])]
        cd = D.encode(blocks)
        assert zlib.decompress(cd, -15) == _expand(blocks)
        rows = D.walk(cd)
        assert [r["type"] for r in rows] == [0, 1 if kind == "fixed" else 2, 0, 1 if kind == "fixed" else 2]
        assert [r["out"] for r in rows] == [33000, len(_expand(blocks)) - 33003, 0, 3] and rows[1]["nsym"] == len(tok) + 1
        assert rows[1]["max_len"] == 258 and rows[1]["max_dist"] > 24576
        if kind == "dynamic":
            assert rows[1]["ll"] == ll and rows[1]["dl"] == dl
    with pytest.raises(AssertionError):                     # a code-length sequence that does not spell the trees is refused
        D.encode([dict(kind="dynamic", ll=ll, dl=dl, tokens=[1], clseq=ll + dl[:-1] + [5])])
