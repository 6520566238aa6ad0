"""CPU: the host side of the BGZF writers (pyfastx_amd/bgzf.py) on streams built here with zlib and hand-made headers, the
`compress` argument rule, and the encoder's code construction (fx_deflate_code_lengths: the routine the kernel runs, on the host)."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from pyfastx_amd import bgzf

# the 28 bytes htslib writes at the end of every BGZF file
HTSLIB_EOF = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"


def member(payload, lvl=6):
    c = zlib.compressobj(lvl, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    size = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + b"\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + body +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def stream(data, lvl=6):
    return b"".join(member(data[i:i + bgzf.MEMBER], lvl) for i in range(0, len(data), bgzf.MEMBER))


DATA = np.random.default_rng(5).integers(65, 70, 3 * bgzf.MEMBER + 1234, dtype=np.uint8).tobytes()


def test_eof_is_the_member_htslib_writes():
    assert bgzf.EOF == HTSLIB_EOF and len(bgzf.EOF) == 28
    assert gzip.decompress(bgzf.EOF) == b""
    coff, clen, isize, crc = bgzf.members(bgzf.EOF)
    assert (coff.tolist(), clen.tolist(), isize.tolist(), crc.tolist()) == ([0], [28], [0], [0])


@pytest.mark.parametrize("lvl", [0, 1, 6])
def test_members_of_a_multi_member_stream(lvl):
    s = stream(DATA, lvl)
    coff, clen, isize, crc = bgzf.members(s)
    assert coff.size == 4 and coff[0] == 0 and (coff[1:] == np.cumsum(clen)[:-1]).all() and coff[-1] + clen[-1] == len(s)
    assert isize.tolist() == [bgzf.MEMBER] * 3 + [1234]
    assert crc.tolist() == [zlib.crc32(DATA[i:i + bgzf.MEMBER]) for i in range(0, len(DATA), bgzf.MEMBER)]
    assert gzip.decompress(s) == DATA


def test_members_with_the_eof_block_and_of_nothing():
    s = stream(DATA) + bgzf.EOF
    coff, clen, isize, _ = bgzf.members(s)
    assert coff.size == 5 and clen[-1] == 28 and isize[-1] == 0 and coff[-1] == len(s) - 28
    assert [a.size for a in bgzf.members(b"")] == [0, 0, 0, 0]


def test_truncated_and_corrupt_headers_raise():
    s = stream(DATA)
    second = int(bgzf.members(s)[0][1])
    for cut in (len(s) - 1, second + 17, second + 1, 5):
        with pytest.raises(ValueError):
            bgzf.members(s[:cut])
    for at, byte in ((0, 0x1e), (1, 0), (2, 7), (3, 0), (10, 8), (12, ord("X")), (13, ord("X")), (14, 4), (second, 0), (second + 12, 0)):
        bad = bytearray(s)
        bad[at] = byte
        with pytest.raises(ValueError):
            bgzf.members(bytes(bad))
    bad = bytearray(s)                                        # a BSIZE that points past the end, one too small to hold a member
    bad[second + 16:second + 18] = b"\xff\xff"
    with pytest.raises(ValueError):
        bgzf.members(bytes(bad)[:second + 4000])
    bad[16:18] = struct.pack("<H", 20)
    with pytest.raises(ValueError):
        bgzf.members(bytes(bad))
    with pytest.raises(ValueError):
        bgzf.members(gzip.compress(b"plain gzip, no BC subfield"))


def test_virtual_offsets_at_a_member_seam():
    s = stream(DATA)
    coff = bgzf.members(s)[0]
    rec = np.array([0, 1, bgzf.MEMBER - 1, bgzf.MEMBER, bgzf.MEMBER + 1, 2 * bgzf.MEMBER, len(DATA) - 1], dtype=np.int64)
    v = bgzf.virtual_offsets(coff, rec)
    assert v.dtype == np.uint64
    assert (v & np.uint64(0xFFFF)).tolist() == [0, 1, bgzf.MEMBER - 1, 0, 1, 0, 1233]
    assert (v >> np.uint64(16)).tolist() == [0, 0, 0, int(coff[1]), int(coff[1]), int(coff[2]), int(coff[3])]
    for x, r in zip(v.tolist(), rec.tolist()):                 # what a reader does with one: seek, inflate that member, skip uoffset
        c, u = x >> 16, x & 0xFFFF
        d = zlib.decompressobj(-15)
        assert d.decompress(s[c + 18:])[u:u + 1] == DATA[r:r + 1]
    assert bgzf.virtual_offsets(coff, np.zeros(0, dtype=np.int64)).size == 0
    with pytest.raises(ValueError):
        bgzf.virtual_offsets(coff, [4 * bgzf.MEMBER])
    with pytest.raises(ValueError):
        bgzf.virtual_offsets(coff, [-1])


def test_the_compress_argument_rule():
    assert [bgzf.level_of(c) for c in (None, False, True, 0, 1, 2, np.int64(1))] == [None, None, 2, 0, 1, 2, 1]
    for bad in (3, -1, "gz", 1.0, b"1", [1]):
        with pytest.raises(ValueError):
            bgzf.level_of(bad)


def test_tally_writes_the_eof_member_once(tmp_path):
    s1, s2 = stream(DATA[:70000]), stream(DATA[70000:])
    with open(tmp_path / "t.gz", "wb") as f:
        t = bgzf.Tally(f)
        for s in (s1, s2):
            t.add(np.frombuffer(s, dtype=np.uint8), np.append(bgzf.members(s)[0], len(s)))
        r = t.finish()
    raw = (tmp_path / "t.gz").read_bytes()
    assert raw == s1 + s2 + bgzf.EOF and gzip.decompress(raw) == DATA
    assert r == {"compressed_bytes": len(raw), "members": bgzf.members(raw)[0].size}


# ---- the code construction: lengths within the limit, Kraft with equality, the rarest symbols the longest codes
def kraft(lens, limit):
    return sum(1 << (limit - int(v)) for v in lens if v)


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def steep(n):
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2] + 1)
    return f[:n]


def check_code(freq, limit):
    from pyfastx_amd import _lib
    freq = np.asarray(freq, dtype=np.uint32)
    lens, codes = _lib.deflate_code_lengths(freq, limit)
    used = np.flatnonzero(freq)
    assert (lens[freq == 0] == 0).all() and (lens[used] >= 1).all() and lens.max() <= limit
    if used.size >= 2:
        assert kraft(lens, limit) == 1 << limit, (kraft(lens, limit), lens.tolist())
        order = sorted(used.tolist(), key=lambda s: (int(freq[s]), s))
        assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:])), "a rarer symbol has the shorter code"
    # canonical: codes of one length ascend with the symbol, and no code is a prefix of another (MSB first = the stored code reversed)
    msb = {int(s): format(int(codes[s]), "0%db" % lens[s])[::-1] for s in used}
    words = sorted(msb.values())
    assert len(set(words)) == len(words) and not any(b.startswith(a) for a, b in zip(words, words[1:]))
    nxt, code = {}, 0
    per = np.bincount(lens[used], minlength=17)
    for length in range(1, 16):
        code = (code + (int(per[length - 1]) if length > 1 else 0)) << 1
        nxt[length] = code
    for s in used.tolist():
        assert int(msb[s], 2) == nxt[int(lens[s])], s
        nxt[int(lens[s])] += 1
    return lens


def test_code_lengths_are_limited_and_complete():
    # Fibonacci counts beside the end-of-block code's 1 tie their way into a tree of depth 12 (three 1s at the bottom); counts
    # that grow by f[k] = f[k-1] + f[k-2] + 1 from 1, 2 stay a chain whatever is merged first: 20 of them fit one member and
    # reach depth 20 unlimited, so the limit has to act
    f = np.zeros(286, dtype=np.uint32)
    f[:23] = fib(23)
    f[256] = 1
    assert check_code(f, 15).max() == 12
    f[:23] = 0
    f[:20] = steep(20)
    lens = check_code(f, 15)
    assert lens.max() == 15 and int(f.sum()) <= 65280 + 1
    f[:24] = 1 << np.arange(24)
    assert check_code(f, 15).max() == 15
    check_code(steep(19), 7)                                  # the code-length alphabet, limit 7
    check_code(fib(19), 7)
    rng = np.random.default_rng(11)
    for _ in range(30):
        g = rng.integers(0, 4, 286) * rng.integers(1, 5000, 286)
        g[256] = 1
        check_code(g, 15)
        check_code(rng.integers(0, 1000, 30) * rng.integers(0, 2, 30), 15)
        check_code(np.maximum(rng.integers(0, 300, 19) * rng.integers(0, 2, 19), np.eye(19, dtype=np.int64)[3] + np.eye(19, dtype=np.int64)[17]), 7)
    check_code(np.ones(286), 15)
    check_code(np.ones(128), 7)                               # every code of the limit's length


def test_degenerate_alphabets():
    one = np.zeros(30, dtype=np.uint32)
    assert check_code(one, 15).max() == 0                     # no symbol: no length (the encoder then sends one code of length 1)
    one[7] = 99
    assert check_code(one, 15).tolist() == [0] * 7 + [1] + [0] * 22
    two = np.zeros(286, dtype=np.uint32)
    two[65], two[256] = 65280, 1                              # one distinct byte and the end of the block
    lens = check_code(two, 15)
    assert lens[65] == 1 and lens[256] == 1 and lens.sum() == 2


def test_code_lengths_argument_errors():
    from pyfastx_amd import _lib
    for freq, limit in ((np.ones(289), 15), (np.ones(10), 16), (np.ones(10), 0), (np.ones(9), 3)):
        with pytest.raises(_lib.FxError) as e:
            _lib.deflate_code_lengths(freq, limit)
        assert e.value.code == _lib.FX_EINVAL


def test_entries_declared_bound_and_their_errors_without_a_device():
    import ctypes as C
    from pyfastx_amd import _lib
    L = _lib.lib()
    for name, nargs in (("fx_bgzf_compress", 8), ("fx_fastq_format_bgzf_alloc", 15), ("fx_fasta_format_bgzf_alloc", 26),
                        ("fx_fastq_pair_merge_bgzf_alloc", 15), ("fx_deflate_code_lengths", 5)):
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs, name
    names = [L.fx_prof_name(i).decode() for i in range(L.fx_prof_count())]
    for k in ("k_bgzf_store", "k_bgzf_deflate", "k_bgzf_crc_put", "k_bgzf_scan", "k_bgzf_pack"):
        assert k in names
    src = np.frombuffer(b"ACGT" * 10, dtype=np.uint8)
    out = lambda: (C.c_void_p(1), C.c_int64(7), C.c_void_p(1), C.c_int64(7))
    for level, n in ((7, 40), (-1, 40), (2, -1)):             # a bad level or size is FX_EINVAL with or without a device, outputs null
        dst, nb, moff, nm = out()
        assert L.fx_bgzf_compress(src.ctypes.data, n, level, 0, C.byref(dst), C.byref(nb), C.byref(moff), C.byref(nm)) == _lib.FX_EINVAL
        assert dst.value is None and moff.value is None and nb.value == 0 and nm.value == 0
    dst, nb, moff, nm = out()
    assert L.fx_bgzf_compress(src.ctypes.data, 40, 2, 0, None, C.byref(nb), C.byref(moff), C.byref(nm)) == _lib.FX_EINVAL
    if L.fx_device_count() <= 0:
        assert L.fx_bgzf_compress(src.ctypes.data, 40, 2, 0, C.byref(dst), C.byref(nb), C.byref(moff), C.byref(nm)) == _lib.FX_EDEVICE
        assert dst.value is None and moff.value is None
        with pytest.raises(_lib.FxError) as e:
            bgzf.compress(b"ACGT")
        assert e.value.code == _lib.FX_EDEVICE
    with pytest.raises(ValueError):
        bgzf.compress(b"ACGT", level=3)
    z = [C.c_void_p() for _ in range(3)]
    c = [C.c_int64() for _ in range(5)]
    rc = L.fx_fastq_format_bgzf_alloc(None, None, 0, None, None, 0, 2, *map(C.byref, z), *map(C.byref, c))
    assert rc == _lib.FX_EINVAL                                # a null handle
