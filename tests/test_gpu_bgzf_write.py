"""-m gpu: BGZF written on the device (csrc/fx_deflate.hpp): every case of deflate_enc_cases at every level against zlib --
the members walked here, inflated by zlib.decompressobj(-15), CRC and ISIZE against the payload --, size conditions derived
from the payload's order-0 entropy, determinism, clean memory (children with FX_DEBUG_FILL), the compressed writers against
their plain twins and read back through gzip and through this library's BGZF open, and the errors."""
import ctypes as C
import gzip
import hashlib
import json
import math
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_enc_cases
from conftest import DATA

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MEMBER = 65280
HEADER = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"
EOF = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"
CASES = deflate_enc_cases.cases()
LEVELS = (0, 1, 2)
_streams = {}


@pytest.fixture(scope="module")
def fx():
    import pyfastx_amd
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() > 0
    return pyfastx_amd


def compressed(name, level):
    """(stream bytes, member offsets) of a case, made once per module."""
    from pyfastx_amd import _lib
    if (name, level) not in _streams:
        s, moff = _lib.bgzf_compress(CASES[name], level)
        _streams[name, level] = (s.tobytes(), moff.tolist())
    return _streams[name, level]


def walk(stream, data, what, full=True):
    """The members of `stream` against `data`, without pyfastx_amd.bgzf -> [(offset, bytes, payload)].  full: every member but the
    last carries 65280 bytes (one call of the encoder; a file of several batches has a short member at the end of each)."""
    out, at, done = [], 0, 0
    while at < len(stream):
        assert stream[at:at + 16] == HEADER, (what, at)
        size = struct.unpack_from("<H", stream, at + 16)[0] + 1
        assert 28 <= size <= 65536 and at + size <= len(stream), (what, at, size)
        d = zlib.decompressobj(-15)
        payload = d.decompress(stream[at + 18:at + size])
        assert d.eof and d.unused_data == stream[at + size - 8:at + size] and d.unconsumed_tail == b"", (what, at, len(d.unused_data))
        crc, isize = struct.unpack_from("<II", stream, at + size - 8)
        assert isize == len(payload) <= MEMBER and crc == zlib.crc32(payload), (what, at)
        assert payload == data[done:done + len(payload)], (what, at)
        out.append((at, size, payload))
        at += size
        done += len(payload)
    assert done == len(data) and at == len(stream), what
    assert all(1 <= len(p) <= MEMBER for _, _, p in out) and (not full or all(len(p) == MEMBER for _, _, p in out[:-1])), what
    return out


def entropy_cap(payload):
    """ceil(len * (H0 + 1) / 8) + 320 + 26, at most the stored bound len + 31: a Huffman code averages below H0 + 1 bits, 320
    bytes bound the code-length header (316 lengths of at most 7 bits, 19 of 3, 17 bits), 26 are the framing."""
    n = len(payload)
    c = np.bincount(np.frombuffer(payload, dtype=np.uint8), minlength=256)
    c = c[c > 0].astype(np.float64)
    h0 = float(-(c / n * np.log2(c / n)).sum())
    return min(math.ceil(n * (h0 + 1) / 8) + 320 + 26, n + 31)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_member_inflates_to_its_payload(fx, name, level):
    data = CASES[name]
    stream, moff = compressed(name, level)
    mem = walk(stream, data, (name, level))
    assert len(mem) == (len(data) + MEMBER - 1) // MEMBER
    assert moff == [at for at, _, _ in mem] + [len(stream)]
    assert gzip.decompress(stream + EOF) == data
    for at, size, payload in mem:
        print("%s level %d: member at %d: %d -> %d bytes (stored bound %d, entropy cap %d)" % (
            name, level, at, len(payload), size, len(payload) + 31, entropy_cap(payload)))
        assert size <= len(payload) + 31
        if level == 0:
            assert size == len(payload) + 31
        else:
            assert size <= entropy_cap(payload), (name, level, at, size, entropy_cap(payload))


@pytest.mark.parametrize("name", ["period_997_x60", "one_value_1000", "one_value_member"])
def test_matches_are_found(fx, name):
    """Level 2 on the periodic and the one-value payloads: at most half of the entropy cap, which no literal coder reaches."""
    for at, size, payload in walk(compressed(name, 2)[0], CASES[name], name):
        print("%s: %d -> %d bytes, entropy cap %d" % (name, len(payload), size, entropy_cap(payload)))
        assert 2 * size <= entropy_cap(payload)


def test_matches_respect_the_distance_limit(fx):
    """Random bytes repeated at distance 32768 inside one member: matches at the limit itself make it smaller than stored (zlib
    has accepted them in walk); repeated at 32769 every candidate is one too far, the bytes are literals and the member is stored."""
    near = walk(compressed("distance_limit", 2)[0], CASES["distance_limit"], "distance_limit")
    assert [len(p) for _, _, p in near] == [MEMBER, 256]
    print("distance_limit: %d -> %d bytes" % (MEMBER, near[0][1]))
    assert near[0][1] < MEMBER + 31 and near[1][1] == 256 + 31
    far = walk(compressed("past_distance_limit", 2)[0], CASES["past_distance_limit"], "past_distance_limit")
    assert [size for _, size, _ in far] == [MEMBER + 31]
    for level in (0, 1):                                                # without matches both are random bytes
        assert [size for _, size, _ in walk(compressed("distance_limit", level)[0], CASES["distance_limit"], level)] == [MEMBER + 31, 256 + 31]


@pytest.mark.parametrize("level", (1, 2))
def test_fasta_text_no_larger_than_zlib_level_1(fx, level):
    data = CASES["fasta_text"]
    mem = walk(compressed("fasta_text", level)[0], data, "fasta_text")
    ours = sum(size for _, size, _ in mem)
    ref = 0
    for _, _, payload in mem:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(c.compress(payload) + c.flush()) + 26
    print("fasta_text level %d: %d bytes, %.4f of the input; zlib level 1 over the same payloads: %d, %.4f" % (
        level, ours, ours / len(data), ref, ref / len(data)))
    assert ours <= ref


def test_two_calls_give_the_same_bytes(fx):
    from pyfastx_amd import bgzf
    for name in ("fasta_text", "period_997_x60", "file_test.fq", "random_130561", "steep_shuffled", "size_130561"):
        for level in LEVELS:
            assert bgzf.compress(CASES[name], level) == compressed(name, level)[0] == bgzf.compress(CASES[name], level), (name, level)


# ------------------------------------------------------------------ clean memory
_children = {"dead": None, "runs": {}}
TIMEOUT = 120                                                # ends a child that hangs, nothing else


def child(tmp, order, fill):
    if _children["dead"]:
        pytest.fail("no further process is started: " + _children["dead"], pytrace=False)
    if (order, fill) in _children["runs"]:
        return _children["runs"][order, fill]
    out = os.path.join(tmp, "digests_%s_%s.json" % (order, fill))
    env = {k: v for k, v in os.environ.items() if k != "FX_DEBUG_FILL"}
    if fill is not None:
        env["FX_DEBUG_FILL"] = str(fill)
    what = "bgzf_write_child %s FX_DEBUG_FILL=%s" % (order, fill)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "bgzf_write_child.py"), order, out], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _children["dead"] = what + " did not end within %d s" % TIMEOUT
        pytest.fail(_children["dead"], pytrace=False)
    if r.returncode != 0:
        _children["dead"] = "%s ended with status %d" % (what, r.returncode)
        pytest.fail(_children["dead"] + "\n" + r.stdout[-2000:] + r.stderr[-3000:], pytrace=False)
    with open(out) as f:
        res = json.load(f)
    _children["runs"][order, fill] = res
    return res


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("bgzf_children"))


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("fill", [None, 0, 255])
def test_device_memory_before_the_call_changes_nothing(fx, work, fill, order):
    got = child(work, order, fill)
    byte, blocks, _ = got.pop("__fill")
    assert byte == (-1 if fill is None else fill) and (blocks > 0) == (fill is not None)
    want = {"%s/%d" % (name, level): hashlib.sha256(compressed(name, level)[0]).hexdigest() for name in CASES for level in LEVELS}
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert sorted(got) == sorted(want) and not bad, bad[:10]


# ------------------------------------------------------------------ the writers
def synthetic_fastq(n=3000, seed=3):
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(n):
        m = int(rng.integers(30, 151))
        s = "".join("ACGTN"[k] for k in rng.choice(5, m, p=[0.24, 0.26, 0.26, 0.23, 0.01]))
        q = "".join("FFFF:,#"[k] for k in rng.integers(0, 7, m))
        parts.append("@read%d lane %d\n%s\n+\n%s\n" % (i, i % 8, s, q))
    return "".join(parts).encode()


def file_members(raw):
    mem, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        mem.append((at, size, struct.unpack_from("<I", raw, at + size - 4)[0]))
        at += size
    assert at == len(raw)
    return mem


def check_file(path, plain_bytes, r, plain_r):
    raw = open(path, "rb").read()
    assert gzip.open(path).read() == plain_bytes
    assert raw.endswith(EOF) and raw[:-28].count(EOF) == 0
    mem = file_members(raw)
    assert r["members"] == len(mem) and r["compressed_bytes"] == len(raw) == os.path.getsize(path)
    assert {k: v for k, v in r.items() if k not in ("members", "compressed_bytes")} == plain_r
    walk(raw[:-28], plain_bytes, path, full=False)
    return raw, mem


@pytest.mark.parametrize("compress", [True, 0, 1])
def test_fastq_write_compressed(fx, tmp_path, compress):
    src = tmp_path / "syn.fq"
    src.write_bytes(synthetic_fastq())
    fq = fx.Fastq(str(src))
    plain, out = str(tmp_path / "plain.fq"), str(tmp_path / "out.fq.gz")
    pr = fq.write(plain, batch_bytes=150000)
    r = fq.write(out, batch_bytes=150000, compress=compress)
    data = open(plain, "rb").read()
    raw, mem = check_file(out, data, r, pr)
    short = [k for k, (_, _, isize) in enumerate(mem[:-1]) if isize < MEMBER]    # the last member of every batch
    assert sum(b - a >= 2 for a, b in zip([-1] + short, short)) >= 3, short      # three batches or more of several members each
    back = fx.Fastq(out)                                                     # the BGZF open path
    assert len(back) == len(fq) == 3000
    for i in list(range(0, 3000, 97)) + [2999]:
        assert (back[i].name, back[i].seq, back[i].qual) == (fq[i].name, fq[i].seq, fq[i].qual), i


def test_fastq_write_compressed_small_file_and_selection(fx, tmp_path):
    fq = fx.Fastq(os.path.join(DATA, "test.fq"))
    n = len(fq)
    plain, out = str(tmp_path / "p.fq"), str(tmp_path / "o.fq.gz")
    pr = fq.write(plain)
    r = fq.write(out, compress=True)
    check_file(out, open(plain, "rb").read(), r, pr)
    back = fx.Fastq(out)
    assert len(back) == n
    for i in range(n):
        assert (back[i].name, back[i].seq, back[i].qual) == (fq[i].name, fq[i].seq, fq[i].qual), i
    ids = np.arange(n - 1, -1, -3, dtype=np.int64)
    start = np.minimum(5, fq._rlen_host[ids]).astype(np.int64)
    end = np.maximum(start, fq._rlen_host[ids].astype(np.int64) - 7)
    pr = fq.write(plain, ids=ids, start=start, end=end, min_len=20)
    r = fq.write(out, ids=ids, start=start, end=end, min_len=20, compress=True)
    check_file(out, open(plain, "rb").read(), r, pr)


def test_fasta_write_compressed(fx, tmp_path):
    from pyfastx_amd import _lib, bgzf
    fa = fx.Fasta(os.path.join(DATA, "test.fa"))
    plain, out = str(tmp_path / "p.fa"), str(tmp_path / "o.fa.gz")
    for kw in (dict(), dict(batch_bytes=30000, compress=2), dict(width=80, strand="-", mask=fa.class_runs("masked"), compress=1)):
        level = kw.pop("compress", True)
        pr = fa.write(plain, **kw)
        r = fa.write(out, compress=level, **kw)
        data = open(plain, "rb").read()
        check_file(out, data, r, pr)
    pr = fa.write(plain, batch_bytes=30000)
    r = fa.write(out, batch_bytes=30000, compress=True)
    data = open(plain, "rb").read()
    raw, mem = check_file(out, data, r, pr)
    assert sum(isize < MEMBER for _, _, isize in mem[:-1]) >= 3              # three batches or more
    back = fx.Fasta(out)                                                     # the BGZF open path
    assert len(back) == len(fa)
    for k in range(len(fa)):
        assert (back[k].name, back[k].seq) == (fa[k].name, fa[k].seq), k
    # virtual offsets of records of one batch: inflate the named member, read at uoffset
    blob = fa._st.blob
    stream, moff, offs, kept, _ = blob.fasta_format_alloc(len(fa), width=60, level=2)
    buf, offs_plain, _, _ = blob.fasta_format_alloc(len(fa), width=60)
    assert offs.tolist() == offs_plain.tolist() and kept == len(fa) and moff.size >= 3
    v = bgzf.virtual_offsets(moff[:-1], offs[:-1])
    sb = stream.tobytes()
    for k in (0, 1, len(fa) // 2, len(fa) - 1):
        c, u = int(v[k]) >> 16, int(v[k]) & 0xFFFF
        payload = zlib.decompressobj(-15).decompress(sb[c + 18:])
        want = buf[offs[k]:offs[k + 1]].tobytes()
        m = min(20, len(payload) - u, len(want))
        assert c in moff.tolist() and m > 0 and payload[u:u + m] == want[:m] and want.startswith(b">"), k


def test_demux_and_merge_write_compressed(fx, tmp_path):
    rng = np.random.default_rng(8)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    p1, p2 = [], []
    for i in range(12):
        frag = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 180).tobytes()
        bc = (b"ACGTACGT", b"TTGGCCAA")[i % 2]
        r1, r2 = bc + frag[:112], bytes(comp[c] for c in frag[::-1][:120])
        p1.append(b"@p%d\n%s\n+\n%s\n" % (i, r1, b"F" * len(r1)))
        p2.append(b"@p%d\n%s\n+\n%s\n" % (i, r2, b"F" * len(r2)))
    (tmp_path / "a_1.fq").write_bytes(b"".join(p1))
    (tmp_path / "a_2.fq").write_bytes(b"".join(p2))
    fq1, fq2 = fx.Fastq(str(tmp_path / "a_1.fq")), fx.Fastq(str(tmp_path / "a_2.fq"))
    dm = fq1.demux(["ACGTACGT", "TTGGCCAA"], where="5p", mismatches=0)
    plain = fq1.demux_write(dm, str(tmp_path / "d_{sample}.fq"))
    comp_out = fq1.demux_write(dm, str(tmp_path / "z_{sample}.fq.gz"), compress=True)
    assert sorted(plain) == sorted(comp_out) == ["0", "1"]
    for key in plain:
        assert comp_out[key][1] == plain[key][1] == 6
        raw = open(comp_out[key][0], "rb").read()
        assert gzip.decompress(raw) == open(plain[key][0], "rb").read() and raw.endswith(EOF)
    pair = fx.FastqPair(fq1, fq2)
    pm = pair.write_merged(str(tmp_path / "m.fq"))
    zm = pair.write_merged(str(tmp_path / "m.fq.gz"), compress=True)
    assert pm["merged"] == zm["merged"] > 0 and pm["bases"] == zm["bases"] and pm["unmerged"].tolist() == zm["unmerged"].tolist()
    raw = open(tmp_path / "m.fq.gz", "rb").read()
    assert gzip.decompress(raw) == open(tmp_path / "m.fq", "rb").read() and raw.endswith(EOF)
    assert zm["compressed_bytes"] == len(raw) and zm["members"] == len(file_members(raw))
    pw = pair.write(str(tmp_path / "w1.fq"), str(tmp_path / "w2.fq"))
    zw = pair.write(str(tmp_path / "w1.fq.gz"), str(tmp_path / "w2.fq.gz"), compress=1)
    assert {k: zw[k] for k in pw} == pw
    for k in (1, 2):
        raw = open(tmp_path / ("w%d.fq.gz" % k), "rb").read()
        assert gzip.decompress(raw) == open(tmp_path / ("w%d.fq" % k), "rb").read()
        assert zw["compressed_bytes"][k - 1] == len(raw)
    pd = pair.demux_write(pair.demux(["ACGTACGT", "TTGGCCAA"], where="5p", mismatches=0), str(tmp_path / "x_{sample}_1.fq.gz"),
                          str(tmp_path / "x_{sample}_2.fq.gz"), compress=True)
    assert sorted(pd) == ["0", "1"] and all(v[2] == 6 for v in pd.values())
    assert gzip.decompress(open(pd["0"][1], "rb").read()).count(b"\n") == 24


# ------------------------------------------------------------------ errors
def test_bad_compress_arguments_leave_no_file(fx, tmp_path):
    fq = fx.Fastq(os.path.join(DATA, "test.fq"))
    fa = fx.Fasta(os.path.join(DATA, "test.fa"))
    for k, bad in enumerate((3, -1, "gz")):
        for w in (fq, fa):
            path = tmp_path / ("bad%d" % k)
            with pytest.raises(ValueError):
                w.write(str(path), compress=bad)
            assert not path.exists()


def test_level_outside_the_range_through_the_c_entry(fx):
    from pyfastx_amd import _lib
    src = np.frombuffer(b"ACGT" * 100, dtype=np.uint8)
    for level in (7, -1, 3):
        dst, moff, nb, nm = C.c_void_p(1), C.c_void_p(1), C.c_int64(5), C.c_int64(5)
        rc = _lib.lib().fx_bgzf_compress(src.ctypes.data, src.size, level, 0, C.byref(dst), C.byref(nb), C.byref(moff), C.byref(nm))
        assert rc == _lib.FX_EINVAL and dst.value is None and moff.value is None and nb.value == 0 and nm.value == 0
    assert _lib.lib().fx_bgzf_compress(src.ctypes.data, -1, 2, 0, C.byref(dst), C.byref(nb), C.byref(moff), C.byref(nm)) == _lib.FX_EINVAL
    assert _lib.lib().fx_bgzf_compress(src.ctypes.data, 4, 2, 0, None, C.byref(nb), C.byref(moff), C.byref(nm)) == _lib.FX_EINVAL
    blob = _lib.Blob.from_bytes(open(os.path.join(DATA, "test.fq"), "rb").read(), device=0)
    blob.fastq_build()
    with pytest.raises(_lib.FxError) as e:
        blob.fastq_format_alloc(level=5)
    assert e.value.code == _lib.FX_EINVAL
    s, moff, offs, kept = blob.fastq_format_alloc(ids=np.zeros(0, dtype=np.int64), level=2)      # no query: no member, one offset each
    assert s.size == 0 and moff.tolist() == [0] and offs.tolist() == [0] and kept == 0
