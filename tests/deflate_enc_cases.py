"""Named payloads for the deflate encoder (tests/test_gpu_bgzf_write.py and its child): the smallest inputs that reach its
traps -- member seams, the match length and distance limits, degenerate alphabets, code depths past the limit, incompressible
bytes -- from one seeded generator, so that every process builds the same bytes."""
import gzip
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MEMBER = 65280


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def steep(n):
    """f[k] = f[k-1] + f[k-2] + 1 from 1, 2: beside the end-of-block code's count of 1 a Huffman tree of these stays a chain."""
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2] + 1)
    return f[:n]


def cases():
    """-> {name: bytes}, in a fixed order."""
    rng = np.random.default_rng(20240607)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    acgt = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    out = {}
    text = (b"The quick brown fox jumps over the lazy dog. " * 3000)
    for n in (0, 1, 2, 3, 4, MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER, 2 * MEMBER + 1):
        out["size_%d" % n] = text[:n]
    out["one_value_1000"] = b"A" * 1000
    out["one_value_member"] = b"\x00" * MEMBER
    for p in (2, 3, 4):
        out["period_%d" % p] = (acgt(p) if p > 2 else b"AC") * (20000 // p)
    out["period_997_x60"] = acgt(997) * 60
    blk = rnd(32768)
    out["distance_limit"] = blk + blk                                   # every match exactly 32768 back
    blk = rnd(32769)
    out["past_distance_limit"] = blk + blk[:32511]                      # every candidate one past the limit: literals
    out["runs_258_261"] = b"".join(rnd(37) + bytes([65 + k]) * (258 + k) for k in range(4)) + rnd(41)
    out["random_member"] = rnd(MEMBER)
    out["random_130561"] = rnd(2 * MEMBER + 1)
    f = np.repeat(np.arange(1, 23, dtype=np.uint8), fib(22))           # byte i, F(i) times, i = 1..22: 46367 bytes
    out["fibonacci_sorted"] = f.tobytes()
    out["fibonacci_shuffled"] = rng.permutation(f).tobytes()
    s = np.repeat(np.arange(20, dtype=np.uint8) + 97, steep(20))       # 46345 bytes; code depth 20 when unlimited
    out["steep_shuffled"] = rng.permutation(s).tobytes()
    out["all_bytes_once"] = bytes(range(256))
    for name in sorted(os.listdir(os.path.join(HERE, "data"))):
        raw = open(os.path.join(HERE, "data", name), "rb").read()
        if name.endswith(".gz"):
            raw = gzip.decompress(raw)
        if os.path.isfile(os.path.join(HERE, "data", name)):
            out["file_" + name] = raw
    seq = acgt(600000)
    out["fasta_text"] = b">random\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n"
    return out
