"""BGZF framing on the host side of the compressed writers (csrc/fx_deflate.hpp makes the members on the GPU).

Nothing here needs a device except compress / write, which hand their bytes to fx_bgzf_compress: the member walk, the
virtual offsets, the `compress` argument rule of the writers and the tally that puts the EOF member at the end of a file."""
import struct

import numpy as np

MEMBER = 65280                                               # uncompressed bytes of every member but a batch's last
# the empty member that ends a BGZF file
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_HEAD = bytes.fromhex("1f8b0804")
_SUB = b"\x06\x00BC\x02\x00"                                 # XLEN 6, the BC subfield of 2 bytes


def members(buf):
    """The members of a BGZF stream, found by walking BSIZE -> (coff, clen, isize, crc) as int64 / uint32 arrays: where each
    member begins, its bytes, the bytes it inflates to and the CRC-32 its trailer holds.  The EOF member is one of them.  A
    header that is cut short or is not the 18 bytes a BGZF member begins with: ValueError."""
    buf = memoryview(buf).cast("B")
    n, at = len(buf), 0
    coff, clen, isize, crc = [], [], [], []
    while at < n:
        if at + 18 > n:
            raise ValueError("member %d at byte %d: %d bytes left, a header takes 18" % (len(coff), at, n - at))
        head = bytes(buf[at:at + 18])
        if head[:4] != _HEAD or head[10:16] != _SUB:
            raise ValueError("member %d at byte %d does not begin with a BGZF header" % (len(coff), at))
        size = struct.unpack_from("<H", head, 16)[0] + 1
        if size < 18 + 2 + 8 or at + size > n:
            raise ValueError("member %d at byte %d: BSIZE says %d bytes, %d are there" % (len(coff), at, size, n - at))
        c, i = struct.unpack_from("<II", buf, at + size - 8)
        coff.append(at), clen.append(size), isize.append(i), crc.append(c)
        at += size
    return (np.array(coff, dtype=np.int64), np.array(clen, dtype=np.int64), np.array(isize, dtype=np.int64), np.array(crc, dtype=np.uint32))


def virtual_offsets(member_off, record_off, member=MEMBER):
    """(coffset << 16) | uoffset of every record: member_off[m] = the compressed offset of member m, which carries the
    uncompressed bytes [m * member, (m + 1) * member); record_off = offsets in the uncompressed stream -> uint64 array."""
    member_off = np.asarray(member_off, dtype=np.int64).reshape(-1)
    rec = np.asarray(record_off, dtype=np.int64)
    m = rec // member
    if rec.size and (rec.min() < 0 or m.max() >= member_off.size):
        raise ValueError("a record offset lies outside the members")
    return (member_off[m].astype(np.uint64) << np.uint64(16)) | (rec - m * member).astype(np.uint64)


def level_of(compress):
    """The `compress` argument of the writers -> None (plain text) or the level: None / False: plain; True: 2; 0, 1, 2."""
    if compress is None or compress is False:
        return None
    if compress is True:
        return 2
    if isinstance(compress, (int, np.integer)) and 0 <= int(compress) <= 2:
        return int(compress)
    raise ValueError("compress must be None, a bool or a level 0, 1 or 2, not %r" % (compress,))


class Tally:
    """What a compressed writer keeps per file: the batches' streams go to `f` as they come, the EOF member once, at the end."""

    def __init__(self, f):
        self.f, self.bytes, self.members = f, 0, 0

    def add(self, stream, member_off):
        self.f.write(memoryview(stream))
        self.bytes += int(stream.size)
        self.members += int(member_off.size) - 1

    def finish(self):
        self.f.write(EOF)
        self.bytes += len(EOF)
        self.members += 1                                    # (the file's size and every member a walk of it finds, the EOF one too)
        return {"compressed_bytes": self.bytes, "members": self.members}


def compress(data, level=2, device=0):
    """`data` (bytes-like) as a BGZF stream without the EOF member, made on the GPU -> bytes."""
    from . import _lib
    level = level_of(level if level is not True else 2)
    if level is None:
        raise ValueError("level must be 0, 1 or 2")
    return _lib.bgzf_compress(data, level, device)[0].tobytes()


def write(path, data, level=2, device=0):
    """`data` as the BGZF file `path` (the EOF member at its end) -> {"compressed_bytes", "members"}."""
    from . import _lib
    level = level_of(level if level is not True else 2)
    if level is None:
        raise ValueError("level must be 0, 1 or 2")
    stream, moff = _lib.bgzf_compress(data, level, device)
    with open(path, "wb") as f:
        t = Tally(f)
        t.add(stream, moff)
        return t.finish()
