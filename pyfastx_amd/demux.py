"""Barcode demultiplexing on the resident FASTQ stream (extension; the reference has no counterpart): every read against a
sheet of up to 4096 barcodes, in its first or last bases or in the index field of its header.

Fastq.demux / demux_write check their arguments here and hand them to fx_fastq_demux (csrc/fx_fastq_demux.hpp); the
definition is the one of include/fxgpu.h.  Everything is integer.  What the Demux object derives from the device's columns --
the ids of a bin, the intervals that cut inline barcodes off, the summary -- is host numpy."""
from collections.abc import Mapping

import numpy as np

from . import trim as _trim

MAX_SAMPLES, MAX_LEN, MAX_MARGIN = 4096, 32, 64
NONE, AMBIGUOUS = -1, -2                                      # FX_DEMUX_NONE, FX_DEMUX_AMBIGUOUS
SEQ5, SEQ3, HEADER = 0, 1, 2                                  # FX_DEMUX_SEQ5, FX_DEMUX_SEQ3, FX_DEMUX_HEADER
SOURCES = {"5p": SEQ5, "3p": SEQ3, "header": HEADER}
LETTERS = frozenset(b"ACGTN")
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _letters(b, what):
    """str or bytes -> upper-case bytes of A C G T N, 1..32 of them."""
    if isinstance(b, str):
        try:
            b = b.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("%s: barcode letters must be A C G T N" % what)
    if not isinstance(b, (bytes, bytearray)):
        raise ValueError("%s: a barcode must be a str or bytes" % what)
    b = bytes(b).upper()
    if not 1 <= len(b) <= MAX_LEN:
        raise ValueError("%s: barcode length %d outside 1..%d" % (what, len(b), MAX_LEN))
    if not set(b) <= LETTERS:
        raise ValueError("%s: barcode letters must be A C G T N" % what)
    return b


def parse_samples(samples):
    """A mapping name -> barcode or name -> (barcode, barcode), or a sequence of the same (names "0", "1", ...) -> (names,
    rows): rows[k] = the tuple of the upper-case segments of sample k.  ValueError for an empty set, more than 4096 samples,
    unequal segment counts or lengths, a letter outside A C G T N, or two samples with identical barcodes."""
    if isinstance(samples, Mapping):
        items = list(samples.items())
    elif isinstance(samples, (str, bytes, bytearray)) or not hasattr(samples, "__iter__"):
        raise ValueError("samples must be a mapping name -> barcode(s) or a sequence of barcodes")
    else:
        items = [(str(k), v) for k, v in enumerate(samples)]
    if not 1 <= len(items) <= MAX_SAMPLES:
        raise ValueError("%d samples outside 1..%d" % (len(items), MAX_SAMPLES))
    names, rows = [], []
    for name, v in items:
        if not isinstance(name, str):
            raise ValueError("sample names must be str")
        segs = (v,) if isinstance(v, (str, bytes, bytearray)) else v
        if not isinstance(segs, (tuple, list)) or not 1 <= len(segs) <= 2:
            raise ValueError("sample %s: one barcode or a pair of barcodes" % name)
        names.append(name)
        rows.append(tuple(_letters(b, "sample %s" % name) for b in segs))
    if any([len(b) for b in r] != [len(b) for b in rows[0]] for r in rows):
        raise ValueError("all samples must have the same number of segments and the same length per segment")
    if len(set(rows)) != len(rows):
        raise ValueError("two samples have identical barcodes")
    return names, rows


def _per_segment(v, n_seg, what, check):
    """One value, or one per segment -> a list of n_seg checked values."""
    vals = list(v) if isinstance(v, (tuple, list)) else [v] * n_seg
    if len(vals) != n_seg:
        raise ValueError("%s: one value, or one per segment (%d)" % (what, n_seg))
    return [check(x) for x in vals]


def _flag(v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("revcomp must be a bool")
    return bool(v)


def _source(v):
    if not isinstance(v, str) or v not in SOURCES:
        raise ValueError("where must be one of '5p', '3p', 'header'")
    return v


def demux_args(samples, where="header", offset=0, mismatches=1, margin=1, revcomp=False):
    """The arguments of Fastq.demux as fx_fastq_demux takes them -> dict(names, where, barcodes uint8[n_samples, sum of the
    lengths], src, off, length, mm (one entry per segment), margin).  ValueError for anything outside the rules."""
    names, rows = parse_samples(samples)
    n_seg = len(rows[0])
    lens = [len(b) for b in rows[0]]
    if isinstance(where, (tuple, list)) and len(where) != n_seg:
        raise ValueError("where: one source, or one per segment (%d)" % n_seg)
    wh = _per_segment(where, n_seg, "where", _source)
    default_parts = n_seg == 2 and wh == ["header", "header"] and not isinstance(offset, (tuple, list)) and not isinstance(offset, bool) and offset == 0
    off = [0, 1] if default_parts else _per_segment(offset, n_seg, "offset", lambda x: _trim._int(x, "offset", 0, 2**31 - 1))
    for g in range(n_seg):
        if wh[g] == "header" and off[g] > 1:
            raise ValueError("offset %d: the part of the header's index field is 0 or 1" % off[g])
    mm = _per_segment(mismatches, n_seg, "mismatches", lambda x: _trim._int(x, "mismatches", 0, MAX_LEN))
    for g in range(n_seg):
        if mm[g] > lens[g]:
            raise ValueError("mismatches %d outside 0..%d" % (mm[g], lens[g]))
    rc = _per_segment(revcomp, n_seg, "revcomp", _flag)
    margin = _trim._int(margin, "margin", 1, MAX_MARGIN)
    rows = [tuple(b.translate(_COMP)[::-1] if rc[g] else b for g, b in enumerate(r)) for r in rows]
    bc = np.frombuffer(b"".join(b"".join(r) for r in rows), dtype=np.uint8).reshape(len(rows), sum(lens)).copy()
    return {"names": names, "where": wh, "barcodes": bc, "src": [SOURCES[w] for w in wh], "off": off, "length": lens, "mm": mm, "margin": margin}


class Demux:
    """What Fastq.demux returns.  names: the samples; sample / dist / second: int32, one row per query -- the sample's index,
    NONE (-1) or AMBIGUOUS (-2); the total distance of the best passing sample (-1: none); that of the runner-up (-1: none);
    counts: int64[len(names) + 2], reads per sample, then unassigned, then ambiguous.  order / bin_off: the query positions
    grouped by bin (sample index, len(names) for unassigned, len(names) + 1 for ambiguous), bin k =
    order[bin_off[k]:bin_off[k + 1]], in query order within a bin."""

    def __init__(self, names, sample, dist, second, counts, order, bin_off, rlen, query_ids=None, segments=()):
        self.names = list(names)
        self.sample, self.dist, self.second = sample, dist, second
        self.counts, self.order, self.bin_off = counts, order, bin_off
        self._rlen = np.asarray(rlen, dtype=np.int64)          # the length of every query's read
        self._ids = query_ids                                 # None: query k is read k
        self._segments = tuple(segments)                      # (where, offset, length) per segment
        self._index = {n: k for k, n in enumerate(self.names)}
        self.mate = 1                                         # which mate of a FastqPair was looked at

    def __len__(self):
        return int(self.sample.size)

    @property
    def n_assigned(self):
        return int(self.counts[:len(self.names)].sum())

    @property
    def n_unassigned(self):
        return int(self.counts[len(self.names)])

    @property
    def n_ambiguous(self):
        return int(self.counts[len(self.names) + 1])

    def positions(self, k):
        """The query positions of bin k (0 .. len(names) + 1), ascending."""
        return self.order[int(self.bin_off[k]):int(self.bin_off[k + 1])]

    def _bin_ids(self, k):
        pos = self.positions(k)
        return np.array(pos, dtype=np.int64) if self._ids is None else self._ids[pos]

    def bin_of(self, name_or_index):
        if isinstance(name_or_index, str):
            if name_or_index not in self._index:
                raise KeyError(name_or_index)
            return self._index[name_or_index]
        k = _trim._int(name_or_index, "sample index", 0, len(self.names) - 1)
        return k

    def ids(self, name_or_index):
        """The read ids assigned to a sample (by name or index), in query order."""
        return self._bin_ids(self.bin_of(name_or_index))

    @property
    def unassigned_ids(self):
        return self._bin_ids(len(self.names))

    @property
    def ambiguous_ids(self):
        return self._bin_ids(len(self.names) + 1)

    def intervals(self):
        """(start, end), int64 per query: the read without its inline windows -- start = min(L, offset + length) of a "5p"
        segment (the larger of two), end = max(start, L - offset - length) of a "3p" one (the smaller of two); a header
        segment cuts nothing."""
        L = self._rlen
        start, end = np.zeros(L.size, dtype=np.int64), L.copy()
        for where, off, length in self._segments:
            if where == "5p":
                start = np.maximum(start, np.minimum(L, off + length))
            elif where == "3p":
                end = np.minimum(end, L - off - length)
        return start, np.maximum(start, end)

    def summary(self):
        """Rows of (name, reads, share of the queries, reads at distance 0): one per sample, then "unassigned" and "ambiguous"."""
        n = len(self)
        ns = len(self.names)
        ok = self.sample >= 0
        perfect = np.bincount(self.sample[ok & (self.dist == 0)], minlength=ns) if n else np.zeros(ns, dtype=np.int64)
        rows = [(nm, int(self.counts[k]), (int(self.counts[k]) / n if n else 0.0), int(perfect[k])) for k, nm in enumerate(self.names)]
        for k, nm in ((ns, "unassigned"), (ns + 1, "ambiguous")):
            rows.append((nm, int(self.counts[k]), (int(self.counts[k]) / n if n else 0.0), 0))
        return rows


def demux_blob(blob, rlen_host, ids, args):
    """-> Demux, from the columns of fx_fastq_demux."""
    ids = _trim.check_ids(ids, rlen_host.size)
    cols = blob.fastq_demux(args["barcodes"], args["src"], args["off"], args["length"], args["mm"], args["margin"], ids, want_order=True)
    rlen = rlen_host if ids is None else rlen_host[ids]
    return Demux(args["names"], cols["sample"], cols["dist"], cols["second"], cols["counts"], cols["order"], cols["bin_off"], rlen,
                 ids, tuple(zip(args["where"], args["off"], args["length"])))


def bin_paths(dm, pattern, unassigned, ambiguous):
    """[(key, bin, path)] of the bins demux_write writes: every sample through `pattern` (it must hold "{sample}"), then the
    unassigned and the ambiguous reads where a path is given."""
    if not isinstance(pattern, str) or "{sample}" not in pattern:
        raise ValueError('pattern must be a path that holds "{sample}"')
    out = [(nm, k, pattern.replace("{sample}", nm)) for k, nm in enumerate(dm.names)]
    ns = len(dm.names)
    for key, k, path in (("unassigned", ns, unassigned), ("ambiguous", ns + 1, ambiguous)):
        if path is not None:
            if key in dm._index:
                raise ValueError("a sample is called %r: its file and the %s reads' cannot share a key" % (key, key))
            out.append((key, k, path))
    return out
