"""Paired-end FASTQ on two resident streams (extension; the reference reads one file at a time): the overlap of the mates of
every pair, adapter removal by read-through, merged fragment records, and output that keeps the two files in step.

FastqPair checks its arguments here and hands them to fx_fastq_pair_overlap and fx_fastq_pair_merge_alloc
(csrc/fx_fastq_pair.hpp); the definitions are those of include/fxgpu.h.  Everything is integer: the error rate becomes a
ratio of two integers (qc.as_ratio) before it reaches the device.  What joins the columns of the two mates -- the insert,
the intervals of trim, the pairs write keeps -- is host numpy."""
import numpy as np

from . import _lib, qc
from . import trim as _trim

NONE = -2**31                                                 # FX_PAIR_NONE: no diagonal was accepted


def overlap_args(min_overlap=30, max_diff=5, max_error_rate=0.2):
    """The arguments of FastqPair.overlap as fx_fastq_pair_overlap takes them -> dict(min_overlap, max_diff, err = (num,
    den)); the rate by the rule of trim.trim_args: the closest fraction with a denominator <= 1000.  ValueError otherwise."""
    return {"min_overlap": _trim._int(min_overlap, "min_overlap", 1, 2**31 - 1), "max_diff": _trim._int(max_diff, "max_diff", 0, 2**31 - 1),
            "err": qc.as_ratio(max_error_rate, "max_error_rate")}


def insert_of(diag, len1, len2):
    """The fragment length of every pair from its diagonal and the two read lengths: -1 where diag is NONE, max(L1, d + L2)
    for d >= 0, L2 + d for d < 0 -> int64."""
    d, len1, len2 = np.asarray(diag, dtype=np.int64), np.asarray(len1, dtype=np.int64), np.asarray(len2, dtype=np.int64)
    return np.where(d == NONE, -1, np.where(d >= 0, np.maximum(len1, d + len2), len2 + d)).astype(np.int64)


def insert_histogram(insert):
    """int64[max + 1]: the pairs of every non-negative insert (no such pair: an empty array)."""
    ins = np.asarray(insert, dtype=np.int64)
    ins = ins[ins >= 0]
    return np.bincount(ins).astype(np.int64) if ins.size else np.zeros(0, dtype=np.int64)


def check_diag(diag, n):
    diag = np.ascontiguousarray(diag, dtype=np.int32)
    if diag.ndim != 1 or diag.size != n:
        raise ValueError("diag must have one row per query (%d)" % n)
    return diag


def overlap_blob(blob1, blob2, n_reads, ids, args):
    """-> the five columns of fx_fastq_pair_overlap, pinned."""
    ids = _trim.check_ids(ids, n_reads)
    return blob1.fastq_pair_overlap(blob2, ids, **args)


def merge_blob(blob1, blob2, n_reads, ids, diag, min_len, level=None):
    """-> (buffer, offsets, merged); with a BGZF level (bgzf.level_of): (stream, member offsets, offsets, merged)"""
    ids = _trim.check_ids(ids, n_reads)
    diag = check_diag(diag, n_reads if ids is None else ids.size)
    min_len = _trim._int(min_len, "min_len", 0)
    try:
        if level is not None:
            return blob1.fastq_pair_merge_alloc(blob2, diag, ids, min_len, level=level)
        return blob1.fastq_pair_merge_alloc(blob2, diag, ids, min_len)
    except _lib.FxError as e:
        raise _lib.outside(e, "diagonal", "pair")


def clamp_intervals(t1, t2, ov):
    """The intervals of the two mates' trim, lowered to what the overlap leaves: end = min(end, end1 / end2), start = min(start,
    end) -> {"start1", "end1", "start2", "end2", "diag"}.  ov = None: the intervals as they are, every diag NONE."""
    out = {}
    for k, t in (("1", t1), ("2", t2)):
        start, end = np.asarray(t["start"], dtype=np.int64), np.asarray(t["end"], dtype=np.int64)
        if ov is not None:
            end = np.minimum(end, np.asarray(ov["end" + k], dtype=np.int64))
            start = np.minimum(start, end)
        out["start" + k], out["end" + k] = start.copy(), end.copy()
    out["diag"] = np.full(out["end1"].size, NONE, dtype=np.int32) if ov is None else np.array(ov["diag"], dtype=np.int32)
    return out


def kept_pairs(len1, len2, min_len):
    """bool[n]: the pairs of which BOTH mates keep min_len bases."""
    return (np.asarray(len1, dtype=np.int64) >= min_len) & (np.asarray(len2, dtype=np.int64) >= min_len)


def strip_mate(name):
    """A read name without a trailing /1 or /2."""
    return name[:-2] if name.endswith(("/1", "/2")) else name


class FastqPair:
    """The two files of a paired-end run, read i of one the mate of read i of the other.  fq1, fq2: Fastq objects on one device
    with as many reads; each one resident stream (a sharded or windowed one: NotImplementedError)."""

    def __init__(self, fq1, fq2):
        from .api import Fastq
        for fq in (fq1, fq2):
            if not isinstance(fq, Fastq):
                raise TypeError("FastqPair takes two Fastq objects")
            if fq._sharded:
                raise NotImplementedError("paired-end passes on a sharded or windowed stream")
        if fq1._st.device != fq2._st.device:
            raise ValueError("the mates lie on different devices (%s, %s)" % (fq1._st.device, fq2._st.device))
        if len(fq1) != len(fq2):
            raise ValueError("the mates have different numbers of reads (%d, %d)" % (len(fq1), len(fq2)))
        self.fq1, self.fq2 = fq1, fq2

    def __len__(self):
        return len(self.fq1)

    def __repr__(self):
        return "<FastqPair> %s + %s with %d pairs" % (self.fq1.file_name, self.fq2.file_name, len(self))

    def check_names(self, n=1000):
        """The names of the first and the last n pairs, a trailing /1 or /2 stripped: ValueError naming the first pair whose
        mates are not called the same."""
        n = _trim._int(n, "n", 0)
        total = len(self)
        for i in sorted(set(range(min(n, total))) | set(range(max(total - n, 0), total))):
            a, b = self.fq1[i].name, self.fq2[i].name
            if strip_mate(a) != strip_mate(b):
                raise ValueError("pair %d: the mates are called %r and %r" % (i, a, b))

    def _blobs(self):
        b1, b2 = self.fq1._qc_blob(), self.fq2._qc_blob()
        return b1, b2, self.fq1._rlen_host.size

    def _lengths(self, ids):
        sel = slice(None) if ids is None else ids
        return self.fq1._rlen_host[sel].astype(np.int64), self.fq2._rlen_host[sel].astype(np.int64)

    def overlap(self, ids=None, min_overlap=30, max_diff=5, max_error_rate=0.2):
        """Per pair the diagonal on which read 1 and the reverse complement of read 2 overlap, found on the GPU
        (csrc/fx_fastq_pair.hpp) -> dict of numpy columns, row k for ids[k] (0-based, any order, repeats allowed; None: every
        pair): diag (int32, pair.NONE where the mates do not overlap), overlap (its letters), mismatches, end1 / end2 (int64:
        what survives adapter read-through) and insert (int64: the fragment length, -1 where none).  Diagonal d puts letter
        k of the reverse complement under seq1[k + d]; it is accepted with at least min_overlap letters of overlap, at
        most max_diff mismatches and at most max_error_rate mismatches per letter, and the diagonals are tried longest
        overlap first, d = 0, 1, ..., then -1, -2, ...  Only upper-case A C G T match.  A bad id: IndexError."""
        args = overlap_args(min_overlap, max_diff, max_error_rate)
        b1, b2, n = self._blobs()
        ids = _trim.check_ids(ids, n)
        cols = dict(overlap_blob(b1, b2, n, ids, args))
        cols["insert"] = insert_of(cols["diag"], *self._lengths(ids))
        return cols

    def trim(self, ids=None, overlap=True, **trim_kwargs):
        """Fastq.trim of both mates with the same arguments, and -- overlap true, or a dict of overlap's arguments -- every end
        lowered to what adapter read-through leaves (end1 / end2 of overlap), the start clamped to it -> {"start1", "end1",
        "start2", "end2", "diag"}, what write takes."""
        t1, t2 = self.fq1.trim(ids=ids, **trim_kwargs), self.fq2.trim(ids=ids, **trim_kwargs)
        ov = None
        if isinstance(overlap, dict):
            ov = self.overlap(ids=ids, **overlap)
        elif overlap:
            ov = self.overlap(ids=ids)
        return clamp_intervals(t1, t2, ov)

    def merge(self, ids=None, diag=None, min_len=0):
        """The merged records of the pairs, formatted on the GPU -> (uint8 buffer, int64 offsets[n + 1]) in pinned memory.  diag:
        what overlap returned for the same ids (None: overlap with its defaults).  A record is the header of read 1, the
        fragment -- read 1, then what the reverse complement of read 2 adds; where both cover a position and disagree, the
        base of the higher quality byte (read 1 on a tie), where they agree the higher of the two qualities -- and its
        quality; a pair that does not overlap, or whose fragment is shorter than min_len, produces no bytes."""
        b1, b2, n = self._blobs()
        ids = _trim.check_ids(ids, n)
        if diag is None:
            diag = overlap_blob(b1, b2, n, ids, overlap_args())["diag"]
        buf, offs, _ = merge_blob(b1, b2, n, ids, diag, min_len)
        return buf, offs

    def write(self, path1, path2, ids=None, start1=None, end1=None, start2=None, end2=None, min_len=0, batch_bytes=1 << 30, compress=None):
        """Both mates through Fastq.write, in step: a pair is kept only when BOTH mates keep min_len bases of their interval
        (start / end of a mate both None: whole reads), and the two files get the same pairs in the same order ->
        {"pairs": written, "bases1", "bases2", "dropped"}.  compress: as Fastq.write takes it, for both files (their
        "compressed_bytes" and "members" come back as pairs)."""
        from . import bgzf
        level = bgzf.level_of(compress)
        n_reads = self._blobs()[2]
        ids = _trim.check_ids(ids, n_reads)
        n = n_reads if ids is None else ids.size
        min_len = _trim._int(min_len, "min_len", 0)
        start1, end1 = _trim.check_intervals(start1, end1, n)
        start2, end2 = _trim.check_intervals(start2, end2, n)
        L1, L2 = self._lengths(ids)
        keep = kept_pairs(L1 if start1 is None else end1 - start1, L2 if start2 is None else end2 - start2, min_len)
        q = (np.arange(n, dtype=np.int64) if ids is None else ids)[keep]
        cut = lambda a: None if a is None else a[keep]
        zk = {} if level is None else {"compress": level}       # (plain: the call as it always was)
        r1 = self.fq1.write(path1, ids=q, start=cut(start1), end=cut(end1), min_len=min_len, batch_bytes=batch_bytes, **zk)
        r2 = self.fq2.write(path2, ids=q, start=cut(start2), end=cut(end2), min_len=min_len, batch_bytes=batch_bytes, **zk)
        if r1["reads"] != r2["reads"] or r1["reads"] != q.size:
            raise RuntimeError("the two files fell out of step (%d, %d records for %d pairs)" % (r1["reads"], r2["reads"], q.size))
        out = {"pairs": int(q.size), "bases1": r1["bases"], "bases2": r2["bases"], "dropped": int(n - q.size)}
        if level is not None:
            out.update({k: (r1[k], r2[k]) for k in ("compressed_bytes", "members")})
        return out

    def demux(self, samples, mate=1, **demux_kwargs):
        """Fastq.demux on one mate (1 or 2) with its arguments -> demux.Demux; it remembers the mate for demux_write."""
        if mate not in (1, 2) or isinstance(mate, bool):
            raise ValueError("mate must be 1 or 2")
        dm = (self.fq1 if mate == 1 else self.fq2).demux(samples, **demux_kwargs)
        dm.mate = mate
        return dm

    def demux_write(self, dm, pattern1, pattern2, unassigned=None, ambiguous=None, cut=False, min_len=0, batch_bytes=1 << 30, compress=None):
        """Both mates of every bin of `dm` through write, in step: pattern1 / pattern2 hold "{sample}"; unassigned / ambiguous:
        a pair of paths, or None to drop those pairs; cut=True takes the inline barcodes off the mate that was looked at;
        compress: as write takes it -> {name: (path1, path2, pairs written)}."""
        from . import bgzf, demux as _demux
        level = bgzf.level_of(compress)
        if not isinstance(dm, _demux.Demux) or (dm._ids is None and len(dm) != len(self)):
            raise ValueError("dm must be what demux returned for this pair")
        for extra in (unassigned, ambiguous):
            if extra is not None and (not isinstance(extra, (tuple, list)) or len(extra) != 2):
                raise ValueError("unassigned / ambiguous: a pair of paths, or None")
        two = lambda k: (None, None) if (unassigned, ambiguous)[k] is None else (unassigned, ambiguous)[k]
        bins1 = _demux.bin_paths(dm, pattern1, two(0)[0], two(1)[0])
        bins2 = _demux.bin_paths(dm, pattern2, two(0)[1], two(1)[1])
        start, end = dm.intervals() if cut else (None, None)
        out = {}
        for (key, k, path1), (_, _, path2) in zip(bins1, bins2):
            pos = dm.positions(k)
            if pos.size == 0:
                continue
            cutk = {} if start is None else {"start%d" % dm.mate: start[pos], "end%d" % dm.mate: end[pos]}
            r = self.write(path1, path2, ids=pos if dm._ids is None else dm._ids[pos], min_len=min_len, batch_bytes=batch_bytes, **cutk,
                           **({} if level is None else {"compress": level}))
            out[key] = (path1, path2, r["pairs"])
        return out

    def write_merged(self, path, ids=None, diag=None, min_len=0, batch_bytes=1 << 30, compress=None):
        """The records of merge written to the plain file `path`, in batches of consecutive queries whose upper bound fits
        batch_bytes of pinned memory -> {"merged": records written, "bases": their bases, "unmerged": the ids (int64) of the
        queries that produced no record -- what write takes to keep them as pairs}.  compress: as Fastq.write takes it."""
        from . import bgzf
        level = bgzf.level_of(compress)
        b1, b2, n_reads = self._blobs()
        ids = _trim.check_ids(ids, n_reads)
        n = n_reads if ids is None else ids.size
        if diag is None:
            diag = overlap_blob(b1, b2, n_reads, ids, overlap_args())["diag"]
        diag = check_diag(diag, n)
        # an upper bound per query: the header of read 1, a fragment of at most L1 + L2 letters twice, six bytes around them
        bound = {"dlen": self.fq1._tab_host["dlen"], "rlen": self.fq1._rlen_host.astype(np.int64) + self.fq2._rlen_host.astype(np.int64)}
        merged = bases = 0
        rest = []
        with open(path, "wb") as f:
            z = None if level is None else bgzf.Tally(f)
            for lo, hi in _trim.batches(bound, ids, n_reads, batch_bytes):
                q = np.arange(lo, hi, dtype=np.int64) if ids is None else ids[lo:hi]
                if z is None:
                    buf, offs, k = merge_blob(b1, b2, n_reads, q, diag[lo:hi], min_len)
                    f.write(memoryview(buf))
                else:
                    stream, moff, offs, k = merge_blob(b1, b2, n_reads, q, diag[lo:hi], min_len, level)
                    z.add(stream, moff)
                merged += k
                there = np.diff(offs) > 0
                L1, L2 = self._lengths(q)
                bases += int(insert_of(diag[lo:hi], L1, L2)[there].sum())
                rest.append(q[~there])
            tail = {} if z is None else z.finish()
        return {"merged": int(merged), "bases": int(bases), "unmerged": np.concatenate(rest) if rest else np.zeros(0, dtype=np.int64), **tail}

    insert_histogram = staticmethod(insert_histogram)
