"""Host-side mirror of the reference's Python objects (Fasta, Sequence, Fastq,
Read; src/fasta.c, sequence.c, fastq.c, read.c): same constructor kwargs, same
getters, same exception classes, same repr strings -- with the hot path behind
them (index scan, composition, sub-sequence / read fetch, reverse-complement,
phred) running as HIP kernels through libfxgpu.so.  The `.fxi` SQLite file is
written host-side from the GPU-produced arrays (fxi.py).

There is no CPU fallback: building an index or touching sequence data needs the
MI355X; only pure SQLite metadata (len, size, names ...) works without one.
"""
import gzip
import os
import time

import numpy as np

from . import _lib, fxi
try:
    from . import _fxobj      # C base types of Fasta / Sequence / Fastq / Read: the per-object getter path (csrc/fxobj.c)
except ImportError as _e:     # not built, or built for another interpreter (the ABI tag of the file name is the builder's)
    import sys as _sys
    raise ImportError("pyfastx_amd._fxobj (csrc/fxobj.c) is missing or was built for another Python than %s: build it with "
                      "`make -C pyfastx_amd/csrc PYTHON=%s` (or `python -c 'import __graft_entry__ as g; g.build()'`): %s"
                      % (_sys.version.split()[0], _sys.executable, _e)) from _e

VERSION = "2.3.1"          # API level mirrored (reference src/version.h:1)

_COMP_BULK_MIN = 50_000          # records from which the comp table is bulk-loaded (see Fasta._calc_composition)
_ITER_BATCH_BASES = 64 << 20     # bases fetched ahead of an iteration over an indexed file, per batch
_F_UP, _F_REV, _F_COMP, _F_RAW = _lib.FX_UPPER, _lib.FX_REVERSE, _lib.FX_COMPLEMENT, _lib.FX_RAW


def _is_gzip(path):
    """util.c:307-325"""
    try:
        with open(path, "rb") as f:
            m = f.read(4)
    except OSError:
        return False
    return len(m) == 4 and m[0] == 0x1F and m[1] == 0x8B and m[2] == 0x08


def _first_nonspace(path, gz):
    """fasta_validator / fastq_validator (util.c:95-150) without staging the file."""
    op = gzip.open if gz else open
    with op(path, "rb") as f:
        while True:
            chunk = f.read(65536)
            if not chunk:
                return -1
            s = chunk.lstrip(b" \t\n\r\x0b\x0c")
            if s:
                return s[0]


def _decode(b):
    return bytes(b).decode("latin-1")


def _text(b):
    """Header text (names, descriptions, raw records) as the reference's "s" format / SQLite TEXT reads it: UTF-8; bytes
    that are not valid UTF-8 survive as surrogate escapes instead of raising (fxi.connect reads names back the same way)."""
    return bytes(b).decode("utf-8", "surrogateescape")


def _fx_to_py(e):
    """fx_status -> the exception class the reference raises at that point."""
    c = e.code
    if c == _lib.FX_ENOENT:
        return FileExistsError(str(e))
    if c == _lib.FX_ERANGE:
        return IndexError(str(e))
    if c == _lib.FX_EINVAL:
        return ValueError(str(e))
    return RuntimeError(str(e))


class _Staged:
    """Lazily staged HBM-resident stream shared by an index object and its children."""

    def __init__(self, path, device):
        self.path, self.device, self._blob = path, device, None
        self.gzindex = None          # callable -> restart points of the index file (fxi.read_gzindex), set by the owner
        self.on_stage = None         # callable(blob): the owner learns the handle of the staged stream (the getters' fast path)
        self.windowed = None         # callable(plan) -> windows.WindowedFasta / WindowedFastq: set by an owner that can work out of core
        self.forced = None           # callable() -> the same kind of object whatever the size: Fastq(path, devices=[...])
        self.win_factor = 1.15       # what a build needs in HBM beside the stream itself, as a factor of its size
        self._md = None              # the windowed build, once the stream turned out not to fit (pyfastx_amd/windows.py)

    @property
    def md(self):
        """The windowed build when the stream does not fit the HBM it may use, else None (decided at the first touch)."""
        self.blob
        return self._md

    @property
    def blob(self):
        if self._blob is None and self.forced is not None:
            try:
                self._md = self.forced()
            except _lib.FxError as e:
                raise _fx_to_py(e)
            self._blob = self._md.blob
        if self._blob is None and self.windowed is not None:
            from . import windows
            try:
                plan = windows.plan(self.path, self.device, self.win_factor)
                if plan is not None:                          # larger than the budget: windows that take turns on the device
                    self._md = self.windowed(plan)
                    self._blob = self._md.blob
            except _lib.FxError as e:
                raise _fx_to_py(e)
        if self._blob is None:
            pts = None
            if self.gzindex is not None:                     # a gzip file with an index: inflate the segments in parallel
                try:
                    pts = self.gzindex()
                except Exception:                            # noqa: BLE001  (an unreadable gzindex table: inflate serially)
                    pts = None
                if pts is not None and (pts["windows"] is None or int(pts["has"].sum()) == 0
                                        or pts["compressed_size"] != os.path.getsize(self.path)):
                    pts = None
            try:
                self._blob = _lib.Blob.from_file(self.path, self.device, gzindex=pts)
            except _lib.FxError as e:
                # (a BGZF file that was taken to fit from the ratio of its first members and does not: the exact size, then windows)
                if e.code == _lib.FX_ENOMEM and self.windowed is not None:
                    from . import windows
                    try:
                        _lib.lib().fx_release_scratch()
                        plan = windows.plan(self.path, self.device, self.win_factor, exact=True)
                        if plan is not None:
                            self._md = self.windowed(plan)
                            self._blob = self._md.blob
                            return self._blob
                    except _lib.FxError as e2:
                        raise _fx_to_py(e2)
                raise _fx_to_py(e)
            if self.on_stage is not None:
                self.on_stage(self._blob)
        return self._blob

    def write_gzindex(self, db):
        """The gzindex table of a gzip input: BGZF member boundaries, or the restart points captured while a single
        stream was inflated (util.c:442-540)."""
        blob = self.blob
        c, u, _ = blob.gz_points()
        if len(c):
            fxi.write_gzindex(db, os.path.getsize(self.path), blob.size, c, u)
            return
        p = blob.gz_checkpoints()
        fxi.write_gzindex(db, os.path.getsize(self.path), blob.size, p["cmp"], p["uncmp"], bits=p["bits"], has_data=p["has"],
                          windows=p["windows"])

    def raw(self, off, n):
        """pyfastx_index_random_read (index.c:683-692): bytes as they are."""
        if n <= 0:
            return b""
        if n <= 65536:                                       # a getter's worth of bytes: the resident kernel (fx_fetch_one, FX_RAW)
            b = self.blob.fetch_one(off, n, n, flags=_F_RAW)
            return b if len(b) == n else b + b"\0" * (n - len(b))    # past the end of the stream: zeros, as fx_read_bytes gives them
        return self.blob.read_bytes(off, n)

    def fetch(self, off, blen, slen, flags):
        """pyfastx_index_fill_cache + the getter's slen-byte copy (index.c:694-707, sequence.c:346-347)."""
        if slen <= 0 or blen <= 0:
            return b""
        return self.blob.fetch_one(off, blen, slen, flags=flags)


class _ShardedStaged(_Staged):
    """The stream spread over several devices by byte range (multi.MultiDevice): built lazily like _Staged.blob; `.blob`
    is the ShardedBlob adapter, `.md` the sharded build itself (merged table, fetcher, composition)."""

    def __init__(self, path, devices, full_name):
        super().__init__(path, devices[0])
        self.devices, self.full_name, self._md = list(devices), full_name, None
        self.windowed = None

    @property
    def md(self):
        if self._md is None:
            from .multi import MultiDevice
            try:
                self._md = MultiDevice(self.path, self.devices, self.full_name)
            except _lib.FxError as e:
                raise _fx_to_py(e)
            self._blob = self._md.blob
        return self._md

    @property
    def blob(self):
        return self.md.blob


# =========================================================================== FASTA
def _dev_index_applies(path):
    return not (path == ":memory:" or os.path.exists(path) or os.environ.get("FX_FXI_HOST"))


def _dev_index(path, blob, kind, n, total, presized=False):
    """A NEW .fxi whose two big b-trees are formatted on the device (fxi._bulk_table_dev): from FX_FXI_DEV_MIN records
    (default 200 000; below that the host loaders are as fast and keep their arrays for the getters).  presized: the file
    is there already, schema in place, made by fxi.presize_fastq for this very build.  -> (connection, phases) or None when
    this route does not apply: an existing file, an in-memory index, a row that needs an overflow page, a database without
    4 KiB pages."""
    if not presized and not _dev_index_applies(path):
        return None
    if n < int(os.environ.get("FX_FXI_DEV_MIN", 200_000)) or not hasattr(blob, "fxi_dev_write"):
        if presized and os.path.exists(path):
            os.remove(path)
        return None
    try:
        if kind == 1:
            return fxi.write_fastq_dev(path, blob, n, total, schema_done=presized)
        return fxi.write_fasta_dev(path, blob, n, total)
    except _lib.FxError as e:
        # a row that needs an overflow page / a database without 4 KiB pages -- or no room on the device for the slab and the
        # sort beside a stream close to the HBM budget (FX_ENOMEM, FX_EDEVICE; FX_EIO: the file could not be grown): the host
        # loaders still produce the index (the half-written file is gone: fxi._bulk_table_dev removed it)
        if e.code not in (_lib.FX_ERANGE, _lib.FX_EINVAL, _lib.FX_ENOMEM, _lib.FX_EDEVICE, _lib.FX_EIO):
            raise
        if e.code in (_lib.FX_ENOMEM, _lib.FX_EDEVICE):
            _lib.lib().fx_release_scratch()
        return None


def _bulk_index(path, blob, kind, n, name_off, name_len, write):
    """The bulk route to a NEW .fxi (fxi._bulk_table): the names come off the GPU as one packed buffer (one gather),
    their sorted order from Blob.names_sort, and both b-trees are written as pages instead of n INSERTs + a CPU
    sort.  -> open connection, or None when this route does not apply (an existing file, an in-memory index, a
    record too large for a page) and the caller writes the index with INSERTs."""
    if path == ":memory:" or os.path.exists(path):
        return None
    ln = np.maximum(np.asarray(name_len, dtype=np.int64), 0)
    packed, offs = blob.names_pack(kind, n, guess=int(ln.sum()))
    order, ndup = blob.names_sort(kind, n)
    try:
        return write(path, packed, offs, None if ndup else order)
    except _lib.FxError as e:
        if e.code != _lib.FX_ERANGE:
            raise
        return None


class Fasta(_fxobj.FastaCore):
    """pyfastx.Fasta (fasta.c:39-135, 1156-1210).  fa[name] for a name met before is answered by the C base type
    (csrc/fxobj.c); every other subscript comes through _getitem_slow."""

    def __init__(self, file_name, index_file=None, uppercase=False, build_index=True, full_index=False,
                 full_name=False, memory_index=False, key_func=None, device=0, devices=None):
        """devices: several GPUs for ONE file (extension): the stream is cut into len(devices) byte ranges,
        each device stages and scans only its own, the boundary summaries stitch the records that cross the cuts and ONE
        index file is written; batched fetches are answered by the device that holds the bytes.  Plain and BGZF files."""
        if key_func is not None and not callable(key_func):
            raise TypeError("key_func must be a callable function")                       # fasta.c:71-74
        if not os.path.isfile(file_name):
            raise FileExistsError("the input fasta file %s does not exists" % file_name)   # fasta.c:84-87
        self.file_name = file_name
        self._uppercase, self._full_name, self._key_func = bool(uppercase), bool(full_name), key_func
        self._has_index = bool(build_index)
        self.is_gzip = _is_gzip(file_name)
        self._explicit_shards = devices is not None and len(devices) > 1
        if self._explicit_shards:
            if key_func is not None or not build_index:
                raise ValueError("devices=[...] builds a plain index: no key_func, build_index must stay on")
            self._st = _ShardedStaged(file_name, devices, bool(full_name))
        else:
            self._st = _Staged(file_name, devices[0] if devices else device)
            if key_func is None and build_index:
                # a stream larger than the HBM it may use (FX_HBM_BUDGET / what is free): built and served in windows that take
                # turns on the device -- the multi-GPU machinery on one GPU (pyfastx_amd/windows.py); decided at the first touch
                def windowed(plan, path=file_name, dev=self._st.device, fn=bool(full_name)):
                    from .windows import WindowedFasta
                    return WindowedFasta(path, dev, fn, window=plan[2], capacity=plan[3])
                self._st.windowed = windowed
            import weakref
            me = weakref.ref(self)

            def staged(blob, me=me):                           # the C getters talk to the resident kernel through this handle
                fa = me()
                if fa is not None:
                    _bind_fxobj()
                    # ... and, for a plain file, read single small answers from the page cache (csrc/fxobj.c: seq_fast)
                    fa._core_stage(int(blob._h.value or 0), None if fa.is_gzip or os.environ.get("FX_NO_HOST_GETTERS") else fa.file_name)

                    def closed(me=me):                          # Blob.close(): the C getters must not keep the freed handle
                        f2 = me()
                        if f2 is not None:
                            f2._core_stage(0)
                    blob.on_close.append(closed)
            self._st.on_stage = staged
        self._core_upper = 1 if uppercase else 0
        self._index_file = ":memory:" if memory_index else (index_file or file_name + ".fxi")   # index.c:45-61
        self._db = None
        self._full_index = False
        self._seq_counts = 0
        self.size = 0
        if _first_nonspace(file_name, self.is_gzip) != ord(">"):                          # fasta.c:107-110
            raise RuntimeError("%s is not plain or gzip compressed fasta formatted file" % file_name)
        self._want_comp = bool(build_index and full_index)   # the index build then counts the letters on the way (one read of the stream)
        self._comp_in_build = False
        if build_index:
            self.build_index()
            if full_index:
                self._calc_composition()

    @property
    def _sharded(self):
        """Is the stream held as byte-range shards -- over several devices (devices=[...]) or as windows of one (out of core)?
        Asking stages the stream (or runs the windowed build): every caller is about to need it."""
        return self._explicit_shards or self._st.md is not None

    # ---------------------------------------------------------------- index
    def build_index(self):
        """pyfastx_build_index (index.c:418-429): load the .fxi if present else create it."""
        if self._db is not None:
            return
        if fxi.exists(self._index_file):
            self._db = fxi.connect(self._index_file)
            if not fxi.has_fasta_index(self._db):                                         # index.c:402-411
                raise RuntimeError("the index file %s was damaged" % self._index_file)
            if self.is_gzip and not self._explicit_shards:   # pyfastx_load_index imports the zran points (index.c:433): so do we
                self._st.gzindex = lambda: fxi.read_gzindex(self._db)
        else:
            self._create_index()
        row = self._db.execute("SELECT * FROM stat LIMIT 1").fetchone()                    # fasta.c:17-37
        if row is None:
            raise RuntimeError("get seq count and length error")
        self._seq_counts, self.size = int(row[0]), int(row[1])
        self._has_index = True

    def _create_index(self):
        """pyfastx_create_index (index.c:109-388) with the scan on the GPU."""
        if self._sharded:                                     # byte-range shards over several devices, ONE index file
            from .shard import write_merged_index
            md = self._st.md
            self._scanned_here = False
            self._db = write_merged_index(self._index_file, md.table)
            if self.is_gzip:
                c, u, _ = md.blobs[0].gz_points()
                fxi.write_gzindex(self._db, os.path.getsize(self.file_name), md.size, c, u)
            return
        blob = self._st.blob
        try:
            s = blob.fasta_build(self._full_name, comp=self._want_comp)
        except _lib.FxError as e:
            raise _fx_to_py(e)
        self._comp_in_build = self._want_comp
        self._scanned_here = True
        t = blob.fasta_table(s.n_seq)
        self._db = None
        self.index_phases = None
        if self._key_func is None and s.n_seq:
            dv = _dev_index(self._index_file, blob, 0, s.n_seq, s.seq_len)
            if dv is not None:
                self._db, self.index_phases = dv
        if self._db is None and self._key_func is None and s.n_seq:
            self._db = _bulk_index(self._index_file, blob, 0, s.n_seq, t["hoff"] + 1, t["name_len"],
                                   lambda p, names, offs, order: fxi.write_fasta_bulk(p, names, offs, t, s.seq_len, order))
        if self._db is None:
            if self._key_func is None:
                names = self._gather(t["hoff"] + 1, t["name_len"])          # raw bytes: stored verbatim, like sqlite3_bind_text
            else:    # index.c:303-318: key_func(header text after '>'), '\r' of a CRLF header included
                hl = t["dlen"].astype(np.int64) + (t["elen"] == 2)
                names = [self._key_func(_text(h)) for h in self._gather(t["hoff"] + 1, hl)]
            self._db = fxi.connect(self._index_file)
            fxi.write_fasta(self._db, names, t, s.seq_len)
        if self.is_gzip:
            self._st.write_gzindex(self._db)

    def _gather(self, off, length):
        """Raw byte spans of the resident stream as a list of bytes (one batched GPU gather)."""
        length = np.asarray(length, dtype=np.int64)
        if length.size == 0:
            return []
        buf, offs, _ = self._st.blob.fetch_ranges(off, length, length, flags=_F_RAW)
        b = buf.tobytes()
        o = offs.tolist()
        return [b[o[i]:o[i + 1]] for i in range(length.size)]

    def _calc_composition(self):
        """pyfastx_fasta_calc_composition (fasta.c:851-961)."""
        if self._full_index:
            return
        if self._db.execute("SELECT * FROM comp LIMIT 1").fetchone() is not None:
            self._full_index = True
            return
        if self._sharded:
            fxi.write_fasta_comp(self._db, self._st.md.composition())
            self._full_index = True
            return
        blob = self._st.blob
        if self._comp_in_build:                                  # the build that made the index has counted already
            s = blob.fasta_build_end()
            self._comp_in_build = False
        else:
            s = blob.fasta_build(self._full_name, comp=True)    # index scan and letter counts in one read of the stream
        if s.n_seq >= _COMP_BULK_MIN and self._index_file != ":memory:":
            # many records: the non-zero bins come off the GPU as triples (the dense matrix stays in HBM) and the
            # comp table + seqidx go into the file as b-tree pages instead of ~10 INSERTs per record
            seqid, abc, num, total = blob.fasta_comp_sparse(guess=s.n_seq * 12)
            rows = (np.concatenate([seqid, np.zeros(128, dtype=np.int64)]), np.concatenate([abc, np.arange(128, dtype=np.int64)]),
                    np.concatenate([num, total]))
            self._db.close()
            try:
                self._db = fxi.write_fasta_comp_bulk(self._index_file, *rows)
            except Exception:
                # disk full, a table that is not empty, ...: the page loader has given its pages back (fx_fxi.hpp);
                # reconnect, clear what the attempt left behind and write the rows with INSERTs
                self._db = fxi.connect(self._index_file)
                self._db.execute("DROP INDEX IF EXISTS seqidx")
                self._db.execute("DELETE FROM comp")
                fxi.write_fasta_comp_rows(self._db, *rows)
        else:
            fxi.write_fasta_comp(self._db, blob.fasta_comp(s.n_seq))
        self._full_index = True

    def _total_comp(self):
        self._calc_composition()
        return {int(l): int(n) for _, _, l, n in self._db.execute("SELECT * FROM comp WHERE seqid=0")}

    # ------------------------------------------------------------ protocols
    def __len__(self):
        return self._seq_counts

    def __repr__(self):
        if self._has_index:
            return "<Fasta> %s contains %d sequences" % (self.file_name, self._seq_counts)      # fasta.c:138-144
        return "<Fasta> %s" % self.file_name

    def _make(self, row):
        return Sequence(self, *row[:9])

    def _getitem_slow(self, item):
        """pyfastx_fasta_subscript (fasta.c:521-546); names whose row is cached never get here (FastaCore.__getitem__)."""
        self._need_index()
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            i = int(item)
            if i < 0:
                i += self._seq_counts
            if i >= self._seq_counts:
                raise IndexError("index out of range")
            row = self._db.execute("SELECT * FROM seq WHERE ID=? LIMIT 1", (i + 1,)).fetchone()
            if row is None:
                raise IndexError("Index Error")
            return self._make(row)
        if type(item) is str:
            cache = self._rows_by_name                                # the B-tree probe (index.c:527-566) once per name: a genome has few
            row = cache.get(item)
            if row is None:
                row = self._db.execute("SELECT * FROM seq WHERE chrom=? LIMIT 1", (item,)).fetchone()
                if row is None:
                    raise KeyError("%s does not exist in fasta file" % item)
                if len(cache) < 1_000_000:
                    cache[item] = row
            return self._make(row)
        raise KeyError("the key must be index number or sequence name")

    def __contains__(self, key):
        if type(key) is not str or self._db is None:
            return False
        return self._db.execute("SELECT 1 FROM seq WHERE chrom=? LIMIT 1", (key,)).fetchone() is not None

    def __iter__(self):
        if not self._has_index:
            # build_index=False: (name, seq) tuples from kseq_read (index.c:609-664) -- the same device path as Fastx (fx_kseq.hpp)
            # over the staged stream, a C iterator building the tuples; full_name joins a non-empty comment to the name with
            # one space ("%s %s"), whatever the delimiter was
            return _kseq_iter(lambda: self._st.blob, False, fastq=False, upper=self._uppercase, comment_mode=2 if self._full_name else 0)
        return self._iter_indexed()

    def _iter_indexed(self):
        # fasta.c:146-172 -> Sequence objects in file order.  SURVEY 8f-3: the sequences of the records ahead come off the GPU
        # in batches (one gather per ~64 MB of bases or 4096 records) and ride along in the Sequence objects; `.seq` of an
        # object taken from the iterator costs nothing more.  A record larger than a batch is fetched when (and if) it is
        # asked for.  The rows of the `seq` table are stepped from C (_fxobj.RowCursor, as index.c:525-560 steps them) and the
        # objects of a batch made by one call; without that connection (a memory index, a locked file) the sqlite3 module's
        # rows do the same, more slowly.
        self._need_index()
        fl = _F_UP if self._uppercase else 0
        batch = None
        try:
            cur = _fxobj.RowCursor(self._index_file, "SELECT ID, chrom, boff, blen, slen, llen, elen, norm, dlen FROM seq ORDER BY ID")
            batch = cur.fetch(4096)
        except RuntimeError:
            cur = None
        if cur is not None:
            none8, none64 = np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64)
            while batch is not None:
                k, names, raw = batch
                cols = np.frombuffer(raw, dtype=np.int64).reshape(8, k)                     # ID, boff, blen, slen, llen, elen, norm, dlen
                slen = np.maximum(cols[3], 0)
                i = 0
                while i < k:
                    j = i + max(1, int(np.searchsorted(np.cumsum(slen[i:]), _ITER_BATCH_BASES, side="right")))
                    sel = np.nonzero((slen[i:j] > 0) & (slen[i:j] <= _ITER_BATCH_BASES))[0].astype(np.int64)
                    if sel.size:
                        buf, offs, ol = self._st.blob.fetch_ranges(cols[1, i:j][sel], cols[2, i:j][sel], slen[i:j][sel], flags=fl)
                    else:
                        buf, offs, ol = none8, none64, none64
                    yield from _fxobj.seq_batch_cols(Sequence, self, names[i:j], np.ascontiguousarray(cols[:, i:j]), buf,
                                                     np.ascontiguousarray(offs[:sel.size]), np.ascontiguousarray(ol), sel)
                    i = j
                batch = cur.fetch(4096)
            return
        if True:
            rows = self._db.execute("SELECT * FROM seq ORDER BY ID").fetchall()
            i, n = 0, len(rows)
            while i < n:
                j, tot = i, 0
                while j < n and j - i < 4096 and (tot == 0 or tot + max(rows[j][4], 0) <= _ITER_BATCH_BASES):
                    tot += max(rows[j][4], 0)
                    j += 1
                pick = [k for k in range(i, j) if 0 < rows[k][4] <= _ITER_BATCH_BASES]
                got = {}
                if pick:
                    buf, offs, ol = self._st.blob.fetch_ranges([rows[k][2] for k in pick], [rows[k][3] for k in pick],
                                                               [rows[k][4] for k in pick], flags=fl)
                    ball, o, l = _decode(buf), offs.tolist(), ol.tolist()                 # one decode per batch
                    got = {k: ball[o[m]:o[m] + l[m]] for m, k in enumerate(pick)}
                for k in range(i, j):
                    sq = self._make(rows[k])
                    if k in got:
                        sq._prefetched = got[k]
                    yield sq
                i = j
            return
        # (build_index=False is answered by __iter__ itself)

    def _need_index(self):
        if self._db is None:
            raise RuntimeError("the index has not been built: call build_index()")

    def keys(self):
        self._need_index()
        return FastaKeys(self, self._seq_counts)

    # ----------------------------------------------------------- statistics
    # fasta.c:573-849.  The reference sorts / scans the seq table in SQLite for each of them; here they come from ONE
    # device sort of the lengths (fx_fasta_len_stats) whenever the record table is resident in HBM (an index
    # built or used for batched fetches in this process) and from the same SQL otherwise (an index file opened for
    # metadata only is not staged for a median).  The stat-table caching of the reference is kept, quirks included.
    def _dev_stats(self, count_min=0, half=0.0):
        b = self._st._blob
        if b is None or not getattr(b, "_table_ready", False) or getattr(b, "_n_fasta", None) != self._seq_counts or not self._seq_counts \
                or not hasattr(b, "fasta_len_stats"):
            return None
        try:
            return b.fasta_len_stats(count_min, half)
        except _lib.FxError:
            return None

    def _cache_stat(self, sql, args):
        """The reference ignores the result of the sqlite3_step that caches a statistic in `stat` (fasta.c:651-659,
        770-782, 827-839): an index file that cannot be written (read-only mount, shared directory) still answers."""
        import sqlite3
        try:
            self._db.execute(sql, args)
        except sqlite3.Error:
            pass

    def count(self, n):
        st = self._dev_stats(count_min=int(n))
        if st is not None:
            return int(st.count_ge)
        return int(self._db.execute("SELECT COUNT(*) FROM seq WHERE slen>=?", (int(n),)).fetchone()[0])

    def nl(self, p=50):
        if p < 0 or p > 100:
            raise ValueError("the value must between 0 and 100")
        i = j = 0
        if p == 50:                                            # fasta.c:609-625: the cached pair
            row = self._db.execute("SELECT n50,l50 FROM stat LIMIT 1").fetchone()
            if row is not None and row[0]:
                j, i = int(row[0]), int(row[1] or 0)
        if not j:
            half = p / 100.0 * self.size                       # fasta.c:628
            st = self._dev_stats(half=half)
            if st is not None:
                j, i = int(st.nx_len), int(st.nx_count)
            else:
                acc = 0
                for (j,) in self._db.execute("SELECT slen FROM seq ORDER BY slen DESC"):
                    i += 1
                    acc += j
                    if acc >= half:
                        break
        if not j:
            raise RuntimeError("can not calculate N50 and L50")
        # fasta.c:651-659 stores the pair in n50 / l50 WHATEVER p was (so nl(90) followed by nl(50) answers nl(90)'s pair
        # from the cache there): mirrored, the columns are part of the index file
        self._cache_stat("UPDATE stat SET n50=?, l50=?", (int(j), int(i)))
        return (int(j), int(i))

    @property
    def longest(self):
        st = self._dev_stats()
        if st is not None:
            return self[int(st.longest_id)]
        row = self._db.execute("SELECT ID,MAX(slen) FROM seq LIMIT 1").fetchone()
        return self[int(row[0]) - 1]

    @property
    def shortest(self):
        st = self._dev_stats()
        if st is not None:
            return self[int(st.shortest_id)]
        row = self._db.execute("SELECT ID,MIN(slen) FROM seq LIMIT 1").fetchone()
        return self[int(row[0]) - 1]

    @property
    def mean(self):
        row = self._db.execute("SELECT avglen FROM stat LIMIT 1").fetchone()          # fasta.c:740-752
        m = float(row[0]) if row is not None and row[0] else 0.0
        if not m:
            st = self._dev_stats()
            if st is not None:
                m = float(st.sum_len) / float(st.n_seq)         # AVG(): the double sum over the double count
            else:
                m = float(self._db.execute("SELECT AVG(slen) FROM seq").fetchone()[0] or 0.0)
        if not m:
            raise RuntimeError("could not calculate average length")        # fasta.c:770-782: a mean of 0 is an error there
        self._cache_stat("UPDATE stat SET avglen=?", (m,))
        return m

    @property
    def median(self):
        row = self._db.execute("SELECT medlen FROM stat LIMIT 1").fetchone()          # fasta.c:792-804
        m = float(row[0]) if row is not None and row[0] else 0.0
        if not m:
            n = self._seq_counts                               # fasta.c:806-825
            st = self._dev_stats()
            if st is not None:
                m = (float(st.med_lo) + float(st.med_hi)) / 2.0 if n % 2 == 0 else float(st.med_lo)
            else:
                if n % 2 == 0:
                    sql = "SELECT AVG(slen) FROM (SELECT slen FROM seq ORDER BY slen LIMIT %d,2)" % ((n - 1) // 2)
                else:
                    sql = "SELECT slen FROM seq ORDER BY slen LIMIT %d,1" % ((n - 1) // 2)
                m = float(self._db.execute(sql).fetchone()[0] or 0.0)
        if not m:
            raise RuntimeError("could not calculate median length")         # fasta.c:827-839: so is a median of 0
        self._cache_stat("UPDATE stat SET medlen=?", (m,))
        return m

    @property
    def composition(self):
        return {chr(l): n for l, n in sorted(self._total_comp().items()) if n > 0 and 32 <= l < 127}

    @property
    def gc_content(self):
        c = self._total_comp()
        a, cc, g, t = (c.get(65, 0) + c.get(97, 0), c.get(67, 0) + c.get(99, 0),
                       c.get(71, 0) + c.get(103, 0), c.get(84, 0) + c.get(116, 0))
        if a + cc + g + t <= 0:
            raise RuntimeError("could not calculate gc content")
        return float(np.float32(g + cc) / np.float32(a + cc + g + t) * np.float32(100))      # (float) arithmetic, fasta.c:1013

    @property
    def gc_skew(self):
        c = self._total_comp()
        cc, g = c.get(67, 0) + c.get(99, 0), c.get(71, 0) + c.get(103, 0)
        if cc + g <= 0:
            raise RuntimeError("could not calculate gc skew")
        return float(np.float32(g - cc) / np.float32(g + cc))

    @property
    def type(self):
        """fasta.c:1106-1154"""
        letters = {chr(l) for l, n in self._total_comp().items() if 32 < l < 127 and n > 0}

        def subset(alpha):
            return letters <= set(alpha)
        if subset("ACGTNacgtn") or subset("abcdghkmnrstvwyABCDGHKMNRSTVWY*-"):
            return "DNA"
        if subset("ACGUNacgun") or subset("abcdghkmnrsuvwyABCDGHKMNRSUVWY*-"):
            return "RNA"
        if subset("acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY*-"):
            return "protein"
        return "unknown"

    # -------------------------------------------------------- fetch / flank
    def _info(self, name, exc=NameError, msg="Sequence %s does not exists"):
        row = self._db.execute("SELECT * FROM seq WHERE chrom=? LIMIT 1", (name,)).fetchone()
        if row is None:
            raise exc(msg % name)
        return row

    def fetch(self, chrom, intervals, strand="+"):
        """pyfastx_fasta_fetch (fasta.c:384-515): 1-based inclusive intervals of one
        sequence, concatenated; strand '-' reverse-complements the result.  One GPU
        batch of byte ranges instead of loading the whole chromosome."""
        if not isinstance(intervals, (tuple, list)):
            raise ValueError("intervals must be list or tuple")
        if len(intervals) == 0:
            raise ValueError("intervals must be list or tuple")
        row = self._info(chrom)
        seq = self._make(row)
        if isinstance(intervals[0], (int, np.integer)):
            if len(intervals) != 2:
                raise ValueError("list or tuple should include only start and end")
            pairs = [(int(intervals[0]), int(intervals[1]))]
        else:
            pairs = [(int(iv[0]), int(iv[1])) for iv in intervals]
        for s, e in pairs:
            if s > e:
                raise ValueError("start position should less than end position")
        out = seq._fetch_many([s - 1 for s, _ in pairs], [e for _, e in pairs])
        res = b"".join(out)
        if strand == "-":
            res = _lib.revcomp_bytes(res, _F_REV | _F_COMP, self._st.device)
        return _decode(res)

    def flank(self, chrom, start, end, flank_length=50, use_cache=False):
        """pyfastx_fasta_flank (fasta.c:322-382)."""
        if flank_length < 0:
            raise ValueError("Flank length must be non-negative")
        seq = self._make(self._info(chrom, NameError, "sequence %s does not exists"))
        ls = max(start - flank_length - 1, 0)
        le = max(start - 1, ls)
        re_ = min(end + flank_length, seq._seq_len)
        rs = min(end, re_)
        left, right = seq._fetch_many([ls, rs], [le, re_])
        return _decode(left), _decode(right)

    def _regular(self, sq):
        """Sequence._line_regular for one record (cached per record; the whole column once the table is in HBM)."""
        reg = getattr(self, "_reg", None)
        if reg is None and getattr(self._st._blob, "_table_ready", False) and getattr(self._st._blob, "_n_fasta", None) == self._seq_counts:
            self._reg = reg = self._st.blob.fasta_line_regular(self._seq_counts)
        if reg is not None:
            return bool(reg[sq.id - 1])
        cache = self.__dict__.setdefault("_regular_one", {})
        ok = cache.get(sq.id)
        if ok is None:
            from .shard import line_regular_rule
            size = self._st.blob.size

            def byte_at(p):
                return self._st.raw(p, 1)[0] if 0 <= p < size else None
            ok = bool(line_regular_rule(sq._offset, sq._byte_len, sq._full_len, sq._line_len, sq._end_len, sq._normal, byte_at))
            cache[sq.id] = ok
        return ok

    def _table(self):
        """The seq table as numpy columns (cached): what the batched calls index into."""
        if getattr(self, "_tab", None) is None:
            rows = self._db.execute("SELECT chrom,boff,blen,slen,llen,elen,norm FROM seq ORDER BY ID").fetchall()
            index = {}
            for i in range(len(rows) - 1, -1, -1):          # the FIRST record of a name wins, as `SELECT ... LIMIT 1` does (index.c:527-566)
                index[rows[i][0]] = i
            self._tab = {"index": index,
                         "boff": np.array([r[1] for r in rows], np.int64), "blen": np.array([r[2] for r in rows], np.int64),
                         "slen": np.array([r[3] for r in rows], np.int64), "llen": np.array([r[4] for r in rows], np.int64),
                         "elen": np.array([r[5] for r in rows], np.int64), "norm": np.array([r[6] for r in rows], np.int64)}
        return self._tab

    def fetch_many(self, names_or_ids, starts, stops, strand=None):
        """Batched extension: 0-based half-open (start, stop) on many sequences in ONE
        kernel launch -> (uint8 buffer, int64 offsets[n+1]).  names_or_ids: sequence names or 0-based
        ids; strand: optional per-query '+'/'-' (or 0/1).
        Host to host the call is a handful of milliseconds for a million intervals: names become ids in one C pass
        (_fxobj.ids_of_names), the intervals are checked on the device against the resident table, the answers are laid
        out by a device scan and arrive by DMA in pinned memory (fx_fasta_fetch_alloc) -- the arrays returned are views
        of pinned blocks that go back to the library's pool when they are garbage-collected."""
        self._need_index()
        t = self._table()
        n = len(names_or_ids)
        starts = np.asarray(starts, dtype=np.int64)
        stops = np.asarray(stops, dtype=np.int64)
        first = names_or_ids[0] if n else 0
        if isinstance(first, str):
            ids = np.empty(n, dtype=np.int64)
            if not isinstance(names_or_ids, (list, tuple)):
                names_or_ids = list(names_or_ids)
            bad = _fxobj.ids_of_names(names_or_ids, t["index"], ids)
            if bad >= 0:
                raise KeyError("%s does not exist in fasta file" % names_or_ids[bad])
        else:
            ids = np.asarray(names_or_ids, dtype=np.int64)
        fl = (_F_UP if self._uppercase else 0)
        fpq = None
        if strand is not None:
            neg = np.array([s in ("-", 1, True) for s in strand], dtype=bool) if not isinstance(strand, np.ndarray) \
                else (strand != 0) & (strand != ord("+"))
            fpq = neg.view(np.uint8) * np.uint8(_F_REV | _F_COMP) | np.uint8(fl)
        if self._sharded:                                   # routed to the devices that hold the bytes (shard.ShardFetcher)
            if ids.size and (ids.min() < 0 or ids.max() >= self._seq_counts):
                raise IndexError("index out of range")
            if starts.size and (starts.min() < 0 or (stops < starts).any() or (stops > t["slen"][ids]).any()):
                raise ValueError("interval outside the sequence")
            qidx, sbuf, soffs = self._st.md.fetcher().fetch(ids, starts, stops, flags=fl, flags_per_query=fpq)
            offs = np.zeros(ids.size + 1, dtype=np.int64)
            np.cumsum(stops - starts, out=offs[1:])
            buf = np.zeros(max(int(offs[-1]), 1), dtype=np.uint8)
            ln = soffs[1:] - soffs[:-1]
            if sbuf.size:
                buf[np.repeat(offs[qidx] - soffs[:-1], ln) + np.arange(int(soffs[-1]), dtype=np.int64)] = sbuf[:int(soffs[-1])]
            return buf[:int(offs[-1])], offs
        blob = self._st.blob
        if not getattr(blob, "_table_ready", False):       # index loaded from an existing .fxi: install its rows once
            blob.fasta_set_table(t["boff"], t["blen"], t["slen"], t["llen"], t["elen"], t["norm"])
        # (record id, start, stop) resolved on the GPU with the sequence.c:498-510 arithmetic (line-regular
        # records) or despace-then-slice (sequence.c:100-110); ids and intervals are checked there too
        try:
            return blob.fasta_fetch_alloc(ids, starts, stops, flags=fl, flags_per_query=fpq)
        except _lib.FxError as e:
            k = getattr(e, "first_bad", -1)
            if e.code != _lib.FX_ERANGE or k < 0:
                raise _fx_to_py(e)
            # ids first, then intervals -- the order of the sharded path above
            if ids.size and (ids.min() < 0 or ids.max() >= self._seq_counts):
                raise IndexError("index out of range")
            if (starts < 0).any() or (stops < starts).any() or (stops > np.asarray(t["slen"])[ids]).any():
                raise ValueError("interval outside the sequence")
            # every query is valid: one of them is longer than the 2^31 - 1 bytes the device-side layout counts in (a whole
            # chromosome of a 32 Gbp genome) -- the batch goes through the path that lays the answers out on the host in int64
            buf, offs, _ = blob.fasta_fetch(ids, starts, stops, flags=fl, flags_per_query=fpq)
            return buf, offs


    def search_all(self, pattern, strand="both", degenerate=False, ids=None, max_hits=10**8):
        """Extension: every overlapping hit of `pattern` (1..64 letters) in the `seq` of every record -- what fa[i].seq
        presents: white space dropped, upper case under uppercase=True -- on strand '+', '-' or 'both'.  Exact by default
        (the '-' pattern is the reverse complement Sequence.search uses); degenerate=True reads the pattern as IUPAC codes
        (a text letter matches when its base set lies inside the pattern letter's).  -> SearchHits(ids, starts, stops,
        strands) of numpy arrays in pinned memory, 0-based half-open forward-strand coordinates as fetch_many takes them,
        ordered by (record, start), '+' before '-' at one start.  ids: restrict to these records (names or 0-based ids).
        More than max_hits hits: ValueError with the count, nothing allocated.  Two passes over the resident stream on
        the GPU (csrc/fx_search.hpp)."""
        from . import search
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()
        return search.search_blob(blob, pattern, strand, degenerate, self._uppercase, sel, max_hits, self._st.device)

    def search_counts(self, pattern, strand="both", degenerate=False):
        """Extension: hits of search_all per record -> int64[len(fa), 2] (column 0 '+', column 1 '-'); the hits themselves
        are never materialised."""
        from . import search
        blob = self._search_blob()
        return search.count_blob(blob, pattern, strand, degenerate, self._uppercase, self._st.device)

    def search_approx(self, pattern, mismatches, anchor=None, strand="both", degenerate=False, ids=None, max_hits=10**8):
        """Extension: search_all with up to `mismatches` (0..8, below the pattern's length) substituted letters per hit --
        every window of len(pattern) letters of a record's `seq` whose Hamming distance to the pattern is at most
        `mismatches`; no insertions or deletions.  A letter mismatches exactly where search_all would not match it (byte
        inequality, or the IUPAC subset rule under degenerate=True), so mismatches=0 gives search_all's rows.  anchor: the
        positions of the pattern, as written (forward strand), where no mismatch may fall -- None, a slice or an iterable of
        0-based positions, e.g. slice(20, 23) for the NGG of a 20 nt guide + PAM; on '-' the same letters are held.
        -> ApproxHits(ids, starts, stops, strands, mismatches): SearchHits' columns and order plus the distance of every
        hit (uint8).  ids, max_hits: as for search_all.  On the GPU from the resident stream (csrc/fx_search_approx.hpp)."""
        from . import search
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()
        return search.approx_blob(blob, pattern, mismatches, anchor, strand, degenerate, self._uppercase, sel, max_hits, self._st.device)

    def search_approx_counts(self, pattern, mismatches, anchor=None, strand="both", degenerate=False):
        """Extension: hits of search_approx per record -> int64[len(fa), 2] (column 0 '+', column 1 '-'); the hits themselves
        are never materialised."""
        from . import search
        blob = self._search_blob()
        return search.approx_count_blob(blob, pattern, mismatches, anchor, strand, degenerate, self._uppercase, self._st.device)

    def search_edit(self, pattern, edits, strand="both", degenerate=False, report="best", ids=None, max_hits=10**8):
        """Extension: search_all with up to `edits` (0..8, below the pattern's length) substituted, inserted or deleted
        letters -- every place of a record's `seq` where the pattern ENDS within that Levenshtein distance: letter e is an end
        when D[e], the least distance between the pattern and any stretch of the text that ends with letter e, is at most
        `edits`.  A text letter matches a pattern letter exactly where search_all would match it (byte equality, or the IUPAC
        subset rule under degenerate=True); '-' searches the reverse complement on the forward text, as search_all does.
        -> EditHits(ids, starts, stops, strands, edits): per reported end stop = e + 1, edits = D[e] (uint8) and start = the
        beginning of the SHORTEST stretch that has that distance (a hit never begins with a letter it pays for), so
        len(pattern) - edits <= stop - start <= len(pattern) + edits; ordered by (record, stop), '+' before '-' at one
        stop -- the starts are not monotone.  report='all': every end (with edits=0: search_all's rows).  report='best':
        per record and strand the leftmost minimum of every dip of D -- end e stays when e - 1 is no end or has more
        edits, and e + 1 is no end or has no fewer; every stretch of consecutive ends keeps at least one row.  ids: as for
        search_all.  max_hits bounds the ENDS, which the device holds before 'best' thins them out: more of them is a
        ValueError with their count.  On the GPU from the resident stream (csrc/fx_search_edit.hpp)."""
        from . import search
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()
        return search.edit_blob(blob, pattern, edits, strand, degenerate, report, self._uppercase, sel, max_hits, self._st.device)

    def search_edit_counts(self, pattern, edits, strand="both", degenerate=False, report="best"):
        """Extension: rows of search_edit per record -> int64[len(fa), 2] (column 0 '+', column 1 '-'); the rows themselves
        are never materialised and no start is computed."""
        from . import search
        blob = self._search_blob()
        return search.edit_count_blob(blob, pattern, edits, strand, degenerate, report, self._uppercase, self._st.device)

    def pwm_scan(self, pwm, min_score=None, threshold=None, pvalue=None, strand="both", ids=None, max_hits=10**8):
        """Extension: every window of len(pwm) letters of a record's `seq` whose score under the position weight matrix
        `pwm` (pwm.Pwm) reaches a threshold, on strand '+', '-' or 'both'.  Letters A C G T in either case, U = T
        (uppercase= plays no part); a window that holds any other byte (N, IUPAC codes, ...) has no score; windows run
        across line ends, never across records.  The '-' score of a window is the score of its reverse complement.
        Exactly one threshold: min_score (integer units of pwm.ints), threshold (units of the float matrix: a hit iff the
        integer score is >= ceil(threshold * pwm.scale - 1e-9)) or pvalue (pwm.threshold_for_pvalue).  -> PwmHits(ids,
        starts, stops, strands, scores): SearchHits' columns and order plus the int32 score of every hit
        (pwm.to_float for float units).  ids, max_hits: as for search_all.  On the GPU from the resident stream
        (csrc/fx_pwm.hpp)."""
        from . import pwm as _pwm
        t = _pwm.resolve_min_score(pwm, min_score, threshold, pvalue)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        return _pwm.scan_blob(self._search_blob(), pwm, t, strand, sel, max_hits)

    def pwm_counts(self, pwm, min_score=None, threshold=None, pvalue=None, strand="both"):
        """Extension: hits of pwm_scan per record -> int64[len(fa), 2] (column 0 '+', column 1 '-'); the hits themselves
        are never materialised."""
        from . import pwm as _pwm
        t = _pwm.resolve_min_score(pwm, min_score, threshold, pvalue)
        return _pwm.count_blob(self._search_blob(), pwm, t, strand)

    def pwm_best(self, pwm, strand="both", ids=None):
        """Extension: the best-scoring window of every record under `pwm` -> PwmBest(scores int32[n, 2], starts int64[n, 2]),
        column 0 '+', column 1 '-', one row per record -- or per entry of ids (names or 0-based ids), in the order given.
        The largest score, and the smallest start that has it; (INT32_MIN, -1) for a record without a scorable window and
        for a strand that was not asked for."""
        from . import pwm as _pwm
        sel = None if ids is None else self._ids_of(ids)
        return _pwm.best_blob(self._search_blob(), pwm, strand, sel)

    def minimizers(self, k, w, canonical=True, order="hash", ids=None, max_hits=10**8):
        """Extension: the (w, k) minimizers of every record's `seq` -- of every w consecutive k-mers the smallest, each
        distinct choice once.  1 <= k <= 31, 1 <= w <= 32.  Position p holds the k-mer seq[p:p+k], valid when all its letters
        are ACGTacgt (uppercase= plays no part; U, N, IUPAC codes and everything else are not); windows run across line ends,
        never across records.  fw: its base-4 code (A=0 C=1 G=2 T=3, first letter most significant), rc: that of its reverse
        complement.  canonical=True: code = min(fw, rc), strand '+' when fw <= rc (a k-mer that is its own reverse
        complement is '+'), else '-'; canonical=False: code = fw, strand '+'.  order="lex": key = code; order="hash":
        key = minimizer.mix(code, k), a bijection of the 2k-bit words.  Window j holds the positions j .. j+w-1; its selection
        is the leftmost position with the smallest key among its valid k-mers (none: no selection).  A record shorter than
        w + k - 1 letters has no window.  -> Minimizers(ids, starts, stops, strands, codes): the distinct selections, by
        (record, start); int64, int64, int64 (starts + k), uint8, uint64, in pinned memory.  ids, max_hits: as for
        search_all.  On the GPU from the resident stream (csrc/fx_minimizer.hpp)."""
        from . import minimizer
        minimizer.check_args(k, w, order)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        return minimizer.minimizers_blob(self._search_blob(), k, w, canonical, order, sel, max_hits)

    def minimizer_counts(self, k, w, canonical=True, order="hash"):
        """Extension: rows of minimizers per record -> int64[len(fa), 2] (column 0 '+', column 1 '-'); the rows themselves
        are never materialised."""
        from . import minimizer
        minimizer.check_args(k, w, order)
        return minimizer.count_blob(self._search_blob(), k, w, canonical, order)

    def sketch(self, k=21, scaled=None, size=None, canonical=True, ids=None, pooled=False, oversample=None):
        """Extension: MinHash / FracMinHash sketches of the records -> sketch.Sketch, one set per selected record in ascending
        record order (ids: names or 0-based ids, None: every record), or one set for all of them with pooled=True, such as a
        multi-contig assembly.  The windows and codes are kmer_table's; key = minimizer.mix(code, k).  A set keeps the distinct
        keys below max_key = ceil(4^k / scaled) (scaled None: 4^k) and, with size, the `size` smallest of them; at least one of
        scaled and size must be given.  The sets stay in device memory: Sketch.compare / jaccard / containment / mash_distance /
        ani compare them there.  oversample (1..64, None: 4) sizes the first threshold of a bottom-`size` sketch; no result
        depends on it, only Sketch.n_rounds does.  On the GPU from the resident stream (csrc/fx_sketch.hpp)."""
        from . import sketch
        sketch.check_args(k, scaled, size)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()
        names = [r[0] for r in self._db.execute("SELECT chrom FROM seq ORDER BY ID")]
        if sel is not None:
            names = [names[i] for i in sel.tolist()]
        if pooled:
            names = [os.path.basename(self.file_name)]
        return sketch.fasta_sketch_blob(blob, k, scaled, size, canonical, sel, pooled, names, oversample or 0, self._st.device)

    def kmer_counts(self, k, canonical=False, ids=None):
        """Extension: the k-mer spectrum of the `seq` of every record -> int64[4**k] in pinned memory, counted on the GPU
        from the resident stream (csrc/fx_kmer.hpp).  Letters A C G T in either case (A = 0, C = 1, G = 2, T = 3; uppercase=
        plays no part); the index of a k-mer is its base-4 number, first base most significant; a window that holds any
        other byte (N, IUPAC codes, ...) is not counted; windows run across line ends, never across records.  canonical=True
        counts a window under the smaller of its code and its reverse complement's (a palindrome once); the other entries
        stay 0.  ids: restrict to these records (names or 0-based ids; a record listed twice counts twice).  1 <= k <= 13:
        the dense table is 8 * 4**k bytes, 512 MiB at k = 13; for larger k see kmer_table."""
        from . import kmer
        k = kmer.check_k(k)
        sel = None if ids is None else self._ids_of(ids)
        return kmer.fasta_counts_blob(self._search_blob(), k, canonical, sel)

    def kmer_table(self, k, canonical=False, ids=None, min_count=1, max_bytes=None):
        """Extension: the sparse k-mer table of the `seq` of every record, 1 <= k <= 31 -> kmer.KmerTable: the codes that
        occur (int64, ascending) with their exact counts, by the definition of kmer_counts; sorted and reduced on the GPU from
        the resident stream (csrc/fx_kmer_table.hpp).  min_count: entries that occur less often are dropped on the device.
        max_bytes: device working memory of the call (None: the library's default, 8 GiB; at least 1 MiB) -- a smaller budget
        takes more rounds (KmerTable.n_parts), the table is the same."""
        from . import kmer
        kmer.check_table(k, min_count, max_bytes)
        sel = None if ids is None else self._ids_of(ids)
        return kmer.fasta_table_blob(self._search_blob(), k, canonical, sel, min_count, max_bytes)

    def kmer_hits(self, table, ids=None):
        """Extension: per record, how many of the k-mers of its `seq` occur in `table` (a kmer.KmerTable: another assembly's
        kmer_table, KmerTable.from_strings of a primer list, ...) -> (n_windows, n_hits), int64 arrays in pinned memory, one
        row per id (names or 0-based ids, a record listed twice has two rows; None: every record).  k and the canonical form
        are the table's; windows are those of kmer_table; a window that occurs twice counts twice.  n_hits / n_windows is the
        containment index of the record in the table's source.  The table's codes become a hash set in device memory on
        first use (csrc/fx_kmer_screen.hpp), kept on the table until it is collected or table.release()."""
        from . import kmer
        kmer.check_screen_table(table)
        sel = None if ids is None else self._ids_of(ids)
        return kmer.fasta_hits_blob(self._search_blob(), self._st.device, table, sel)

    def kmer_profile(self, k, canonical=False, ids=None, max_bytes=1 << 30):
        """Extension: one k-mer spectrum per record -> int64[n_sel, 4**k] in pinned memory, rows in the order of ids (all
        records in file order when None); the definition is kmer_counts'.  1 <= k <= 6; rows that would take more than
        max_bytes: ValueError with the size, nothing allocated."""
        from . import kmer
        sel = None if ids is None else self._ids_of(ids)
        kmer.check_profile(k, self._seq_counts if sel is None else len(sel), max_bytes)
        return kmer.fasta_profile_blob(self._search_blob(), k, canonical, sel, self._seq_counts, max_bytes)

    def region_stats(self, names_or_ids, starts, stops):
        """Batched composition of intervals -- what fa[name][a:b].composition, .gc_content and .gc_skew answer one slice at a
        time on the host (sequence.c:562-749): 0-based half-open (start, stop) on many sequences in one kernel launch ->
        annot.RegionStats with ids, starts, stops, counts (int64[n, 7]; columns A C G T N other masked: either case, U in
        other, masked = letters in a..z) and the derived length, gc_content (percent), gc_skew and masked_fraction.  The
        file's own letters are counted (uppercase= plays no part).  names_or_ids and the errors are fetch_many's: an unknown
        name KeyError, an id outside the table IndexError, an interval outside its sequence ValueError; an empty interval
        gives zeros.  Counted on the GPU from the rank index of the table (csrc/fx_annot.hpp), built on first use: two runs
        of the stream are read per interval, whatever its length."""
        from . import annot
        n = len(names_or_ids)
        ids = self._ids_of(names_or_ids)
        starts, stops = np.asarray(starts, dtype=np.int64), np.asarray(stops, dtype=np.int64)
        if starts.shape != (n,) or stops.shape != (n,):
            raise ValueError("ids, starts and stops differ in length")
        blob = self._search_blob()
        try:
            return annot.region_blob(blob, ids, starts, stops)
        except _lib.FxError as e:
            if e.code != _lib.FX_ERANGE or getattr(e, "first_bad", -1) < 0:
                raise _fx_to_py(e)
            raise ValueError("interval outside the sequence")

    def window_stats(self, window, step=None, ids=None, partial=True, max_windows=10**8):
        """Extension: composition of every window [j * step, min(j * step + window, len)) with j * step < len of every record
        (ids: restrict to these names or 0-based ids) -> annot.RegionStats, rows by record, then by j.  step=None tiles (step =
        window); partial=False keeps only whole windows.  More than max_windows windows: ValueError with the count, nothing
        allocated.  The windows are made and counted on the GPU (csrc/fx_annot.hpp); no array of windows crosses the link."""
        from . import annot
        annot.check_windows(window, step, max_windows)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()
        return annot.window_blob(blob, self._table()["slen"], window, step, sel, partial, max_windows)

    def class_runs(self, kind=None, min_len=1, ids=None, max_runs=10**8, letters=None):
        """Extension: every maximal stretch of the `seq` of the records whose letters all belong to one class and that is at
        least min_len letters long -> annot.ClassRuns(ids, starts, stops) ordered by (record, start), with .lengths and
        .write_bed(path).  kind: 'N' (N, n: assembly gaps), 'masked' (a..z: soft-masked repeats), 'unmasked' (A..Z), or an
        explicit set of letters used exactly as written -- a str / bytes of more than one distinct letter, or any given as
        letters=...  A stretch never joins across two records.  ids: restrict to these records.  More than max_runs:
        ValueError with the count, nothing allocated.  On the GPU from the resident stream (csrc/fx_annot.hpp)."""
        from . import annot
        annot.class_set(kind, letters)
        annot.check_runs(min_len, max_runs)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()

        def name_of(r):
            return self._db.execute("SELECT chrom FROM seq WHERE ID=?", (int(r) + 1,)).fetchone()[0]
        return annot.runs_blob(blob, kind, min_len, sel, max_runs, letters, name_of)

    def low_complexity(self, window=64, threshold=20, min_len=1, ids=None, max_rows=10**8):
        """Extension: the low-complexity intervals of the `seq` of the records by the windowed DUST triplet score ->
        annot.ClassRuns(ids, starts, stops) ordered by (record, start), with .lengths and .write_bed(path);
        records(mask=...) and write(mask=...) take it as it is.  Letters fold A a C c G g T t, every other letter is invalid.
        For every letter e >= 2 of a record the window [max(0, e - window + 1), e] is scored: with c_x the valid triplets of
        code x wholly inside it, n their number and S = sum c_x (c_x - 1) / 2, the window qualifies iff n >= 2 and
        10 S > threshold (n - 1) -- threshold in tenths as sdust and dustmasker write it, 20 is a score of 2.0.  The rows are
        the maximal intervals of the union of the qualifying windows (touching ones are one row), those shorter than min_len
        dropped.  window: 4..64, or a tuple of up to 4 lengths whose rows are joined before min_len.  This is the windowed
        form: a whole window is masked, so flanks of up to window minus about 23 letters go with a repeat at the defaults; a
        smaller window is the finer knob.  sdust's perfect intervals are not implemented, parity with sdust / dustmasker is
        not claimed.  Nothing joins across two records.  ids: restrict to these records.  More than max_rows: ValueError
        with the count, nothing allocated.  On the GPU from the resident stream (csrc/fx_dust.hpp)."""
        from . import complexity
        complexity.check_mask(window, threshold, min_len, max_rows)
        sel = None if ids is None else np.unique(self._ids_of(ids))
        blob = self._search_blob()

        def name_of(r):
            return self._db.execute("SELECT chrom FROM seq WHERE ID=?", (int(r) + 1,)).fetchone()[0]
        return complexity.mask_blob(blob, window, threshold, min_len, sel, max_rows, name_of)

    def tandem_repeats(self, min_copies=(12, 7, 5, 4, 4, 4), min_len=0, ids=None, max_repeats=10**8):
        """Extension: the perfect tandem repeats (microsatellites) of period 1..8 of the `seq` of the records ->
        tandem.TandemRepeats(ids, starts, stops, periods, motif_codes) ordered by record, stop, period, with .lengths, .copies,
        .motifs, .canonical_motifs, .counts_by_motif(), .sorted_by_start() and .write_bed(path).  A repeat of period p is a
        maximal stretch of A C G T letters (either case; N and every other letter break it) in which each letter equals the
        one p places before it, at least max(2 p, p * min_copies[p - 1], min_len) long, whose motif is not a shorter word
        written several times (ATATAT has period 2 only).  Repeats of different periods may overlap and all are reported:
        maximal repetitions, not MISA's greedy scan.  min_copies: 1 to 8 integers (entry p - 1: period p) or {period: copies};
        0 = period not searched, else at least 2; the default is Krait's.  ids: restrict to these names or 0-based ids, rows
        in their order.  A repeat never joins across two records.  More than max_repeats: ValueError with the count, nothing
        allocated.  On the GPU from the resident stream (csrc/fx_tandem.hpp)."""
        from . import tandem
        tandem.check_min_copies(min_copies)
        tandem.check_limits(min_len, max_repeats)
        sel = None if ids is None else self._ids_of(ids)
        blob = self._search_blob()

        def name_of(r):
            return self._db.execute("SELECT chrom FROM seq WHERE ID=?", (int(r) + 1,)).fetchone()[0]
        return tandem.repeats_blob(blob, min_copies, min_len, sel, max_repeats, name_of)

    def orfs(self, min_len=75, table=1, starts=("ATG",), mode="start", strand="both", ids=None, max_orfs=10**8):
        """Extension: the open reading frames of the `seq` of the records in all six frames -> orf.Orfs(ids, starts, stops,
        frames, flags) with .lengths, .strands, .has_stop, .has_start, .complete, .sorted_by_start(), .write_bed(path),
        .proteins() and .write_faa(path).  Letters are A C G T of either case; every other letter makes its codons invalid.
        Per strand and frame a segment is a maximal run of codons that are neither a stop of `table` (an NCBI id in 1, 2, 4,
        11 or a pair of 64-letter strings in TCAG order) nor invalid.  mode "stop": the rows are the segments; mode "start":
        a row begins at the first START codon of its segment (`starts`: codons written with T, or "table" for the table's own
        set), a segment without one gives no row.  Rows have at least max(min_len, 3) letters and never hold the stop codon
        that ends them.  Coordinates are 0-based, half-open, on the forward strand; frames are +1..+3 and -1..-3.  strand:
        "+", "-" or "both".  ids: restrict to these names or 0-based ids, rows in their order; within a record rows come in
        the order a left-to-right walk closes their segments.  An ORF never joins across two records.  More than max_orfs:
        ValueError with the count, nothing allocated.  On the GPU from the resident stream (csrc/fx_orf.hpp)."""
        from . import orf
        args = orf.search_args(min_len, table, starts, mode, strand, max_orfs)      # argument errors come first
        sel = None if ids is None else self._ids_of(ids)
        blob = self._search_blob()

        def name_of(r):
            return self._db.execute("SELECT chrom FROM seq WHERE ID=?", (int(r) + 1,)).fetchone()[0]
        return orf.orfs_run(blob, args, sel, name_of)

    def translate_many(self, names_or_ids, starts, stops, strand=None, table=1):
        """Extension: the 0-based half-open intervals (start, stop) of many sequences translated by a genetic code ->
        (uint8 buffer of amino acids, int64 offsets[n+1]), shaped like fetch_many.  strand: optional per-query '+'/'-' (or
        0/1): '-' translates the reverse complement of the interval.  table: as in orfs().  An interval yields
        (stop - start) // 3 amino acids; a codon with a letter outside A C G T (either case) gives X; no codon is rewritten
        to M.  Ids and intervals are checked on the device; errors are those of fetch_many (csrc/fx_orf.hpp)."""
        from . import orf
        aa64 = orf.genetic_code(table)[0]
        n = len(names_or_ids)
        sd = orf.strands_of(strand, n)
        starts = np.asarray(starts, dtype=np.int64)
        stops = np.asarray(stops, dtype=np.int64)
        first = names_or_ids[0] if n else 0
        if isinstance(first, str):                           # _ids_of without its range check of ids: the device makes that one,
            ix = self._table()["index"]                      # and reports the first bad query as fetch_many does
            try:
                ids = np.fromiter((ix[k] for k in names_or_ids), dtype=np.int64, count=n)
            except KeyError as e:
                raise KeyError("%s does not exist in fasta file" % e.args[0])
        else:
            ids = np.asarray(names_or_ids, dtype=np.int64)
        blob = self._search_blob()
        try:
            return blob.fasta_translate_alloc(ids, starts, stops, aa64, strand=sd)
        except _lib.FxError as e:
            if e.code != _lib.FX_ERANGE or getattr(e, "first_bad", -1) < 0:
                raise _fx_to_py(e)
            k = e.first_bad                                  # the error of fetch_many, of the first query that is not valid
            err = IndexError("index out of range (query %d)" % k) if ids[k] < 0 or ids[k] >= self._seq_counts \
                else ValueError("interval outside the sequence (query %d)" % k)
            err.first_bad = k
            raise err

    def _search_blob(self):
        """The blob with the record table resident (installed once from the .fxi, as fetch_many does); a sharded or windowed
        stream has no halo for hits that straddle its cuts."""
        self._need_index()
        if self._sharded:
            raise NotImplementedError("search on a sharded or windowed stream: a hit can straddle a cut")
        blob = self._st.blob
        if not getattr(blob, "_table_ready", False):
            t = self._table()
            blob.fasta_set_table(t["boff"], t["blen"], t["slen"], t["llen"], t["elen"], t["norm"])
        return blob

    def _ids_of(self, names_or_ids):
        """Sequence names or 0-based ids -> int64 ids (KeyError / IndexError as the subscript raises them)."""
        first = names_or_ids[0] if len(names_or_ids) else 0
        if isinstance(first, str):
            ix = self._table()["index"]
            try:
                return np.fromiter((ix[k] for k in names_or_ids), dtype=np.int64, count=len(names_or_ids))
            except KeyError as e:
                raise KeyError("%s does not exist in fasta file" % e.args[0])
        ids = np.asarray(names_or_ids, dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= self._seq_counts):
            raise IndexError("index out of range")
        return ids

    def raw_many(self, names_or_ids):
        """Batched `Sequence.raw` (sequence.c:314-335) -- whole records as they are in the file, header line included:
        ONE gather for all of them instead of one read per record (what `pyfastx extract` / `sample` write,
        pyfastxcli.py:282-387).  -> (uint8 buffer, int64 offsets[n+1])."""
        self._need_index()
        ids = self._ids_of(names_or_ids)
        if getattr(self, "_raw_cols", None) is None:
            rows = self._db.execute("SELECT boff,blen,elen,dlen FROM seq ORDER BY ID").fetchall()
            a = np.array(rows, dtype=np.int64).reshape(-1, 4)
            self._raw_cols = (a[:, 0] - a[:, 3] - a[:, 2] - 1, a[:, 1] + a[:, 3] + a[:, 2] + 1)
        off, ln = self._raw_cols[0][ids], self._raw_cols[1][ids]
        ln = np.minimum(ln, self._st.blob.size - off)          # blen counts a newline an unterminated file lacks
        buf, offs, _ = self._st.blob.fetch_ranges(off, ln, ln, flags=_F_RAW)
        return buf, offs

    # ------------------------------------------------------------- records written back out (fasta_out.py)
    def _records_plan(self, names_or_ids, starts, stops, strand, width, mask, mask_mode, mask_char, uppercase, headers, min_len):
        """The arguments of records / write, checked, as one dict of per-query arrays that _records_call cuts batches from."""
        from . import fasta_out as fo
        width = fo.check_width(width)
        mode = fo.check_mask_mode(mask_mode)
        byte = fo.check_mask_char(mask_char)
        min_len = fo._int(min_len, "min_len", 0)
        rows = fo.mask_rows(mask)
        blob = self._search_blob()
        t = self._table()
        names = None
        if names_or_ids is None:
            ids, n = None, self._seq_counts
        else:
            n = len(names_or_ids)
            if n and isinstance(names_or_ids[0], str):
                names = list(names_or_ids)
                ids = np.empty(n, dtype=np.int64)
                bad = _fxobj.ids_of_names(names, t["index"], ids)
                if bad >= 0:
                    raise KeyError("%s does not exist in fasta file" % names[bad])
            else:
                ids = np.ascontiguousarray(names_or_ids, dtype=np.int64)
                if ids.ndim != 1:
                    raise ValueError("ids must be one-dimensional")
        starts, stops = fo.check_intervals(starts, stops, n)
        if ids is None and starts is not None:
            ids = np.arange(n, dtype=np.int64)
        neg = fo.strand_flags(strand, n)
        fl = _F_UP if (uppercase or self._uppercase) else 0
        fpq = (neg.view(np.uint8) * np.uint8(_F_REV | _F_COMP) | np.uint8(fl)) if neg.any() else None
        hdr = None
        if isinstance(headers, str) and headers == "auto":
            if starts is not None:
                if names is None:
                    self._check_id_rows(ids)
                    chroms = self._chrom_names()
                    names = [chroms[i] for i in ids.tolist()]
                hdr = fo.pack_headers(fo.auto_headers(names, starts, stops, neg), n)
            elif not getattr(blob, "_hdr_cols", False):     # a table installed from the .fxi: the header lines in ONE gather
                hdr = self._own_headers(ids)
        else:
            hdr = fo.pack_headers(headers, n)
        return {"blob": blob, "n": n, "ids": ids, "starts": starts, "stops": stops, "neg": neg, "flags": fl, "fpq": fpq, "width": width,
                "mask": rows if mode else None, "mode": mode, "byte": byte, "hdr": hdr, "min_len": min_len}

    def _check_id_rows(self, ids):
        """The IndexError of the first id outside the table, naming its row (what the device reports for the batch)."""
        if ids.size and (ids.min() < 0 or ids.max() >= self._seq_counts):
            k = int(np.flatnonzero((ids < 0) | (ids >= self._seq_counts))[0])
            err = IndexError("index out of range (query %d)" % k)
            err.first_bad = k
            raise err

    def _chrom_names(self):
        if getattr(self, "_chroms", None) is None:
            self._chroms = [r[0] for r in self._db.execute("SELECT chrom FROM seq ORDER BY ID")]
        return self._chroms

    def _hdr_cols_host(self):
        """(offset, length) of every record's header line behind '>', from the .fxi rows (sequence.c:299-313)."""
        if getattr(self, "_hdr_host", None) is None:
            a = np.array(self._db.execute("SELECT boff,elen,dlen FROM seq ORDER BY ID").fetchall(), dtype=np.int64).reshape(-1, 3)
            self._hdr_host = (a[:, 0] - a[:, 2] - a[:, 1], a[:, 2])
        return self._hdr_host

    def _own_headers(self, ids):
        off, ln = self._hdr_cols_host()
        if ids is not None:
            self._check_id_rows(ids)
            off, ln = off[ids], ln[ids]
        if off.size == 0:
            return np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64)
        buf, offs, _ = self._st.blob.fetch_ranges(off, ln, ln, flags=_F_RAW)
        return (buf if buf.size else np.zeros(1, dtype=np.uint8)), np.ascontiguousarray(offs, dtype=np.int64)

    def _records_call(self, q, lo, hi, level=None):
        """Queries [lo, hi) of a plan through fx_fasta_format_alloc -> (buffer, offsets, records kept, their letters); with a
        BGZF level (bgzf.level_of): (stream, member offsets, offsets, records kept, their letters)."""
        from . import fasta_out as fo
        whole = lo == 0 and hi == q["n"]
        cut = (lambda a: a if a is None or whole else a[lo:hi])
        ids = q["ids"]
        if ids is None and lo:
            ids = np.arange(lo, hi, dtype=np.int64)
        else:
            ids = cut(ids)
        hdr = hdr_off = None
        if q["hdr"] is not None:
            hdr, hdr_off = q["hdr"]
            if not whole:
                b0, b1 = int(hdr_off[lo]), int(hdr_off[hi])
                hdr, hdr_off = (hdr[b0:b1] if b1 > b0 else np.zeros(1, dtype=np.uint8)), hdr_off[lo:hi + 1] - b0
        mask = q["mask"]
        if mask is not None and not whole:
            mask = fo.slice_mask(mask, ids if ids is not None else np.arange(lo, hi, dtype=np.int64))
        try:
            return q["blob"].fasta_format_alloc(hi - lo, ids, cut(q["starts"]), cut(q["stops"]), flags=q["flags"], flags_per_query=cut(q["fpq"]),
                                                width=q["width"], hdr=hdr, hdr_off=hdr_off, mask=mask, mask_mode=q["mode"], mask_byte=q["byte"],
                                                min_len=q["min_len"], **({} if level is None else {"level": level}))
        except _lib.FxError as e:
            err = fo.bad_query(e, ids, self._seq_counts, lo)
            raise (_fx_to_py(e) if err is e else err)

    def records(self, names_or_ids=None, starts=None, stops=None, strand=None, width=60, mask=None, mask_mode="soft", mask_char="N",
                uppercase=False, headers="auto", min_len=0):
        """Extension: FASTA records of whole sequences (names_or_ids None: every record) or of 0-based half-open intervals
        (starts, stops), formatted and laid out back to back on the GPU (csrc/fx_fasta_format.hpp) -> (uint8 buffer, int64
        offsets[n + 1]) in pinned memory.  A record is '>' header, then the letters in lines of `width` (0: one line).  The
        letters are those of fetch_many, then: upper-cased (uppercase=True, or a file opened with it); masked where `mask`
        -- any object with .ids / .starts / .stops (ClassRuns, TandemRepeats, Orfs, hit rows) or a 3-tuple of arrays, merged
        first -- covers their forward coordinate (mask_mode "soft": lower case, "upper": upper case, "hard": mask_char,
        "none"); reverse-complemented where strand (None, '+', '-' or one per row) says '-', case kept.  headers "auto": a
        whole record keeps its own header line, an interval gets name:start+1-stop, "(-)" appended on the minus strand;
        else one str / bytes per row.  A query with fewer than min_len letters produces no bytes (an empty range).  An
        unknown name: KeyError; a bad id or interval: IndexError / ValueError naming the row; a bad width, mask_mode or
        mask_char: ValueError."""
        q = self._records_plan(names_or_ids, starts, stops, strand, width, mask, mask_mode, mask_char, uppercase, headers, min_len)
        buf, offs, _, _ = self._records_call(q, 0, q["n"])
        return buf, offs

    def write(self, path, names_or_ids=None, starts=None, stops=None, strand=None, width=60, mask=None, mask_mode="soft", mask_char="N",
              uppercase=False, headers="auto", min_len=0, batch_bytes=1 << 30, compress=None):
        """Extension: the records of `records` written to the plain file `path`, in batches of consecutive queries whose
        size bound fits batch_bytes of pinned memory (a single larger query goes alone) -> {"records": records written,
        "bases": their letters, "dropped": queries that fell below min_len}.  compress: None or False: plain text; True (level
        2) or a level 0, 1, 2: a BGZF file, compressed on the GPU (csrc/fx_deflate.hpp) so that only compressed bytes come
        to the host -- every batch its own members (its last may be short), the EOF member once at the end; the result
        gains "compressed_bytes" (the file's size) and "members" (the EOF member included).  Anything else: ValueError."""
        from . import bgzf, fasta_out as fo
        level = bgzf.level_of(compress)
        q = self._records_plan(names_or_ids, starts, stops, strand, width, mask, mask_mode, mask_char, uppercase, headers, min_len)
        n, ids = q["n"], q["ids"]
        slen = np.asarray(self._table()["slen"], dtype=np.int64)
        if ids is not None:
            self._check_id_rows(ids)
        sl = slen if ids is None else slen[ids]
        if q["starts"] is not None:
            bad = np.flatnonzero((q["starts"] < 0) | (q["stops"] < q["starts"]) | (q["stops"] > sl))
            if bad.size:
                err = ValueError("interval outside the sequence (query %d)" % int(bad[0]))
                err.first_bad = int(bad[0])
                raise err
            letters = q["stops"] - q["starts"]
        else:
            letters = sl
        if q["hdr"] is not None:
            hl = np.diff(q["hdr"][1])
        else:
            hl = self._hdr_cols_host()[1]
            hl = hl if ids is None else hl[ids]
        bound = fo.size_bound(hl, letters, q["width"])
        fo._int(batch_bytes, "batch_bytes", 1)
        kept = bases = 0
        with open(path, "wb") as f:
            z = None if level is None else bgzf.Tally(f)
            for lo, hi in fo.batches(bound, batch_bytes):
                if z is None:
                    buf, _, k, b = self._records_call(q, lo, hi)
                    f.write(memoryview(buf))
                else:
                    stream, moff, _, k, b = self._records_call(q, lo, hi, level)
                    z.add(stream, moff)
                kept += k
                bases += b
            tail = {} if z is None else z.finish()
        return {"records": int(kept), "bases": int(bases), "dropped": int(n - kept), **tail}


class FastaKeys:
    """pyfastx.FastaKeys (fakeys.c): a view of the sequence names over the .fxi with the reference's sort / filter
    vocabulary -- `keys.sort(by='id'|'name'|'length', reverse=False)`, `keys.filter(keys > 700, keys % 'JZ8226')`,
    `keys.reset()`.  Comparisons and `%` do not filter by themselves: they return SQL fragments (comparisons accumulate,
    so that `600 <= keys <= 700` yields both bounds, fakeys.c:310-352) which filter() joins with AND."""

    _SORTS = {"id": "ID", "name": "chrom", "length": "slen"}                       # fakeys.c:7-8, 284-295

    def __init__(self, owner, n):
        self._owner, self._n = owner, n                      # the Fasta: its connection may be re-opened (bulk-loaded comp table)
        self._filter = self._order = self._temp = None
        self._cursor = None

    @property
    def _db(self):
        return self._owner._db

    def _where(self):
        return "WHERE %s" % self._filter if self._filter else ""

    def _select(self, tail=""):
        return "SELECT chrom FROM seq %s %s %s" % (self._where(), self._order or "ORDER BY ID", tail)

    def __len__(self):
        return self._n

    def __repr__(self):
        return "<FastaKeys> contains %d keys" % self._n                             # fakeys.c:168-170

    def __iter__(self):
        self._cursor = self._db.execute(self._select())                              # fakeys.c:140-145: restarts, returns self
        return self

    def __next__(self):
        if self._cursor is None:
            raise StopIteration
        row = self._cursor.fetchone()
        if row is None:
            self._cursor = None
            raise StopIteration
        return row[0]

    def __getitem__(self, item):
        if isinstance(item, slice):                                                  # fakeys.c:215-246 (the step is ignored there too)
            start, stop, step = item.indices(self._n)
            n = len(range(start, stop, step))
            if n <= 0:
                return []
            return [r[0] for r in self._db.execute(self._select("LIMIT %d OFFSET %d" % (n, start)))]
        if not hasattr(item, "__index__"):
            raise TypeError("fakeys indices must be integers or slices")
        i = item.__index__()
        if i < 0:
            i += self._n
        if i + 1 > self._n:
            raise IndexError("index out of range")
        if self._filter or self._order:
            row = self._db.execute(self._select("LIMIT 1 OFFSET ?"), (i,)).fetchone()
        else:
            row = self._db.execute("SELECT chrom FROM seq WHERE ID=?", (i + 1,)).fetchone()
        if row is None:
            raise ValueError("get item error")
        return row[0]

    def __contains__(self, name):
        if type(name) is not str:
            return False
        sql = "SELECT 1 FROM seq %s chrom=? LIMIT 1" % ("WHERE %s AND" % self._filter if self._filter else "WHERE")
        return self._db.execute(sql, (name,)).fetchone() is not None

    def sort(self, by="id", reverse=False):
        if by not in self._SORTS:
            raise ValueError("key only can be id, name or length")
        if by != "id" or reverse:                                                    # fakeys.c:297-299: sort('id') keeps the previous order
            self._order = "ORDER BY %s %s" % (self._SORTS[by], "DESC" if reverse else "ASC")
        return self

    def _compare(self, sign, other):
        if not isinstance(other, int):                                                # PyLong_Check, fakeys.c:316
            raise ValueError("the compared item must be an integer")
        term = "slen %s %d" % (sign, int(other))
        self._temp = term if self._temp is None else self._temp + " AND " + term
        return self._temp

    def __lt__(self, other):
        return self._compare("<", other)

    def __le__(self, other):
        return self._compare("<=", other)

    def __eq__(self, other):
        return self._compare("=", other)

    def __ne__(self, other):
        return self._compare("<>", other)

    def __gt__(self, other):
        return self._compare(">", other)

    def __ge__(self, other):
        return self._compare(">=", other)

    __hash__ = object.__hash__

    def __mod__(self, tag):
        if type(tag) is not str:
            raise ValueError("the tag after % must be a string")
        return "chrom LIKE '%%%s%%'" % tag                                            # fakeys.c:354-361

    def filter(self, *conds):
        if not conds:
            raise ValueError("no comparison condition provided")
        self._filter = " AND ".join(conds)
        self._temp = None
        self._n = int(self._db.execute("SELECT COUNT(1) FROM seq %s LIMIT 1" % self._where()).fetchone()[0])
        return self

    def reset(self):
        self._filter = self._order = self._temp = None
        row = self._db.execute("SELECT seqnum FROM stat").fetchone()
        if row is None:
            raise RuntimeError("get sequence counts error")
        self._n = int(row[0])
        return self


class FastqKeys:
    """pyfastx.FastqKeys (fqkeys.c): read names in file order -- len, index, `in`, iteration; no slices (sq_item only)."""

    def __init__(self, owner, n):
        self._owner, self._n = owner, n
        self._cursor = None

    def __len__(self):
        return self._n

    def __repr__(self):
        return "<FastqKeys> contains %d keys" % self._n                              # fqkeys.c:45-47

    def __iter__(self):
        self._cursor = self._owner._db.execute("SELECT name FROM read ORDER BY ID")
        return self

    def __next__(self):
        row = self._cursor.fetchone() if self._cursor is not None else None
        if row is None:
            self._cursor = None
            raise StopIteration
        return row[0]

    def __getitem__(self, i):
        if not hasattr(i, "__index__"):
            raise TypeError("sequence index must be integer, not '%s'" % type(i).__name__)
        i = i.__index__()
        if i < 0:
            i += self._n
        if i < 0 or i + 1 > self._n:
            raise IndexError("index out of range")
        row = self._owner._db.execute("SELECT name FROM read WHERE ID=? LIMIT 1", (i + 1,)).fetchone()
        if row is None:
            raise ValueError("get item error")
        return row[0]

    def __contains__(self, name):
        if type(name) is not str:
            return False
        return self._owner._db.execute("SELECT 1 FROM read WHERE name=? LIMIT 1", (name,)).fetchone() is not None


class Sequence(_fxobj.SeqCore):
    """pyfastx.Sequence (sequence.c:755-807).  start/end are 1-based inclusive.  The fields, slicing and the four sequence
    getters live in the C base type (csrc/fxobj.c): a slice of a line-regular record goes from there straight to the
    resident kernel; everything else lands in _get / _subscript_slow below."""

    __slots__ = ()                                            # every field is the base type's: no instance dict, the objects stay out of the cyclic GC

    def __init__(self, fasta, sid, name, boff, blen, slen, llen, elen, norm, dlen, start=1, end=None, complete=True):
        self._fa = fasta
        self.id, self._name = int(sid), name
        self._offset, self._byte_len, self._full_len = int(boff), int(blen), int(slen)
        self._line_len, self._end_len, self._normal, self._desc_len = int(llen), int(elen), int(norm), int(dlen)
        self.start = int(start)
        self.end = int(slen if end is None else end)
        self._complete = bool(complete)
        self._seq_len = self.end - self.start + 1 if not complete else int(slen)

    # ----------------------------------------------------------- arithmetic
    def _range(self, a, b):
        """0-based [a,b) of the FULL record -> (offset, byte_len); sequence.c:498-510, fasta.c:293-320."""
        bpl = self._line_len - self._end_len
        if bpl <= 0:
            raise ZeroDivisionError("record has an empty first line (llen == elen)")
        bs, be = a // bpl, b // bpl
        return self._offset + a + self._end_len * bs, (b - a) + (be - bs) * self._end_len

    def _line_regular(self):
        """May slices of this record go through the line arithmetic?  `norm` says "at most one line of another length"
        (index.c:342): true of a record whose last line is the short one, and of a record with ONE odd line anywhere
        else, which the arithmetic gets wrong.  The two are told apart by the line-regular column of the resident table
        (fx_fasta_line_regular: the scan, fx_fasta_set_table and the shard stitch all fill it with the same rule) or,
        for an index loaded from a file whose table has not been installed, by the same rule on the row and one byte
        of the stream (shard.line_regular_rule); the odd kind is sliced after despacing the whole record, which is what
        the reference returns from a warm cache and from Fasta.fetch() (sequence.c:100-110, fasta.c:440-461)."""
        return self._fa._regular(self)

    def _fetch_many(self, starts, stops, flags=0):
        """Bases [a,b) (0-based, of the full record) for several intervals, one GPU batch."""
        fl = flags | (_F_UP if self._fa._uppercase else 0)
        st = self._fa._st
        if self._line_regular():
            offs, bls, sls = [], [], []
            for a, b in zip(starts, stops):
                if b > a:
                    o, l = self._range(a, b)
                else:
                    o, l = self._offset, 0
                offs.append(o); bls.append(l); sls.append(max(b - a, 0))
            if len(offs) == 1:                               # a getter of one Sequence: one launch, no staging copies
                return [st.blob.fetch_one(offs[0], bls[0], sls[0], flags=fl) if sls[0] > 0 and bls[0] > 0 else b""]
            buf, o, ol = st.blob.fetch_ranges(offs, bls, sls, flags=fl)
            return [buf[o[i]:o[i] + ol[i]].tobytes() for i in range(len(offs))]
        # norm = 0: despace the whole record, then slice (sequence.c:100-110)
        full = st.fetch(self._offset, self._byte_len, max(self._full_len, 0), fl & _F_UP)
        out = []
        for a, b in zip(starts, stops):
            s = full[a:b]
            if flags & _F_COMP:
                s = _lib.revcomp_bytes(s, _F_COMP, st.device)
            if flags & _F_REV:
                s = s[::-1]
            out.append(s)
        return out

    def _get(self, flags=0):
        if self._seq_len <= 0:
            return ""
        if flags == 0 and self._complete and getattr(self, "_prefetched", None) is not None:
            return self._prefetched                             # came with the iterator's batch (Fasta.__iter__)
        if self._complete:
            # a whole sequence is the whole record despaced (pyfastx_sequence_get_fullseq, sequence.c:76-98) -- not the
            # line arithmetic, which a record with ONE odd line (norm = 1 all the same, index.c:342) would get wrong
            fl = flags | (_F_UP if self._fa._uppercase else 0)
            return _decode(self._fa._st.fetch(self._offset, self._byte_len, self._seq_len, fl))
        return _decode(self._fetch_many([self.start - 1], [self.end], flags)[0])

    # -------------------------------------------------------------- getters
    @property
    def name(self):
        return self._name if self._complete else "%s:%d-%d" % (self._name, self.start, self.end)    # sequence.c:291-297

    @property
    def description(self):
        return _text(self._fa._st.raw(self._offset - self._desc_len - self._end_len, self._desc_len))   # sequence.c:299-313

    @property
    def raw(self):
        if self._complete:                                                                               # sequence.c:314-335
            return _text(self._fa._st.raw(self._offset - self._desc_len - self._end_len - 1,
                                          self._byte_len + self._desc_len + self._end_len + 1))
        if self._normal and self._seq_len > 0:
            o, l = self._range(self.start - 1, self.end)
            return _decode(self._fa._st.raw(o, l))
        return _decode(self._fa._st.raw(self._offset, self._byte_len))

    def _counts(self):
        b = np.frombuffer(self.seq.encode("latin-1"), dtype=np.uint8)
        return np.bincount(b, minlength=256)

    @property
    def composition(self):
        c = self._counts()
        return {chr(l): int(c[l]) for l in range(32, 127) if c[l] > 0}

    @property
    def gc_content(self):
        c = self._counts()
        a, cc, g, t = c[65] + c[97], c[67] + c[99], c[71] + c[103], c[84] + c[116]
        return float(np.float32(g + cc) / np.float32(a + cc + g + t) * np.float32(100))

    @property
    def gc_skew(self):
        c = self._counts()
        cc, g = c[67] + c[99], c[71] + c[103]
        return float(np.float32(int(g) - int(cc)) / np.float32(g + cc))

    def search(self, subseq, strand="+"):
        """sequence.c:519-558: 1-based position of the first hit (of its last base for '-')."""
        q = subseq
        if strand == "-":
            q = _decode(_lib.revcomp_bytes(subseq.encode("latin-1"), _F_REV | _F_COMP, self._fa._st.device))
        i = self.seq.find(q)
        if i < 0:
            return None
        return i + len(q) if strand == "-" else i + 1

    # ------------------------------------------------------------ protocols
    def __len__(self):
        return self._seq_len

    def __str__(self):
        return self.seq

    def __repr__(self):
        if self._complete:
            return "<Sequence> %s with length of %d" % (self._name, self._seq_len)           # sequence.c:400-406
        return "<Sequence> %s from %d to %d" % (self._name, self.start, self.end)

    def __contains__(self, key):
        return type(key) is str and key in self.seq

    def __iter__(self):
        """Line iteration (sequence.c:162-263): complete sequences only, line ends stripped."""
        if not self._complete:
            raise RuntimeError("sliced subsequence cannot be read line by line")
        raw = self._fa._st.raw(self._offset, self._byte_len)
        for ln in raw.split(b"\n"):
            if ln.endswith(b"\r"):
                ln = ln[:-1]
            if ln:
                yield _decode(ln)

    def _subscript_slow(self, item):
        """pyfastx_sequence_subscript (sequence.c:412-517) for an integer (slices: SeqCore.__getitem__, from ABSOLUTE
        coordinates -- the reference's nested slicing is cache-history dependent)."""
        i = int(item)
        if i < 0:
            i += self._seq_len
        if i < 0 or i >= self._seq_len:
            raise IndexError("index out of range")
        return _decode(self._fetch_many([self.start - 1 + i], [self.start + i])[0])


_FXOBJ_BOUND = False


def _bind_fxobj():
    """Give the C types the address of fx_fetch_one (once the library is loaded: the first staged stream)."""
    global _FXOBJ_BOUND
    if not _FXOBJ_BOUND:
        import ctypes
        _fxobj.set_api(ctypes.cast(_lib.lib().fx_fetch_one, ctypes.c_void_p).value, Sequence)
        _FXOBJ_BOUND = True


_fxobj.set_api(0, Sequence)          # the types first; the entry point follows with the first staged stream


# =========================================================================== FASTQ
class Fastq(_fxobj.FastqCore):
    """pyfastx.Fastq (fastq.c:257-380, 1057-1107).  The subscript -- fq[i], fq[name] -- is the C base type's (csrc/fxobj.c:
    prepared statements on a read-only connection of its own, fastq.c:454-545); `_counts` and `_phred` are its members.

    What the subscript costs, and what the object keeps in HOST memory for it (none of it changes an answer; rates of a 2 M-read
    file, profiles/r05_iter_rate.json; the reference: 147 k fq[i].seq / s, 117 k fq[name].seq / s):
      * always: one prepared statement per subscript on the index file, 150-250 k reads/s.
      * an object that BUILT the index of at most FX_FQ_HOST_TABLE reads (default 16 000 000; 0: never) keeps the read table it
        wrote the file from -- six columns, 40 bytes per read, up to 640 MB -- and answers fq[i] from it: 1.2 M reads/s from the
        first subscript on.  It also keeps the names as they were packed for the file (up to 1 GiB); once fq[name] has been
        asked 64 times AND once per 90 reads of the file (22 000 look-ups for 2 M reads: those run at the statement's rate) it
        makes an open-addressing table of ids from them (8 bytes per read more) and answers by name from that: 0.84 M reads/s.
      * an object that LOADED an index file reads the integer columns from it in one pass once fq[i] has been asked 64 times and
        once per 22 reads (then 1.5 M reads/s; 246 k/s over the first 200 000 subscripts, the pass included), and the names once
        fq[name] has been asked 64 times and once per 25 reads -- the same arrays, the same limits.
      * above FX_FQ_HOST_TABLE reads nothing is kept and the statements stay (a 10^8-read index is written from the device and
        no table comes to the host at all)."""

    def __init__(self, file_name, index_file=None, phred=0, build_index=True, full_index=False, full_name=False,
                 device=0, devices=None):
        """devices=[0, 1, ...] (extension): the stream over several GPUs by byte range, one host thread per device,
        ONE index file, batches routed by read id (windows.WindowedFastq)."""
        if not os.path.isfile(file_name):
            raise FileExistsError("input fastq file %s does not exists" % file_name)          # fastq.c:278-281
        if devices is not None and len(devices) > 1 and not build_index:
            raise ValueError("devices=[...] builds an index: build_index must stay on")
        if devices:
            device = devices[0]
        self.file_name = file_name
        self.is_gzip = _is_gzip(file_name)
        if _first_nonspace(file_name, self.is_gzip) != ord("@"):                              # fastq.c:300-304
            raise RuntimeError("%s is not plain or gzip compressed fastq formatted file" % file_name)
        self._st = _Staged(file_name, device)
        import weakref
        me = weakref.ref(self)

        def staged(blob, me=me):                               # single getters of a plain file: from the page cache (csrc/fxobj.c: read_get_seq)
            fq = me()
            if fq is not None:
                fq._core_stage(int(blob._h.value or 0), None if fq.is_gzip or os.environ.get("FX_NO_HOST_GETTERS") else fq.file_name)

                def closed(me=me):
                    f2 = me()
                    if f2 is not None:
                        f2._core_stage(0)
                blob.on_close.append(closed)
        self._st.on_stage = staged
        self._want_comp = bool(build_index and full_index)
        if build_index:
            self._st.win_factor = 1.7                          # line records + read table beside the stream

            def windowed(plan, me=me, path=file_name, dev=device):
                from .windows import WindowedFastq
                fq = me()
                return WindowedFastq(path, dev, window=plan[2], capacity=plan[3], want_comp=bool(fq is not None and fq._want_comp),
                                     index_file=(fq._index_file if fq is not None and _dev_index_applies(fq._index_file) else None))
            self._st.windowed = windowed
            if devices is not None and len(devices) > 1:
                def forced(me=me, path=file_name, devs=list(devices)):
                    from .windows import WindowedFastq
                    fq = me()
                    return WindowedFastq(path, devices=devs, want_comp=bool(fq is not None and fq._want_comp))
                self._st.forced = forced
        self._index_file = index_file or file_name + ".fxi"
        self._phred = int(phred)
        self._has_index = bool(build_index)
        self._full_name = bool(full_name)
        self._db = None
        self._counts, self.size, self.avglen = 0, 0, 0.0
        self._meta = None
        self.build_phases = self.index_phases = None
        t0 = time.perf_counter()
        if fxi.exists(self._index_file):                                                      # fastq.c:347-351
            self._load_index()
        elif build_index:
            self._create_index()
        t1 = time.perf_counter()
        if build_index and full_index:
            self._calc_composition()
        t2 = time.perf_counter()
        self._bind_core()
        # where the constructor's time went, in seconds (build_phases / index_phases: the parts of the first one)
        self.ctor_phases = {"index_s": t1 - t0, "composition_s": t2 - t1, "bind_s": time.perf_counter() - t2}

    def _bind_core(self):
        """fq[i] / fq[name] from C once the index is a file on disk (csrc/fxobj.c: FastqCore)."""
        ok = self._db is not None and self._index_file != ":memory:" and os.path.isfile(self._index_file) and not os.environ.get("FX_NO_C_SUBSCRIPT")
        self._core_open(self._index_file if ok else None)
        t = getattr(self, "_host_tab", None)
        if ok and t is not None and len(t["soff"]) == self._counts:
            self._core_table(t["name_off"], t["name_len"], t["dlen"], t["rlen"], t["soff"], t["qoff"])
        else:
            self._core_table()
        nm = getattr(self, "_host_names", None)
        if ok and nm is not None and self._core_table_rows == self._counts == len(nm[1]) - 1:
            self._core_names(nm[0], nm[1])
        else:
            self._core_names()
        # an object that loaded its index file reads the table from it once fq[i] has been asked for often enough (csrc/fxobj.c)
        self._core_table_cap = int(os.environ.get("FX_FQ_HOST_TABLE", 16_000_000)) if ok else 0

    def build_index(self):
        if self._db is None:
            if fxi.exists(self._index_file):
                self._load_index()
            else:
                self._create_index()
            self._bind_core()
        self._has_index = True
        return True

    def _load_index(self):
        self._db = fxi.connect(self._index_file)
        if self.is_gzip:                                     # fastq.c:396: the zran points of the index file are used by the next open
            self._st.gzindex = lambda: fxi.read_gzindex(self._db)
        try:
            row = self._db.execute("SELECT * FROM stat LIMIT 1").fetchone()
        except Exception:
            row = None
        if row is None:
            raise RuntimeError("the index file %s was damaged" % self._index_file)            # fastq.c:210-214
        self._counts, self.size, self.avglen = int(row[0]), int(row[1]), float(row[2])
        m = self._db.execute("SELECT phred FROM meta LIMIT 1").fetchone()
        if m and not self._phred:
            self._phred = int(m[0])

    def _create_index(self):
        """pyfastx_fastq_create_index (fastq.c:8-182) with the scan on the GPU."""
        # a large plain file: the index file is created now and grows to its estimated size while the input is staged
        # (fxi.presize_fastq; the pages that fill it are formatted on the device once the table exists)
        fits = True
        if not self.is_gzip and self._st.windowed is not None and self._st._blob is None:
            from . import windows
            try:                                              # (a stream built in windows writes its own file, range by range: no early file)
                fits = windows.plan(self.file_name, self._st.device, self._st.win_factor) is None
            except _lib.FxError:
                fits = True
        early = None
        if fits and not self.is_gzip and _dev_index_applies(self._index_file) and self._st.forced is None and not os.environ.get("FX_FXI_NO_PRESIZE"):
            def presize():
                try:
                    return fxi.presize_fastq(self._index_file, self.file_name, device=self._st.device, with_index=True)     # (the index holds names cut at the first white space whatever full_name says: fastq.c:112-117)
                except Exception:                             # noqa: BLE001  (no early file: the build makes it -- and must find none)
                    if os.path.exists(self._index_file):
                        os.remove(self._index_file)
                    return None
            # in a thread of its own: the estimate reads eight windows of the input and sizes their records in Python (9 ms for
            # C3) -- beside the first milliseconds of the staging instead of in front of it; the body asks for the token when it
            # needs it (once the stream is staged)
            import threading
            box = {}
            th = threading.Thread(target=lambda: box.__setitem__("tok", presize()))
            th.start()

            def early():
                th.join()
                return box.get("tok")
        try:
            self._create_index_body(early)
        except BaseException:
            tok = early() if early is not None else None
            _lib.fxi_presize_end(tok, cancel=True)
            if tok is not None and os.path.exists(self._index_file):
                os.remove(self._index_file)
            raise

    def _create_index_pipelined(self, tok, t_begin):
        """A large plain file whose index file has its room already (fxi.presize_fastq): the input is staged in the background
        (Blob.from_file_async) and taken in byte ranges as they land -- scan + rows of the range through a VIEW of the blob (the
        sharded build's machinery: line counts of the ranges before, a halo behind), its table leaves formatted on the device and
        copied into the file (fxi.PartsWriter) while the next ranges are still arriving: host-to-device and device-to-host run at
        the same time, the link is full duplex.  When everything has landed: one build over the whole blob (the object's table,
        11 ms), one sort of all names, the index leaves.  -> True; False when this route does not apply (then nothing was done)."""
        from . import shard, windows
        st = self._st
        # Off unless FX_FQ_PIPELINE=1.  Measured for C3 (10^8 reads, tools/c3_phases.py, two constructors each on one box): 1.32 / 1.58 s
        # this way, 1.32 / 1.35 when nothing is written before the index file's room is all there, 1.36 / 1.11 with one blob and one
        # build (round 5's route, the default): on this host the copy-out, the staging and the allocation of the file's pages share
        # the memory bandwidth of one socket -- the staging slows from 0.63 to 0.73-0.97 s while leaves are written beside it.
        if st._blob is not None or st.windowed is None or os.environ.get("FX_FQ_NO_PIPELINE") or os.environ.get("FX_FQ_PIPELINE", "0") == "0":
            return False
        size = os.path.getsize(self.file_name)
        step = int(os.environ.get("FX_FQ_PIPELINE_RANGE", 4 << 30)) & ~4095
        if step < (1 << 16) or size < 2 * step or windows.plan(self.file_name, st.device, st.win_factor) is not None:
            return False
        R = -(-size // step)
        try:
            blob = _lib.Blob.from_file_async(self.file_name, st.device)
        except _lib.FxError:
            return False
        views, jobs, laps = [], [], {}
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=1)                  # the parts go into the writer in order, one after the other
        w = None
        try:
            wait_room = os.environ.get("FX_FQ_PIPELINE_WAIT_ROOM", "0") != "0"
            if wait_room:                                         # (experiment: nothing is written before all the room is there)
                _lib.fxi_presize_end(tok)
                tok = None
            w = fxi.PartsWriter(self._index_file, 1, st.device, schema_done=True)
            ptr = int(blob.device_ptr)
            cores, prev = [], 10
            for r in range(R):
                a, e = r * step, min(size, (r + 1) * step)
                halo = min(1 << 16, size - e)
                while True:
                    blob.stage_wait(e + halo)
                    v = _lib.Blob.from_device(ptr + a, (e - a) + halo, st.device)
                    v.set_shard(a, prev, e + halo >= size and halo == size - e)
                    v.set_halo(halo)
                    core = v.fastq_scan()
                    ctx = shard.fastq_contexts(cores + [core])[r]
                    try:
                        v.fastq_build_ctx(*ctx)
                        break
                    except _lib.FxError as ex:                    # a read longer than the halo: the range with a larger one
                        v.close()
                        if ex.code != _lib.FX_ERANGE or halo >= size - e:
                            raise
                        halo = min(halo * 8, size - e)
                cores.append(core)
                if e < size:
                    prev = v.read_bytes(e - 1, 1)[0]
                views.append(v)
                jobs.append(pool.submit(w.add_local, v, st.device))
            blob.stage_wait(-1)
            t_staged = time.perf_counter()
            s = blob.fastq_build(comp=self._want_comp)            # the object's own table: one pass over the whole blob
            t_ready = time.perf_counter()
            scan_laps = _lib.build_laps()
            for j in jobs:
                j.result()
            t_leaves = time.perf_counter()
            if w.rows != int(s.n_reads):
                raise RuntimeError("the ranges hold %d reads, the whole stream %d" % (w.rows, int(s.n_reads)))
            _lib.fxi_presize_end(tok)                             # (the thread that made the room: done long ago)
            tok = None
            self._db = w.finish()
            n, size_b = int(s.n_reads), int(s.size)
            self._db.execute("INSERT INTO stat VALUES (?,?,?)", (n, size_b, size_b * 1.0 / n if n else float("nan")))     # fastq.c:161
        except BaseException:
            pool.shutdown(wait=True)
            _lib.fxi_presize_end(tok, cancel=True)
            for v in views:
                v.close()
            blob.close()
            if w is not None:
                w.abort()
            elif os.path.exists(self._index_file):
                os.remove(self._index_file)
            raise
        pool.shutdown(wait=True)
        for v in views:
            v.close()
        st._blob = blob
        if st.on_stage is not None:
            st.on_stage(blob)
        t_done = time.perf_counter()
        self._host_tab = self._host_names = None
        self.index_phases = dict(w.laps, table_leaves_done_after_staging_s=t_leaves - t_ready)
        al, _ = _lib.open_laps()
        self.build_phases = {"staging_s": t_staged - t_begin, "device_alloc_s": al, "page_cache_to_hbm_s": t_staged - t_begin - al, "scan_s": t_ready - t_staged,
                             "index_ready_s": t_ready - t_begin, "fxi_s": t_done - t_ready, "fxi_durable_s": t_done - t_begin, "room_set_aside_early": True,
                             "pipelined_ranges": R, "scan_laps_s": {k: round(v, 4) for k, v in scan_laps.items()}}
        self._counts, self.size = int(s.n_reads), int(s.size)
        self.avglen = self.size * 1.0 / self._counts if self._counts else float("nan")
        keep = 0 < s.n_reads <= int(os.environ.get("FX_FQ_HOST_TABLE", 16_000_000))
        if keep:
            t = self._host_tab = blob.fastq_table(s.n_reads)
            names, offs = blob.names_pack(1, s.n_reads, guess=int(np.maximum(t["name_len"], 0).astype(np.int64).sum()))
            if names.nbytes <= (1 << 30):
                self._host_names = (np.ascontiguousarray(names), offs)
        return True

    def _create_index_body(self, early):
        """early: None, or a callable -> the token of the index file's room set aside in the background (fxi.presize_fastq), None
        when nothing was set aside; asked once the stream is staged (the pipelined route, off by default, asks at once)."""
        t_begin = time.perf_counter()
        tok = None
        if early is not None and os.environ.get("FX_FQ_PIPELINE", "0") != "0":
            tok = early()
            early = None
            if tok is not None and self._create_index_pipelined(tok, t_begin):
                return
        wq = self._st.md
        if early is not None:
            tok = early()
        presized = tok is not None
        if presized and wq is not None:                       # (built in windows after all: that route writes its own file)
            _lib.fxi_presize_end(tok, cancel=True)
            os.remove(self._index_file)
            presized = False
        if wq is not None:                                    # larger than the HBM it may use: built window after window (windows.WindowedFastq)
            self._db = None
            riding = getattr(wq, "_writer", None) is not None and wq._writer.path == self._index_file      # (the ranges' leaves are in that file already)
            if wq.n_reads and self._index_file != ":memory:" and (riding or not os.path.exists(self._index_file)):
                try:
                    self._db = wq.write_index(self._index_file)
                except _lib.FxError:
                    self._db = None
            if self._db is None:
                if riding and os.path.exists(self._index_file):   # (a writer that gave up removes its file; one that was never asked does not)
                    os.remove(self._index_file)
                nm, no = wq.names.tobytes(), wq.name_off.tolist()
                self._db = fxi.connect(self._index_file)
                fxi.write_fastq(self._db, [nm[no[i]:no[i + 1]] for i in range(wq.n_reads)], wq.table, wq.size)
            if self.is_gzip:
                c, u, _ = wq.blobs[0].gz_points()
                fxi.write_gzindex(self._db, os.path.getsize(self.file_name), wq.stream_bytes, c, u)
            self._counts, self.size = int(wq.n_reads), int(wq.size)
            self.avglen = self.size * 1.0 / self._counts if self._counts else float("nan")
            return
        blob = self._st.blob
        t_staged = time.perf_counter()
        try:
            s = blob.fastq_build(comp=self._want_comp)        # full_index: base / meta are counted on the way, one read of the stream for both
        except _lib.FxError as e:
            raise _fx_to_py(e)
        t_ready = time.perf_counter()                         # the read table is in HBM: batches by read id can be served from here on
        scan_laps = _lib.build_laps()
        # the table the index file is written from stays with the object (up to FX_FQ_HOST_TABLE rows, 16 M = 640 MB; 0: never):
        # fq[i] then is six array elements in C instead of a statement on the index file (csrc/fxobj.c: _core_table)
        keep = 0 < s.n_reads <= int(os.environ.get("FX_FQ_HOST_TABLE", 16_000_000))
        t = None
        self._host_tab = self._host_names = None
        self._db = None
        self.index_phases = None
        if presized:
            _lib.fxi_presize_end(tok)                         # (done long before the staging is)
        if s.n_reads or presized:
            dv = _dev_index(self._index_file, blob, 1, s.n_reads, s.size, presized) if s.n_reads else None     # pages formatted on the device: nothing but pages comes to the host
            if dv is None and presized and os.path.exists(self._index_file):
                os.remove(self._index_file)
            if dv is not None:
                self._db, self.index_phases = dv
                if keep:
                    t = self._host_tab = blob.fastq_table(s.n_reads)
                    names, offs = blob.names_pack(1, s.n_reads, guess=int(np.maximum(t["name_len"], 0).astype(np.int64).sum()))
                    if names.nbytes <= (1 << 30):
                        self._host_names = (np.ascontiguousarray(names), offs)
        if self._db is None and s.n_reads:
            t = blob.fastq_table(s.n_reads)
            self._host_tab = t if keep else None

            def write(p, names, offs, order):
                # the names as they were packed for the index file stay too (up to 1 GiB of them): fq[name] is a hash look-up in C
                if self._host_tab is not None and names.nbytes <= (1 << 30):
                    self._host_names = (np.ascontiguousarray(names), offs)
                return fxi.write_fastq_bulk(p, names, offs, t, s.size, order)
            self._db = _bulk_index(self._index_file, blob, 1, s.n_reads, t["name_off"], t["name_len"], write)
        if self._db is None:
            if t is None:
                t = blob.fastq_table(s.n_reads)
            names = []
            step = 1 << 20
            for a in range(0, s.n_reads, step):
                b = min(s.n_reads, a + step)
                ln = t["name_len"][a:b].astype(np.int64)
                buf, offs, _ = blob.fetch_ranges(t["name_off"][a:b], ln, ln, flags=_F_RAW)
                raw = buf.tobytes()
                o = offs.tolist()
                names.extend(raw[o[i]:o[i + 1]] for i in range(b - a))        # raw bytes, stored verbatim
            self._db = fxi.connect(self._index_file)
            fxi.write_fastq(self._db, names, t, s.size)
        if self.is_gzip:
            self._st.write_gzindex(self._db)
        t_done = time.perf_counter()
        # where the constructor's time went (seconds): the stream to HBM, the index kernels ("index ready": the table is
        # resident), the index file durable on disk; index_phases has the parts of the last step when the device wrote it
        al, st = _lib.open_laps() if not self.is_gzip else (0.0, 0.0)
        self.build_phases = {"staging_s": t_staged - t_begin, "device_alloc_s": al, "page_cache_to_hbm_s": st, "scan_s": t_ready - t_staged, "index_ready_s": t_ready - t_begin,
                             "fxi_s": t_done - t_ready, "fxi_durable_s": t_done - t_begin, "room_set_aside_early": bool(presized),
                             "scan_laps_s": {k: round(v, 4) for k, v in scan_laps.items()}}
        self._counts, self.size = int(s.n_reads), int(s.size)
        self.avglen = self.size * 1.0 / self._counts if self._counts else float("nan")

    def _calc_composition(self):
        """pyfastx_fastq_calc_composition (fastq.c:663-795)."""
        if self._meta is not None:
            return
        row = self._db.execute("SELECT * FROM meta LIMIT 1").fetchone()
        if row is None:
            if self._st.md is not None:                       # windows: five sums, two minima, two maxima over them
                base, meta = self._st.md.composition()
            else:
                blob = self._st.blob
                if getattr(blob, "_n_fastq", None) is None:       # (an index that was loaded: the stream has not been scanned yet)
                    blob.fastq_build(comp=True)
                base, meta = blob.fastq_comp()
            fxi.write_fastq_comp(self._db, base, meta)
            row = tuple(int(x) for x in meta)
        self._meta = {"maxlen": int(row[0]), "minlen": int(row[1]), "minqs": int(row[2]), "maxqs": int(row[3]),
                      "phred": int(row[4])}
        if not self._phred:
            self._phred = self._meta["phred"]

    # ------------------------------------------------------------ protocols
    def __len__(self):
        return self._counts

    def __repr__(self):
        if self._has_index:
            return "<Fastq> %s contains %d reads" % (self.file_name, self._counts)             # fastq.c:547-553
        return "<Fastq> %s" % self.file_name

    def _getitem_slow(self, item):
        """pyfastx_fastq_subscript (fastq.c:521-545) through the sqlite3 module: what the C base type does not take (an
        index in memory, numpy integers, a library it could not bind)."""
        if isinstance(item, str):
            row = self._db.execute("SELECT * FROM read WHERE name=? LIMIT 1", (item,)).fetchone()
            if row is None:
                raise KeyError("%s does not exist in fastq file" % item)
            return Read(self, *row)
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            i = int(item)
            if i < 0:
                i += self._counts
            if i >= self._counts:
                raise IndexError("index out of range")
            row = self._db.execute("SELECT * FROM read WHERE ID=? LIMIT 1", (i + 1,)).fetchone()
            if row is None:
                raise IndexError("Index Error")
            return Read(self, *row)
        raise KeyError("the key must be index number or read name")

    def __contains__(self, key):
        if not isinstance(key, str) or self._db is None:
            return False
        return self._db.execute("SELECT 1 FROM read WHERE name=? LIMIT 1", (key,)).fetchone() is not None

    def __iter__(self):
        if not self._has_index:
            # build_index=False: (name, seq, qual) tuples from kseq_read (fastq.c:598-622): the device path of Fastx
            return _kseq_iter(lambda: self._st.blob, False, fastq=True, upper=False, comment_mode=2 if self._full_name else 0)
        return self._iter_indexed()

    def _iter_indexed(self):
        # sequence and quality lines of 16384 reads per gather ride along in the Read objects.  The rows of the
        # `read` table are stepped from C (_fxobj.RowCursor: sqlite3_step / sqlite3_column_* as fastq.c:566-596 does, a
        # read-only connection of its own through the library the sqlite3 module has loaded) and the objects of a batch made
        # by one call; when that connection cannot be had (an index another connection holds exclusively), the sqlite3
        # module's rows do the same, more slowly.
        if self._st.md is None and not os.environ.get("FX_ITER_SQLITE"):
            # the rows from the read table of the DEVICE (one copy to the host, fx_fastq_table), the names gathered with the
            # sequence and quality lines: no statement stepped per read (0.19 of the 0.9 us a read cost in round 3)
            blob = self._dev()
            tab, n, B = self._tab_host, int(self._counts), 16384
            if n == tab["rlen"].size:
                for a in range(0, n, B):
                    b = min(n, a + B)
                    seq, qual, _, offs = blob.read_fetch(tab["soff"][a:b], tab["qoff"][a:b], tab["rlen"][a:b], want=("seq", "qual"))
                    ln = np.maximum(tab["name_len"][a:b].astype(np.int64), 0)
                    nbuf, noffs, _ = blob.fetch_ranges(tab["name_off"][a:b], ln, ln, flags=_F_RAW)
                    yield from _fxobj.read_batch_arrays(Read, self, a + 1, nbuf, noffs, tab["dlen"][a:b].astype(np.int64), tab["rlen"][a:b],
                                                        tab["soff"][a:b], tab["qoff"][a:b], seq, qual, offs)
                return
        batch = None
        try:
            cur = _fxobj.RowCursor(self._index_file, "SELECT ID, name, dlen, rlen, soff, qoff FROM read ORDER BY ID")
            batch = cur.fetch(16384)
        except RuntimeError:
            cur = None
        if cur is not None:
            while batch is not None:
                k, names, raw = batch
                cols = np.frombuffer(raw, dtype=np.int64).reshape(5, k)                     # ID, dlen, rlen, soff, qoff
                seq, qual, _, offs = self._st.blob.read_fetch(cols[3], cols[4], cols[2], want=("seq", "qual"))
                yield from _fxobj.read_batch_cols(Read, self, names, raw, seq, qual, offs)
                batch = cur.fetch(16384)
            return
        if True:
            cur = self._db.execute("SELECT * FROM read ORDER BY ID")
            while True:
                rows = cur.fetchmany(16384)
                if not rows:
                    return
                seq, qual, _, offs = self._st.blob.read_fetch([r[4] for r in rows], [r[5] for r in rows], [r[3] for r in rows],
                                                              want=("seq", "qual"))
                yield from _fxobj.read_batch(Read, self, rows, seq, qual, offs)          # the batch's objects made in C, strings included

    def keys(self):
        return FastqKeys(self, self._counts)                                                   # fastq.c:555-557

    # -------------------------------------------------------------- getters
    @property
    def phred(self):
        self._calc_composition()
        return self._phred

    @property
    def composition(self):
        self._calc_composition()
        a, c, g, t, n = self._db.execute("SELECT * FROM base LIMIT 1").fetchone()
        return {"A": a, "C": c, "G": g, "T": t, "N": n}

    @property
    def gc_content(self):
        self._calc_composition()
        a, c, g, t, n = self._db.execute("SELECT * FROM base LIMIT 1").fetchone()
        return float(np.float32(g + c) / np.float32(a + c + g + t) * np.float32(100))          # fastq.c:809-878

    @property
    def maxlen(self):
        self._calc_composition()
        return self._meta["maxlen"]

    @property
    def minlen(self):
        self._calc_composition()
        return self._meta["minlen"]

    @property
    def maxqual(self):
        self._calc_composition()
        return self._meta["maxqs"]

    @property
    def minqual(self):
        self._calc_composition()
        return self._meta["minqs"]

    @property
    def encoding_type(self):
        """fastq.c:797-878: platforms compatible with the observed quality range."""
        self._calc_composition()
        lo, hi = self._meta["minqs"], self._meta["maxqs"]
        if lo < 33 or hi > 126:
            return ["Unknown"]
        out = []
        for name, a, b in (("Sanger Phred+33", 33, 73), ("Illumina 1.8+ Phred+33", 33, 74),
                           ("Solexa Solexa+64", 59, 104), ("Illumina 1.3+ Phred+64", 64, 104),
                           ("Illumina 1.5+ Phred+64", 66, 104), ("PacBio HiFi Phred+33", 33, 126)):
            if lo >= a and hi <= b:
                out.append(name)
        return out

    def ids_of(self, names):
        """Batched `fq[name].id - 1`: read names -> 0-based ids (-1 when absent) through the name table in HBM
        (fx_names_lookup) instead of one SQLite probe per name (fastq.c:486-519)."""
        blob = self._dev()
        if self._st.md is not None:                           # windows: no name table in HBM -- one probe of the index file per name (fastq.c:486-519)
            if isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, int)):
                o = np.frombuffer(names[1], dtype=np.int64) if not isinstance(names[1], np.ndarray) else names[1]
                raw = bytes(memoryview(names[0]))
                names = [raw[int(o[i]):int(o[i + 1])].decode("utf-8", "surrogateescape") for i in range(len(o) - 1)]
            out = np.full(len(names), -1, dtype=np.int64)
            for i, nm in enumerate(names):
                row = self._db.execute("SELECT ID FROM read WHERE name=? LIMIT 1", (nm if isinstance(nm, str) else nm.decode("utf-8", "surrogateescape"),)).fetchone()
                if row is not None:
                    out[i] = int(row[0]) - 1
            return out
        if not getattr(self, "_names_ready", False):
            blob.names_build(1)
            self._names_ready = True
        return blob.names_lookup(names)

    def _dev(self):
        blob = self._st.blob
        if self._st.md is not None:                           # windows: the merged table lives on the host, the windows answer by byte range
            if not getattr(self, "_dev_table", False):
                self._tab_host = self._st.md.table
                self._rlen_host = self._tab_host["rlen"]
                self._dev_table = True
            return blob
        if not getattr(self, "_dev_table", False):
            s = blob.fastq_build()
            self._tab_host = blob.fastq_table(s.n_reads)       # host copy of the read table: what batches index into
            self._rlen_host = self._tab_host["rlen"]
            self._dev_table = True
        return blob

    def fetch_many(self, ids_or_names, want=("seq", "qual", "quali")):
        """Batched extension: reads by 0-based id (or by name; or names pre-packed as a (bytes, int64 offsets[n + 1]) pair)
        in one launch -> dict of buffers + offsets.  Read lengths are gathered and laid out on the device, the outputs
        arrive by DMA in pinned memory (fx_fastq_fetch_alloc)."""
        blob = self._dev()
        packed = isinstance(ids_or_names, tuple) and len(ids_or_names) == 2 and isinstance(ids_or_names[0], (bytes, bytearray, memoryview, np.ndarray)) \
            and not isinstance(ids_or_names[1], (str, int))
        if packed or (len(ids_or_names) and isinstance(ids_or_names[0], str)):
            ids = self.ids_of(ids_or_names)
            if (ids < 0).any():
                k = int(np.nonzero(ids < 0)[0][0])
                if packed:
                    o = np.frombuffer(ids_or_names[1], dtype=np.int64) if not isinstance(ids_or_names[1], np.ndarray) else ids_or_names[1]
                    nm = bytes(memoryview(ids_or_names[0])[int(o[k]):int(o[k + 1])]).decode("utf-8", "surrogateescape")
                else:
                    nm = ids_or_names[k]
                raise KeyError("%s does not exist in fastq file" % nm)
        else:
            ids = np.asarray(ids_or_names, dtype=np.int64)
        if self._st.md is not None:                           # windows: routed by read id, staged on demand
            seq, qual, qi, offs = self._st.md.fetch(ids, phred=self._phred, want=want)
            return {"seq": seq, "qual": qual, "quali": qi, "offsets": offs}
        try:
            seq, qual, qi, offs = blob.fastq_fetch_alloc(ids, phred=self._phred, want=want)
        except _lib.FxError as e:
            if e.code == _lib.FX_ERANGE and getattr(e, "first_bad", -1) >= 0:
                raise IndexError("index out of range")
            raise
        return {"seq": seq, "qual": qual, "quali": qi, "offsets": offs}

    def _qc_blob(self):
        """The blob with the read table resident, for the quality-control passes; they run over one whole stream."""
        if self._sharded:
            raise NotImplementedError("quality control on a sharded or windowed stream")
        return self._dev()

    @property
    def _sharded(self):
        """Several devices or several windows: the stream is not one resident blob (windows.WindowedFastq)."""
        return self._st.md is not None

    def read_stats(self, ids=None, low_qual=20):
        """Extension: per-read quality statistics, computed on the GPU from the resident stream (csrc/fx_fastq_qc.hpp) ->
        dict of numpy columns in pinned memory, one row per id (0-based, any order, repeats allowed; None: every read in
        read order).  With s = fq[i].seq, q = fq[i].qual as bytes and p = fq.phred (33 when 0): length = len(s); qsum = sum
        of q[j] - p; qmin / qmax = its smallest / largest term (0 for an empty read); n_low = terms below low_qual
        (0..255); n_gc = G and C in s; n_other = bytes of s outside upper-case A C G T.  A bad id: IndexError."""
        from . import qc
        return qc.read_stats_blob(self._qc_blob(), self._rlen_host.size, ids, self.phred, low_qual)

    def cycle_profile(self, cycles=None):
        """Extension: quality and base histograms per cycle (position in the read) over all reads -> qc.CycleProfile with
        qual int64[cycles, 256] (reads per raw quality byte), base int64[cycles, 5] (A C G T other), depth int64[cycles]
        (reads longer than the cycle), and the derived qual_scores / mean_qual.  cycles: 1..65536, default fq.maxlen;
        positions at or beyond it are not counted, rows beyond the longest read are zero."""
        from . import qc
        if cycles is not None:
            cycles = qc.check_cycles(cycles)
        blob = self._qc_blob()
        return qc.cycle_profile_blob(blob, max(int(self.maxlen), 1) if cycles is None else cycles, self.phred)

    def select(self, min_len=None, max_len=None, min_mean_qual=None, max_low_frac=None, max_other=None, low_qual=20):
        """Extension: the ascending 0-based ids (int64, pinned memory) of the reads that pass every criterion given, with the
        columns of read_stats: min_len <= length <= max_len; mean of q - p at least min_mean_qual; at most the fraction
        max_low_frac of the terms below low_qual; at most max_other bytes outside A C G T.  The two ratios are taken as
        fractions with a denominator <= 1000 and compared in integers on the device (an empty read passes both); only the
        ids come to the host, and fetch_many / raw_many take them as they are."""
        from . import qc
        args = qc.select_args(min_len, max_len, min_mean_qual, max_low_frac, max_other, low_qual)
        return self._qc_blob().fastq_select(phred=self.phred, **args)

    def trim(self, ids=None, clip_front=0, clip_tail=0, adapter=None, min_overlap=3, max_error_rate=0.1, front_qual=None,
             window=None, tail_qual=None):
        """Extension: per read the interval [start, end) that survives trimming, computed on the GPU from the resident stream
        (csrc/fx_fastq_trim.hpp) -> {"start": int64[n], "end": int64[n]} in pinned memory; row k belongs to ids[k] (0-based,
        any order, repeats allowed), or to read k.  The steps run in this order, each on what the one before left, with s =
        fq[i].seq, q = fq[i].qual as bytes, d = q - fq.phred (33 when 0): 1 clip_front / clip_tail bases off the ends; 2 the
        3' adapter (1..64 letters of A C G T N, N matches anything; read bytes as they are): cut at the first position where
        the adapter -- or, at the read's end, its first min_overlap or more letters -- matches with at most max_error_rate
        mismatches per compared letter (no indels); 3 front_qual: bases with d below it off the 5' end; 4 window = (length,
        mean): cut at the start of the first window of that many bases (the whole read, if shorter) whose mean d is below
        mean; 5 tail_qual: bases with d below it off the 3' end.  A step that is not given does nothing.  A bad id:
        IndexError; a bad argument: ValueError."""
        from . import trim as _trim
        args = _trim.trim_args(clip_front, clip_tail, adapter, min_overlap, max_error_rate, front_qual, window, tail_qual)
        return _trim.trim_blob(self._qc_blob(), self._rlen_host.size, ids, self.phred, args)

    def kmer_counts(self, k, canonical=False, ids=None, start=None, end=None):
        """Extension: the k-mer spectrum of seq[start:end] of the reads `ids` -> int64[4**k] in pinned memory, counted on the
        GPU from the resident stream (csrc/fx_kmer.hpp); the definition is Fasta.kmer_counts' (1 <= k <= 13).  ids, start and
        end follow the rules of records: ids 0-based, any order, repeats allowed, None for every read; start / end both
        None (whole reads) or what trim returned for the same ids -- fq.kmer_counts(11, ids=keep, start=iv["start"],
        end=iv["end"]) is the spectrum of the selected, trimmed reads without a byte of them leaving the device."""
        from . import kmer
        k = kmer.check_k(k)
        return kmer.fastq_counts_blob(self._qc_blob(), self._rlen_host.size, k, canonical, ids, start, end)

    def complexity(self, ids=None, start=None, end=None):
        """Extension: per-read sequence complexity of s = seq[start:end] of the reads `ids`, counted on the GPU from the
        resident stream (csrc/fx_dust.hpp) -> dict of numpy columns, one row per query; ids, start and end follow
        kmer_counts.  length = len(s); n_triplets (int32) = the triplets of s whose three letters are A C G T (either case);
        dust_sum (int64) = sum c (c - 1) / 2 over the counts c of the 64 triplet codes; n_diff (int32) = the positions j
        with s[j] != s[j + 1] as bytes.  Derived on the host: dust = 10 * dust_sum / (n_triplets - 1), 0 below two triplets --
        prinseq's scale over the whole interval, without its averaging over windows of 64: random letters score about 0.08
        per letter (12 for a read of 150), a homopolymer 5 per letter, so prinseq's cut of 7 fits reads of up to about 64
        letters and longer reads want a larger one -- and complexity = n_diff / (length - 1), fastp's measure (0 below two
        letters).  fq.write(path, ids=np.nonzero(c["dust"] <= cut)[0]) is the low-complexity filter.  A bad id or an interval
        outside its read: IndexError."""
        from . import complexity
        return complexity.complexity_blob(self._qc_blob(), self._rlen_host.size, ids, start, end)

    def kmer_table(self, k, canonical=False, ids=None, start=None, end=None, min_count=1, max_bytes=None):
        """Extension: the sparse k-mer table of seq[start:end] of the reads `ids`, 1 <= k <= 31 -> kmer.KmerTable; the
        definition and the arguments min_count / max_bytes are Fasta.kmer_table's, ids / start / end follow kmer_counts."""
        from . import kmer
        kmer.check_table(k, min_count, max_bytes)
        return kmer.fastq_table_blob(self._qc_blob(), self._rlen_host.size, k, canonical, ids, start, end, min_count, max_bytes)

    def sketch(self, k=21, scaled=None, size=None, canonical=True, ids=None, start=None, end=None, oversample=None):
        """Extension: the MinHash / FracMinHash sketch of the read set -> sketch.Sketch with one pooled set of the windows of
        seq[start:end] of the reads `ids`; k, scaled, size, canonical and oversample are Fasta.sketch's, ids / start / end follow
        kmer_counts."""
        from . import sketch
        sketch.check_args(k, scaled, size)
        return sketch.fastq_sketch_blob(self._qc_blob(), self._rlen_host.size, k, scaled, size, canonical, ids, start, end,
                                        os.path.basename(self.file_name), oversample or 0, self._st.device)

    def kmer_hits(self, table, ids=None, start=None, end=None):
        """Extension: per query, the valid k-mer windows of seq[start:end] and how many of them occur in `table` (a
        kmer.KmerTable of a contaminant, adapter list, rRNA set, ...: k and the canonical form are the table's) ->
        (n_windows, n_hits), int32 arrays in pinned memory; ids / start / end follow kmer_counts.  A window that occurs twice
        counts twice.  The table's codes become a hash set in device memory on first use (csrc/fx_kmer_screen.hpp), kept on
        the table until it is collected or table.release()."""
        from . import kmer
        kmer.check_screen_table(table)
        return kmer.fastq_hits_blob(self._qc_blob(), self._st.device, self._rlen_host.size, table, ids, start, end)

    def screen(self, table, min_hits=1, min_frac=None, invert=False, ids=None, start=None, end=None):
        """Extension: the k-mer filter -- the ascending positions (int64, pinned memory) of the queries with at least min_hits
        windows in `table` and, where min_frac (0..1) is given, at least that share of their valid windows (taken as a
        fraction with a denominator <= 1000 and compared in integers on the device; a query without windows passes it);
        invert=True returns the others instead.  The columns of kmer_hits stay on the device.  With ids=None the positions
        are read ids: fq.write(path, ids=fq.screen(phix, invert=True)) drops the contaminated reads; with trimmed intervals
        index ids, start and end with them."""
        from . import kmer
        kmer.check_screen_table(table)
        kmer.check_screen(min_hits, min_frac, invert)
        return kmer.fastq_screen_blob(self._qc_blob(), self._st.device, self._rlen_host.size, table, min_hits, min_frac, invert, ids, start, end)

    def duplicates(self, ids=None, start=None, end=None, revcomp=False):
        """Extension: exact duplicate detection on the GPU (csrc/fx_fastq_dedup.hpp) -> first, int64 in pinned memory, one row
        per query: first[q] is the smallest query position whose key is a duplicate of query q's, so first[q] == q exactly for
        the first occurrence of each group.  The key of a query is seq[start:end] as bytes -- case-sensitive, N an ordinary
        byte, name and quality play no part --; two queries are duplicates when their keys are equal, with revcomp=True also
        when one is the reverse complement of the other.  ids / start / end follow kmer_counts; a read listed twice in ids is
        a duplicate of its first listing.  A bad id: IndexError; a bad argument: ValueError."""
        from . import dedup
        dedup.check_flag(revcomp, "revcomp")
        return dedup.duplicates_blob(self._qc_blob(), self._rlen_host.size, ids, start, end, revcomp)[0]

    def dedup(self, ids=None, start=None, end=None, revcomp=False, min_copies=1, max_copies=None, return_counts=False):
        """Extension: duplicate removal -- the ascending positions (int64, pinned memory) of the first occurrence of every
        group of duplicates (see duplicates) that has at least min_copies and, where given, at most max_copies members; with
        return_counts=True -> (positions, copies), copies[k] = the members of the group of positions[k] (what
        dedup.duplication_levels takes).  first stays on the device.  With ids=None the positions are read ids:
        fq.write(path, ids=fq.dedup()) writes every distinct sequence once; with trimmed intervals index ids, start and end
        with them, as for screen."""
        from . import dedup
        dedup.check_flag(revcomp, "revcomp")
        dedup.check_flag(return_counts, "return_counts")
        dedup.check_copies(min_copies, max_copies)
        pos, copies, _, _ = dedup.dedup_blob(self._qc_blob(), self._rlen_host.size, ids, start, end, revcomp, min_copies, max_copies, return_counts)
        return (pos, copies) if return_counts else pos

    def records(self, ids=None, start=None, end=None, min_len=0):
        """Extension: four-line FASTQ records of the reads `ids` (None: every read), cut to [start, end) -- what trim returned
        for the same ids; both None: whole reads -- formatted and laid out back to back on the GPU -> (uint8 buffer, int64
        offsets[n + 1]) in pinned memory.  A record is header + "\\n" + seq[a:b] + "\\n+\\n" + qual[a:b] + "\\n", the header as
        Read.description shows it; a read with fewer than min_len bases left produces no bytes (an empty range)."""
        from . import trim as _trim
        buf, offs, _ = _trim.records_blob(self._qc_blob(), self._rlen_host.size, ids, start, end, min_len)
        return buf, offs

    def write(self, path, ids=None, start=None, end=None, min_len=0, batch_bytes=1 << 30, compress=None):
        """Extension: the records of `records` written to the plain file `path`, in batches of consecutive queries whose
        upper bound fits batch_bytes of pinned memory -> {"reads": records written, "bases": their bases, "dropped": queries
        that fell below min_len}.  compress: None or False: plain text; True (level 2) or a level 0, 1, 2: a BGZF file,
        compressed on the GPU (csrc/fx_deflate.hpp) so that only compressed bytes come to the host -- every batch its own
        members (its last may be short), the EOF member once at the end; the result gains "compressed_bytes" (the file's
        size) and "members" (the EOF member included).  Anything else: ValueError."""
        from . import bgzf, trim as _trim
        level = bgzf.level_of(compress)
        blob = self._qc_blob()
        n_reads = self._rlen_host.size
        ids = _trim.check_ids(ids, n_reads)
        n = n_reads if ids is None else ids.size
        start, end = _trim.check_intervals(start, end, n)
        kept = bases = 0
        with open(path, "wb") as f:
            z = None if level is None else bgzf.Tally(f)
            for lo, hi in _trim.batches(self._tab_host, ids, n_reads, batch_bytes):
                q = np.arange(lo, hi, dtype=np.int64) if ids is None else ids[lo:hi]
                a, b = (None, None) if start is None else (start[lo:hi], end[lo:hi])
                if z is None:
                    buf, offs, k = _trim.records_blob(blob, n_reads, q, a, b, min_len)
                    f.write(memoryview(buf))
                else:
                    stream, moff, offs, k = _trim.records_blob(blob, n_reads, q, a, b, min_len, level)
                    z.add(stream, moff)
                kept += k
                there = np.diff(offs) > 0
                ln = self._rlen_host[q].astype(np.int64) if a is None else b - a
                bases += int(ln[there].sum())
            tail = {} if z is None else z.finish()
        return {"reads": int(kept), "bases": int(bases), "dropped": int(n - kept), **tail}

    def demux(self, samples, where="header", offset=0, mismatches=1, margin=1, revcomp=False, ids=None):
        """Extension: barcode demultiplexing on the GPU from the resident stream (csrc/fx_fastq_demux.hpp) -> demux.Demux, one
        row per id (0-based, any order, repeats allowed; None: every read).  samples: a mapping name -> barcode or name ->
        (barcode, barcode), or a sequence of the same (names "0", "1", ...): 1..4096 samples of one or two segments, 1..32
        letters of A C G T N each (N matches anything), the same lengths in every sample.  where: "5p" (the bases from
        `offset` on), "3p" (the bases that end `offset` before the read's end) or "header" (part `offset`, 0 or 1, of the
        index field behind the header's last ':', the parts split at '+'; a longer part is compared by its prefix), or one
        per segment; two header segments with offset left at 0 are parts 0 and 1.  A sample passes when every segment has at
        most `mismatches` (one value, or one per segment) letters that differ -- a missing base differs, no indels --; the
        read goes to the passing sample with the smallest total, is unassigned when none passes and ambiguous when the
        runner-up is fewer than `margin` mismatches behind.  revcomp (a bool, or one per segment) reverse-complements that
        segment's barcodes first.  A bad id: IndexError; a bad argument: ValueError."""
        from . import demux as _demux
        args = _demux.demux_args(samples, where, offset, mismatches, margin, revcomp)
        return _demux.demux_blob(self._qc_blob(), self._rlen_host, ids, args)

    def demux_write(self, dm, pattern, unassigned=None, ambiguous=None, cut=False, min_len=0, batch_bytes=1 << 30, compress=None):
        """Extension: one file per sample of `dm` (what demux returned for this file) through write: `pattern` holds
        "{sample}"; unassigned / ambiguous: a path for those reads, or None to drop them; cut=True writes the reads without
        their inline barcodes (dm.intervals()); compress: as write takes it.  A bin without reads gets no file -> {name:
        (path, records written)}, the two extra bins under "unassigned" and "ambiguous"."""
        from . import bgzf, demux as _demux
        level = bgzf.level_of(compress)
        if not isinstance(dm, _demux.Demux) or (dm._ids is None and len(dm) != self._rlen_host.size):
            raise ValueError("dm must be what demux returned for this file")
        start, end = dm.intervals() if cut else (None, None)
        out = {}
        for key, k, path in _demux.bin_paths(dm, pattern, unassigned, ambiguous):
            pos = dm.positions(k)
            if pos.size == 0:
                continue
            ids = pos if dm._ids is None else dm._ids[pos]
            r = self.write(path, ids=ids, start=None if start is None else start[pos], end=None if end is None else end[pos],
                           min_len=min_len, batch_bytes=batch_bytes, **({} if level is None else {"compress": level}))
            out[key] = (path, r["reads"])
        return out


    def raw_many(self, ids_or_names):
        """Batched `Read.raw` (read.c:124-150): whole four-line records, one gather for all of them.
        -> (uint8 buffer, int64 offsets[n+1])."""
        blob = self._dev()
        if len(ids_or_names) and isinstance(ids_or_names[0], str):
            ids = self.ids_of(ids_or_names)
            if (ids < 0).any():
                raise KeyError("%s does not exist in fastq file" % ids_or_names[int(np.nonzero(ids < 0)[0][0])])
        else:
            ids = np.asarray(ids_or_names, dtype=np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= self._rlen_host.size):
                raise IndexError("index out of range")
        t = self._tab_host
        off = t["soff"][ids] - t["dlen"][ids] - 1
        n = t["qoff"][ids] + t["rlen"][ids] - off + 2          # read.c:131: two bytes past the quality line
        buf, offs, _ = blob.fetch_ranges(off, n, n, flags=_F_RAW)      # bytes past the end of the stream come back as 0
        # read.c:138-147: the record ends at its newline -- "\n" right after the quality line, or "\r\n"; neither: the
        # file ends without one
        end = offs[1:]
        b2, b1 = buf[end - 2], buf[end - 1]
        keep = np.where(b2 == 10, n - 1, np.where((b2 == 13) & (b1 == 10), n, n - 2))
        if (keep == n).all():
            return buf, offs
        out_offs = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(keep, out=out_offs[1:])
        sel = np.repeat(offs[:-1] - out_offs[:-1], keep) + np.arange(int(out_offs[-1]), dtype=np.int64)
        return buf[sel], out_offs


class Read(_fxobj.ReadCore):
    """pyfastx.Read (read.c:288-323).  The row's fields (id, name, _desc_len, _read_len, _soff, _qoff) live in the C base type
    (csrc/fxobj.c: ReadCore, constructed as Read(fq, id, name, dlen, rlen, soff, qoff)); the objects of Fastq's iterator are
    made a batch at a time by _fxobj.read_batch and carry their sequence and quality strings (_pre_seq / _pre_qual)."""

    __slots__ = ()                                            # no instance dict: the objects stay out of the cyclic GC's lists

    def __repr__(self):
        return "<Read> %s with length of %d" % (self.name, self._read_len)                     # read.c:280-282

    def __str__(self):
        return self.seq

    def _bytes(self, off, n):
        return self._fq._st.raw(off, n)

    # .seq, .qual and len() are the C base type's: the strings that came with the iterator's batch, else these
    def _name_slow(self):
        """the name of a read that came out of the host table (fq[i]) when the file is not a plain one: its bytes from the stream"""
        return self._bytes(self._name_off, self._name_len).decode("utf-8", "surrogateescape")

    def _seq_slow(self):
        return _decode(self._bytes(self._soff, self._read_len))                                # read.c:152-167

    def _qual_slow(self):
        return _decode(self._bytes(self._qoff, self._read_len))                                # read.c:237-249

    def _quali_slow(self):
        """read.c:251-278 -- `qual - phred` (phred 0 -> 33) computed by the read-fetch kernel."""
        _, _, qi, _ = self._fq._st.blob.read_fetch([self._soff], [self._qoff], [self._read_len],
                                                    phred=self._fq._phred, want=("quali",))
        return qi[:self._read_len].tolist()

    def _rc(self, mode):
        return _decode(_lib.revcomp_bytes(self._bytes(self._soff, self._read_len), mode, self._fq._st.device))

    @property
    def reverse(self):
        return self._rc(_F_REV)

    @property
    def complement(self):
        return self._rc(_F_COMP)

    @property
    def antisense(self):
        return self._rc(_F_REV | _F_COMP)

    @property
    def description(self):
        d = self._bytes(self._soff - self._desc_len - 1, self._desc_len)                        # read.c:214-235
        if d.endswith(b"\r"):
            d = d[:-1]
        return _text(d)

    @property
    def raw(self):
        off = self._soff - self._desc_len - 1                                                   # read.c:124-150
        n = self._qoff + self._read_len - off + 2
        r = self._bytes(off, n)
        if len(r) >= 2 and r[n - 2:n - 1] == b"\n":
            r = r[:n - 1]
        elif len(r) >= 2 and r[n - 2:n - 1] == b"\r" and r[n - 1:n] == b"\n":
            r = r[:n]
        else:
            r = r[:n - 2]
        return _text(r.rstrip(b"\x00"))


# ============================================================== Fastx
def _kseq_header(raw, unterminated):
    """kseq_read's cut of a header line (kseq.c:148-149): the name runs to the first isspace() byte; when that byte is not
    the line's '\n', ks_getuntil2 reads the rest of the line into the comment buffer -- and drops a trailing CR only from
    a string longer than one byte (kseq.c:106).  raw = the bytes behind the '>' / '@' up to the '\n'.
    -> (name bytes, comment bytes -- None when the comment buffer was not written: nothing follows the name, or the
    stream ends right behind the delimiter)."""
    for i, c in enumerate(raw):
        if c in _SPACE_BYTES:
            rest = raw[i + 1:]
            if unterminated and not rest:
                return raw[:i], None
            if len(rest) > 1 and rest[-1] == 13:
                rest = rest[:-1]
            return raw[:i], rest
    return raw, None


_SPACE_BYTES = frozenset(b" \t\n\r\x0b\x0c")            # isspace() in the C locale: what ends a name (KS_SEP_SPACE, kseq.h:9)


def _cstr(b):
    """Py_BuildValue "s" (fastx.c:6-30): the bytes up to the first NUL, as text."""
    b = bytes(b)
    z = b.find(b"\0")
    return _text(b if z < 0 else b[:z])


class Fastx:
    """pyfastx.Fastx (fastx.c:32-147): iteration over a FASTA or FASTQ file WITHOUT an index file -- tuples
    (name, seq[, comment]) or (name, seq, qual[, comment]).  The reference walks the file with kseq_read (kseq.c:138-179);
    here the stream is staged in HBM, ONE pass finds its lines, one workgroup walks the line table with kseq_read's own
    rules (fx_kseq_scan: FASTA and FASTQ records mixed, sequence and quality over any number of lines, text between
    records skipped, white space kept inside the lines, one trailing CR dropped per line read) and the strings of a batch
    of records are gathered by one kernel (fx_kseq_fetch).  `format` only selects the tuple builder, as in the reference
    (fastx.c:86-106): a FASTA-style record seen through the FASTQ builder carries what the reference's quality buffer
    still holds -- the previous quality string, None before the first."""

    BATCH_RECORDS = 65536
    BATCH_BYTES = 64 << 20

    def __init__(self, file_name, format="auto", uppercase=False, comment=False, device=0):
        if not os.path.isfile(file_name):
            raise FileExistsError("the input file %s does not exists" % file_name)             # fastx.c:47-50
        self.file_name, self._uppercase, self._comment, self._device = file_name, bool(uppercase), bool(comment), device
        if format == "auto":                                                                     # fastx.c:61-69
            c = _first_nonspace(file_name, _is_gzip(file_name))
            self._format = 1 if c == ord(">") else 2 if c == ord("@") else 0
        else:
            self._format = {"fasta": 1, "fastq": 2}.get(format, 0)
        if self._format == 0:
            raise RuntimeError("%s is not fasta or fastq sequence file" % file_name)           # fastx.c:71-74
        self.end_code = None                      # after an iteration: what ended it in the reference (-1 end of file, -2 truncated quality)

    def __repr__(self):
        return "<Fastx> %s %s" % ("fasta" if self._format == 1 else "fastq", self.file_name)    # fastx.c:126-132

    def __iter__(self):
        # The tuples of fastx.c:6-30 come out of a C iterator (_fxobj.FastxIter, the counterpart of pyfastx_fastx_next): per
        # record the header cut of kseq.c:148-149 (_kseq_header), "s" strings (_cstr), and the buffer rules -- a record
        # without a comment yields None until the reference's comment buffer exists (from the first header whose name is
        # followed by anything but the newline, a CR included) and "" afterwards (kseq.c:146 with Py_BuildValue "s#" on a
        # NULL pointer, fastx.c:10-12, 28-30); a FASTA-style record seen through the FASTQ builder carries the last
        # quality string.
        fastq = self._format == 2
        return _kseq_iter(lambda: _lib.Blob.from_file(self.file_name, device=self._device), True, fastq=fastq,
                          upper=self._uppercase and not fastq, comment_mode=1 if self._comment else 0, owner=self)   # fastx.c:14-22, 97-103


def _kseq_batches(get_blob, close_blob, fastq, upper, owner=None):
    """(hdr bytes, their offsets, seq bytes, qual bytes | None, record table) per batch of kseq_read's records over a staged
    stream (fx_kseq_scan / _records / _fetch), None at the end.  The NEXT batch is gathered and copied to the host by a helper
    thread while the consumer makes the tuples of this one (the C calls release the interpreter lock; one call at a time on the
    handle): the device side of the iteration -- a sixth of its time -- hides behind the object creation."""
    from concurrent.futures import ThreadPoolExecutor
    blob = get_blob()
    pool = ThreadPoolExecutor(max_workers=1)
    try:
        n_rec, _, _, code = blob.kseq_scan()
        if owner is not None:
            owner.end_code = code

        def pieces():                                            # (first record, count, bytes) of every batch, chunk of records by chunk
            for a in range(0, n_rec, Fastx.BATCH_RECORDS):
                recs = blob.kseq_records(a, min(Fastx.BATCH_RECORDS, n_rec - a))
                cum, slen = recs["seq_cum"], recs["seq_len"]
                i = 0
                while i < recs.size:
                    ends = cum[i:] + slen[i:] - cum[i]
                    k = i + max(1, int(np.searchsorted(ends, Fastx.BATCH_BYTES, side="right")))
                    yield a, recs, i, k, int(ends[k - i - 1])
                    i = k

        def fetch(job):
            a, recs, i, k, nbytes = job
            seq, qual = blob.kseq_fetch(a + i, k - i, nbytes, upper=upper, want_qual=fastq)
            hl = recs["hdr_len"][i:k].astype(np.int64)
            hdr, ho, _ = blob.fetch_ranges(recs["hdr_off"][i:k], hl, hl, flags=_lib.FX_RAW)
            return hdr, ho, seq, qual, recs[i:k]

        jobs = pieces()
        if not close_blob:
            # the handle is shared (Fasta / Fastq(build_index=False).__iter__ hand out their own blob): a second live iterator on
            # the same object would run fx_kseq_scan on the main thread while this one's helper is inside fx_kseq_fetch -- two
            # calls at a time on one handle.  Only a generator that OWNS its blob gathers ahead; a shared one stays strictly serial.
            for job in jobs:
                yield fetch(job)
            yield None
            return
        ahead = None
        job = next(jobs, None)
        if job is not None:
            ahead = pool.submit(fetch, job)
        while ahead is not None:
            out = ahead.result()
            job = next(jobs, None)                               # (kseq_records of the next chunk runs here, after the fetch before it is done)
            ahead = pool.submit(fetch, job) if job is not None else None
            yield out
    finally:
        pool.shutdown(wait=True)
        if close_blob:
            blob.close()
    yield None


def _kseq_iter(get_blob, close_blob, fastq, upper, comment_mode, owner=None):
    """The C iterator over kseq_read's records (comment_mode: 0 none, 1 the comment as last element, 2 joined to the name)."""
    return _fxobj.FastxIter(_kseq_batches(get_blob, close_blob, fastq, upper, owner).__next__, fastq, comment_mode)


# ============================================================== module functions
def version(debug=False):
    """module.c:14-28"""
    if debug:
        return "pyfastx_amd: %s; %s" % (VERSION, _lib.lib().fx_version().decode())
    return VERSION


def gzip_check(file_name):
    """module.c:30-42"""
    return _is_gzip(file_name)


def reverse_complement(seq, device=0):
    """module.c:44-59 -> reverse_complement_seq (util.c:239-249) on the GPU."""
    return _decode(_lib.revcomp_bytes(seq.encode("latin-1"), _F_REV | _F_COMP, device))


_fxobj.set_read_type(Read)          # what the C subscript of Fastq makes (csrc/fxobj.c: fqc_subscript)
