"""MinHash and FracMinHash sketches of records and read sets, compared on the device (extension; the reference has no k-mer of
any kind).

Fasta.sketch / Fastq.sketch hand k, a threshold and a size to fx_fasta_sketch / fx_fastq_sketch (csrc/fx_sketch.hpp) and return a
Sketch: sorted key lists that stay in device memory.  The definition, as include/fxgpu.h has it:

Windows.  Those of kmer_table, word for word: 1 <= k <= 31, valid letters ACGTacgt, across line ends, never across records, never
past slen; FASTQ windows are those of s[start:end] of the selected reads.
Key.  key = minimizer.mix(code, k), a bijection of the 2k-bit words; canonical: code = min(fw, rc), else code = fw.
Sets.  Fasta: one set per selected record in ascending record order, or one for all of them with pooled=True.  Fastq: always one
pooled set of the selected reads.
What a set keeps.  The distinct keys of its valid windows below max_key, and with size > 0 the `size` smallest of those.
scaled (an integer >= 1) means max_key = ceil(4^k / scaled), that is key * scaled < 4^k; size alone means max_key = 4^k, the
classic bottom-s MinHash.  Every set is ascending and distinct.
Comparison.  Sets A and B, a limit L >= 0 and a restriction max_key (both sets are first cut to their keys below it).  U = the
ascending distinct union, U_L its first min(L, |U|) elements (all of U when L = 0): total = |U_L|, shared = the elements of U_L
that lie in both.  Jaccard = shared / total; containment of A in B = shared / |A| at L = 0; Mash distance =
-ln(2j / (1 + j)) / k with j at L = the sketch size, clipped to [0, 1], 1 when j = 0; ANI = containment^(1/k)."""
import numpy as np

from . import _lib, minimizer

MAX_K = 31
MAX_OVERSAMPLE = 64


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (name, v))
    return int(v)


def max_key_of(k, scaled):
    """ceil(4^k / scaled): key < max_key exactly when key * scaled < 4^k (Python ints, no overflow); scaled None: 4^k."""
    return 4 ** k if scaled is None else -(-4 ** k // scaled)


def check_args(k, scaled=None, size=None):
    """The argument rules of every entry -> (k, scaled or None, size (0: no cap), max_key).  ValueError otherwise."""
    k = _int("k", k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside 1..%d" % (k, MAX_K))
    if scaled is None and size is None:
        raise ValueError("at least one of scaled and size must be given")
    if scaled is not None:
        scaled = _int("scaled", scaled)
        if scaled < 1:
            raise ValueError("scaled = %d below 1" % scaled)
    if size is not None:
        size = _int("size", size)
        if size < 0:
            raise ValueError("size = %d below 0" % size)
    return k, scaled, size or 0, max_key_of(k, scaled)


def _size_arg(scaled, size):
    """The size argument that gives `size` back through check_args: 0 stands for "no cap" only beside a scaled."""
    return size if scaled is None else (size or None)


def _flags(canonical, pooled=False):
    return (_lib.FX_SK_CANONICAL if canonical else 0) | (_lib.FX_SK_POOLED if pooled else 0)


# ------------------------------------------------------------------ what follows from (shared, total)
def jaccard_of(shared, total):
    """shared / total, 0 where the union is empty."""
    shared, total = np.asarray(shared, dtype=np.float64), np.asarray(total, dtype=np.float64)
    return np.divide(shared, total, out=np.zeros(np.broadcast(shared, total).shape), where=total > 0)


def containment_of(shared, size_a):
    """shared / |A| (row i of `shared` belongs to set i of A), 0 for an empty A."""
    shared = np.asarray(shared, dtype=np.float64)
    size_a = np.asarray(size_a, dtype=np.float64).reshape((-1,) + (1,) * (shared.ndim - 1)) if shared.ndim else np.asarray(size_a, dtype=np.float64)
    return np.divide(shared, size_a, out=np.zeros(np.broadcast(shared, size_a).shape), where=size_a > 0)


def mash_distance_of(j, k):
    """-ln(2j / (1 + j)) / k clipped to [0, 1]; 1 where j = 0."""
    j = np.asarray(j, dtype=np.float64)
    with np.errstate(divide="ignore"):
        d = -np.log(2.0 * j / (1.0 + j)) / k
    return np.where(j > 0, np.clip(d, 0.0, 1.0), 1.0)


def ani_of(containment, k):
    """containment^(1/k)."""
    return np.asarray(containment, dtype=np.float64) ** (1.0 / k)


class Sketch:
    """The sets of one sketch call, or of from_hashes / load / concat / select: ascending distinct uint64 keys per set, in device
    memory.  k, canonical, scaled (None without one), max_key, size (0: no cap), n_sets, names (one per set), n_rounds (the
    rounds the device took, 0 for a sketch that was not built from a stream), device."""

    def __init__(self, obj, scaled, names, device=0, n_rounds=0):
        self._obj, self.scaled, self.device, self.n_rounds = obj, scaled, int(device), int(n_rounds)
        self.k, self.canonical, self.max_key, self.size, self.n_sets = obj.k, bool(obj.flags & _lib.FX_SK_CANONICAL), obj.max_key, obj.size, obj.n_sets
        self.names = [str(i) for i in range(self.n_sets)] if names is None else [str(n) for n in names]
        if len(self.names) != self.n_sets:
            raise ValueError("%d names for %d sets" % (len(self.names), self.n_sets))
        self._host = None

    # -------------------------------------------------------------- data
    def _arrays(self):
        if self._host is None:
            self._host = self._obj.read()
        return self._host

    @property
    def sizes(self):
        """Keys per set, int64[n_sets]."""
        return np.diff(self._arrays()[0]).astype(np.int64)

    def hashes(self, i):
        """The keys of set i, uint64 ascending."""
        off, keys = self._arrays()
        i = range(self.n_sets)[i]
        return keys[off[i]:off[i + 1]]

    def kmers(self, i):
        """The k-mers of set i as strings, in the order of hashes(i) (through minimizer.unmix)."""
        codes = minimizer.unmix(self.hashes(i), self.k)
        if not codes.size:
            return []
        sh = (np.arange(self.k - 1, -1, -1, dtype=np.uint64) * np.uint64(2))[None, :]
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)[((codes[:, None] >> sh) & np.uint64(3)).astype(np.intp)]
        return [row.tobytes().decode() for row in letters]

    def cardinality(self):
        """The estimated number of distinct k-mers per set: sizes * 4^k / max_key (meaningful without a size cap)."""
        return self.sizes.astype(np.float64) * (float(4 ** self.k) / float(self.max_key))

    # -------------------------------------------------------------- sets
    @classmethod
    def from_hashes(cls, hashes, k, canonical=True, scaled=None, size=None, names=None, device=0):
        """A sketch from one ascending distinct uint64 array per set.  A key >= max_key, keys that do not ascend strictly, or a
        set longer than size: ValueError (the device checks them, fx_sketch_from_host)."""
        k, scaled, size, max_key = check_args(k, scaled, size)
        arrays = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in hashes]
        off = np.zeros(len(arrays) + 1, dtype=np.int64)
        off[1:] = np.cumsum([a.size for a in arrays], dtype=np.int64)
        keys = np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.uint64)
        return cls._from_arrays(off, keys, k, canonical, scaled, size, max_key, names, device)

    @classmethod
    def _from_arrays(cls, off, keys, k, canonical, scaled, size, max_key, names, device):
        try:
            obj = _lib.SketchObj.from_host(device, k, _flags(canonical), max_key, size, off, keys)
        except _lib.FxError as e:
            if e.code == _lib.FX_EINVAL:
                raise ValueError(str(e))
            raise
        return cls(obj, scaled, names, device)

    def select(self, indices):
        """The sets `indices` (any order, repeats allowed) as a sketch of their own."""
        idx = [range(self.n_sets)[int(i)] for i in indices]
        return Sketch.from_hashes([self.hashes(i) for i in idx], self.k, self.canonical, self.scaled, _size_arg(self.scaled, self.size),
                                  [self.names[i] for i in idx], self.device)

    @staticmethod
    def concat(sketches):
        """The sets of several sketches of the same k, canonical form, scaled and size in one (joined on the host): how many
        files are compared."""
        sketches = list(sketches)
        if not sketches:
            raise ValueError("no sketch to join")
        a = sketches[0]
        for b in sketches[1:]:
            if (b.k, b.canonical, b.max_key, b.size) != (a.k, a.canonical, a.max_key, a.size):
                raise ValueError("sketches of different k, canonical form, max_key or size do not join")
        return Sketch.from_hashes([s.hashes(i) for s in sketches for i in range(s.n_sets)], a.k, a.canonical, a.scaled,
                                  _size_arg(a.scaled, a.size), [n for s in sketches for n in s.names], a.device)

    # -------------------------------------------------------------- persistence
    def save(self, path):
        """One .npz with the parameters, names, offsets and keys."""
        off, keys = self._arrays()
        with open(path, "wb") as f:
            np.savez(f, k=np.int64(self.k), canonical=np.int64(self.canonical), scaled=np.int64(self.scaled or 0), size=np.int64(self.size),
                     names=np.array(self.names, dtype=np.str_), off=np.asarray(off), keys=np.asarray(keys))

    @classmethod
    def load(cls, path, device=0):
        with np.load(path, allow_pickle=False) as z:
            k, canonical, scaled, size = int(z["k"]), bool(z["canonical"]), int(z["scaled"]) or None, int(z["size"])
            names, off, keys = [str(n) for n in z["names"]], z["off"].astype(np.int64), z["keys"].astype(np.uint64)
        k, scaled, size, max_key = check_args(k, scaled, _size_arg(scaled, size))
        return cls._from_arrays(off, keys, k, canonical, scaled, size, max_key, names, device)

    # -------------------------------------------------------------- comparison
    def compare(self, other=None, limit=0, max_key=None, max_pairs=10**8, ia=None, ib=None):
        """(shared, total), int64[nA, nB], every set of this sketch with every set of `other` (None: with itself); ia / ib
        restrict either side to some of its sets.  Sketches that differ in max_key are compared below the smaller one unless
        max_key says otherwise (sourmash's downsampling).  Different k or canonical form: ValueError; more than max_pairs pairs:
        ValueError with the count."""
        other = self if other is None else other
        if (self.k, self.canonical) != (other.k, other.canonical):
            raise ValueError("sketches of k = %d%s and k = %d%s do not compare" % (self.k, " canonical" if self.canonical else "", other.k,
                                                                                 " canonical" if other.canonical else ""))
        if limit < 0:
            raise ValueError("limit must not be negative")
        if max_key is None:
            max_key = min(self.max_key, other.max_key) if self.max_key != other.max_key else 0
        pairs = (self.n_sets if ia is None else len(ia)) * (other.n_sets if ib is None else len(ib))
        if pairs > max_pairs:
            raise ValueError("%d pairs, more than max_pairs=%d" % (pairs, max_pairs))
        try:
            return self._obj.compare(other._obj, ia, ib, limit, max_key, max_pairs)
        except _lib.FxError as e:
            if e.code in (_lib.FX_EINVAL, _lib.FX_ERANGE):
                raise ValueError(str(e))
            raise

    def _sizes_below(self, max_key):
        off, keys = self._arrays()
        if not max_key or max_key >= self.max_key:
            return self.sizes
        return np.array([np.searchsorted(keys[off[i]:off[i + 1]], np.uint64(max_key)) for i in range(self.n_sets)], dtype=np.int64)

    def jaccard(self, other=None):
        """shared / total over the whole union, float64[nA, nB]."""
        return jaccard_of(*self.compare(other))

    def containment(self, other=None):
        """The share of every set of this sketch found in every set of `other`: shared / |A|, float64[nA, nB]."""
        o = self if other is None else other
        shared, _ = self.compare(other)
        return containment_of(shared, self._sizes_below(min(self.max_key, o.max_key) if self.max_key != o.max_key else 0))

    def mash_distance(self, other=None):
        """-ln(2j / (1 + j)) / k with j over the first s elements of the union, s the smaller sketch size; both sketches need one."""
        o = self if other is None else other
        if not self.size or not o.size:
            raise ValueError("mash_distance needs sketches with a size")
        return mash_distance_of(jaccard_of(*self.compare(other, limit=min(self.size, o.size))), self.k)

    def ani(self, other=None):
        """containment^(1/k)."""
        return ani_of(self.containment(other), self.k)

    # -------------------------------------------------------------- lifetime
    def release(self):
        """Frees the device memory now (the host copy, where one was read, stays)."""
        self._obj.close()

    def __len__(self):
        return self.n_sets

    def __repr__(self):
        return "<Sketch k=%d %s scaled=%s size=%d sets=%d>" % (self.k, "canonical" if self.canonical else "forward", self.scaled, self.size, self.n_sets)


def _wrap(call, what):
    try:
        return call()
    except _lib.FxError as e:
        if e.code == _lib.FX_ERANGE and getattr(e, "first_bad", -1) < 0:
            raise ValueError("%s: %s" % (what, e))
        raise _lib.outside(e)


def fasta_sketch_blob(blob, k, scaled=None, size=None, canonical=True, ids=None, pooled=False, names=None, oversample=0, device=0):
    """The sketch on a Blob whose FASTA table is resident; ids: distinct ascending record ids or None -> Sketch."""
    k, scaled, size, max_key = check_args(k, scaled, size)
    obj, rounds = _wrap(lambda: blob.fasta_sketch(k, _flags(canonical, pooled), ids, max_key, size, oversample), "sketch")
    return Sketch(obj, scaled, names, device, rounds)


def fastq_sketch_blob(blob, n_reads, k, scaled=None, size=None, canonical=True, ids=None, start=None, end=None, name="reads", oversample=0, device=0):
    """The pooled sketch of seq[start:end] of the reads `ids`; ids, start and end by the rules of Fastq.records -> Sketch."""
    from . import trim
    k, scaled, size, max_key = check_args(k, scaled, size)
    ids = trim.check_ids(ids, n_reads)
    start, end = trim.check_intervals(start, end, n_reads if ids is None else ids.size)
    obj, rounds = _wrap(lambda: blob.fastq_sketch(k, _flags(canonical), ids, start, end, max_key, size, oversample), "sketch")
    return Sketch(obj, scaled, [name], device, rounds)
