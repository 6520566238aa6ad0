"""Position weight matrices on the resident stream (extension; the reference has no scored motif).

A Pwm holds an integer matrix int32 [W, 4] (row j = position j of the motif, columns A C G T), the scale that turned
log-odds into those integers, and the background the log-odds and the p-values are taken against.  Fasta.pwm_scan /
pwm_counts / pwm_best hand the integers to fx_fasta_pwm_scan / fx_fasta_pwm_best (csrc/fx_pwm.hpp): every window of W
letters whose score reaches a threshold, on one or both strands, and the best window of every record.  All scoring on the
device is exact integer arithmetic; floats exist only here."""
import math
import re
from collections import namedtuple

import numpy as np

from . import _lib

PwmHits = namedtuple("PwmHits", ["ids", "starts", "stops", "strands", "scores"])
PwmBest = namedtuple("PwmBest", ["scores", "starts"])

MAX_WIDTH = 64
MAX_ENTRY = 32767
NO_SCORE = int(np.iinfo(np.int32).min)                       # the best score of a record without a scorable window
_STRANDS = {"+": _lib.FX_SEARCH_PLUS, "-": _lib.FX_SEARCH_MINUS, "both": _lib.FX_SEARCH_PLUS | _lib.FX_SEARCH_MINUS}
_UNIFORM = (0.25, 0.25, 0.25, 0.25)


def _background(bg):
    try:
        b = np.asarray(bg, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("background must be four positive numbers that sum to 1")
    if b.shape != (4,) or not np.isfinite(b).all() or (b <= 0).any() or abs(float(b.sum()) - 1.0) > 1e-9:
        raise ValueError("background must be four positive numbers that sum to 1, not %r" % (bg,))
    return b


def _matrix(m, what, rows_first):
    """A numeric matrix [W, 4] (rows_first) or [4, W] -> float64 [W, 4]; ValueError for any other shape or W outside 1..64."""
    try:
        a = np.asarray(m, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s is not a numeric matrix" % what)
    want = "[W, 4]" if rows_first else "[4, W]"
    if a.ndim != 2 or a.shape[1 if rows_first else 0] != 4:
        raise ValueError("%s must have the shape %s, not %r" % (what, want, a.shape))
    if not rows_first:
        a = a.T
    if not 1 <= a.shape[0] <= MAX_WIDTH:
        raise ValueError("matrix width %d outside 1..%d" % (a.shape[0], MAX_WIDTH))
    return np.ascontiguousarray(a)


class Pwm:
    """One position weight matrix in integer units: ints int32 [W, 4] (columns A C G T), scale (integer units per unit of
    the float matrix), background (probabilities of A C G T)."""

    def __init__(self, ints, scale=1, background=_UNIFORM, name=None):
        a = _matrix(ints, "ints", True)
        if not np.isfinite(a).all() or (a != np.rint(a)).any():
            raise ValueError("matrix entries must be integers")
        if (np.abs(a) > MAX_ENTRY).any():
            raise ValueError("quantised entry %d beyond +-%d: use a smaller scale" % (int(a.flat[int(np.abs(a).argmax())]), MAX_ENTRY))
        if not (isinstance(scale, (int, float, np.integer, np.floating)) and math.isfinite(scale) and scale > 0):
            raise ValueError("scale must be a positive number, not %r" % (scale,))
        self.ints = a.astype(np.int32)
        self.ints.setflags(write=False)
        self.scale = scale
        self.background = _background(background)
        self.name = name
        self._dist = None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_ints(cls, ints, scale=1, background=_UNIFORM):
        """An integer matrix [W, 4] as it is."""
        return cls(ints, scale, background)

    @classmethod
    def from_log_odds(cls, matrix, scale=100, background=_UNIFORM):
        """A float matrix [W, 4] of log-odds (or any additive weights): entries np.rint(scale * matrix)."""
        a = _matrix(matrix, "matrix", True)
        if not np.isfinite(a).all():
            raise ValueError("matrix entries must be finite")
        return cls(np.rint(scale * a), scale, background)

    @classmethod
    def from_counts(cls, counts, background=_UNIFORM, pseudocount=0.8, scale=100, name=None):
        """A count matrix [4, W], rows A C G T as JASPAR prints them: entries
        np.rint(scale * log2(((c + pseudocount * bg) / (N_j + pseudocount)) / bg)), N_j the sum of column j."""
        c = _matrix(counts, "counts", False)
        bg = _background(background)
        if not np.isfinite(c).all() or (c < 0).any():
            raise ValueError("counts must be finite and not negative")
        if not (math.isfinite(pseudocount) and pseudocount >= 0):
            raise ValueError("pseudocount must not be negative")
        n = c.sum(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.log2(((c + pseudocount * bg) / (n + pseudocount)) / bg)
        if not np.isfinite(lo).all():
            raise ValueError("a zero count without a pseudocount has no finite log-odds")
        return cls(np.rint(scale * lo), scale, bg, name)

    @classmethod
    def from_jaspar(cls, text, **kw):
        """JASPAR text: an optional '>ID name' line and four rows 'A [ 1 2 3 ]' in the order A C G T (the letters and the
        brackets may be left out) -> from_counts(counts, **kw)."""
        if isinstance(text, (bytes, bytearray)):
            text = text.decode("latin-1")
        name, rows = None, []
        for line in str(text).splitlines():
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                if name is not None or rows:
                    raise ValueError("JASPAR text: more than one matrix, or a header after the rows")
                name = line[1:].strip()
                continue
            m = re.fullmatch(r"(?:([ACGTacgt])\s*)?(\[)?([^\[\]]*)(\])?", line)
            if not m or (m.group(2) is None) != (m.group(4) is None):
                raise ValueError("JASPAR text: cannot read the row %r" % line)
            if m.group(1) and m.group(1).upper() != "ACGT"[len(rows) % 4]:
                raise ValueError("JASPAR text: row %d is labelled %r, rows come in the order A C G T" % (len(rows), m.group(1)))
            try:
                rows.append([float(x) for x in m.group(3).replace(",", " ").split()])
            except ValueError:
                raise ValueError("JASPAR text: a count in %r is not a number" % line)
        if len(rows) != 4 or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("JASPAR text: four rows of equal length expected, found %r" % ([len(r) for r in rows],))
        kw.setdefault("name", name)
        return cls.from_counts(np.array(rows), **kw)

    # ------------------------------------------------------------------ geometry
    def __len__(self):
        return self.ints.shape[0]

    def revcomp(self):
        """The matrix that scores the reverse complement: rows reversed, columns A<->T and C<->G."""
        bg = self.background[::-1]
        return Pwm(self.ints[::-1, ::-1], self.scale, bg, self.name)

    @property
    def max_score(self):
        return int(self.ints.max(axis=1).sum())

    @property
    def min_score(self):
        return int(self.ints.min(axis=1).sum())

    def score_at(self, frac):
        """The integer score `frac` of the way from min_score to max_score, rounded up."""
        return int(math.ceil(self.min_score + frac * (self.max_score - self.min_score)))

    def to_float(self, scores):
        """Integer scores in the units of the float matrix."""
        return np.asarray(scores, dtype=np.float64) / self.scale

    # ------------------------------------------------------------------ the score distribution
    def distribution(self):
        """The exact probability of every integer score of a window of independent letters drawn from `background` ->
        (scores int64 = min_score .. max_score, probabilities float64), by convolving the columns one after another."""
        if self._dist is None:
            d = (self.ints - self.ints.min(axis=1, keepdims=True)).astype(np.int64)
            p = np.ones(1, dtype=np.float64)
            for row in d:
                q = np.zeros(p.size + int(row.max()), dtype=np.float64)
                for c in range(4):
                    q[row[c]:row[c] + p.size] += self.background[c] * p
                p = q
            p.setflags(write=False)
            tail = np.minimum(np.cumsum(p[::-1])[::-1], 1.0)
            tail.setflags(write=False)
            self._dist = (p, tail)
        return np.arange(self.min_score, self.max_score + 1, dtype=np.int64), self._dist[0]

    def pvalue(self, score):
        """P(S >= score) under `background`."""
        self.distribution()
        tail = self._dist[1]
        i = int(math.ceil(score)) - self.min_score
        return 1.0 if i <= 0 else 0.0 if i >= tail.size else float(tail[i])

    def threshold_for_pvalue(self, p):
        """The smallest integer t with P(S >= t) <= p; max_score + 1 when even the best window is likelier than p."""
        if not 0 <= p <= 1:
            raise ValueError("p-value %r outside 0..1" % (p,))
        self.distribution()
        tail = self._dist[1]                                 # not increasing
        return self.min_score + int(np.searchsorted(-tail, -float(p), side="left"))

    def __repr__(self):
        return "Pwm(%s%d columns, scale=%r, scores %d..%d)" % ("%r, " % self.name if self.name else "", len(self), self.scale,
                                                               self.min_score, self.max_score)


def _as_pwm(pwm):
    if not isinstance(pwm, Pwm):
        raise ValueError("pwm must be a Pwm (Pwm.from_counts, from_log_odds, from_ints, from_jaspar), not %r" % type(pwm).__name__)
    return pwm


def strand_mode(strand):
    if strand not in _STRANDS:
        raise ValueError("strand must be '+', '-' or 'both', not %r" % (strand,))
    return _STRANDS[strand]


def resolve_min_score(pwm, min_score=None, threshold=None, pvalue=None):
    """Exactly one of the three thresholds -> the integer a window's score is compared with (int32 range).  min_score: integer
    units; threshold: the float matrix's units, a window hits iff its integer score is >= ceil(threshold * scale - 1e-9);
    pvalue: threshold_for_pvalue."""
    pwm = _as_pwm(pwm)
    if (min_score is not None) + (threshold is not None) + (pvalue is not None) != 1:
        raise ValueError("exactly one of min_score, threshold and pvalue must be given")
    if min_score is not None:
        if isinstance(min_score, bool) or not isinstance(min_score, (int, np.integer)):
            raise ValueError("min_score must be an integer (quantised units), not %r" % (min_score,))
        t = int(min_score)
    elif threshold is not None:
        if not math.isfinite(threshold):
            raise ValueError("threshold must be finite")
        t = int(math.ceil(threshold * pwm.scale - 1e-9))
    else:
        t = pwm.threshold_for_pvalue(pvalue)
    return max(-2**31 + 1, min(t, 2**31 - 1))


def scan_blob(blob, pwm, min_score, strand="both", ids=None, max_hits=10**8):
    """Every hit on a Blob whose FASTA table is resident -> PwmHits (arrays in pinned memory)."""
    pwm, mode = _as_pwm(pwm), strand_mode(strand)
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    try:
        total, hits, _ = blob.fasta_pwm_scan(pwm.ints, mode, min_score, ids=ids, cap=int(max_hits))
    except _lib.FxError as e:
        raise _lib.too_many(e, "hits", "max_hits", max_hits)
    if hits is None:
        z = np.zeros(0, dtype=np.int64)
        return PwmHits(z, z.copy(), z.copy(), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32))
    rec, starts, strands, scores = hits
    stops = _lib.pinned_empty(total, np.int64)
    np.add(starts, len(pwm), out=stops)
    return PwmHits(rec, starts, stops, strands, scores)


def count_blob(blob, pwm, min_score, strand="both"):
    """Hits per record on + and on - -> int64[n_records, 2]; the hits themselves never leave the device."""
    pwm, mode = _as_pwm(pwm), strand_mode(strand)
    _, _, counts = blob.fasta_pwm_scan(pwm.ints, mode, min_score, cap=0, counts=True)
    return counts


def best_blob(blob, pwm, strand="both", ids=None):
    """The best window of every selected record and strand -> PwmBest(scores int32[n, 2], starts int64[n, 2])."""
    pwm, mode = _as_pwm(pwm), strand_mode(strand)
    return PwmBest(*blob.fasta_pwm_best(pwm.ints, mode, ids=ids))
