"""The definition of the k-mer spectra (Fasta.kmer_counts / kmer_profile, Fastq.kmer_counts) in plain Python / numpy; it
imports nothing of the package.

Alphabet A C G T and a c g t (A = 0, C = 1, G = 2, T = 3); every other byte is invalid and a window that holds one is not
counted.  The code of b0 b1 .. b(k-1) is sum(code(bj) * 4**(k-1-j)).  canonical: a window counts under min(code, code of
its reverse complement), a window that is its own reverse complement once.  Windows never span two sequences."""
import numpy as np

CODE = np.full(256, 4, dtype=np.int64)
for _j, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _j


def as_bytes(s):
    if isinstance(s, str):
        s = s.encode("latin-1")
    if isinstance(s, (bytes, bytearray)):
        return np.frombuffer(bytes(s), dtype=np.uint8)
    return np.asarray(s, dtype=np.uint8)


def revcomp_code(code, k):
    code = np.asarray(code, dtype=np.int64)
    out = np.zeros_like(code)
    for _ in range(k):
        out = out * 4 + (3 - (code & 3))
        code = code >> 2
    return out


def window_codes(seq, k):
    """-> (codes int64[n], valid bool[n]) of the n = max(len - k + 1, 0) windows of one sequence."""
    c = CODE[as_bytes(seq)]
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    code = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        w = c[j:j + n]
        bad |= w > 3
        code = code * 4 + (w & 3)
    return code, ~bad


def counted_codes(seq, k, canonical=False):
    """The index every valid window of one sequence is counted under."""
    code, ok = window_codes(seq, k)
    code = code[ok]
    if canonical:
        code = np.minimum(code, revcomp_code(code, k))
    return code


def kmer_counts_one(seq, k, canonical=False):
    return np.bincount(counted_codes(seq, k, canonical), minlength=4 ** k).astype(np.int64)


def kmer_profile_truth(seqs, k, canonical=False):
    """One row per sequence -> int64[len(seqs), 4**k]."""
    out = np.zeros((len(seqs), 4 ** k), dtype=np.int64)
    for i, s in enumerate(seqs):
        out[i] = kmer_counts_one(s, k, canonical)
    return out


def kmer_counts_truth(seqs, k, canonical=False):
    """The spectrum of all the sequences together -> int64[4**k]."""
    codes = [counted_codes(s, k, canonical) for s in seqs]
    codes = np.concatenate(codes) if codes else np.zeros(0, dtype=np.int64)
    return np.bincount(codes, minlength=4 ** k).astype(np.int64)


def fold_canonical(counts, k):
    """Plain counts -> canonical counts: every entry moved to the smaller of its index and its reverse complement's."""
    counts = np.asarray(counts, dtype=np.int64)
    idx = np.arange(4 ** k, dtype=np.int64)
    out = np.zeros_like(counts)
    np.add.at(out, np.minimum(idx, revcomp_code(idx, k)), counts)
    return out


def flat_counts(flat, rec_start, slen, k, canonical=False, chunk=1 << 24):
    """The spectrum of records laid back to back in `flat` (record r = flat[rec_start[r] : rec_start[r] + slen[r]],
    rec_start[r + 1] = rec_start[r] + slen[r]), by rolling codes in chunks; the k - 1 windows in front of every record
    start would cross from one record into the next and are masked."""
    flat = as_bytes(flat)
    rec_start = np.asarray(rec_start, dtype=np.int64)
    slen = np.asarray(slen, dtype=np.int64)
    assert rec_start.size == 0 or ((rec_start[1:] == rec_start[:-1] + slen[:-1]).all() and rec_start[-1] + slen[-1] == flat.size)
    lut = CODE.astype(np.uint8)
    out = np.zeros(4 ** k, dtype=np.int64)
    n = flat.size - k + 1
    for a in range(0, max(n, 0), chunk):
        m = min(chunk, n - a)
        c = lut[flat[a:a + m + k - 1]]
        code = np.zeros(m, dtype=np.int64)
        bad = np.zeros(m, dtype=bool)
        for j in range(k):
            w = c[j:j + m]
            bad |= w > 3
            code *= 4
            code += w & 3
        s = rec_start[(rec_start > a) & (rec_start < a + m + k - 1)] - a      # record starts inside the windows of this chunk
        for j in range(1, k):
            t = s - j
            bad[t[(t >= 0) & (t < m)]] = True
        code = code[~bad]
        if canonical:
            code = np.minimum(code, revcomp_code(code, k))
        out += np.bincount(code, minlength=4 ** k)
    return out
