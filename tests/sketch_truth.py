"""The oracle of the sketch tests: a brute-force model of the definition in include/fxgpu.h over fa[i].seq and the read strings.
Per position the key of minimizer_truth.keys (every word read on its own, in Python ints), then Python sets, sorted, slicing to
`size`; compare_model merges two sorted lists.  Nothing is rolled, carried or retried.

key_set(seq, k, canonical)                       -> the set of keys of the valid windows of one text
keys_np / key_set_np(seq, k, canonical)          -> per position (valid, key) / the set as a sorted uint64 array, built on
                                                    minimizer.mix (the large cases; test_sketch_host pins it against key_set)
cut(keys, max_key, size)                         -> what a set keeps, a sorted list
fasta_sets(seqs, k, canonical, max_key, size, ids, pooled), fastq_set(reads, k, canonical, max_key, size, ids, start, end)
compare_model(A, B, limit, max_key)              -> (shared, total)"""
import numpy as np

from minimizer_truth import keys


def key_set(seq, k, canonical=True):
    return {e[0] for e in keys(seq, k, canonical, "hash") if e is not None}


def keys_np(seq, k, canonical=True):
    """Per position p of seq[p:p+k]: (valid, key) as numpy arrays -- the numpy form, built on minimizer.mix."""
    from pyfastx_amd import minimizer
    b = np.frombuffer(seq.encode("latin-1") if isinstance(seq, str) else seq, dtype=np.uint8)
    lut = np.full(256, 4, dtype=np.uint64)
    for ch, d in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        lut[ch] = d
    d = lut[b]
    n = d.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint64)
    bad = np.concatenate(([0], np.cumsum(d > 3)))
    ok = (bad[k:] - bad[:-k]) == 0
    d = np.where(d > 3, np.uint64(0), d)
    fw = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        fw = fw * np.uint64(4) + d[i:i + n]
        rc = rc * np.uint64(4) + (np.uint64(3) - d[k - 1 - i:k - 1 - i + n])
    code = np.minimum(fw, rc) if canonical else fw
    return ok, minimizer.mix(code, k)


def key_set_np(seq, k, canonical=True):
    ok, key = keys_np(seq, k, canonical)
    return np.unique(key[ok])


def cut(keyset, max_key, size=0):
    out = sorted(x for x in keyset if x < max_key)
    return out[:size] if size else out


def fasta_sets(seqs, k, canonical, max_key, size=0, ids=None, pooled=False, form=key_set):
    sel = range(len(seqs)) if ids is None else sorted(set(int(i) for i in ids))
    per = [set(int(x) for x in form(seqs[i], k, canonical)) for i in sel]
    if pooled:
        per = [set().union(*per)]
    return [cut(s, max_key, size) for s in per]


def fastq_set(reads, k, canonical, max_key, size=0, ids=None, start=None, end=None, form=key_set):
    ids = range(len(reads)) if ids is None else ids
    pool = set()
    for q, i in enumerate(ids):
        s = reads[int(i)]
        pool |= set(int(x) for x in form(s if start is None else s[int(start[q]):int(end[q])], k, canonical))
    return cut(pool, max_key, size)


def compare_model(A, B, limit=0, max_key=0):
    """A, B ascending distinct.  The merge of the two lists is the ascending distinct union; its first `limit` elements count."""
    if max_key:
        A, B = [x for x in A if x < max_key], [x for x in B if x < max_key]
    i = j = shared = total = 0
    while (i < len(A) or j < len(B)) and (limit == 0 or total < limit):
        if j >= len(B) or (i < len(A) and A[i] < B[j]):
            i += 1
        elif i >= len(A) or B[j] < A[i]:
            j += 1
        else:
            shared += 1
            i += 1
            j += 1
        total += 1
    return shared, total
