"""Plain Python truth of Fasta.tandem_repeats, straight from the definition: per period the maximal stretches of a `seq`
string whose every letter equals the one `period` places before it, kept when long enough and when the motif is not a
shorter word written several times.  Brute force, quadratic in places, for test-sized texts; it shares nothing with the
package."""

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
DEFAULT = (12, 7, 5, 4, 4, 4)


def codes(seq):
    """The folded letters: 0..3 for A C G T of either case, None for every other letter."""
    return [CODE.get(ch) for ch in seq]


def min_copies_list(min_copies):
    """A sequence of 1..8 thresholds or a dict {period: copies} -> the eight thresholds, 0 = period not searched."""
    if isinstance(min_copies, dict):
        return [int(min_copies.get(p, 0)) for p in range(1, 9)]
    mc = [int(v) for v in min_copies]
    return mc + [0] * (8 - len(mc))


def is_power(word):
    """word is a shorter word written two or more times"""
    n = len(word)
    return any(n % q == 0 and word == word[:q] * (n // q) for q in range(1, n))


def repeats(seq, min_copies=DEFAULT, min_len=0):
    """-> [(start, stop, period, motif code)] ordered by (stop, period)."""
    c, mc, rows = codes(seq), min_copies_list(min_copies), []
    n = len(c)
    for p in range(1, 9):
        if mc[p - 1] == 0:
            continue
        need = max(2 * p, p * mc[p - 1], min_len)
        # every maximal stretch, left to right: extend while valid and periodic
        a = 0
        while a < n:
            if c[a] is None:
                a += 1
                continue
            b = a + 1
            while b < n and c[b] is not None and (b - a < p or c[b] == c[b - p]):
                b += 1
            if b - a >= need:
                word = tuple(c[a:a + p])
                if not is_power(word):
                    m = 0
                    for x in word:
                        m = m * 4 + x
                    rows.append((a, b, p, m))
            # stopped by a letter that differs from the one p before it: the next stretch holds the p - 1 letters in front
            # of it; stopped by an invalid letter or the end: it begins behind
            a = b - p + 1 if b < n and c[b] is not None else b
    rows.sort(key=lambda r: (r[1], r[2]))
    return rows


def motif_string(code, p):
    return "".join("ACGT"[(code >> (2 * (p - 1 - i))) & 3] for i in range(p))


def canonical(code, p):
    """The smallest code among all rotations of the motif and of its reverse complement."""
    w = [(code >> (2 * (p - 1 - i))) & 3 for i in range(p)]
    rc = [3 - x for x in reversed(w)]
    best = None
    for word in (w, rc):
        for r in range(p):
            v = 0
            for x in word[r:] + word[:r]:
                v = v * 4 + x
            best = v if best is None or v < best else best
    return best
