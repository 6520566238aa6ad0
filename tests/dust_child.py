"""Child of test_gpu_dust.py::test_memory_hygiene: one Fasta.low_complexity call and one Fastq.complexity call on the seam
inputs of write_inputs, in a process of its own, the arrays dumped to an .npz.

    python dust_child.py WORK MODE OUT      MODE: plain | behind (each call behind a wider call of the same entry on the same handle)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def write_inputs(work):
    """seam.fa / seam.fq in `work` (the same bytes on every call) -> (the sequences of the records, those of the reads)."""
    rng = np.random.default_rng(612)

    def rand(n, alphabet="ACGT"):
        return "".join(rng.choice(list(alphabet), n)) if n else ""
    seqs = ["A" * 40 + rand(500) + "AC" * 200 + rand(300, "ACGTN") + "t" * 9 + rand(400),       # rows from 0, over several runs
            "AAAA", "AAAA",                                                                    # nothing joins across records
            rand(130) + "GATTACA" * 60 + rand(250) + "N" * 70 + "CAG" * 30 + rand(90) + "G" * 33]  # a row that ends at slen
    with open(os.path.join(work, "seam.fa"), "w") as f:
        for i, s in enumerate(seqs):
            f.write(">s%d\n" % i + "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60)))
    reads = []
    for i, n in enumerate((0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 150, 151, 1000, 150, 150, 4000)):
        reads.append([rand(n), "A" * n, ("AC" * n)[:n], rand(n, "ACGTNacgt")][i % 4])
    with open(os.path.join(work, "seam.fq"), "w") as f:
        for i, s in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return seqs, reads


def main(work, mode, out):
    sys.path.insert(0, os.path.dirname(HERE))
    import pyfastx_amd
    from pyfastx_amd import _lib
    fa, fq = pyfastx_amd.Fasta(os.path.join(work, "seam.fa")), pyfastx_amd.Fastq(os.path.join(work, "seam.fq"))
    if mode == "behind":
        fa.low_complexity(8, 1)                              # more rows, from the same handle
    r = fa.low_complexity(64, 20)
    if mode == "behind":
        fq.complexity(ids=np.tile(np.arange(len(fq)), 5))
    c = fq.complexity()
    byte, blocks, nbytes = _lib.debug_fill_info()
    np.savez(out, ids=np.asarray(r.ids), starts=np.asarray(r.starts), stops=np.asarray(r.stops), fill_byte=byte, fill_blocks=blocks, fill_bytes=nbytes,
             **{k: np.asarray(c[k]) for k in ("length", "n_triplets", "dust_sum", "n_diff")})


if __name__ == "__main__":
    main(*sys.argv[1:4])
