"""CPU: the generator of the seam sweeps (tests/seam_cases.py) does what the GPU sweeps rely on -- the marked byte of a probe
lies at seam + d, what stands in front of the probe is whole lines of one regular record (whole FASTQ records of one size),
the placements of a probe show every byte of it on both sides of the seam, the island granules overflow a record slot and
their neighbours do not.  Where oracle/_ref is built, the oracle's rows of every probe and placement at the 4 KiB seam are
those of the compiled reference."""
import glob
import os
import sqlite3
import sys

import numpy as np
import pytest

import seam_cases as sc
from conftest import ROOT


def _rng(*key):
    return np.random.default_rng([7] + [int(x) for x in key])


def _whole_fasta_lines(front, eol):
    """front: a header line, then lines of exactly WIDTH letters, all terminated"""
    assert front.endswith(eol) and front.startswith(b">bg")
    h = front.index(b"\n") + 1
    body = np.frombuffer(front[h:], dtype=np.uint8)
    w = sc.WIDTH + len(eol)
    assert body.size % w == 0
    body = body.reshape(-1, w)
    assert (body[:, sc.WIDTH:] == np.frombuffer(eol, dtype=np.uint8)).all()
    assert np.isin(body[:, :sc.WIDTH], np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    assert set(front[3:h - len(eol)]) <= {ord("x")}
    return body.shape[0]


@pytest.mark.parametrize("eol", ["lf", "crlf"])
@pytest.mark.parametrize("kind", sc.FASTA_SEAMS)
def test_fasta_placement_invariant(kind, eol):
    E, seam = sc.EOLS[eol], sc.SEAMS[kind]
    big = seam >= (1 << 20)
    for name, (probe, places) in sc.fasta_probes(E).items():
        for i, (mark, d) in enumerate(places):
            if big and 0 < i < len(places) - 1 and i % 8:      # the arithmetic is the same at every size: the large seams take a sample
                continue
            raw = sc.place_fasta(probe, mark, seam, d, E, _rng(seam, i))
            start = seam + d - mark
            assert raw[start:start + len(probe)] == probe, (name, mark, d)
            assert raw[seam + d] == probe[mark]
            _whole_fasta_lines(raw[:start], E)
            tail = raw[start + len(probe):]
            assert len(tail) == 3 * (sc.WIDTH + len(E)) and tail.endswith(E) and tail.count(b"\n") == 3


@pytest.mark.parametrize("eol", ["lf", "crlf"])
def test_every_probe_byte_is_seen_on_both_sides(eol):
    E = sc.EOLS[eol]
    probes = dict(sc.fasta_probes(E))
    probes.update({"fq:" + k: v for k, v in sc.fastq_probes(E).items()})
    for name, (probe, places) in probes.items():
        if name in ("LH", "fq:RL"):                          # named placements: the seam at the listed bytes, and one to either side
            for m in sorted({m for m, _ in places}):
                assert {d for mm, d in places if mm == m} == {-1, 0, 1}
            continue
        assert len(places) == len(probe) + 5
        rel = np.array([d - m for m, d in places])           # offset of the probe's first byte relative to the seam
        for i in range(len(probe)):
            assert ((rel + i) < 0).any() and ((rel + i) >= 0).any(), (name, i)
        assert sorted(-rel) == list(range(-2, len(probe) + 3))  # the seam in front of every byte, behind the last, two more on either side


@pytest.mark.parametrize("bg", sc.FASTQ_BACKGROUNDS)
@pytest.mark.parametrize("kind", ["16B", "4K", "16K", "64K", "1M"])
def test_fastq_placement_invariant(kind, bg):
    E = sc.fastq_bg_eol(bg)
    for name, (probe, places) in sc.fastq_probes(E).items():
        seam = sc.seam_offset(kind, sc.fastq_need(len(probe), bg))
        assert (seam - sc.SEAMS[kind]) % 65536 == 0 and (seam % (1 << 20) or kind.endswith("M"))
        for i, (mark, d) in enumerate(places):
            if seam >= (1 << 20) and 0 < i < len(places) - 1 and i % 8:
                continue
            raw, island = sc.place_fastq(probe, mark, seam, d, bg, _rng(seam, i))
            start = seam + d - mark
            assert raw[start:start + len(probe)] == probe, (name, mark, d)
            front = raw[:start] if bg != "island_before" else raw[:island[0]]
            assert front.endswith(E) and front.count(b"\n") % 4 == 0
            lines = front.split(b"\n")
            rlen = 20 if bg == "r20" else 150
            assert all(len(x.rstrip(b"\r")) == rlen for x in lines[1::4]) and all(x.rstrip(b"\r") == b"+" for x in lines[2::4])
            assert len({len(x) for x in lines[4::4] if x}) <= 1          # one record size; only the first name is padded
            assert raw.count(b"\n") % 4 == 0 and raw.endswith(E)
            if island:
                assert (island[1] == start) if bg == "island_before" else (island[0] == start + len(probe))


@pytest.mark.parametrize("bg", ["island_before", "island_after"])
def test_island_granules_overflow_and_their_neighbours_do_not(bg):
    probe, places = sc.fastq_probes(b"\n")["R"]
    for kind in ("4K", "16K", "1M"):
        for mark, d in places[::6]:
            raw, (a, b) = sc.place_fastq(probe, mark, sc.seam_offset(kind, sc.fastq_need(len(probe), bg)), d, bg, _rng(1))
            assert len(raw) >= sc.ISLAND_MIN_STREAM
            nl = sc.newlines_per_granule(raw)[:len(raw) // 4096]
            inside = np.arange((a + 4095) // 4096, b // 4096)            # granules that lie entirely in the island
            assert inside.size >= 3 and (nl[inside] > sc.FQL_CAP).all()
            outside = np.r_[0:a // 4096, (b + 4095) // 4096:nl.size]
            assert (nl[outside] < sc.FQL_CAP).all()
            # the density the build samples (the first, middle and last 256 KiB) stays that of a one-read build
            assert nl.sum() * 1.0 / nl.size <= 0.7 * sc.FQL_CAP


def test_short_read_background_is_dense():
    probe, places = sc.fastq_probes(b"\n")["R"]
    raw, _ = sc.place_fastq(probe, 0, sc.SEAMS["16K"], 0, "r20", _rng(2))
    nl = sc.newlines_per_granule(raw)[:len(raw) // 4096]
    assert (nl > 0.7 * sc.FQL_CAP).all()


def test_truncations_end_every_way():
    """the END cuts of probe H hold a terminated line, an unterminated one, one ending in CR and a bare header; d = 0 gives a
    stream of a whole number of granules"""
    for eol in ("lf", "crlf"):
        E = sc.EOLS[eol]
        probe = sc.fasta_probes(E)["H"][0]
        ends = set()
        for m in sc.end_marks(probe):
            for d in (-2, -1, 0, 1, 2):
                raw = sc.truncated_fasta(probe, m, sc.SEAMS["4K"], d, E, _rng(m))
                assert len(raw) == sc.SEAMS["4K"] + d
                last = raw[raw.rstrip(b"\r\n").rfind(b"\n") + 1:]
                ends.add(("hdr" if last.startswith(b">") else "seq", "lf" if raw.endswith(b"\n") else "cr" if raw.endswith(b"\r") else "open"))
        want = {("hdr", "lf"), ("hdr", "open"), ("seq", "lf"), ("seq", "open")}
        if eol == "crlf":
            want |= {("hdr", "cr"), ("seq", "cr")}
        assert want <= ends, (eol, ends)


def test_width_sweep_and_record_counts(oracle):
    widths = [1, 2, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]
    for eol in ("lf", "crlf"):
        raw = sc.width_sweep(widths, sc.EOLS[eol], _rng(3))
        recs, _ = oracle.fasta_index(raw)
        assert len(recs) == len(widths)
        assert [int(x) for x in recs["llen"]] == [w + len(sc.EOLS[eol]) for w in widths]
        assert (recs["blen"] >= 3 * 4096).all() and (recs["norm"] == 1).all()
    for n in (4095, 4096, 4097):
        recs, tot = oracle.fasta_index(sc.one_line_records(n))
        assert len(recs) == n and tot == 8 * n and len(sc.one_line_records(n)) == 20 * n


def test_run_seam_stream_places_six_probes(oracle):
    for eol in ("lf", "crlf"):
        E = sc.EOLS[eol]
        H = sc.fasta_probes(E)["H"][0]
        raw, where = sc.run_seam_stream(1 << 20, 16384, E, _rng(4))
        assert len(raw) > (1 << 20) and len(where) == 6
        for seam, mark, d in where:
            assert seam % 16384 == 0 and raw[seam + d - mark:seam + d - mark + len(H)] == H
        recs, _ = oracle.fasta_index(raw)
        assert len(recs) == 18                               # per seam: the aligning record, p1 and p2


# ------------------------------------------------------------------------------------------------- against the reference
@pytest.fixture(scope="module")
def ref():
    if not glob.glob(os.path.join(ROOT, "oracle", "_ref", "pyfastx*.so")):
        pytest.skip("oracle/_ref not built here")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
    import pyfastx
    return pyfastx


@pytest.mark.parametrize("eol", ["lf", "crlf"])
def test_oracle_rows_equal_the_reference_at_the_granule_seam(oracle, ref, tmp_path, eol):
    E, seam = sc.EOLS[eol], sc.SEAMS["4K"]
    p = str(tmp_path / "s.fa")
    for name, (probe, places) in sc.fasta_probes(E).items():
        for i, (mark, d) in enumerate(places):
            raw = sc.place_fasta(probe, mark, seam, d, E, _rng(seam, i))
            for q in (p, p + ".fxi"):
                if os.path.exists(q):
                    os.remove(q)
            open(p, "wb").write(raw)
            full_name = bool(i & 1)
            ref.Fasta(p, full_index=False, full_name=full_name)
            db = sqlite3.connect(p + ".fxi")
            want = db.execute("SELECT * FROM seq ORDER BY ID").fetchall()
            db.close()
            recs, tot = oracle.fasta_index(raw, full_name=full_name)
            got = [(k + 1, raw[r["name_off"]:r["name_off"] + r["name_len"]].decode("latin-1")) +
                   tuple(int(r[c]) for c in ("boff", "blen", "slen", "llen", "elen", "norm", "dlen")) for k, r in enumerate(recs)]
            assert got == want, (name, mark, d)


@pytest.mark.parametrize("bg", ["r150", "r150crlf", "r20"])
def test_oracle_reads_equal_the_reference_at_the_granule_seam(oracle, ref, tmp_path, bg):
    E = sc.fastq_bg_eol(bg)
    p = str(tmp_path / "s.fq")
    for name, (probe, places) in sc.fastq_probes(E).items():
        seam = sc.seam_offset("4K", sc.fastq_need(len(probe), bg))
        for i, (mark, d) in enumerate(places):
            raw, _ = sc.place_fastq(probe, mark, seam, d, bg, _rng(seam, i))
            for q in (p, p + ".fxi"):
                if os.path.exists(q):
                    os.remove(q)
            open(p, "wb").write(raw)
            ref.Fastq(p, full_index=False)
            db = sqlite3.connect(p + ".fxi")
            want = db.execute("SELECT * FROM read ORDER BY ID").fetchall()
            db.close()
            rq, size, ln = oracle.fastq_index(raw)
            got = [(k + 1, raw[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])].decode("latin-1")) +
                   tuple(int(r[c]) for c in ("dlen", "rlen", "soff", "qoff")) for k, r in enumerate(rq)]
            assert got == want, (name, mark, d)
