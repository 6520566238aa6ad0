"""-m gpu: the BGZF decoders on the corpus of deflate_truth.py -- valid deflate of shapes the other BGZF tests never produce
(large second-level tables, 15-bit codes, hundreds of short blocks, empty blocks, distance 32768, repeat codes across the
HLIT boundary; test_deflate_truth_host.py proves each shape on the CPU).  Every member must come out byte for byte as zlib
gives it, in every selectable form of the decoder, and who decoded it -- the wave kernel, or the serial kernel after a
hand-over, and why -- is pinned per class."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import deflate_truth as D
from conftest import ROOT

pytestmark = pytest.mark.gpu

INFL_RETRY = 100
HANDOVER_REASONS = {INFL_RETRY + r for r in (1, 2, 3, 4, 5, 6, 9)}       # what a VALID member may be handed over for
VARIANTS = {
    "default": {},
    "serial": {"FX_BGZF_SERIAL": "1"},
    "stage": {"FX_BGZF_STAGE": "1"},
    "replay": {"FX_BGZF_REPLAY": "1"},
    "stage_replay": {"FX_BGZF_STAGE": "1", "FX_BGZF_REPLAY": "1"},
    "fixed_shares": {"FX_BGZF_FIXED_SHARES": "1"},
}
SWITCHES = ("FX_BGZF_SERIAL", "FX_BGZF_STAGE", "FX_BGZF_REPLAY", "FX_BGZF_FIXED_SHARES")


def _variant():
    """The decoder form this process runs (the library reads the switches once)."""
    on = {k: "1" for k in SWITCHES if os.environ.get(k, "0") not in ("", "0")}
    return next(name for name, env in VARIANTS.items() if env == on)


# (handed over, reason of the first member handed over) per class, as observed on the MI355X; 0, 0: the wave kernel decoded
# every member itself.  FX_BGZF_SERIAL=1 is not in the table: there every member is the serial kernel's, (members, 0).
WAVE_DECODES_ALL = {name: (0, 0) for name in D.NAMES}
PINNED = {
    "default": dict(WAVE_DECODES_ALL),
    "stage": dict(WAVE_DECODES_ALL),
    "replay": dict(WAVE_DECODES_ALL),
    "stage_replay": dict(WAVE_DECODES_ALL),
    "fixed_shares": dict(WAVE_DECODES_ALL),
}
MUST_NOT_HAND_OVER = ("dna", "qual", "rle", "fixed_big", "dna_n_run", "fastq_records")                 # the contract of test_members_are_decoded_by_the_wave_kernel


@pytest.fixture(scope="module")
def L():
    from pyfastx_amd import _lib
    assert _lib.lib().fx_device_count() >= 1
    return _lib


def _open_and_compare(L, path, members, what):
    """Opens the BGZF file of `members` ((deflate, raw) each) and compares every byte; -> (members, handed over, reason)."""
    path.write_bytes(b"".join(D.member(cd, raw) for cd, raw in members))
    raw = b"".join(r for _, r in members)
    try:
        b = L.Blob.from_file(str(path))
    except L.FxError as e:                                 # (a wrong byte shows as a CRC or inflate error that names the member)
        pytest.fail("%s (%s): %s; member sizes %s" % (what, _variant(), e, [len(r) for _, r in members][:60]))
    assert b.is_gzip and b.size == len(raw), (what, b.size, len(raw))
    got = b.read_bytes(0, b.size)
    if got != raw:
        at = next(i for i in range(len(raw)) if got[i] != raw[i])
        ends = np.cumsum([len(r) for _, r in members])
        m = int(np.searchsorted(ends, at, side="right"))
        pytest.fail("%s (%s): first wrong byte at %d: member %d, offset %d of %d in it" % (what, _variant(), at, m, at - (int(ends[m - 1]) if m else 0), len(members[m][1])))
    counts = tuple(int(x) for x in b.bgzf_counts())
    b.close()
    return counts


@pytest.mark.parametrize("name", D.NAMES)
def test_class_decodes_to_the_bytes_of_zlib(L, tmp_path, name):
    members = D.CORPUS[name]
    first = _open_and_compare(L, tmp_path / (name + ".gz"), members, name)
    again = _open_and_compare(L, tmp_path / (name + "_again.gz"), members, name)
    print("observed", _variant(), name, first)
    n, handed, reason = first
    assert n == len(members) and again == first           # the decode of a member is deterministic
    if _variant() == "serial":
        assert (handed, reason) == (n, 0)
        return
    # a valid member handed over as damaged (INFL_RETRY + 16 + code) is a bug of the wave kernel, not a value to pin
    assert handed == 0 or reason in HANDOVER_REASONS, (name, first)
    if name in MUST_NOT_HAND_OVER:
        assert handed == 0, (name, first)
    assert (handed, reason) == PINNED[_variant()][name], (name, first)


def _all_in_a_shuffle_and_back():
    members = [(cd, raw) for _, _, cd, raw in D.all_members()]
    order = list(range(len(members)))
    np.random.default_rng(17).shuffle(order)
    return [members[i] for i in order + order[::-1]]


def _expected_handed(n):
    """Of the n members of the shuffle and back: all under FX_BGZF_SERIAL=1, else what the classes hand over, twice."""
    return n if _variant() == "serial" else 2 * sum(PINNED[_variant()][name][0] for name in D.NAMES)


def test_neighbours_keep_their_first_and_last_bytes(L, tmp_path, monkeypatch):
    """Every member of every class next to others, in a seeded shuffle and then in the reverse order: each has at some point a
    neighbour whose first and last bytes must survive its own last and first stores (eight bytes at a time in the wave kernel,
    four in the serial one), and the per-class counts add up."""
    monkeypatch.setenv("FX_BGZF_GROUP", "0")
    members = _all_in_a_shuffle_and_back()
    n, handed, reason = _open_and_compare(L, tmp_path / "all.gz", members, "all classes")
    print("observed", _variant(), "neighbours", (n, handed, reason))
    assert n == len(members) == 2 * len(D.all_members())
    assert handed == _expected_handed(n)


def test_neighbours_across_groups(L, tmp_path, monkeypatch):
    """The same file opened in groups of 64 KiB of compressed bytes: members straddle groups, the counts are the one-shot open's."""
    monkeypatch.setenv("FX_BGZF_GROUP", "65536")
    members = _all_in_a_shuffle_and_back()
    n, handed, reason = _open_and_compare(L, tmp_path / "groups.gz", members, "all classes in groups")
    assert n == len(members)
    assert handed == _expected_handed(n)


# One run of the three tests above in a fresh process: 5.0 s on the MI355X in the default form (measured once, from the start of
# the interpreter to its end; 3.2 s of it inside pytest); the other forms took 4.8 .. 6.3 s (the slowest: the serial kernel
# alone).  A child gets three times the 5.0.
CHILD_SECONDS = 5.0
CHILD_TIMEOUT = 3 * CHILD_SECONDS


def test_every_decoder_form():
    """The switches are read once per process, so every other form of the decoder runs the tests above in a child of its own:
    the serial kernel alone (the zipf classes, fib15, dist_32768, dist15 and greedy_pool among others are the first valid input
    that drives its canonical walk, decode_slow: their trees need more second-level entries than its POOL; the host tests
    guarantee that), the payload staged in LDS, phase B replaying the symbols of phase A, both, and the members in fixed
    shares.  One after the other: a child that fails, faults or runs into its time limit ends the test and no further child
    is started."""
    for name, switches in VARIANTS.items():
        if name == "default":
            continue
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(switches)
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k",
                            "class_decodes or neighbours"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        print("variant %s: exit %d after %.1f s" % (name, r.returncode, time.time() - t0))
        assert r.returncode == 0, "%s:\n%s%s" % (name, r.stdout[-4000:], r.stderr[-2000:])
        assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-1000:]
