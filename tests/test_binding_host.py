"""CPU: the call path of the ctypes binding (_lib._sel, _call, _ragged) and the two error translations (_lib.too_many,
_lib.outside), driven with fake entries -- no library and no GPU."""
import ctypes as C
import gc
import types

import numpy as np
import pytest

from pyfastx_amd import _lib


def _read(addr, n, ctype=C.c_int64):
    return list((ctype * n).from_address(addr))


@pytest.fixture
def host(monkeypatch):
    """_lib without a library: pinned_array views the memory a fake entry handed out, fx_last_error is a fixed text."""
    def view(ptr, count, dtype=np.uint8):
        dt = np.dtype(dtype)
        return np.frombuffer((C.c_char * (int(count) * dt.itemsize)).from_address(int(ptr)), dtype=dt, count=int(count))
    monkeypatch.setattr(_lib, "pinned_array", view)
    monkeypatch.setattr(_lib, "_LIB", types.SimpleNamespace(fx_last_error=lambda: b"refused by the fake"))
    return _lib


# ------------------------------------------------------------------ the selection
def test_selection_none_is_null():
    assert _lib._sel(None) == (None, 0)


@pytest.mark.parametrize("empty", [[], (), np.zeros(0, dtype=np.int32), np.arange(6)[3:3]])
def test_selection_empty_hands_over_a_valid_pointer(empty):
    buf, n = _lib._sel(empty)
    assert n == 0 and buf.dtype == np.int64 and buf.size >= 1 and buf.ctypes.data != 0 and buf.flags.c_contiguous


@pytest.mark.parametrize("ids", [[4, 0, 2], np.array([4, 0, 2], dtype=np.int32), np.arange(12, dtype=np.int64)[2::4],
                                 np.array([[4, 9], [0, 9], [2, 9]])[:, 0]])
def test_selection_is_int64_and_contiguous(ids):
    buf, n = _lib._sel(ids)
    assert n == 3 and buf.dtype == np.int64 and buf.flags.c_contiguous and buf.ctypes.data != 0
    assert _read(buf.ctypes.data, 3) == [int(x) for x in ids]          # what an entry reads through the pointer


def test_selection_keeps_an_int64_array_as_it_is():
    ids = np.array([1, 2], dtype=np.int64)
    assert _lib._sel(ids)[0] is ids


# ------------------------------------------------------------------ the call
class Entry:
    """A fake fx_* entry of the shape fn(handle, ids, n_ids, cap, 3 out-pointers, n, total, counts): it answers with one row per
    id, reading every array through the address it was given, and refuses more than `cap` rows."""

    def __init__(self):
        self.blocks, self.saw = [], None

    def __call__(self, h, ids, n_ids, cap, p0, p1, p2, n, total, counts):
        gc.collect()                                            # whatever the caller no longer holds is gone by now
        np.zeros(1 << 16)                                       # and its memory may have been handed out again
        assert isinstance(ids, int) and isinstance(counts, int)
        got = _read(ids, n_ids)
        self.saw = (h, got, cap)
        total._obj.value = n_ids
        (C.c_int64 * (2 * n_ids)).from_address(counts)[:] = [v for x in got for v in (x, -x)]
        if n_ids > cap:
            return _lib.FX_ERANGE
        n._obj.value = n_ids
        cols = (np.array(got + [99] * 3, dtype=np.int64), np.array(got + [99] * 3, dtype=np.uint8),
                np.array([7 * x + j for x in got for j in range(7)] + [99] * 7, dtype=np.int32))
        self.blocks.append(cols)                                # the "pinned" blocks: longer than n rows, as the library's may be
        for p, a in zip((p0, p1, p2), cols):
            if p is not None:                                   # NULL: the caller does not want this column
                p._obj.value = a.ctypes.data
        return 0


def test_call_returns_the_columns_cut_to_n_and_the_counters(host):
    fn = Entry()
    cols, vals = host._call(fn, (5, *host._sel(np.array([3, 1, 2], dtype=np.int32)), 10), (np.int64, np.uint8, (np.int32, 7)),
                            counters=(0, 0), err=("n_rows", 1), tail=(np.zeros((3, 2), dtype=np.int64),))
    assert fn.saw == (5, [3, 1, 2], 10) and vals == [3, 3]
    assert [c.dtype for c in cols] == [np.int64, np.uint8, np.int32] and [c.shape for c in cols] == [(3,), (3,), (3, 7)]
    assert cols[0].tolist() == [3, 1, 2] and cols[1].tolist() == [3, 1, 2] and cols[2][:, 0].tolist() == [21, 7, 14]


def test_call_holds_every_array_while_the_entry_runs(host):
    fn = Entry()
    cnt = np.zeros((4, 2), dtype=np.int64)
    # the selection and the view of the counts exist nowhere but in the argument tuples
    cols, _ = host._call(fn, (1, *host._sel(list(range(100, 104))), 4), (np.int64, None, host.RAW), counters=(0, 0), tail=(cnt.reshape(-1).view(),))
    assert fn.saw == (1, [100, 101, 102, 103], 4) and cnt.tolist() == [[x, -x] for x in range(100, 104)]
    assert cols[0].tolist() == [100, 101, 102, 103] and cols[1] is None and cols[2] == fn.blocks[0][2].ctypes.data


def test_call_passes_null_for_none(host):
    seen = []
    cols, vals = host._call(lambda *a: seen.append(a) or 0, (1, None, 0), (None,), counters=(), tail=(None,))
    assert seen == [(1, None, 0, None, None)] and cols == (None,) and vals == []


def test_call_gives_none_for_a_pointer_left_null(host):
    cols, vals = host._call(lambda h, p, n: 0, (1,), (np.int64,))
    assert cols == (None,) and vals == [0]


@pytest.mark.parametrize("err,counters,want", [(("n_rows", 1), (0, 0), 3), (("n_hits", 0), (0, 0), 0), (("first_bad", 0), (-1, 0), -1)])
def test_call_raises_with_the_named_attribute(host, err, counters, want):
    with pytest.raises(host.FxError) as e:
        host._call(Entry(), (5, *host._sel([3, 1, 2]), 2), (np.int64,) * 3, counters=counters, err=err, tail=(np.zeros(6, dtype=np.int64),))
    assert e.value.code == host.FX_ERANGE and str(e.value) == "refused by the fake" and getattr(e.value, err[0]) == want
    assert {"n_rows", "n_hits", "first_bad"} & set(vars(e.value)) == {err[0]}


def test_call_without_err_raises_a_plain_error(host):
    with pytest.raises(host.FxError) as e:
        host._call(lambda h, n: host.FX_ESTATE, (1,))
    assert e.value.code == host.FX_ESTATE and set(vars(e.value)) == {"code"}


# ------------------------------------------------------------------ the ragged pair
@pytest.mark.parametrize("lens", [[], [3, 0]])
def test_ragged(host, lens):
    n = len(lens)
    offs = np.array(np.concatenate([[0], np.cumsum(lens), [77]]), dtype=np.int64)          # n + 2 items, the last is not an offset
    dst = np.arange(max(int(offs[n]), 1) + 4, dtype=np.uint8)
    buf, o = host._ragged(dst.ctypes.data, offs.ctypes.data, n)
    assert buf.dtype == np.uint8 and buf.tolist() == list(range(sum(lens)))
    assert o.dtype == np.int64 and o.tolist() == offs[:n + 1].tolist()


# ------------------------------------------------------------------ the two translations
def _error(code, **attrs):
    e = _lib.FxError(code, "the library's text")
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("attr,noun,arg,text", [
    ("n_hits", "hits", "max_hits", "12 hits, more than max_hits=11"),
    ("n_hits", "minimizers", "max_hits", "12 minimizers, more than max_hits=11"),
    ("n_rows", "windows", "max_windows", "12 windows, more than max_windows=11"),
    ("n_rows", "runs", "max_runs", "12 runs, more than max_runs=11"),
    ("n_rows", "repeats", "max_repeats", "12 repeats, more than max_repeats=11"),
    ("n_rows", "open reading frames", "max_orfs", "12 open reading frames, more than max_orfs=11"),
])
def test_too_many(attr, noun, arg, text):
    got = _lib.too_many(_error(_lib.FX_ERANGE, **{attr: 12}), noun, arg, 11)
    assert type(got) is ValueError and str(got) == text
    for e in (_error(_lib.FX_ERANGE, **{attr: 11}), _error(_lib.FX_ERANGE), _error(_lib.FX_ENOMEM, **{attr: 12})):
        assert _lib.too_many(e, noun, arg, 11) is e


def test_outside():
    got = _lib.outside(_error(_lib.FX_ERANGE, first_bad=3))
    assert type(got) is ValueError and str(got) == "the interval of query 3 lies outside its read"
    got = _lib.outside(_error(_lib.FX_ERANGE, first_bad=0), "diagonal", "pair")
    assert type(got) is ValueError and str(got) == "the diagonal of query 0 lies outside its pair"
    for e in (_error(_lib.FX_ERANGE, first_bad=-1), _error(_lib.FX_ERANGE), _error(_lib.FX_EINVAL, first_bad=3)):
        assert _lib.outside(e) is e
