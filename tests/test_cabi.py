"""CPU: libfxgpu.so loads, exports every function include/fxgpu.h declares, and
refuses to compute without a GPU (no silent CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def declared():
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_symbol_is_exported():
    from pyfastx_amd import _lib
    L = _lib.lib()
    names = declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), "%s declared in include/fxgpu.h but not exported" % n
    assert set(names) == set(_lib.SYMBOLS), set(names) ^ set(_lib.SYMBOLS)
    assert b"gfx950" in L.fx_version()


_POINTERS = (C.c_void_p, C.c_char_p, C._Pointer)
_SCALARS = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "int64_t": (C.c_int64,), "uint64_t": (C.c_uint64,),
            "uint8_t": (C.c_uint8,), "double": (C.c_double,)}


def _agrees(ctype, text, what):
    """One argument or return type of the binding against the header's text for it, by class."""
    text = " ".join(w for w in re.sub(r"[*\[]", " * ", text).split() if w != "const")
    if "*" in text:
        assert isinstance(ctype, type) and issubclass(ctype, _POINTERS), "%s: %r is a pointer, bound as %r" % (what, text, ctype)
    elif text == "void":
        assert ctype is None, "%s: void, bound as %r" % (what, ctype)
    else:
        assert text in _SCALARS, "%s: %r is outside the mapping" % (what, text)
        assert any(ctype is t for t in _SCALARS[text]), "%s: %r bound as %r" % (what, text, ctype)


def test_every_prototype_matches_the_binding_table():
    """include/fxgpu.h against _lib.PROTOTYPES: the return type, the number of arguments and the class of every argument (an
    int bound where the header says int64_t would load, run and truncate).  Reads the table, not the library."""
    from pyfastx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", "", hdr, flags=re.M)                     # line comments, preprocessor lines
    seen, n_args = set(), 0
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s]*?[\s*]+)(fx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        assert name not in seen, "%s is declared twice" % name
        seen.add(name)
        assert name in _lib.PROTOTYPES, "%s is declared but not in the table" % name
        res, bound = _lib.PROTOTYPES[name]
        _agrees(res, ret, name + " returns")
        args = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        assert len(args) == len(bound), "%s: %d arguments declared, %d bound" % (name, len(args), len(bound))
        for j, (a, t) in enumerate(zip(args, bound)):
            m = re.fullmatch(r"(.*?)\b[A-Za-z_]\w*\s*((?:\[\w*\])?)", a)             # type, parameter name, [n]
            assert m and m.group(1).strip(), "%s: argument %d (%r) does not read as `type name`" % (name, j, a)
            _agrees(t, m.group(1) + m.group(2), "%s argument %d" % (name, j))
        n_args += len(args)
    assert sorted(seen) == declared() and len(seen) == len(_lib.PROTOTYPES), set(declared()) ^ seen
    assert n_args == sum(len(a) for _, a in _lib.PROTOTYPES.values()) > 0


def test_summary_struct_layout_matches_header():
    from pyfastx_amd import _lib, shard
    assert C.sizeof(_lib.ShardSummary) == 8 * shard.NWORDS == 224
    assert [f[0] for f in _lib.ShardSummary._fields_] == shard.FIELDS


def test_no_cpu_fallback_without_gpu():
    from pyfastx_amd import _lib
    L = _lib.lib()
    if L.fx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.FxError) as e:
        _lib.Blob.from_bytes(b">a\nACGT\n")
    assert e.value.code == _lib.FX_EDEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(_lib.FxError):
        _lib.revcomp_bytes(b"ACGT")
    import pyfastx_amd
    with pytest.raises(RuntimeError):                     # the object API surfaces it, it does not route around it
        pyfastx_amd.Fasta(os.path.join(ROOT, "tests", "data", "test.fa"), memory_index=True)


@pytest.mark.parametrize("value,byte", [(None, -1), ("", -1), ("255", 255), ("0", 0), ("010", 10), ("0x7f", -1), ("256", -1), ("-1", -1), ("12x", -1)])
def test_debug_fill_switch_is_read_once_at_load(value, byte):
    """FX_DEBUG_FILL: unset or empty is off, a decimal 0..255 the byte in force, anything else off; nothing is filled before a block is
    asked for.  A process of its own each: the library reads the variable when it is loaded."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "FX_DEBUG_FILL"}
    env["FX_NO_TORCH"] = "1"
    if value is not None:
        env["FX_DEBUG_FILL"] = value
    r = subprocess.run([sys.executable, "-c", "from pyfastx_amd import _lib; print(*_lib.debug_fill_info())"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(byte), "0", "0"], (r.stdout, r.stderr[-500:])


def test_missing_file_status():
    from pyfastx_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().fx_open_file(b"/nonexistent/file.fa", 0, C.byref(h))
    assert rc == _lib.FX_ENOENT
