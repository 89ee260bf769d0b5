"""The ctypes bindings of shipyard_amd.ops against the C prototypes.

``ops.SIGNATURES`` is the one place that says how many arguments of
which width every ``sy_*`` entry point takes; a row that disagrees with
its prototype would put garbage into a register on the device instead of
raising.  This module compares the table with the ``SY_EXPORT int``
prototypes in csrc/ (text only, no compiler), drives ``ops._call``
against a recording stand-in for the library, and checks that
``ops._load`` applies every row.  No device is needed."""
import ctypes
import re
from pathlib import Path
from unittest import mock

import numpy as np
import pytest

from shipyard_amd import ops

CSRC = Path(ops.__file__).resolve().parent / "csrc"
PROTOTYPE = re.compile(r"SY_EXPORT\s+int\s+(\w+)\s*\(([^)]*)\)")
SCALARS = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "int": ctypes.c_int, "int64_t": ctypes.c_int64}


def _prototypes() -> dict:
    """{entry point: [argument kind, ...]} of every exported prototype;
    a kind is "pointer" or the ctype of a scalar."""
    found = {}
    for path in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.cpp")):
        for name, arg_text in PROTOTYPE.findall(path.read_text()):
            assert name not in found, f"{name} is exported twice"
            kinds = []
            for arg in arg_text.split(","):
                words = [w for w in arg.split() if w != "const"]
                if "*" in arg or "hipStream_t" in words:
                    kinds.append("pointer")
                else:
                    assert len(words) == 2, (name, arg)  # type and name
                    kinds.append(SCALARS[words[0]])
            found[name] = kinds
    return found


def _kind(ctype):
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or \
            issubclass(ctype, ctypes._Pointer):
        return "pointer"
    return ctype


def test_table_matches_the_prototypes():
    protos = _prototypes()
    assert protos, "no prototype found: the pattern or the path is stale"
    assert set(ops.SIGNATURES) == set(protos)
    for name, kinds in protos.items():
        row = ops.SIGNATURES[name]
        assert len(row) == len(kinds), name
        assert [_kind(c) for c in row] == kinds, name


def test_entry_points_with_one_prototype_share_a_row():
    for group in (("sy_byte_shuffle", "sy_delta_filter", "sy_bit_shuffle"),
                  ("sy_lz4_decode_blocks", "sy_lz4_decode_blocks_pc"),
                  ("sy_lz4_compress_blocks_gpu",
                   "sy_lz4_compress_blocks_gpu2")):
        assert all(ops.SIGNATURES[e] is ops.SIGNATURES[group[0]]
                   for e in group), group


class _Recorder:
    """Stands in for the ctypes library: notes every attribute looked up
    on it and the arguments of every call."""

    def __init__(self, rc: int = 0):
        self.rc = rc
        self.looked_up = []
        self.calls = []

    def __getattr__(self, name):
        self.looked_up.append(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry


STREAM = ctypes.c_void_p(0x5EED)


@pytest.fixture()
def lib():
    lib = _Recorder()
    with mock.patch("shipyard_amd.ops._load", return_value=lib) as load, \
            mock.patch("shipyard_amd.ops._stream", return_value=STREAM):
        lib.load = load
        yield lib


def test_call_converts_pointers_and_leaves_the_rest(lib):
    torch = pytest.importorskip("torch")
    t = torch.zeros(64, dtype=torch.uint8)[16:]
    a = np.zeros(8, dtype=np.uint32)
    tail = ctypes.c_void_p(t.data_ptr() + 4)
    rc = ops._call("sy_anything", t, a, 7, -3, b"raw", tail)
    assert rc == 0
    (name, args), = lib.calls
    assert name == "sy_anything"
    assert isinstance(args[0], ctypes.c_void_p)
    assert args[0].value == t.data_ptr()
    assert isinstance(args[1], ctypes.c_void_p)
    assert args[1].value == a.ctypes.data
    assert args[2:5] == (7, -3, b"raw")
    assert all(type(x) is int for x in args[2:4])
    assert args[5] is tail
    assert args[6] is STREAM and len(args) == 7


def test_call_without_stream(lib):
    with mock.patch("shipyard_amd.ops._stream",
                    side_effect=AssertionError("stream asked for")):
        ops._call("sy_host_only", 1, 2, stream=False)
    assert lib.calls == [("sy_host_only", (1, 2))]


def test_call_touches_the_library_once(lib):
    ops._call("sy_one", 1)
    assert lib.load.call_count == 1
    assert lib.looked_up == ["sy_one"]
    ops._call("sy_two", 2, stream=False)
    assert lib.load.call_count == 2
    assert lib.looked_up == ["sy_one", "sy_two"]
    assert len(lib.calls) == 2


def test_call_raises_on_a_non_zero_return():
    lib = _Recorder(rc=-22)
    with mock.patch("shipyard_amd.ops._load", return_value=lib), \
            mock.patch("shipyard_amd.ops._stream", return_value=STREAM):
        with pytest.raises(RuntimeError,
                           match="sy_gather_copy failed with code -22"):
            ops._call("sy_gather_copy", 1)
    assert len(lib.calls) == 1


def test_call_resolves_the_library_at_call_time():
    with mock.patch("shipyard_amd.ops._load",
                    side_effect=AssertionError("library loaded")):
        with pytest.raises(AssertionError, match="library loaded"):
            ops._call("sy_gather_copy", 1, stream=False)


@pytest.mark.skipif(not ops.is_built(), reason="ops library not built")
def test_load_applies_every_row():
    lib = ops._load()
    assert ops._load() is lib  # cached
    for name, row in ops.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == list(row), name
