"""Shards, rows and expected values shared by the typed row read tests
(test_shard_rows on the CPU, test_rows_gpu on the device).  Everything
is computed once and must not be modified by a test."""
import functools

import numpy as np

from shipyard_amd.data import shardfmt

BLOCK = 4096
# 5 full blocks and a ragged one whose length is no multiple of 2 or 4
N_RAW = 5 * BLOCK + 1003

# every allowed (src_dtype, out_dtype)
PAIRS = [(s, o) for o in ("int32", "int64")
         for s in ("u1", "u2", "i2", "u4", "i4")
         if (s, o) != ("u4", "int32")]
SIZE = {"u1": 1, "u2": 2, "i2": 2, "u4": 4, "i4": 4}
NUMPY = {"u1": "<u1", "u2": "<u2", "i2": "<i2", "u4": "<u4", "i4": "<i4"}


def pair_id(p):
    return "%s-%s" % p


def filters(size: int):
    """(name, writer keywords): none, shuffle, delta + shuffle and
    bitshuffle over the source element; a 1-byte element has none."""
    if size == 1:
        return [("plain", {})]
    return [("plain", {}),
            ("shuffle", {"shuffle_elem": size}),
            ("delta-shuffle", {"delta_elem": size, "shuffle_elem": size}),
            ("bitshuffle", {"bitshuffle_elem": size})]


@functools.lru_cache(maxsize=None)
def raw() -> bytes:
    """Three blocks of slowly rising int32 values (LZ4 blocks), then
    random bytes (stored; every bit pattern of every type, among them
    set sign bits)."""
    rng = np.random.default_rng(77)
    vals = np.cumsum(rng.integers(0, 5, 3 * BLOCK // 4)).astype("<u4")
    noise = rng.integers(0, 256, N_RAW - 3 * BLOCK, dtype=np.uint8)
    return vals.tobytes() + noise.tobytes()


@functools.lru_cache(maxsize=None)
def packed(filt: str, size: int) -> bytes:
    kw = dict(filters(size))[filt]
    return shardfmt.pack(raw(), block_raw=BLOCK, **kw)


@functools.lru_cache(maxsize=None)
def elements(src_dtype: str):
    """The addressable elements of the shard as a read-only array."""
    size = SIZE[src_dtype]
    arr = np.frombuffer(raw()[:N_RAW // size * size], dtype=NUMPY[src_dtype])
    arr.flags.writeable = False
    return arr


def rows(size: int):
    """(starts, counts, row_elems) in elements: inside one block, over
    one block boundary, over three, up to the last addressable element,
    empty rows (one behind the last element), a repeat; unsorted."""
    eb = BLOCK // size
    n_el = N_RAW // size
    starts = [n_el - 5, 10, eb - 3, 77, eb - 1, n_el, 10, 4 * eb + 1]
    counts = [5, 20, 6, 0, 2 * eb + 2, 0, 20, 1]
    return starts, counts, 2 * eb + 2


def pads(out_dtype: str):
    info = np.iinfo(out_dtype)
    return [0, -100, 50256, int(info.min), int(info.max)]


def want(src_dtype: str, out_dtype: str, starts, counts, row_elems, pad):
    """The expected [n, row_elems] array by slicing the original data."""
    arr = elements(src_dtype)
    out = np.full((len(starts), row_elems), pad, dtype=out_dtype)
    for i, (s, c) in enumerate(zip(starts, counts)):
        out[i, :c] = arr[s:s + c].astype(out_dtype)
    return out
