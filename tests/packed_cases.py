"""Shards, plans and expected values shared by the packed read tests
(test_packed on the CPU, test_packed_gpu on the device).  Everything is
computed once and must not be modified by a test."""
import functools

import numpy as np

from shipyard_amd.data import shardfmt

BLOCK = 8192
# 5 full blocks and a ragged one of 6 bytes
N_RAW = 40 * 1024 + 6

# name -> (source type, element bytes, writer keywords)
SHARDS = {
    "u2-shuffle": ("u2", 2, {"shuffle_elem": 2}),
    "i4-delta-bitshuffle": ("i4", 4, {"delta_elem": 4, "bitshuffle_elem": 4}),
}


@functools.lru_cache(maxsize=None)
def raw() -> bytes:
    """Two blocks of slowly rising int32 values (LZ4 blocks), then random
    bytes (stored; every bit pattern, among them set sign bits)."""
    rng = np.random.default_rng(1234)
    vals = np.cumsum(rng.integers(0, 5, 2 * BLOCK // 4)).astype("<u4")
    noise = rng.integers(0, 256, N_RAW - 2 * BLOCK, dtype=np.uint8)
    return vals.tobytes() + noise.tobytes()


@functools.lru_cache(maxsize=None)
def packed(name: str) -> bytes:
    return shardfmt.pack(raw(), block_raw=BLOCK, **SHARDS[name][2])


@functools.lru_cache(maxsize=None)
def elements(name: str):
    """The addressable elements of the shard as a read-only array."""
    src, size, _ = SHARDS[name]
    arr = np.frombuffer(raw()[:N_RAW // size * size], dtype="<" + src[0] +
                        src[1])
    arr.flags.writeable = False
    return arr


def samples(size: int):
    """(starts, counts) in elements, unsorted in the source: inside one
    block, over a block boundary, empty samples, a repeat, one up to the
    last addressable element, one that fills a row of 64."""
    eb = BLOCK // size
    n_el = N_RAW // size
    starts = [3 * eb + 100, 5, eb - 10, 77, 5, n_el - 3, 2 * eb + 1, n_el,
              4 * eb - 30]
    counts = [40, 17, 25, 0, 17, 3, 64, 0, 61]
    return starts, counts


def want(name: str, out_dtype: str, starts, counts, row, col, n_rows,
         row_elems, pad):
    """The expected three arrays by slicing the original data, one sample
    after the other; labels by counting."""
    arr = elements(name)
    tokens = np.full((n_rows, row_elems), pad, dtype=out_dtype)
    seg = np.zeros((n_rows, row_elems), dtype=np.int32)
    pos = np.zeros((n_rows, row_elems), dtype=np.int32)
    for i, (s, c, r, k) in enumerate(zip(starts, counts, row, col)):
        if not c:
            continue
        tokens[r, k:k + c] = arr[s:s + c].astype(out_dtype)
        pos[r, k:k + c] = np.arange(c)
        seg[r, k:k + c] = 1 + sum(
            1 for j in range(len(starts))
            if counts[j] and row[j] == r and col[j] < k)
    return tokens, seg, pos
