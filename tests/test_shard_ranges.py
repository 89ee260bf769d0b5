"""CPU tests of the SYSHARD range reader: ShardIndex.select_blocks
against a brute-force loop, and read_ranges_cpu against slices of the
original bytes on every filter combination, with only the touched blocks
decoded and verified.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from shipyard_amd.data import shardfmt

BLOCK = 4096
N_RAW = 4 * BLOCK + 1000  # 5 blocks, the last one 1000 bytes

# (delta_elem, bitshuffle_elem, shuffle_elem): everything the writers take
FILTERS = [(0, 0, 0)] + \
    [(0, 0, e) for e in (2, 4, 8)] + \
    [(e, 0, 0) for e in (2, 4, 8)] + \
    [(0, e, 0) for e in (2, 4, 8)] + \
    [(8, 0, 8), (4, 0, 2), (2, 0, 4)] + \
    [(8, 8, 0), (4, 2, 0), (2, 4, 0)]


def _ids(f):
    return "d%d-b%d-s%d" % f


@functools.lru_cache(maxsize=None)
def _raw() -> bytes:
    """Slowly rising int32 values: compressible under every filter."""
    rng = np.random.default_rng(7)
    vals = np.cumsum(rng.integers(0, 5, N_RAW // 4 + 1)).astype("<u4")
    return vals.tobytes()[:N_RAW]


@functools.lru_cache(maxsize=None)
def _index() -> shardfmt.ShardIndex:
    idx = shardfmt.read_index(shardfmt.pack(_raw(), block_raw=BLOCK))
    assert idx.n_blocks == 5 and int(idx.table["raw_len"][-1]) == 1000
    return idx


def _brute(offs, lens):
    hit = set()
    for o, n in zip(offs, lens):
        for byte in range(o, o + n):
            hit.add(byte // BLOCK)
    return sorted(hit)


def _random_ranges(n, seed):
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, N_RAW + 1, n)
    lens = np.minimum(rng.integers(0, 3 * BLOCK, n), N_RAW - offs)
    return offs.tolist(), lens.tolist()


RANGE_CASES = {
    "empty-list": ([], []),
    "length-0": ([5000], [0]),
    "one-byte": ([5000], [1]),
    "inside-one-block": ([BLOCK + 10], [100]),
    "ends-at-block-edge": ([BLOCK + 10], [BLOCK - 10]),
    "starts-at-block-edge": ([2 * BLOCK], [17]),
    "spans-three-blocks": ([BLOCK - 1], [BLOCK + 2]),
    "reaches-raw-size": ([N_RAW - 5], [5]),
    "length-0-at-raw-size": ([N_RAW], [0]),
    "duplicates-and-overlaps": ([100, 100, 150, 3 * BLOCK - 1, 100],
                                [200, 200, 4000, 2, 200]),
    "unsorted": ([4 * BLOCK + 1, 0, 2 * BLOCK + 5], [3, 1, 10]),
    "random-1000": _random_ranges(1000, seed=11),
    "random-1000-short": (
        np.random.default_rng(12).integers(0, N_RAW - 8, 1000).tolist(),
        np.random.default_rng(13).integers(0, 9, 1000).tolist()),
}


@pytest.mark.parametrize("case", list(RANGE_CASES))
def test_select_blocks_matches_brute_force(case):
    offs, lens = RANGE_CASES[case]
    got = _index().select_blocks(offs, lens)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    assert got.tolist() == _brute(offs, lens)


def test_select_blocks_takes_numpy_arrays():
    offs, lens = RANGE_CASES["random-1000"]
    got = _index().select_blocks(np.asarray(offs), np.asarray(lens))
    assert got.tolist() == _brute(offs, lens)


@pytest.mark.parametrize("offs,lens", [
    ([-1], [4]),
    ([4], [-1]),
    ([N_RAW - 3], [4]),        # off + len == raw_size + 1
    ([0], [N_RAW + 1]),
    ([N_RAW + 1], [0]),
    ([0, 10], [5]),            # unequal lengths
], ids=["neg-off", "neg-len", "one-past", "too-long", "off-past", "uneven"])
def test_select_blocks_rejects(offs, lens):
    with pytest.raises(ValueError):
        _index().select_blocks(offs, lens)


def _want(raw, offs, lens):
    return b"".join(raw[o:o + n] for o, n in zip(offs, lens))


READ_RANGES = (
    [0, N_RAW - 1, BLOCK - 3, 4 * BLOCK - 7, 2 * BLOCK, 777, 777, N_RAW],
    [1, 1, 6, 1007, BLOCK, 0, 2 * BLOCK + 5, 0])


@pytest.mark.parametrize("compress", [True, False],
                         ids=["lz4", "stored"])
@pytest.mark.parametrize("filt", FILTERS, ids=_ids)
def test_read_ranges_cpu_equals_slices(filt, compress):
    raw = _raw()
    D, B, S = filt
    packed = shardfmt.pack(raw, block_raw=BLOCK, compress=compress,
                           delta_elem=D, bitshuffle_elem=B, shuffle_elem=S)
    idx = shardfmt.read_index(packed)
    stored = idx.table["comp_len"] == idx.table["raw_len"]
    assert stored.all() if not compress else not stored.all()
    offs, lens = READ_RANGES
    assert shardfmt.read_ranges_cpu(packed, offs, lens) == \
        _want(raw, offs, lens)
    offs, lens = _random_ranges(40, seed=D + 10 * B + 100 * S)
    for verify in (True, False):
        assert shardfmt.read_ranges_cpu(packed, offs, lens,
                                        verify=verify) == \
            _want(raw, offs, lens)
    assert shardfmt.read_ranges_cpu(packed, [], []) == b""
    assert shardfmt.read_ranges_cpu(packed, [N_RAW], [0]) == b""
    assert shardfmt.read_ranges_cpu(packed, [0], [N_RAW]) == raw


def test_read_ranges_cpu_rejects_bad_ranges():
    packed = shardfmt.pack(_raw(), block_raw=BLOCK)
    for offs, lens in (([-1], [1]), ([0], [-1]), ([N_RAW - 3], [4])):
        with pytest.raises(ValueError):
            shardfmt.read_ranges_cpu(packed, offs, lens)


def _flip(packed: bytes, block: int, at: int = 8) -> bytes:
    idx = shardfmt.read_index(packed)
    buf = bytearray(packed)
    buf[idx.payload_off + int(idx.table["comp_off"][block]) + at] ^= 0x55
    return bytes(buf)


@pytest.mark.parametrize("filt", [(0, 0, 0), (4, 0, 4), (0, 4, 0)],
                         ids=_ids)
def test_stored_block_corruption(filt):
    raw = _raw()
    D, B, S = filt
    packed = shardfmt.pack(raw, block_raw=BLOCK, compress=False,
                           delta_elem=D, bitshuffle_elem=B, shuffle_elem=S)
    offs, lens = [BLOCK + 5, 3 * BLOCK - 2], [100, 4]  # blocks 1, 2, 3
    assert _index().select_blocks(offs, lens).tolist() == [1, 2, 3]
    for blk in (1, 2, 3):
        with pytest.raises(ValueError, match="CRC mismatch"):
            shardfmt.read_ranges_cpu(_flip(packed, blk), offs, lens)
    # the message names the shard's block id, not the compact slot
    with pytest.raises(ValueError, match=r"\[3\]"):
        shardfmt.read_ranges_cpu(_flip(packed, 3), offs, lens)
    for blk in (0, 4):
        bad = _flip(packed, blk)
        assert shardfmt.read_ranges_cpu(bad, offs, lens) == \
            _want(raw, offs, lens)
        with pytest.raises(ValueError):
            shardfmt.unpack_cpu(bad)
    # verify=False returns the corrupt bytes without complaint
    got = shardfmt.read_ranges_cpu(_flip(packed, 1), offs, lens,
                                   verify=False)
    assert len(got) == sum(lens)


def test_only_touched_blocks_are_decoded():
    """A shard of LZ4 blocks only: a flipped byte in a block that no
    range touches does not disturb the range read, while the whole-shard
    reader trips over it (in the decoder or at the CRC)."""
    raw = _raw()
    packed = shardfmt.pack(raw, block_raw=BLOCK, compress=True)
    idx = shardfmt.read_index(packed)
    assert (idx.table["comp_len"] < idx.table["raw_len"]).all()
    offs, lens = [10, 4 * BLOCK + 3], [BLOCK, 50]  # blocks 0, 1 and 4
    for blk in (2, 3):
        bad = _flip(packed, blk)
        assert shardfmt.read_ranges_cpu(bad, offs, lens) == \
            _want(raw, offs, lens)
        with pytest.raises(ValueError):
            shardfmt.unpack_cpu(bad)
    with pytest.raises(ValueError):
        shardfmt.read_ranges_cpu(_flip(packed, 4), offs, lens)
