"""SYSHARD FILTER_BITSHUFFLE (bit-shuffle filter for float and
narrow-range shards) on the CPU: the numpy reference against a naive
per-bit loop, CPU writer/reader round trips, header and validation
rules (the exclusion of the byte shuffle among them), the
ops.bit_shuffle argument guards (they fire before the device assert),
the device chains against stub ops, and the size orderings the filter
is there for.  The device kernel itself is covered by
tests/test_bitshuffle_gpu (-m gpu)."""
import functools
import os
import struct
import sys
from unittest import mock

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shard_stub_ops import (FilterOps, _check_pair, _disjoint,  # noqa: E402
                            aligned_tensor, patched_ops)

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402
from shipyard_amd.data.storage import ObjectStore  # noqa: E402
from shipyard_amd.ops import gf2  # noqa: E402

ELEMS = (2, 4, 8)
BLOCK = 4096
FLAG = 0x8


def _rand(n, seed):
    return np.random.default_rng(seed).integers(
        0, 256, n, dtype=np.uint8).tobytes()


def _header_flags(packed):
    return struct.unpack_from("<I", packed, 8)[0]


def _naive(data: bytes, block_raw: int, B: int) -> bytes:
    """The format's formula, one element and one bit at a time."""
    out = bytearray(data)
    for lo in range(0, len(data), block_raw):
        raw = data[lo:lo + block_raw]
        n8 = len(raw) // B // 8 * 8
        L = n8 // 8
        flt = bytearray(raw)
        flt[:n8 * B] = bytes(n8 * B)
        for e in range(n8):
            for p in range(8 * B):
                bit = (raw[e * B + p // 8] >> (p % 8)) & 1
                flt[p * L + e // 8] |= bit << (e % 8)
        out[lo:lo + len(raw)] = flt
    return bytes(out)


def _lengths(B):
    return sorted({0, 1, B - 1, 8 * B - 1, 8 * B, 8 * B + 1, 4096,
                   4096 + 8 * B * 3 + B + 1, 2 * 4096 + 4095})


# ------------------------------------------------------------- reference
@pytest.mark.parametrize("B", ELEMS)
def test_reference_matches_naive_loop(B):
    for n in _lengths(B):
        x = _rand(n, seed=100 * B + n)
        got = shardfmt.bitshuffle_blocks_numpy(x, BLOCK, B)
        assert got == _naive(x, BLOCK, B), (B, n)
        assert shardfmt.bitshuffle_blocks_numpy(got, BLOCK, B,
                                                inverse=True) == x, (B, n)


def test_reference_by_hand():
    x = np.array([0x0001, 0, 0, 0, 0, 0, 0, 0x8000], dtype="<u2").tobytes()
    want = bytearray(16)
    want[0] = 0x01   # plane 0: bit 0 of element 0 -> bit 0 of byte 0
    want[15] = 0x80  # plane 15: bit 15 of element 7 -> bit 7 of byte 0
    assert shardfmt.bitshuffle_blocks_numpy(x, BLOCK, 2) == bytes(want)
    # 7 elements fill no group of 8: verbatim
    assert shardfmt.bitshuffle_blocks_numpy(x[:14], BLOCK, 2) == x[:14]


def test_reference_rejects_bad_arguments():
    for B in (0, 1, 3, 16):
        with pytest.raises(ValueError, match="elem_size"):
            shardfmt.bitshuffle_blocks_numpy(b"abcd", BLOCK, B)
    with pytest.raises(ValueError, match="block_raw"):
        shardfmt.bitshuffle_blocks_numpy(b"abcd", 0, 2)


# ------------------------------------------------------------ round trips
@pytest.mark.parametrize("compress", [True, False],
                         ids=["lz4", "stored"])
@pytest.mark.parametrize("D", [0, 8, 2], ids=["nodelta", "delta8", "delta2"])
@pytest.mark.parametrize("B", ELEMS)
def test_pack_round_trip(B, D, compress):
    ramp = (np.arange(3 * 2048, dtype=np.int64) * 37).tobytes()
    for x in (b"", ramp + _rand(4096, seed=B) + b"\x07" * 1001,
              _rand(8 * B - 1, seed=1)):
        packed = shardfmt.pack(x, block_raw=BLOCK, compress=compress,
                               bitshuffle_elem=B, delta_elem=D)
        want = FLAG | B << 24 | (0x4 | D << 16 if D else 0) | \
            (shardfmt.FLAG_LZ4 if compress else 0)
        assert _header_flags(packed) == want
        idx = shardfmt.read_index(packed)
        assert idx.bitshuffle_elem == B and idx.delta_elem == D
        assert idx.shuffle_elem == 0
        assert idx.table["crc"].tolist() == \
            gf2.crc32c_chunks_numpy(x, BLOCK)[:idx.n_blocks]
        if len(x) > BLOCK:
            assert int(idx.table["raw_len"][-1]) % (8 * B)  # ragged
        shardfmt.validate_index(idx, len(packed) - idx.payload_off)
        assert shardfmt.unpack_cpu(packed) == x


def test_payload_holds_the_bit_planes():
    x = _rand(BLOCK + 100, seed=9)
    packed = shardfmt.pack(x, block_raw=BLOCK, compress=False,
                           bitshuffle_elem=4)
    idx = shardfmt.read_index(packed)
    assert shardfmt._stored_contiguous(idx)
    assert packed[idx.payload_off:idx.payload_off + len(x)] == \
        _naive(x, BLOCK, 4)


def test_reader_without_the_flag_fails_its_crc():
    x = _rand(8192 + 100, seed=10)
    packed = bytearray(shardfmt.pack(x, compress=False, bitshuffle_elem=4))
    struct.pack_into("<I", packed, 8, 0)
    with pytest.raises(ValueError, match="CRC mismatch"):
        shardfmt.unpack_cpu(bytes(packed))


def test_pack_file_and_object_store(tmp_path):
    x = np.random.default_rng(2).normal(0, 0.02, 5000).astype(
        np.float32).tobytes() + b"\x01\x02\x03"
    (tmp_path / "in.bin").write_bytes(x)
    idx = shardfmt.pack_file(tmp_path / "in.bin", tmp_path / "out.syshard",
                             bitshuffle_elem=4, delta_elem=4)
    assert (idx.bitshuffle_elem, idx.delta_elem) == (4, 4)
    assert shardfmt.unpack_cpu((tmp_path / "out.syshard").read_bytes()) == x
    store = ObjectStore(tmp_path / "store")
    p = store.upload_bytes("w/a.bin", x, pack=True, bitshuffle_elem=4)
    assert shardfmt.read_index(p.read_bytes()).bitshuffle_elem == 4
    assert store.download_bytes("w/a.bin") == x
    p2 = store.upload_file(tmp_path / "in.bin", "w/b.bin", pack=True,
                           bitshuffle_elem=2, delta_elem=8)
    idx2 = shardfmt.read_index(p2.read_bytes())
    assert (idx2.bitshuffle_elem, idx2.delta_elem) == (2, 8)
    assert store.download_bytes("w/b.bin") == x
    with pytest.raises(ValueError, match="bitshuffle_elem.*shuffle_elem"):
        store.upload_bytes("w/c.bin", x, pack=True, bitshuffle_elem=4,
                           shuffle_elem=4)


# ------------------------------------------------------ flags, validation
@pytest.mark.parametrize("B", [0, 1, 3, 16])
def test_read_index_rejects_bad_elem(B):
    packed = bytearray(shardfmt.pack(b"x" * 100, bitshuffle_elem=2))
    struct.pack_into("<I", packed, 8, FLAG | B << 24)
    with pytest.raises(ValueError, match="FILTER_BITSHUFFLE"):
        shardfmt.read_index(bytes(packed))


def test_elem_bits_ignored_without_the_flag():
    x = b"x" * 100
    packed = bytearray(shardfmt.pack(x, compress=False))
    struct.pack_into("<I", packed, 8, 0x7F << 24)
    idx = shardfmt.read_index(bytes(packed))
    assert idx.bitshuffle_elem == 0
    assert shardfmt.unpack_cpu(bytes(packed)) == x


def test_validate_index_enforces_elem():
    packed = shardfmt.pack(_rand(2 * BLOCK, seed=3), block_raw=BLOCK,
                           bitshuffle_elem=4)
    idx = shardfmt.read_index(packed)
    n = len(packed) - idx.payload_off
    shardfmt.validate_index(idx, n)
    for B in (1, 3, 16, -2):
        idx.bitshuffle_elem = B
        with pytest.raises(ValueError, match="bitshuffle_elem"):
            shardfmt.validate_index(idx, n)


def test_writers_reject_bad_elem(tmp_path):
    (tmp_path / "in.bin").write_bytes(b"abcd")
    for B in (1, 3, 16, -2):
        with pytest.raises(ValueError, match="bitshuffle_elem"):
            shardfmt.pack(b"abcd", bitshuffle_elem=B)
        with pytest.raises(ValueError, match="bitshuffle_elem"):
            shardfmt.pack_gpu(b"abcd", bitshuffle_elem=B)
        with pytest.raises(ValueError, match="bitshuffle_elem"):
            shardfmt.pack_auto(b"abcd", bitshuffle_elem=B)
        with pytest.raises(ValueError, match="bitshuffle_elem"):
            shardfmt.pack_file(tmp_path / "in.bin", tmp_path / "o",
                               bitshuffle_elem=B)


def test_both_shuffles_are_rejected_everywhere(tmp_path):
    both = "bitshuffle_elem.*shuffle_elem"
    (tmp_path / "in.bin").write_bytes(b"abcd")
    kw = dict(bitshuffle_elem=4, shuffle_elem=2)
    with pytest.raises(ValueError, match=both):
        shardfmt.pack(b"abcd", **kw)
    with pytest.raises(ValueError, match=both):
        shardfmt.pack_gpu(b"abcd", **kw)
    with pytest.raises(ValueError, match=both):
        shardfmt.pack_auto(b"abcd", **kw)
    with pytest.raises(ValueError, match=both):
        shardfmt.pack_file(tmp_path / "in.bin", tmp_path / "o", **kw)
    assert not (tmp_path / "o").exists()
    # an index that names both
    packed = shardfmt.pack(_rand(BLOCK, seed=4), block_raw=BLOCK,
                           bitshuffle_elem=4)
    idx = shardfmt.read_index(packed)
    idx.shuffle_elem = 2
    with pytest.raises(ValueError, match=both):
        shardfmt.validate_index(idx, len(packed) - idx.payload_off)
    idx2 = shardfmt.ShardIndex(BLOCK, 0, 0, bitshuffle_elem=2,
                               shuffle_elem=2)
    with pytest.raises(ValueError, match=both):
        shardfmt.validate_index(idx2, 0)
    # a header with bits 1 and 3
    bad = bytearray(packed)
    struct.pack_into("<I", bad, 8, FLAG | 4 << 24 | 0x2 | 2 << 8)
    with pytest.raises(ValueError, match=both):
        shardfmt.read_index(bytes(bad))
    with pytest.raises(ValueError, match=both):
        shardfmt.parse_header(bytes(bad))


def test_unfiltered_output_unchanged():
    x = _rand(3 * 8192 + 77, seed=5) + bytes(5000)
    for kw in ({}, {"compress": False}, {"shuffle_elem": 4},
               {"delta_elem": 8, "shuffle_elem": 8}):
        assert shardfmt.pack(x, **kw) == \
            shardfmt.pack(x, bitshuffle_elem=0, **kw)
        assert _header_flags(shardfmt.pack(x, **kw)) & (FLAG | 0xFF << 24) \
            == 0
    idx = shardfmt.ShardIndex(4096, 0, 0)
    assert idx.bitshuffle_elem == 0
    assert shardfmt.read_index(shardfmt.pack(x)).bitshuffle_elem == 0


def test_chains_take_a_dict_without_the_key():
    x = _rand(2 * BLOCK + 99, seed=6)
    old = {"delta_elem": 8, "shuffle_elem": 4}
    want = shardfmt.shuffle_blocks_numpy(
        shardfmt.delta_blocks_numpy(x, BLOCK, 8), BLOCK, 4)
    assert shardfmt.filter_chain_numpy(x, BLOCK, old) == want
    assert shardfmt.filter_chain_numpy(want, BLOCK, old, inverse=True) == x
    assert shardfmt.filter_chain_numpy(x, BLOCK, {}) == x
    assert shardfmt.filter_flags(old) == 0x4 | 8 << 16 | 0x2 | 4 << 8
    only = {"bitshuffle_elem": 2}
    assert shardfmt.filter_chain_numpy(x, BLOCK, only) == \
        shardfmt.bitshuffle_blocks_numpy(x, BLOCK, 2)


# ------------------------------------------------ device chains, stub ops
class BitFilterOps(FilterOps):
    """FilterOps plus a strict stand-in for ops.bit_shuffle."""

    def bit_shuffle(self, src, dst, block_raw, elem_size, inverse=False):
        _check_pair(src, dst, block_raw, elem_size)
        assert _disjoint(src, dst), "bit_shuffle cannot alias"
        self.calls.append(("bitshuffle", src.numel()))
        out = shardfmt.bitshuffle_blocks_numpy(
            bytes(src.numpy().tobytes()), block_raw, elem_size, inverse)
        dst.copy_(torch.frombuffer(bytearray(out), dtype=torch.uint8))


def _patched(fake):
    stack = patched_ops(fake)
    stack.enter_context(mock.patch("shipyard_amd.ops.bit_shuffle",
                                   fake.bit_shuffle, create=True))
    return stack


def _bytes(t) -> bytes:
    return bytes(t.numpy().tobytes())


def _apart(a, b) -> bool:
    return a.data_ptr() + a.numel() <= b.data_ptr() or \
        b.data_ptr() + b.numel() <= a.data_ptr()


CHAIN_CASES = [
    (0, 4, ["bitshuffle"], ["bitshuffle"]),
    (8, 8, ["delta", "bitshuffle"], ["bitshuffle", "delta-inplace"]),
]


@pytest.mark.parametrize("D,B,wrote,unwound", CHAIN_CASES,
                         ids=["bitshuffle4", "delta8+bitshuffle8"])
def test_device_chains(D, B, wrote, unwound):
    n = 2 * BLOCK + 1001
    x = _rand(n, seed=16 * D + B)
    elems = {"delta_elem": D, "bitshuffle_elem": B}
    t = aligned_tensor(x)

    fake = BitFilterOps()
    with _patched(fake):
        flt = shardfmt.filter_chain_device(t, BLOCK, elems)
    assert [k for k, _ in fake.calls] == wrote
    assert all(m == n for _, m in fake.calls)
    assert _bytes(t) == x and _apart(t, flt)  # the input is left alone
    want = shardfmt.filter_chain_numpy(x, BLOCK, elems)
    assert want != x and _bytes(flt) == want

    # reader, borrowed payload: never written
    fake = BitFilterOps()
    with _patched(fake):
        out = shardfmt.unfilter_chain_device(flt, BLOCK, elems,
                                             borrowed=True)
    assert [k for k, _ in fake.calls] == unwound
    assert _bytes(out) == x
    assert _bytes(flt) == want and _apart(flt, out)

    # reader, a tensor it owns: un-bitshuffle into a new tensor, then
    # un-delta in place on that one
    fake = BitFilterOps()
    with _patched(fake):
        out = shardfmt.unfilter_chain_device(flt, BLOCK, elems,
                                             borrowed=False)
    assert [k for k, _ in fake.calls] == unwound
    assert _bytes(out) == x and _apart(flt, out)


@pytest.mark.parametrize("compress", [True, False], ids=["lz4", "stored"])
def test_decode_device_orchestration(compress):
    x = (np.arange(2 * 1024, dtype=np.int64) * 40).tobytes() + \
        _rand(8192, seed=7) + b"\x05" * 1001
    packed = shardfmt.pack(x, block_raw=8192, compress=compress,
                           bitshuffle_elem=8, delta_elem=8)
    idx = shardfmt.read_index(packed)
    fake = BitFilterOps()
    with _patched(fake):
        d_comp = aligned_tensor(packed[idx.payload_off:])
        before = _bytes(d_comp)
        out = shardfmt.decode_device(d_comp, idx, torch.device("cpu"))
    assert _bytes(out) == x
    assert _bytes(d_comp) == before and _apart(d_comp, out)
    kinds = [k for k, _ in fake.calls]
    assert kinds[-3:] == ["bitshuffle", "delta-inplace", "crc"]
    if compress:
        return
    # stored-contiguous path: straight from the payload
    assert kinds == ["bitshuffle", "delta-inplace", "crc"]
    bad = bytearray(packed)
    bad[idx.payload_off + 3] ^= 0x40
    with _patched(BitFilterOps()):
        with pytest.raises(ValueError, match="CRC mismatch"):
            shardfmt.decode_device(
                aligned_tensor(bytes(bad[idx.payload_off:])), idx,
                torch.device("cpu"))


def test_stager_parses_the_flag(tmp_path):
    """The stager reads headers through shardfmt's parser: a bitshuffled
    file's index carries the element size, and a header with both
    shuffles is refused there too."""
    x = _rand(8192 + 5, seed=8)
    p = tmp_path / "w.syshard"
    p.write_bytes(shardfmt.pack(x, bitshuffle_elem=2))
    hdr = shardfmt.parse_header(p.read_bytes())
    assert hdr.elems == {"delta_elem": 0, "bitshuffle_elem": 2,
                         "shuffle_elem": 0}
    idx = shardfmt.index_from_table(hdr, p.read_bytes(),
                                    shardfmt.HEADER.size)
    assert idx.bitshuffle_elem == 2
    bad = bytearray(p.read_bytes())
    struct.pack_into("<I", bad, 8, FLAG | 2 << 24 | 0x2 | 2 << 8)
    p.write_bytes(bytes(bad))
    # stage_file parses the header before it touches a device
    st = ShardStager.__new__(ShardStager)
    st.torch = torch
    with pytest.raises(ValueError, match="bitshuffle_elem.*shuffle_elem"):
        st.stage_file(p)


# ------------------------------------------------------- ops guards, no GPU
def test_bit_shuffle_guards_fire_without_a_device():
    buf = torch.zeros(2 * 8192 + 64, dtype=torch.uint8)
    base = (-buf.data_ptr()) % 16
    src = buf[base:base + 4096]
    dst = buf[base + 8192:base + 8192 + 4096]
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.bit_shuffle(buf[base + 1:base + 1 + 4096], dst, 4096, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.bit_shuffle(src, buf[base + 8200:base + 8200 + 4096], 4096, 4)
    with pytest.raises(ValueError, match="bytes but dst"):
        ops.bit_shuffle(src, buf[base + 8192:base + 8192 + 4080], 4096, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.bit_shuffle(src, buf[base + 16:base + 16 + 4096], 4096, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.bit_shuffle(src, src, 4096, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.bit_shuffle(src, src, 4096, 4, inverse=True)
    for B in (0, 1, 3, 16):
        with pytest.raises(ValueError, match="elem_size"):
            ops.bit_shuffle(src, dst, 4096, B)
    for blk in (0, -4096, 100, 4097, 6144, 1 << 32):
        with pytest.raises(ValueError, match="block_raw"):
            ops.bit_shuffle(src, dst, blk, 4)
    assert not buf.any()  # nothing ran


# ------------------------------------------------------------ size benefit
@functools.lru_cache(maxsize=None)
def _bf16_weights() -> bytes:
    w = np.random.default_rng(0).normal(0, 0.02, 65536).astype(np.float32)
    return (w.view(np.uint32) >> 16).astype("<u2").tobytes()


@functools.lru_cache(maxsize=None)
def _offsets() -> bytes:
    return np.cumsum(np.random.default_rng(1).poisson(40, 32768)).astype(
        "<i8").tobytes()


@functools.lru_cache(maxsize=None)
def _zipf_tokens() -> bytes:
    z = np.random.default_rng(0).zipf(1.2, 32768)
    return (np.minimum(z, 50257) - 1).astype("<i4").tobytes()


@pytest.fixture(params=["native-cxx", "python"])
def matcher(request, monkeypatch):
    """Both block matchers pack(): the native one when the ops library
    is built, and the pure-python one it falls back to."""
    if request.param == "python":
        def no_native(*a, **k):
            raise RuntimeError("native matcher switched off")
        monkeypatch.setattr(ops, "lz4_compress_blocks", no_native)
    return request.param


def test_size_benefit_on_bf16_weights(matcher):
    """Measured, bytes (fraction of the 131072 raw) at 8 KiB blocks,
    native / python matcher: plain 131420 (1.003), shuffle 2 117772 /
    118252 (0.899 / 0.902), bitshuffle 2 99916 / 99980 (0.762 / 0.763);
    docs/35-gpu-data-plane.md."""
    x = _bf16_weights()
    plain = len(shardfmt.pack(x))
    shuf = len(shardfmt.pack(x, shuffle_elem=2))
    bits = shardfmt.pack(x, bitshuffle_elem=2)
    print(f"bf16 weights [{matcher}]: raw {len(x)} plain {plain} "
          f"shuffle {shuf} bitshuffle {len(bits)}")
    assert len(bits) < shuf < plain
    assert shardfmt.unpack_cpu(bits) == x


def test_size_benefit_on_delta_coded_offsets(matcher):
    """Measured, bytes (fraction of the 262144 raw) at 8 KiB blocks,
    native / python matcher: delta 8 + shuffle 8 35340 (0.135), delta 8
    + bitshuffle 8 27468 / 27644 (0.105); docs/35-gpu-data-plane.md."""
    x = _offsets()
    shuf = len(shardfmt.pack(x, delta_elem=8, shuffle_elem=8))
    bits = shardfmt.pack(x, delta_elem=8, bitshuffle_elem=8)
    print(f"offsets [{matcher}]: raw {len(x)} delta+shuffle {shuf} "
          f"delta+bitshuffle {len(bits)}")
    assert len(bits) < shuf
    assert shardfmt.unpack_cpu(bits) == x


def test_skewed_token_ids_are_no_better_bitshuffled(matcher):
    """Why the filter is opt-in: Zipf(1.2) int32 token ids.  Measured,
    bytes (fraction of the 131072 raw) at 8 KiB blocks, native / python
    matcher: shuffle 4 55980 / 56380 (0.427 / 0.430), bitshuffle 4
    59276 / 59548 (0.452 / 0.454)."""
    x = _zipf_tokens()
    shuf = len(shardfmt.pack(x, shuffle_elem=4))
    bits = len(shardfmt.pack(x, bitshuffle_elem=4))
    print(f"zipf tokens [{matcher}]: raw {len(x)} shuffle {shuf} "
          f"bitshuffle {bits}")
    assert bits >= shuf
