"""SYSHARD FILTER_SHUFFLE (byte-shuffle filter for typed shards) on the
CPU: format pin, CPU writer/reader round trips, header rules, the numpy
reference, the ops.byte_shuffle argument guards (they fire before the
device assert) and the decode_device orchestration against stub ops.
The device kernel itself is covered by tests/test_shuffle_gpu (-m gpu)."""
import os
import struct
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shard_stub_ops import FilterOps, decode_packed  # noqa: E402

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.storage import ObjectStore  # noqa: E402
from shipyard_amd.ops import gf2  # noqa: E402

ELEMS = (2, 4, 8)
BLOCKS = (4096, 8192)


def _lengths(E, B):
    return sorted({0, 1, E - 1, E, E + 1, 4095, 4096, 4097,
                   2 * B + 3 * E + 1})


def _bytes(n, seed):
    """Half-compressible content: a typed ramp xor a little noise."""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(n, dtype=np.uint32) // 3).astype(np.uint8)
    noise = rng.integers(0, 4, n, dtype=np.uint8)
    return (ramp ^ noise).tobytes()


def _header_flags(packed):
    return struct.unpack_from("<I", packed, 8)[0]


def test_format_pin():
    raw = bytes(range(16)) + b"xyz"
    packed = shardfmt.pack(raw, block_raw=4096, compress=False,
                           shuffle_elem=4)
    assert _header_flags(packed) == 0x402
    idx = shardfmt.read_index(packed)
    assert idx.shuffle_elem == 4 and idx.n_blocks == 1
    want = bytes.fromhex("0004080c 0105090d 02060a0e 03070b0f 78797a")
    assert packed[idx.payload_off:idx.payload_off + 19] == want
    assert int(idx.table["crc"][0]) == gf2.crc32c(raw)
    assert shardfmt.unpack_cpu(packed) == raw


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("E", ELEMS)
def test_round_trip(E, B, compress):
    for n in _lengths(E, B):
        x = _bytes(n, seed=n + E)
        packed = shardfmt.pack(x, block_raw=B, compress=compress,
                               shuffle_elem=E)
        assert _header_flags(packed) == (0x2 | (E << 8) | int(compress))
        assert shardfmt.read_index(packed).shuffle_elem == E
        assert shardfmt.unpack_cpu(packed) == x, (E, B, n, compress)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("E", ELEMS)
def test_reference_inverse_and_layout(E, B):
    for n in _lengths(E, B):
        x = _bytes(n, seed=7 * n + E)
        f = shardfmt.shuffle_blocks_numpy(x, B, E)
        assert len(f) == n
        assert shardfmt.shuffle_blocks_numpy(f, B, E, inverse=True) == x
        # the definition, element by element, on every block
        for lo in range(0, n, B):
            raw, flt = x[lo:lo + B], f[lo:lo + B]
            n_el = len(raw) // E
            body = n_el * E
            for j in range(E):
                assert flt[j * n_el:(j + 1) * n_el] == raw[j:body:E]
            assert flt[body:] == raw[body:]


@pytest.mark.parametrize("E", [0, 1, 3, 16])
def test_header_rejects_bad_elem(E):
    hdr = shardfmt.HEADER.pack(shardfmt.MAGIC, 0x3 | (E << 8), 4096, 0, 0)
    with pytest.raises(ValueError, match="FILTER_SHUFFLE"):
        shardfmt.read_index(hdr)


def test_validate_index_enforces_elem():
    for E in (1, 3, 16):
        idx = shardfmt.ShardIndex(block_raw=4096, raw_size=0,
                                  payload_off=0, shuffle_elem=E)
        with pytest.raises(ValueError, match="shuffle_elem"):
            shardfmt.validate_index(idx, 0)
    for E in (0, 2, 4, 8):
        shardfmt.validate_index(
            shardfmt.ShardIndex(block_raw=4096, raw_size=0, payload_off=0,
                                shuffle_elem=E), 0)


def test_writers_reject_bad_elem():
    for fn in (shardfmt.pack, shardfmt.pack_auto):
        with pytest.raises(ValueError, match="shuffle_elem"):
            fn(b"abcd" * 10, shuffle_elem=3)
    # pack_gpu checks its arguments before it touches a device
    with pytest.raises(ValueError, match="shuffle_elem"):
        shardfmt.pack_gpu(b"abcd" * 10, shuffle_elem=16)


def test_unfiltered_path_unchanged():
    for flags in (0, 1):
        hdr = shardfmt.HEADER.pack(shardfmt.MAGIC, flags, 4096, 0, 0)
        assert shardfmt.read_index(hdr).shuffle_elem == 0
    # element-size bits without bit 1 are unknown bits: ignored
    hdr = shardfmt.HEADER.pack(shardfmt.MAGIC, 1 | (3 << 8), 4096, 0, 0)
    assert shardfmt.read_index(hdr).shuffle_elem == 0
    x = _bytes(3 * 8192 + 5, seed=5) + os.urandom(9000)
    for compress in (True, False):
        plain = shardfmt.pack(x, compress=compress)
        assert plain == shardfmt.pack(x, compress=compress, shuffle_elem=0)
        assert _header_flags(plain) == int(compress)
        assert shardfmt.read_index(plain).shuffle_elem == 0
        assert shardfmt.unpack_cpu(plain) == x
    # positional construction as before the keyword existed
    assert shardfmt.ShardIndex(4096, 0, 0).shuffle_elem == 0


def test_size_benefit_on_token_ids():
    """int32 token ids: the high bytes are zero planes after the filter.
    The bound holds against whichever writer pack() picks: python
    packer 65180 -> 33340 (0.512), native CPU packer 65404 -> 33340
    (0.510)."""
    x = np.random.default_rng(1234).integers(0, 50257, 16384).astype(
        np.int32).tobytes()
    plain = len(shardfmt.pack(x))
    filt = shardfmt.pack(x, shuffle_elem=4)
    print(f"token shard: plain {plain} filtered {len(filt)} "
          f"ratio {len(filt) / plain:.3f}")
    assert len(filt) < 0.6 * plain
    assert shardfmt.unpack_cpu(filt) == x


def test_crc_protects_filtered_shard():
    x = _bytes(3 * 8192 + 77, seed=9)
    for compress in (True, False):
        packed = bytearray(shardfmt.pack(x, compress=compress,
                                         shuffle_elem=4))
        idx = shardfmt.read_index(bytes(packed))
        packed[idx.payload_off + 8] ^= 0x55
        with pytest.raises(ValueError, match="CRC mismatch"):
            shardfmt.unpack_cpu(bytes(packed))


def test_reader_without_the_flag_fails_its_crc():
    """Clearing the filter bits is what an old reader effectively sees:
    it must fail loudly, not return transposed data."""
    x = _bytes(8192 + 100, seed=10)
    packed = bytearray(shardfmt.pack(x, compress=False, shuffle_elem=4))
    struct.pack_into("<I", packed, 8, 0)
    with pytest.raises(ValueError, match="CRC mismatch"):
        shardfmt.unpack_cpu(bytes(packed))


def test_byte_shuffle_guards_fire_without_a_device():
    buf = torch.zeros(2 * 8192 + 64, dtype=torch.uint8)
    base = (-buf.data_ptr()) % 16
    src = buf[base:base + 4096]
    dst = buf[base + 8192:base + 8192 + 4096]
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.byte_shuffle(buf[base + 1:base + 1 + 4096], dst, 4096, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.byte_shuffle(src, buf[base + 8200:base + 8200 + 4096], 4096, 4)
    with pytest.raises(ValueError, match="bytes but dst"):
        ops.byte_shuffle(src, buf[base + 8192:base + 8192 + 4080], 4096, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.byte_shuffle(src, buf[base + 16:base + 16 + 4096], 4096, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.byte_shuffle(src, src, 4096, 4)
    for E in (0, 1, 3, 16):
        with pytest.raises(ValueError, match="elem_size"):
            ops.byte_shuffle(src, dst, 4096, E)
    for B in (0, -4096, 100, 4097, 6144, 1 << 32):
        with pytest.raises(ValueError, match="block_raw"):
            ops.byte_shuffle(src, dst, B, 4)
    assert not buf.any()  # nothing ran


@pytest.mark.parametrize("compress", [True, False])
def test_decode_device_orchestration(compress):
    """Host side of the GPU reader: one unshuffle launch after decode,
    CRC over the unshuffled bytes, no aliasing of the payload."""
    x = _bytes(2 * 8192, seed=3) + os.urandom(8192) + _bytes(1001, seed=4)
    packed = shardfmt.pack(x, block_raw=8192, compress=compress,
                           shuffle_elem=4)
    fake = FilterOps()
    out, d_comp = decode_packed(packed, fake)
    assert bytes(out.numpy().tobytes()) == x
    kinds = [k for k, _ in fake.calls]
    assert kinds.count("shuffle") == 1
    assert kinds.index("shuffle") < kinds.index("crc")
    if not compress:  # stored-contiguous path: straight from the payload
        assert kinds == ["shuffle", "crc"]
        lo, hi = d_comp.data_ptr(), d_comp.data_ptr() + d_comp.numel()
        assert not lo <= out.data_ptr() < hi

    bad = bytearray(packed)
    bad[shardfmt.read_index(packed).payload_off + 3] ^= 0x40
    with pytest.raises(ValueError, match="CRC mismatch"):
        decode_packed(bytes(bad), FilterOps())


def test_object_store_round_trip(tmp_path):
    store = ObjectStore(tmp_path / "store")
    x = np.random.default_rng(2).integers(0, 50257, 5000).astype(
        np.int32).tobytes() + b"\x01\x02\x03"
    p = store.upload_bytes("tokens/a.bin", x, pack=True, shuffle_elem=4)
    assert shardfmt.read_index(p.read_bytes()).shuffle_elem == 4
    assert store.download_bytes("tokens/a.bin") == x
    src = tmp_path / "local.bin"
    src.write_bytes(x)
    p2 = store.upload_file(src, "tokens/b.bin", pack=True, shuffle_elem=2)
    assert shardfmt.read_index(p2.read_bytes()).shuffle_elem == 2
    assert store.download_bytes("tokens/b.bin") == x


def test_pack_file_forwards_the_filter(tmp_path):
    x = _bytes(8192 + 3, seed=6)
    (tmp_path / "in.bin").write_bytes(x)
    idx = shardfmt.pack_file(tmp_path / "in.bin", tmp_path / "out.syshard",
                             shuffle_elem=8)
    assert idx.shuffle_elem == 8
    assert shardfmt.unpack_cpu((tmp_path / "out.syshard").read_bytes()) == x
