"""GPU tests of the SYSHARD byte-shuffle filter: the ops.byte_shuffle
kernel against shardfmt.shuffle_blocks_numpy byte for byte, and the
filtered shard through every GPU path above it (unpack_gpu, pack_gpu,
the stager).  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from shipyard_amd import ops  # noqa: E402
from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402

pytestmark = pytest.mark.gpu

ELEMS = (2, 4, 8)
CANARY = 0xA5
PAD = 128  # dst sits at this (16 B aligned) offset inside its canary buffer


def _cuda(raw: bytes):
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda:0")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")


def _host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(
        0, 256, n, dtype=np.uint8).tobytes()


def _shuffle_in_canary(src, block_raw, E, inverse=False):
    """Run the kernel into an aligned view inside a canary-filled
    buffer; returns the view's bytes after checking that nothing around
    it (at least 64 bytes each side) changed."""
    n = src.numel()
    big = torch.full((n + 2 * PAD,), CANARY, dtype=torch.uint8,
                     device="cuda:0")
    dst = big[PAD:PAD + n]
    assert dst.data_ptr() % 16 == 0
    ops.byte_shuffle(src, dst, block_raw, E, inverse=inverse)
    torch.cuda.current_stream().synchronize()
    host = big.cpu().numpy()
    assert (host[:PAD] == CANARY).all(), "wrote before dst"
    assert (host[PAD + n:] == CANARY).all(), "wrote past dst"
    return host[PAD:PAD + n].tobytes()


def _kernel_lengths(E):
    return sorted({1, E - 1, E, E + 1, 4095, 4096, 4097, 3 * 4096 + 2048,
                   5 * 8192 + 4093})


@pytest.mark.parametrize("block_raw", [4096, 8192])
@pytest.mark.parametrize("E", ELEMS)
def test_kernel_matches_reference(E, block_raw):
    for n in _kernel_lengths(E):
        x = _rand(n, seed=n * 8 + E)
        want = shardfmt.shuffle_blocks_numpy(x, block_raw, E)
        d_x = _cuda(x)
        got = _shuffle_in_canary(d_x, block_raw, E)
        assert got == want, (E, block_raw, n)
        back = _shuffle_in_canary(_cuda(got), block_raw, E, inverse=True)
        assert back == x, (E, block_raw, n)
        assert _host(d_x) == x  # the source is read-only


@pytest.mark.parametrize("E", ELEMS)
def test_kernel_large_block(E):
    """block_raw above the 64 KiB LZ4 limit (stored-only shards): the
    kernel tiles inside the block."""
    block_raw, n = 131072, 2 * 131072 + 17
    x = _rand(n, seed=E)
    want = shardfmt.shuffle_blocks_numpy(x, block_raw, E)
    got = _shuffle_in_canary(_cuda(x), block_raw, E)
    assert got == want
    assert _shuffle_in_canary(_cuda(got), block_raw, E, inverse=True) == x


def test_kernel_block_not_power_of_two():
    """block_raw = 3 tiles: the tile -> (block, tile-in-block) split is a
    real division, and a 4-tile pass straddles block boundaries."""
    block_raw, n = 12288, 7 * 12288 + 4099
    x = _rand(n, seed=77)
    for E in ELEMS:
        want = shardfmt.shuffle_blocks_numpy(x, block_raw, E)
        got = _shuffle_in_canary(_cuda(x), block_raw, E)
        assert got == want, E
        assert _shuffle_in_canary(_cuda(got), block_raw, E, True) == x, E


def test_kernel_on_non_default_stream():
    E, block_raw, n = 4, 8192, 9 * 8192 + 1234
    x = _rand(n, seed=3)
    d_x = _cuda(x)
    d_y = torch.empty_like(d_x)
    d_z = torch.empty_like(d_x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.byte_shuffle(d_x, d_y, block_raw, E)
        ops.byte_shuffle(d_y, d_z, block_raw, E, inverse=True)
    side.synchronize()
    assert _host(d_y) == shardfmt.shuffle_blocks_numpy(x, block_raw, E)
    assert _host(d_z) == x


def test_kernel_empty_is_a_no_op():
    e = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    ops.byte_shuffle(e, torch.empty_like(e), 4096, 4)
    torch.cuda.synchronize()


def test_kernel_past_4gib():
    """64-bit block offsets and the grid-stride loop: 4 GiB + 2 blocks +
    a ragged tail (more work items than the capped grid).  Blocks are
    independent, so the reference is computed only for sampled blocks
    (both ends, and either side of the 2 GiB and 4 GiB offsets); the
    rest is covered by the full-length device round trip."""
    E, block_raw = 4, 65536
    n = (1 << 32) + 2 * block_raw + 4093
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0",
                      generator=gen)
    y = torch.full_like(x, CANARY)
    ops.byte_shuffle(x, y, block_raw, E)
    n_blocks = (n + block_raw - 1) // block_raw
    picks = [0, 1, (1 << 31) // block_raw - 1, (1 << 31) // block_raw,
             (1 << 32) // block_raw - 1, (1 << 32) // block_raw,
             n_blocks - 2, n_blocks - 1]
    for b in picks:
        lo, hi = b * block_raw, min((b + 1) * block_raw, n)
        want = shardfmt.shuffle_blocks_numpy(_host(x[lo:hi]), block_raw, E)
        assert _host(y[lo:hi]) == want, b
    z = torch.full_like(x, CANARY)
    ops.byte_shuffle(y, z, block_raw, E, inverse=True)
    assert torch.equal(z, x)


# ------------------------------------------------- GPU reader, CPU-authored
@functools.lru_cache(maxsize=None)
def _mixed_case(ragged: bool) -> bytes:
    """Half incompressible, half int32 ramps -> stored and LZ4 blocks;
    ``ragged`` adds a final block of 1001 bytes (no multiple of 2)."""
    rng = np.random.default_rng(21)
    ramp = (np.arange(10 * 2048, dtype=np.int32) * 3 + 7).tobytes()
    tail = rng.integers(0, 7, 1001, dtype=np.uint8).tobytes() if ragged \
        else b""
    return os.urandom(10 * 8192) + ramp + tail


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("E", ELEMS)
def test_unpack_gpu_reads_cpu_authored(E, ragged):
    x = _mixed_case(ragged)
    packed = shardfmt.pack(x, block_raw=8192, shuffle_elem=E)
    idx = shardfmt.read_index(packed)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks  # both block kinds occur
    if ragged:
        assert int(idx.table["raw_len"][-1]) % E
    for verify in (True, False):
        got = shardfmt.unpack_gpu(packed, verify=verify)
        assert got.numel() == len(x)
        assert _host(got) == x, verify


@pytest.mark.parametrize("E", ELEMS)
def test_unpack_gpu_stored_contiguous(E):
    x = _mixed_case(True)
    packed = shardfmt.pack(x, block_raw=8192, compress=False,
                           shuffle_elem=E)
    idx = shardfmt.read_index(packed)
    assert shardfmt._stored_contiguous(idx)
    d_comp = _cuda(packed[idx.payload_off:])
    before = _host(d_comp)
    out = shardfmt.decode_device(d_comp, idx, torch.device("cuda:0"))
    assert _host(out) == x
    # a new tensor, and the payload it came from is untouched
    lo, hi = d_comp.data_ptr(), d_comp.data_ptr() + d_comp.numel()
    assert not lo <= out.data_ptr() < hi
    assert _host(d_comp) == before
    assert _host(shardfmt.unpack_gpu(packed)) == x


def test_unpack_gpu_large_stored_blocks():
    """Stored-only filtered shard at block_raw = 128 KiB."""
    x = _rand(2 * 131072 + 17, seed=8)
    packed = shardfmt.pack(x, block_raw=131072, compress=False,
                           shuffle_elem=8)
    assert _host(shardfmt.unpack_gpu(packed)) == x


# ------------------------------------------------------------ GPU authoring
@functools.lru_cache(maxsize=None)
def _tokens() -> bytes:
    return np.random.default_rng(1234).integers(0, 50257, 16384).astype(
        np.int32).tobytes()


@pytest.mark.parametrize("E", ELEMS)
def test_pack_gpu_round_trips(E):
    x = _mixed_case(True)
    packed = shardfmt.pack_gpu(x, block_raw=8192, shuffle_elem=E)
    idx = shardfmt.read_index(packed)
    assert idx.shuffle_elem == E
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks
    assert shardfmt.unpack_cpu(packed) == x
    assert _host(shardfmt.unpack_gpu(packed)) == x


@pytest.mark.parametrize("E", ELEMS)
def test_pack_gpu_greedy_matches_cpu_writer(E, monkeypatch):
    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", "0")
    for x in (_mixed_case(True), _tokens(), b""):
        assert shardfmt.pack_gpu(x, block_raw=8192, shuffle_elem=E) == \
            shardfmt.pack(x, block_raw=8192, shuffle_elem=E), (E, len(x))


def test_pack_gpu_size_benefit_on_token_ids():
    """Default (wave-screen) matcher.  Measured on an MI355X: plain
    65404, filtered 33852 (0.518); docs/35-gpu-data-plane.md."""
    x = _tokens()
    plain = len(shardfmt.pack_gpu(x))
    filt = shardfmt.pack_gpu(x, shuffle_elem=4)
    print(f"pack_gpu token shard: plain {plain} filtered {len(filt)} "
          f"ratio {len(filt) / plain:.3f}")
    assert len(filt) < plain
    assert shardfmt.unpack_cpu(filt) == x


# ------------------------------------------------------------- CRC, stager
@pytest.mark.parametrize("compress", [True, False])
def test_unpack_gpu_detects_corruption(compress):
    x = _mixed_case(True)
    packed = bytearray(shardfmt.pack(x, block_raw=8192, compress=compress,
                                     shuffle_elem=4))
    idx = shardfmt.read_index(bytes(packed))
    packed[idx.payload_off + 8] ^= 0x55
    with pytest.raises(ValueError, match="CRC mismatch"):
        shardfmt.unpack_gpu(bytes(packed))


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stager_delivers_unshuffled_bytes(tmp_path, native):
    x = _mixed_case(True) + _tokens()
    paths = []
    for E in (4, 2):
        p = tmp_path / f"tokens{E}.syshard"
        p.write_bytes(shardfmt.pack(x, block_raw=8192, shuffle_elem=E))
        paths.append(p)
    st = ShardStager(staging_mb=1, verify=True, native=native)
    tensor, res = st.stage_file(paths[0])
    torch.cuda.synchronize()
    assert res.decoded and res.verified
    assert res.raw_bytes == len(x)
    assert _host(tensor) == x
    many = st.stage_many(paths)
    assert all(r.verified and r.raw_bytes == len(x) for r in many.values())
