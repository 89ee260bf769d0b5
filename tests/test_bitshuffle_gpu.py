"""GPU tests of the SYSHARD bit-shuffle filter: the ops.bit_shuffle
kernel against shardfmt.bitshuffle_blocks_numpy byte for byte, and the
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
BLOCKS = (4096, 8192, 16384)
TILE = 4096
CANARY = 0xA5
GUARD = 4096  # sentinel bytes on either side of dst


def _cuda(raw: bytes):
    if not raw:
        return torch.empty(0, dtype=torch.uint8, device="cuda:0")
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")


def _host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(
        0, 256, n, dtype=np.uint8).tobytes()


def _one_hot(n: int, B: int) -> bytes:
    """Element i has the single bit (i * 5 + i // (8 * B)) % (8 * B)
    set: every plane and every bit position inside a plane byte gets
    its own pattern, so a swapped plane or bit order cannot match."""
    n_el = n // B
    i = np.arange(n_el, dtype=np.uint64)
    bit = (i * np.uint64(5) + i // np.uint64(8 * B)) % np.uint64(8 * B)
    el = (np.uint64(1) << bit).astype(f"<u{B}")
    return el.tobytes() + bytes(range(1, n - n_el * B + 1))


def _in_guards(src, block_raw, B, inverse=False):
    """Run the kernel into an aligned view between two 4 KiB sentinel
    bands; returns the view's bytes after checking both bands."""
    n = src.numel()
    big = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8,
                     device="cuda:0")
    dst = big[GUARD:GUARD + n]
    assert dst.data_ptr() % 16 == 0
    ops.bit_shuffle(src, dst, block_raw, B, inverse=inverse)
    torch.cuda.current_stream().synchronize()
    host = big.cpu().numpy()
    assert (host[:GUARD] == CANARY).all(), "wrote before dst"
    assert (host[GUARD + n:] == CANARY).all(), "wrote past dst"
    return host[GUARD:GUARD + n].tobytes()


def _lengths(B, block_raw):
    tails = (1, B - 1, 8 * B - 1, 8 * B, 8 * B * 3 + B + 1, 4095,
             block_raw - 1)
    full = {TILE,            # exactly one tile (a block only at 4096)
            block_raw,       # one block
            5 * TILE}        # a partial unrolled pass, straddling blocks
    ragged = {2 * block_raw + t for t in tails} | {tails[4], block_raw - 1}
    return sorted(full | ragged)


def _check(x: bytes, block_raw: int, B: int):
    want = shardfmt.bitshuffle_blocks_numpy(x, block_raw, B)
    d_x = _cuda(x)
    got = _in_guards(d_x, block_raw, B)
    assert got == want, (B, block_raw, len(x))
    back = _in_guards(_cuda(got), block_raw, B, inverse=True)
    assert back == x, (B, block_raw, len(x))
    assert _host(d_x) == x  # the source is read-only


@pytest.mark.parametrize("block_raw", BLOCKS)
@pytest.mark.parametrize("B", ELEMS)
def test_kernel_matches_reference(B, block_raw):
    for n in _lengths(B, block_raw):
        _check(_rand(n, seed=n * 8 + B), block_raw, B)


@pytest.mark.parametrize("block_raw", BLOCKS)
@pytest.mark.parametrize("B", ELEMS)
def test_kernel_one_hot_pattern(B, block_raw):
    for n in (5 * TILE, 2 * block_raw + 8 * B * 3 + B + 1):
        x = _one_hot(n, B)
        _check(x, block_raw, B)
    # the pattern is not symmetric: the planes differ from one another
    flt = shardfmt.bitshuffle_blocks_numpy(_one_hot(TILE, B), TILE, B)
    L = TILE // (8 * B)
    assert len({flt[p * L:(p + 1) * L] for p in range(8 * B)}) == 8 * B


def test_kernel_block_not_power_of_two():
    """block_raw = 3 tiles: the tile -> (block, tile-in-block) split is a
    real division, and a 4-tile pass straddles block boundaries."""
    block_raw, n = 12288, 7 * 12288 + 4099
    x = _rand(n, seed=77)
    for B in ELEMS:
        _check(x, block_raw, B)


def test_kernel_empty_is_a_no_op():
    e = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    ops.bit_shuffle(e, torch.empty_like(e), 4096, 4)
    torch.cuda.synchronize()


def _check_blocks(x, y, picks, block_raw, B):
    n = x.numel()
    for b in picks:
        lo, hi = b * block_raw, min((b + 1) * block_raw, n)
        want = shardfmt.bitshuffle_blocks_numpy(_host(x[lo:hi]), block_raw, B)
        assert _host(y[lo:hi]) == want, b


@pytest.mark.parametrize("B", ELEMS)
def test_kernel_grid_stride(B):
    """More work items than the capped grid of 8192 workgroups: 160 MiB
    at 8 KiB blocks is 10240 four-tile passes, plus a ragged tail."""
    block_raw = 8192
    n = 160 * (1 << 20) + 8 * B * 3 + B + 1
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(40 + B)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0",
                      generator=gen)
    y = torch.full_like(x, CANARY)
    ops.bit_shuffle(x, y, block_raw, B)
    n_blocks = (n + block_raw - 1) // block_raw
    rng = np.random.default_rng(B)
    picks = [0, n_blocks - 2, n_blocks - 1] + \
        rng.integers(1, n_blocks - 2, 12).tolist()
    _check_blocks(x, y, picks, block_raw, B)
    z = torch.full_like(x, CANARY)
    ops.bit_shuffle(y, z, block_raw, B, inverse=True)
    assert torch.equal(z, x)


def test_kernel_past_4gib():
    """64-bit block offsets: 4 GiB + 2 blocks + a ragged tail.  Blocks
    are independent, so the reference is computed only for sampled
    blocks (both ends, and either side of the 2 GiB and 4 GiB offsets);
    the rest is covered by the full-length device round trip."""
    B, block_raw = 4, 65536
    n = (1 << 32) + 2 * block_raw + 4093
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * n + (1 << 30):
        pytest.skip(f"needs {3 * n >> 30} GiB of free device memory, "
                    f"{free >> 30} GiB free")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0",
                      generator=gen)
    y = torch.full_like(x, CANARY)
    ops.bit_shuffle(x, y, block_raw, B)
    n_blocks = (n + block_raw - 1) // block_raw
    picks = [0, 1, (1 << 31) // block_raw - 1, (1 << 31) // block_raw,
             (1 << 32) // block_raw - 1, (1 << 32) // block_raw,
             n_blocks - 2, n_blocks - 1]
    _check_blocks(x, y, picks, block_raw, B)
    z = torch.full_like(x, CANARY)
    ops.bit_shuffle(y, z, block_raw, B, inverse=True)
    assert torch.equal(z, x)


# ------------------------------------------------------------- shard level
@functools.lru_cache(maxsize=None)
def _mixed_case() -> bytes:
    """Half incompressible, half int64 ramps -> stored and LZ4 blocks,
    and a ragged final block of 1001 bytes (no multiple of 8*B)."""
    rng = np.random.default_rng(21)
    ramp = (np.arange(10 * 1024, dtype=np.int64) * 3 + 7).tobytes()
    tail = rng.integers(0, 7, 1001, dtype=np.uint8).tobytes()
    return os.urandom(10 * 8192) + ramp + tail


FILTERS = [(2, 0), (4, 0), (8, 0), (8, 8), (2, 4)]
FILTER_IDS = ["bits2", "bits4", "bits8", "delta8+bits8", "delta4+bits2"]


@pytest.mark.parametrize("B,D", FILTERS, ids=FILTER_IDS)
def test_unpack_gpu_reads_cpu_authored(B, D):
    x = _mixed_case()
    packed = shardfmt.pack(x, block_raw=8192, bitshuffle_elem=B,
                           delta_elem=D)
    idx = shardfmt.read_index(packed)
    assert (idx.bitshuffle_elem, idx.delta_elem) == (B, D)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks  # both block kinds occur
    assert int(idx.table["raw_len"][-1]) % (8 * B)
    for verify in (True, False):
        got = shardfmt.unpack_gpu(packed, verify=verify)
        assert got.numel() == len(x)
        assert _host(got) == x, verify


@pytest.mark.parametrize("B,D", FILTERS, ids=FILTER_IDS)
def test_unpack_gpu_stored_contiguous(B, D):
    x = _mixed_case()
    packed = shardfmt.pack(x, block_raw=8192, compress=False,
                           bitshuffle_elem=B, delta_elem=D)
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


@pytest.mark.parametrize("B,D", FILTERS, ids=FILTER_IDS)
def test_pack_gpu_round_trips(B, D):
    x = _mixed_case()
    t = _cuda(x)
    packed = shardfmt.pack_gpu(t, block_raw=8192, bitshuffle_elem=B,
                               delta_elem=D)
    assert _host(t) == x  # the caller's tensor is left alone
    idx = shardfmt.read_index(packed)
    assert (idx.bitshuffle_elem, idx.delta_elem) == (B, D)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks
    assert shardfmt.unpack_cpu(packed) == x
    assert _host(shardfmt.unpack_gpu(packed)) == x


@pytest.mark.parametrize("B,D", [(2, 0), (8, 8)],
                         ids=["bits2", "delta8+bits8"])
def test_pack_gpu_greedy_matches_cpu_writer(B, D, monkeypatch):
    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", "0")
    for x in (_mixed_case(), b""):
        kw = dict(block_raw=8192, bitshuffle_elem=B, delta_elem=D)
        assert shardfmt.pack_gpu(x, **kw) == shardfmt.pack(x, **kw), len(x)


@pytest.mark.parametrize("compress", [True, False])
def test_unpack_gpu_detects_corruption(compress):
    x = _mixed_case()
    packed = bytearray(shardfmt.pack(x, block_raw=8192, compress=compress,
                                     bitshuffle_elem=4))
    idx = shardfmt.read_index(bytes(packed))
    packed[idx.payload_off + 8] ^= 0x55  # inside a stored block
    with pytest.raises(ValueError, match="CRC mismatch"):
        shardfmt.unpack_gpu(bytes(packed))


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stager_delivers_original_bytes(tmp_path, native):
    x = _mixed_case()
    paths = []
    for B, D in ((2, 0), (8, 8)):
        p = tmp_path / f"w{B}{D}.syshard"
        p.write_bytes(shardfmt.pack(x, block_raw=8192, bitshuffle_elem=B,
                                    delta_elem=D))
        paths.append(p)
    st = ShardStager(staging_mb=1, verify=True, native=native)
    for p in paths:
        tensor, res = st.stage_file(p)
        torch.cuda.synchronize()
        assert res.decoded and res.verified
        assert res.raw_bytes == len(x)
        assert _host(tensor) == x
