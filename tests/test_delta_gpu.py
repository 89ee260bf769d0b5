"""GPU tests of the SYSHARD delta filter: the ops.delta_filter kernel
against shardfmt.delta_blocks_numpy byte for byte (both directions, out
of place and in place), and the filtered shard through every GPU path
above it (unpack_gpu, pack_gpu, the stager).  Every comparison is
exact."""
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


def _filter_in_canary(src, block_raw, E, inverse=False):
    """Run the kernel into an aligned view inside a canary-filled
    buffer; returns the view's bytes after checking that nothing around
    it changed."""
    n = src.numel()
    big = torch.full((n + 2 * PAD,), CANARY, dtype=torch.uint8,
                     device="cuda:0")
    dst = big[PAD:PAD + n]
    assert dst.data_ptr() % 16 == 0
    ops.delta_filter(src, dst, block_raw, E, inverse=inverse)
    torch.cuda.current_stream().synchronize()
    host = big.cpu().numpy()
    assert (host[:PAD] == CANARY).all(), "wrote before dst"
    assert (host[PAD + n:] == CANARY).all(), "wrote past dst"
    return host[PAD:PAD + n].tobytes()


def _in_place(raw: bytes, block_raw, E, inverse=False) -> bytes:
    """The kernel with src is dst, inside a canary-filled buffer."""
    n = len(raw)
    big = torch.full((n + 2 * PAD,), CANARY, dtype=torch.uint8,
                     device="cuda:0")
    buf = big[PAD:PAD + n]
    buf.copy_(_cuda(raw))
    ops.delta_filter(buf, buf, block_raw, E, inverse=inverse)
    host = big.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[PAD + n:] == CANARY).all()
    return host[PAD:PAD + n].tobytes()


def _kernel_lengths(E):
    return sorted({1, E - 1, E, E + 1, 4095, 4096, 4097, 3 * 4096 + 2048,
                   5 * 8192 + 4093})


def _check_both_ways(x: bytes, block_raw: int, E: int, tag=None):
    want = shardfmt.delta_blocks_numpy(x, block_raw, E)
    d_x = _cuda(x)
    got = _filter_in_canary(d_x, block_raw, E)
    assert got == want, ("forward", E, block_raw, len(x), tag)
    assert _host(d_x) == x  # the source is read-only
    d_f = _cuda(want)
    back = _filter_in_canary(d_f, block_raw, E, inverse=True)
    assert back == x, ("inverse", E, block_raw, len(x), tag)
    assert _host(d_f) == want


@pytest.mark.parametrize("block_raw", [4096, 8192])
@pytest.mark.parametrize("E", ELEMS)
def test_kernel_matches_reference(E, block_raw):
    """Random full-range bytes: about every second difference wraps."""
    for n in _kernel_lengths(E):
        _check_both_ways(_rand(n, seed=n * 8 + E), block_raw, E)


@pytest.mark.parametrize("E", ELEMS)
def test_carry_all_ones(E):
    """Deltas of 1 everywhere: every block must decode to 1, 2, 3, ...
    A carry lost between lanes, waves or tiles shows as a restart
    inside a block; a carry leaked across blocks shows as a block that
    does not start at 1.  (A 16 KiB block is one 4-tile pass of its
    workgroup; test_carry_many_passes_per_block crosses pass seams.)"""
    block_raw = 16384
    n = 3 * block_raw + 5000
    dt = np.dtype(f"<u{E}")
    ones = np.ones(n // E, dtype=dt).tobytes() + b"\x07" * (n % E)
    got = _filter_in_canary(_cuda(ones), block_raw, E, inverse=True)
    per = block_raw // E
    vals = np.frombuffer(got[:n // E * E], dtype=dt)
    want = (np.arange(n // E, dtype=np.uint64) % per + 1).astype(dt)
    assert np.array_equal(vals, want)
    assert got[n // E * E:] == b"\x07" * (n % E)
    assert got == shardfmt.delta_blocks_numpy(ones, block_raw, E, True)


@pytest.mark.parametrize("E", ELEMS)
def test_carry_many_passes_per_block(E):
    """A 64 KiB block is four passes of the workgroup: the running
    carry crosses three pass seams (E = 2 also wraps past 65535)."""
    block_raw = 65536
    n = 2 * block_raw + 5 * 4096 + 8
    dt = np.dtype(f"<u{E}")
    ones = np.ones(n // E, dtype=dt).tobytes()
    got = _filter_in_canary(_cuda(ones), block_raw, E, inverse=True)
    vals = np.frombuffer(got, dtype=dt)
    want = (np.arange(n // E, dtype=np.uint64) % (block_raw // E)
            + 1).astype(dt)
    assert np.array_equal(vals, want)


def test_carry_across_32_bit_halves():
    """E = 8: 0xFFFFFFFF then 1 sums to 2**32, so the low half's carry
    must reach the high half, in a lane, across lanes, waves and tiles."""
    block_raw = 8192
    n_el = 2 * (block_raw // 8) + 301
    d = np.empty(n_el, dtype="<u8")
    d[0::2] = 0xFFFFFFFF
    d[1::2] = 1
    raw = d.tobytes()
    want = shardfmt.delta_blocks_numpy(raw, block_raw, 8, inverse=True)
    x = np.frombuffer(want, dtype="<u8")
    assert int(x[1]) == 1 << 32 and int(x[1023]) == 512 << 32
    assert int(x[1024]) == 0xFFFFFFFF  # next block restarted
    assert _filter_in_canary(_cuda(raw), block_raw, 8, inverse=True) == want
    # and back: borrows cross the halves in the forward direction
    assert _filter_in_canary(_cuda(want), block_raw, 8) == raw


def test_block_not_power_of_two():
    """block_raw = 3 tiles: the last tile of the 4-tile pass is dead in
    every block."""
    block_raw, n = 12288, 7 * 12288 + 4099
    x = _rand(n, seed=77)
    for E in ELEMS:
        _check_both_ways(x, block_raw, E)


@pytest.mark.parametrize("E", ELEMS)
def test_large_block(E):
    """block_raw above the 64 KiB LZ4 limit (stored-only shards): 8
    passes per block, and a 17-byte ragged block."""
    block_raw, n = 131072, 2 * 131072 + 17
    _check_both_ways(_rand(n, seed=E), block_raw, E)


@pytest.mark.parametrize("E", ELEMS)
def test_in_place_equals_out_of_place(E):
    for block_raw, n in ((8192, 5 * 8192 + 4093), (65536, 2 * 65536 + 12289),
                         (4096, E + 1)):
        x = _rand(n, seed=n + E)
        f = shardfmt.delta_blocks_numpy(x, block_raw, E)
        assert _in_place(x, block_raw, E) == f, (E, block_raw, "forward")
        assert _in_place(f, block_raw, E, inverse=True) == x, \
            (E, block_raw, "inverse")


def test_partial_overlap_raises_and_launches_nothing():
    buf = torch.zeros(3 * 8192, dtype=torch.uint8, device="cuda:0")
    src = buf[:8192]
    for lo in (16, 4096, 8192 - 16):
        for a, b in ((src, buf[lo:lo + 8192]), (buf[lo:lo + 8192], src)):
            for inverse in (False, True):
                with pytest.raises(ValueError, match="overlap"):
                    ops.delta_filter(a, b, 4096, 4, inverse=inverse)
    # same base, other length is not "in place"
    with pytest.raises(ValueError, match="bytes but dst"):
        ops.delta_filter(src, buf[:4096], 4096, 4)
    torch.cuda.synchronize()
    assert not buf.any().item()  # an all-zero buffer decodes to zeros,
    buf.fill_(1)                 # so also prove it on ones
    with pytest.raises(ValueError, match="overlap"):
        ops.delta_filter(src, buf[16:16 + 8192], 4096, 2, inverse=True)
    torch.cuda.synchronize()
    assert bool((buf == 1).all().item())


def test_non_default_stream():
    E, block_raw, n = 8, 8192, 9 * 8192 + 1234
    x = _rand(n, seed=3)
    d_x = _cuda(x)
    d_y = torch.empty_like(d_x)
    d_z = torch.empty_like(d_x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.delta_filter(d_x, d_y, block_raw, E)
        ops.delta_filter(d_y, d_z, block_raw, E, inverse=True)
    side.synchronize()
    assert _host(d_y) == shardfmt.delta_blocks_numpy(x, block_raw, E)
    assert _host(d_z) == x


def test_empty_is_a_no_op_without_the_library(monkeypatch):
    def boom():
        raise AssertionError("library loaded for an empty buffer")

    monkeypatch.setattr(ops, "_load", boom)
    e = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    ops.delta_filter(e, torch.empty_like(e), 4096, 4)
    ops.delta_filter(e, e, 4096, 8, inverse=True)


def test_past_4gib():
    """64-bit block offsets and the grid-stride loop: 4 GiB + 2 blocks +
    a ragged tail (more blocks than the capped grid).  Blocks are
    independent, so the host reference is computed only for the blocks
    on either side of the 4 GiB offset, both ends and the ragged block;
    the in-place inverse over the full length covers the rest."""
    E, block_raw = 8, 65536
    n = (1 << 32) + 2 * block_raw + 4093
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * n + (1 << 30):
        pytest.skip(f"needs {2 * n + (1 << 30)} bytes of free HBM")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0",
                      generator=gen)
    y = torch.full_like(x, CANARY)
    ops.delta_filter(x, y, block_raw, E)
    n_blocks = (n + block_raw - 1) // block_raw
    picks = [0, (1 << 32) // block_raw - 1, (1 << 32) // block_raw,
             n_blocks - 2, n_blocks - 1]
    for b in picks:
        lo, hi = b * block_raw, min((b + 1) * block_raw, n)
        want = shardfmt.delta_blocks_numpy(_host(x[lo:hi]), block_raw, E)
        assert _host(y[lo:hi]) == want, b
    ops.delta_filter(y, y, block_raw, E, inverse=True)
    assert torch.equal(y, x)


# ---------------------------------------------------------- shard level
@functools.lru_cache(maxsize=None)
def _offsets_case() -> bytes:
    """int64 cumulative offsets (LZ4 blocks after filtering), an
    incompressible stretch (stored blocks) and a ragged final block of
    1001 bytes."""
    rng = np.random.default_rng(21)
    offs = np.cumsum(rng.poisson(40, 24 * 1024)).astype("<i8").tobytes()
    tail = rng.integers(0, 7, 1001, dtype=np.uint8).tobytes()
    return offs + os.urandom(3 * 65536) + tail


FILTERS = [(8, 0), (8, 8), (4, 2)]
FILTER_IDS = ["delta8", "delta8+shuf8", "delta4+shuf2"]


@pytest.mark.parametrize("block_raw", [8192, 65536])
@pytest.mark.parametrize("D,S", FILTERS, ids=FILTER_IDS)
def test_unpack_gpu_reads_cpu_authored(D, S, block_raw):
    x = _offsets_case()
    packed = shardfmt.pack(x, block_raw=block_raw, delta_elem=D,
                           shuffle_elem=S)
    idx = shardfmt.read_index(packed)
    assert (idx.delta_elem, idx.shuffle_elem) == (D, S)
    stored = int((idx.table["comp_len"] == idx.table["raw_len"]).sum())
    assert 0 < stored < idx.n_blocks  # both block kinds occur
    for verify in (True, False):
        got = shardfmt.unpack_gpu(packed, verify=verify)
        assert got.numel() == len(x)
        assert _host(got) == x, verify


@pytest.mark.parametrize("block_raw", [8192, 65536])
@pytest.mark.parametrize("D,S", FILTERS, ids=FILTER_IDS)
def test_unpack_gpu_stored_contiguous(D, S, block_raw):
    x = _offsets_case()
    packed = shardfmt.pack(x, block_raw=block_raw, compress=False,
                           delta_elem=D, shuffle_elem=S)
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


@pytest.mark.parametrize("block_raw", [8192, 65536])
@pytest.mark.parametrize("D,S", FILTERS, ids=FILTER_IDS)
def test_pack_gpu_round_trips(D, S, block_raw):
    x = _offsets_case()
    d_x = _cuda(x)
    packed = shardfmt.pack_gpu(d_x, block_raw=block_raw, delta_elem=D,
                               shuffle_elem=S)
    assert _host(d_x) == x  # the caller's tensor is untouched
    idx = shardfmt.read_index(packed)
    assert (idx.delta_elem, idx.shuffle_elem) == (D, S)
    assert shardfmt.unpack_cpu(packed) == x
    assert _host(shardfmt.unpack_gpu(packed)) == x


@pytest.mark.parametrize("D,S", FILTERS, ids=FILTER_IDS)
def test_pack_gpu_greedy_matches_cpu_writer(D, S, monkeypatch):
    monkeypatch.setenv("SHIPYARD_LZ4C_SCREEN", "0")
    for x in (_offsets_case(), b""):
        for block_raw in (8192, 65536):
            assert shardfmt.pack_gpu(x, block_raw=block_raw, delta_elem=D,
                                     shuffle_elem=S) == \
                shardfmt.pack(x, block_raw=block_raw, delta_elem=D,
                              shuffle_elem=S), (D, S, len(x), block_raw)


@pytest.mark.parametrize("compress", [True, False])
def test_unpack_gpu_detects_corruption(compress):
    x = _offsets_case()
    for D, S in ((8, 0), (8, 8)):
        packed = bytearray(shardfmt.pack(x, block_raw=8192,
                                         compress=compress, delta_elem=D,
                                         shuffle_elem=S))
        idx = shardfmt.read_index(bytes(packed))
        # inside the stored stretch: the LZ4 decoder cannot reject it
        # first, only the CRC can
        st = np.nonzero(idx.table["comp_len"] == idx.table["raw_len"])[0]
        off = idx.payload_off + int(idx.table["comp_off"][st[1]]) + 8
        packed[off] ^= 0x55
        with pytest.raises(ValueError, match="CRC mismatch"):
            shardfmt.unpack_gpu(bytes(packed))


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stager_delivers_decoded_bytes(tmp_path, native):
    x = _offsets_case()
    paths = []
    for D, S in ((8, 8), (8, 0)):
        p = tmp_path / f"offsets_{D}_{S}.syshard"
        p.write_bytes(shardfmt.pack(x, block_raw=8192, delta_elem=D,
                                    shuffle_elem=S))
        paths.append(p)
    st = ShardStager(staging_mb=1, verify=True, native=native)
    for p in paths:
        tensor, res = st.stage_file(p)
        torch.cuda.synchronize()
        assert res.decoded and res.verified
        assert res.raw_bytes == len(x)
        assert _host(tensor) == x
    many = st.stage_many(paths)
    assert all(r.verified and r.raw_bytes == len(x) for r in many.values())
