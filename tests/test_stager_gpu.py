"""GPU tests: shard stager pipeline (pinned double-buffer -> HBM ->
decode -> verify) vs CPU references."""
import os
import random
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_edge_corpus as corpus  # noqa: E402

from shipyard_amd.data import shardfmt  # noqa: E402
from shipyard_amd.data.stager import ShardStager  # noqa: E402


@pytest.mark.parametrize("native", [True, False],
                         ids=["native-cxx", "python"])
def test_stage_shard_file(tmp_path, native):
    rng = random.Random(5)
    data = (bytes(rng.choices(b"abcdefgh", k=500_000)) +
            rng.randbytes(300_000))
    src = tmp_path / "shard.syshard"
    src.write_bytes(shardfmt.pack(data))
    st = ShardStager(staging_mb=1, verify=True, native=native)
    tensor, res = st.stage_file(src)
    torch.cuda.synchronize()
    assert res.decoded and res.verified
    assert res.raw_bytes == len(data)
    assert bytes(tensor.cpu().numpy().tobytes()) == data


def test_stage_plain_file(tmp_path):
    data = random.Random(6).randbytes(3_000_000)
    src = tmp_path / "plain.bin"
    src.write_bytes(data)
    st = ShardStager(staging_mb=1)
    tensor, res = st.stage_file(src)
    torch.cuda.synchronize()
    assert not res.decoded
    assert bytes(tensor.cpu().numpy().tobytes()) == data


def test_stage_detects_corruption(tmp_path):
    data = b"all work and no play " * 50_000
    packed = bytearray(shardfmt.pack(data))
    idx = shardfmt.read_index(bytes(packed))
    # corrupt a stored/compressed block payload byte
    packed[idx.payload_off + 2] ^= 0xAA
    src = tmp_path / "bad.syshard"
    src.write_bytes(bytes(packed))
    st = ShardStager(staging_mb=1, verify=True)
    with pytest.raises(ValueError):
        st.stage_file(src)


# ------------------------------------------------- staging-window edges
# staging_mb=1: the payload lengths below sit on, one past and at
# multiples of the 1 MiB window of both upload paths.
MIB = 1 << 20


@pytest.fixture(scope="module", params=[True, False],
                ids=["native-cxx", "python"])
def stager(request):
    return ShardStager(staging_mb=1, verify=True, native=request.param)


def _host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("block_raw", [4096, 65536])
@pytest.mark.parametrize("final", list(corpus.SHARD_FINALS))
def test_stage_corpus_shards(tmp_path, stager, block_raw, final):
    data = corpus.shard_corpus(block_raw, final)
    src = tmp_path / "c.syshard"
    src.write_bytes(shardfmt.pack(data, block_raw=block_raw))
    tensor, res = stager.stage_file(src)
    torch.cuda.synchronize()
    assert res.decoded and res.verified
    assert res.raw_bytes == len(data) == tensor.numel()
    assert res.file_bytes == src.stat().st_size
    assert _host(tensor) == data


@pytest.mark.parametrize("extra", [0, 16], ids=["1MiB", "1MiB+16"])
@pytest.mark.parametrize("compress", [False, True],
                         ids=["stored", "mixed"])
def test_stage_payload_on_the_window_edge(tmp_path, stager, extra,
                                          compress):
    """Payload of exactly one staging window, and one window plus one
    16-byte tail.  ``mixed`` pads an LZ4 shard's payload to the same
    lengths (bytes behind the last block belong to no block)."""
    rng = random.Random(7 + extra)
    if compress:
        data = corpus.text_like(rng, 200_000) + rng.randbytes(700_000)
        packed = shardfmt.pack(data, block_raw=8192)
        idx = shardfmt.read_index(packed)
        fill = MIB + extra - (len(packed) - idx.payload_off)
        assert fill > 0
        packed += b"\0" * fill
    else:
        data = rng.randbytes(MIB + extra)
        packed = shardfmt.pack(data, block_raw=8192, compress=False)
        idx = shardfmt.read_index(packed)
        assert shardfmt._stored_contiguous(idx)
    assert len(packed) - idx.payload_off == MIB + extra
    src = tmp_path / "edge.syshard"
    src.write_bytes(packed)
    tensor, res = stager.stage_file(src)
    torch.cuda.synchronize()
    assert res.decoded and res.raw_bytes == len(data)
    assert _host(tensor) == data


def test_stage_empty_shard(tmp_path, stager):
    src = tmp_path / "empty.syshard"
    src.write_bytes(shardfmt.pack(b""))
    assert src.stat().st_size == shardfmt.HEADER.size
    tensor, res = stager.stage_file(src)
    assert res.decoded and res.raw_bytes == 0
    assert tensor.is_cuda and tensor.numel() == 0


def test_stage_plain_file_of_two_windows(tmp_path, stager):
    data = random.Random(8).randbytes(2 * MIB)
    src = tmp_path / "plain2.bin"
    src.write_bytes(data)
    tensor, res = stager.stage_file(src)
    torch.cuda.synchronize()
    assert not res.decoded and res.raw_bytes == 2 * MIB
    assert tensor.numel() == 2 * MIB and _host(tensor) == data


@pytest.mark.parametrize("where", ["payload_minus_1", "payload_half",
                                   "table", "header"])
def test_stage_truncated_shard_file_raises(tmp_path, stager, where):
    """A shard file cut short is a ValueError from the index checks;
    nothing is decoded from a payload the table points past."""
    data = corpus.shard_corpus(4096, "none")  # no pad behind the end
    packed = shardfmt.pack(data, block_raw=4096)
    idx = shardfmt.read_index(packed)
    last = idx.blocks[-1]
    assert idx.payload_off + last.comp_off + last.comp_len == len(packed)
    cut = {
        "payload_minus_1": len(packed) - 1,
        "payload_half": idx.payload_off + (len(packed) - idx.payload_off) // 2,
        "table": shardfmt.HEADER.size + 2 * shardfmt.ENTRY.size + 3,
        "header": shardfmt.HEADER.size - 4,
    }[where]
    src = tmp_path / "cut.syshard"
    src.write_bytes(packed[:cut])
    with pytest.raises(ValueError):
        stager.stage_file(src)
    # the stager is still good for the whole file afterwards
    src.write_bytes(packed)
    tensor, _ = stager.stage_file(src)
    torch.cuda.synchronize()
    assert _host(tensor) == data


def test_stage_many_returns_one_result_each(tmp_path, stager):
    rng = random.Random(9)
    datas = [corpus.shard_corpus(4096, "zeros_25"),
             rng.randbytes(MIB + 1),
             corpus.shard_corpus(8192, "random_bm1")]
    paths = [tmp_path / "a.syshard", tmp_path / "b.bin",
             tmp_path / "c.syshard"]
    paths[0].write_bytes(shardfmt.pack(datas[0], block_raw=4096))
    paths[1].write_bytes(datas[1])
    paths[2].write_bytes(shardfmt.pack(datas[2], block_raw=8192))
    for prefetch in (True, False):
        out = stager.stage_many(paths, prefetch=prefetch)
        assert list(out) == [str(p) for p in paths]
        assert [r.raw_bytes for r in out.values()] == \
            [len(d) for d in datas]
        assert [r.decoded for r in out.values()] == [True, False, True]
        assert [r.file_bytes for r in out.values()] == \
            [p.stat().st_size for p in paths]
