"""Deterministic edge-case corpora for the HIP data-plane kernels.

A plain helper module (not a conftest): every builder is seeded with
``random.Random(seed)`` so a failure reproduces byte for byte.  The
CPU-only ``test_ops_edge_corpus.py`` pins that each builder really
produces the encoding feature it is named for; ``test_ops_edges_gpu.py``
feeds the same bytes to the kernels.  The shard corpus
(``shard_corpus``) is pinned by ``test_shard_index_validation.py`` and
drives ``test_shard_edges_gpu.py`` and the stager tests.
"""
from __future__ import annotations

import random
from typing import List, Tuple

from shipyard_amd.data import lz4py

# lz4_decode.hip per-block status codes
OK, ERR_OFFSET, ERR_OVERFLOW, ERR_TRUNC, ERR_MISMATCH, ERR_TOOBIG = range(6)

GUARD = 0xA5       # pre-fill byte of guarded output buffers
SLOT_SLACK = 64    # guard bytes behind every slot; keeps slots 16 B aligned

_TEXT = b"the quick brown fox 0123"


# ---------------------------------------------------------------- content
def text_like(rng: random.Random, n: int) -> bytes:
    return bytes(rng.choices(_TEXT, k=n))


def mixed_content(rng: random.Random, n: int) -> bytes:
    """The content mix of the existing decoder fuzz (byte runs, random,
    short-period patterns, text-ish), seeded throughout."""
    parts: List[bytes] = []
    total = 0
    while total < n:
        kind = rng.randrange(4)
        m = rng.randint(1, 9000)
        if kind == 0:
            part = bytes([rng.randrange(256)]) * m
        elif kind == 1:
            part = rng.randbytes(m)
        elif kind == 2:
            pat = rng.randbytes(rng.randint(1, 17))
            part = (pat * (m // len(pat) + 1))[:m]
        else:
            part = text_like(rng, m)
        parts.append(part)
        total += m
    return b"".join(parts)[:n]


# ----------------------------------------------------------- stream parse
def parse_sequences(stream: bytes) -> List[dict]:
    """Split an LZ4 block into its sequences without decoding it.  Each
    entry: lit_len, lit_ext (the literal-length extension bytes),
    offset and match_len (None on the final literals-only sequence) and
    match_ext (the match-length extension bytes)."""
    seqs = []
    pos, n = 0, len(stream)
    while pos < n:
        token = stream[pos]
        pos += 1
        lit, lit_ext = token >> 4, b""
        if lit == 15:
            start = pos
            while stream[pos] == 255:
                pos += 1
            pos += 1
            lit_ext = stream[start:pos]
            lit += sum(lit_ext)
        pos += lit
        if pos > n:
            raise ValueError("literal overrun")
        if pos == n:
            seqs.append(dict(lit_len=lit, lit_ext=lit_ext, offset=None,
                             match_len=None, match_ext=b""))
            break
        offset = stream[pos] | (stream[pos + 1] << 8)
        pos += 2
        mlen, match_ext = (token & 15) + 4, b""
        if token & 15 == 15:
            start = pos
            while stream[pos] == 255:
                pos += 1
            pos += 1
            match_ext = stream[start:pos]
            mlen += sum(match_ext)
        seqs.append(dict(lit_len=lit, lit_ext=lit_ext, offset=offset,
                         match_len=mlen, match_ext=match_ext))
    return seqs


# -------------------------------------------------------- decoder corpora
def malformed_lz4_cases(raw_cap: int = 4096
                        ) -> List[Tuple[str, bytes, int, int]]:
    """(name, stream, out_len, expected kernel status).  Every stream
    raises ValueError in ``lz4py.decompress_block``.  ``raw_cap`` is the
    capacity of the decoder instantiation the launch selects (it only
    shapes the TOOBIG case)."""
    h = bytes.fromhex
    valid = lz4py.compress_block(b"shipyard" * 8)
    return [
        ("off0", h("10780000"), 64, ERR_OFFSET),
        ("off_gt_dpos", h("10780200"), 64, ERR_OFFSET),
        ("trunc_litlen", h("f0ff"), 64, ERR_TRUNC),
        ("trunc_offset", h("107801"), 64, ERR_TRUNC),
        ("trunc_mlen", h("1f780100ff"), 64, ERR_TRUNC),
        ("lit_over_stream", h("506162"), 64, ERR_OVERFLOW),
        ("lit_over_out", h("506162636465"), 3, ERR_OVERFLOW),
        ("match_over_out", h("10780100"), 3, ERR_OVERFLOW),
        ("mismatch_short", h("506162636465"), 6, ERR_MISMATCH),
        ("toobig", valid, raw_cap + 1, ERR_TOOBIG),
    ]


def accepted_lz4_case() -> Tuple[str, bytes, int, bytes]:
    """A match that ends the stream: valid in lz4py and in the kernels."""
    return ("match_ends_stream", bytes.fromhex("10780100"), 5, b"xxxxx")


def many_sequence_text_block(rng: random.Random, n: int) -> bytes:
    """Text-like block of at most ``n`` bytes whose lz4py stream has more
    than 200 sequences, the count not a multiple of 16: it wraps the
    producer/consumer decoder's 64-entry ring several times and ends on
    an unbatched tail publish."""
    words = _TEXT.split() + [b"rocm", b"wave", b"lds", b"shard", b"layer",
                             b"gfx950", b"block", b"crc"]
    text = bytearray()
    while len(text) < n:
        text += rng.choice(words) + rng.choice((b" ", b", ", b"\n"))
    block = bytes(text[:n])
    while True:
        count = len(parse_sequences(lz4py.compress_block(block)))
        if count > 200 and count % 16:
            return block
        if len(block) <= n // 2:
            raise AssertionError("no >200-sequence text block at %d" % n)
        block = block[:-7]


def decode_fuzz_blocks(raw_cap: int, seed: int, many_seq: bool
                       ) -> List[bytes]:
    """About six raw blocks (each <= raw_cap) for the guarded decode
    fuzz: one per content kind, optionally the many-sequence text block,
    and a final block whose length is not a multiple of 16."""
    rng = random.Random(seed)
    blocks = [
        bytes([rng.randrange(256)]) * raw_cap,
        rng.randbytes(raw_cap),
        (rng.randbytes(rng.randint(1, 17)) * raw_cap)[:raw_cap],
        mixed_content(rng, raw_cap),
    ]
    if many_seq:
        blocks.append(many_sequence_text_block(rng, min(raw_cap, 8192)))
    else:
        blocks.append(text_like(rng, raw_cap))
    last = rng.randint(raw_cap // 2, raw_cap - 1) | 1  # odd: never %16
    blocks.append(mixed_content(rng, last))
    return blocks


# ------------------------------------------------------ compressor corpora
_LITERAL_RUNS = (14, 15, 16, 269, 270, 271)
_FINAL_SIZES = (5, 12, 13, 16)


def _literal_run_block(rng: random.Random, run: int) -> bytes:
    """``run`` literal bytes with no repeated 4-gram, then a 40-byte
    repeat of the block's start (the match), then an unrelated tail."""
    while True:
        head = rng.randbytes(run)
        grams = {head[i:i + 4] for i in range(run - 3)}
        if len(grams) == run - 3:
            break
    tail = bytes(b ^ 0xFF for b in head[:16])
    return head + head[:40] + tail


def compress_edge_blocks(block_raw: int) -> List[Tuple[str, bytes]]:
    """(name, data) inputs for the compressors.  Except for
    ``exact_multiple`` each is one full seeded block followed by a final
    block that carries the named feature:

    * ``zeros_790`` / ``zeros_791`` / ``zeros_25`` — zero-filled final
      block; the match-length extension is ``ff ff ff 00``, ``ff ff ff
      01`` and a single ``00``;
    * ``lit_<n>`` — a literal run of exactly n bytes before a match
      (14/15/16 straddle the token nibble, 269/270/271 the first ``ff``
      extension byte);
    * ``final_<n>`` — a final block of n equal bytes (below 13 bytes the
      block is literals only);
    * ``exact_multiple`` — exactly 3 * block_raw bytes."""
    rng = random.Random(0x5EED ^ block_raw)
    out: List[Tuple[str, bytes]] = []
    for n in (790, 791, 25):
        out.append(("zeros_%d" % n,
                    mixed_content(rng, block_raw) + b"\0" * n))
    for run in _LITERAL_RUNS:
        out.append(("lit_%d" % run,
                    mixed_content(rng, block_raw)
                    + _literal_run_block(rng, run)))
    for n in _FINAL_SIZES:
        out.append(("final_%d" % n,
                    mixed_content(rng, block_raw) + b"\x07" * n))
    out.append(("exact_multiple", mixed_content(rng, 3 * block_raw)))
    return out


def final_block(data: bytes, block_raw: int) -> bytes:
    n_blocks = (len(data) + block_raw - 1) // block_raw
    return data[(n_blocks - 1) * block_raw:]


# ---------------------------------------------------------- shard corpora
SHARD_BLOCK_SIZES = (4096, 8192, 16384, 32768, 65536)
# final-block variant -> True when the writer must store it
SHARD_FINALS = {
    "equal_5": True,       # stored, < 16 B: gather_copy's byte tail only
    "zeros_25": False,     # compressed 25-byte block
    "random_bm1": True,    # stored, block_raw - 1 bytes (odd length)
    "text_4k": False,      # compressed, 4001 bytes of text
    "none": None,          # no final block: exact block multiple
}
SHARD_FULL_BLOCKS = 5      # text, random, byte run, random, mixed


def shard_corpus(block_raw: int, final: str) -> bytes:
    """Pipeline input for block size ``block_raw``: five full blocks
    (text, random, a one-byte run, random, mixed) and the named final
    block.  Blocks 1 and 3 are stored and blocks 0 and 2 compressed
    under every writer; the five full blocks are the same for every
    ``final`` of one block size."""
    rng = random.Random(0x5A4D ^ block_raw)
    blocks = [
        text_like(rng, block_raw),
        rng.randbytes(block_raw),
        bytes([rng.randrange(256)]) * block_raw,
        rng.randbytes(block_raw),
        mixed_content(rng, block_raw),
    ]
    frng = random.Random(0xF1A1 ^ block_raw)
    last = {
        "equal_5": lambda: bytes([frng.randrange(256)]) * 5,
        "zeros_25": lambda: b"\0" * 25,
        "random_bm1": lambda: frng.randbytes(block_raw - 1),
        "text_4k": lambda: text_like(frng, 4001),
        "none": lambda: b"",
    }[final]()
    return b"".join(blocks) + last


def shard_blocks(data: bytes, block_raw: int) -> List[bytes]:
    return [data[o:o + block_raw] for o in range(0, len(data), block_raw)]


def reversed_stored_shard(data: bytes, block_raw: int) -> bytes:
    """Hand-built stored-only SYSHARD whose blocks sit in the payload in
    reverse order: valid, but not the contiguous layout, so the GPU
    reader must move every block with gather_copy."""
    from shipyard_amd.data import shardfmt
    from shipyard_amd.ops import gf2

    blocks = shard_blocks(data, block_raw)
    offs, payload = {}, bytearray()
    for i in reversed(range(len(blocks))):
        offs[i] = len(payload)
        payload += blocks[i]
        payload += b"\0" * (-len(payload) % 16)
    table = b"".join(
        shardfmt.ENTRY.pack(offs[i], len(b), len(b), gf2.crc32c(b))
        for i, b in enumerate(blocks))
    return (shardfmt.HEADER.pack(shardfmt.MAGIC, 0, block_raw, len(data),
                                 len(blocks)) + table + bytes(payload))


# ------------------------------------------------- guarded GPU decode run
def slot_stride(raw_cap: int) -> int:
    return raw_cap + SLOT_SLACK


def guarded_decode(streams, out_lens, raw_cap: int, pc: bool,
                   stride: int = None):
    """Decode ``streams`` (concatenated back to back, so most ``in_off``
    are unaligned) into slots of a GUARD-filled output tensor.  Returns
    (per-block status list, output as a numpy array, stride)."""
    import torch

    from shipyard_amd import ops

    dev = torch.device("cuda:0")
    stride = stride or slot_stride(raw_cap)
    assert stride % 16 == 0
    in_off, pos = [], 0
    for s in streams:
        in_off.append(pos)
        pos += len(s)
    comp = b"".join(streams) + b"\0" * 16
    d_comp = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    n = len(streams)
    d_out = torch.full((n * stride,), GUARD, dtype=torch.uint8, device=dev)
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    t32 = lambda v: torch.tensor(v, dtype=torch.int64).to(
        torch.uint32).to(dev)
    status = ops.lz4_decode_blocks(
        d_comp, t64(in_off), t32([len(s) for s in streams]), d_out,
        t64([i * stride for i in range(n)]), t32(list(out_lens)),
        raw_cap=raw_cap, pc=pc)
    torch.cuda.synchronize()
    return (status.cpu().to(torch.int64).tolist(), d_out.cpu().numpy(),
            stride)


def check_slots(got, stride: int, expected) -> None:
    """``expected[i]`` is the payload of slot i (b"" for a slot that
    must stay untouched).  Payloads must be exact and every byte outside
    them must still be GUARD."""
    import numpy as np

    want = np.full(got.shape, GUARD, dtype=np.uint8)
    for i, payload in enumerate(expected):
        lo = i * stride
        seg = bytes(got[lo:lo + len(payload)].tobytes())
        assert seg == payload, "slot %d payload differs" % i
        want[lo:lo + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (
        "bytes outside the payloads were written, first at %d (slot %d "
        "+%d)" % (bad[0], bad[0] // stride, bad[0] % stride))


def check_guarded_fuzz(raw_cap: int, pc: bool, seed: int) -> None:
    blocks = decode_fuzz_blocks(raw_cap, seed, many_seq=pc)
    streams = [lz4py.compress_block(b) for b in blocks]
    assert any(sum(map(len, streams[:i])) % 16 for i in range(len(streams)))
    status, got, stride = guarded_decode(
        streams, [len(b) for b in blocks], raw_cap, pc)
    assert status == [OK] * len(blocks), status
    check_slots(got, stride, blocks)
