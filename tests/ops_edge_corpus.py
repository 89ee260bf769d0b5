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
from collections import namedtuple
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


# ------------------------------------------- hand-assembled decoder corpora
# Streams the format allows but the project's greedy matchers never
# emit.  A sequence is (literals, offset, mlen); the assembler encodes
# it and builds the raw bytes without lz4py.
SeqMark = namedtuple("SeqMark", "token off mext dlit dpos")
SeqMark.__doc__ = (
    "Positions of one assembled sequence: stream index of its token, of "
    "its low offset byte and of its first match-length extension byte "
    "(None without one); decoded position before its literals (dlit) "
    "and before its match (dpos).")

MATCH_OFFSETS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65,
                 66, 127, 128, 129, 255, 256, 257)
MATCH_LENS = (4, 5, 15, 18, 19, 20, 63, 64, 65, 66, 127, 128, 129, 130, 191,
              192, 193, 273, 274, 275, 529)
REL_LENS = (5, 63, 64, 65, 128, 129)
LIT_RUNS = (1, 0, 14, 15, 16, 63, 64, 65, 66, 127, 128, 129, 269, 270, 271,
            525)
FAR_REACH_RUNGS = (4096, 8192, 16384, 32768, 65536)
DEEP_K = (1, 15, 16, 63, 64, 65)   # and the last sequence
SEQ_CLASSES = ("lit_short", "lit_loop", "match_single", "match_loop",
               "match_doubling_2", "match_doubling_3plus")


def _lsic(out: bytearray, value: int) -> None:
    while value >= 255:
        out.append(255)
        value -= 255
    out.append(value)


def assemble_lz4_marks(seqs, tail: bytes = b"", terminator: bool = None):
    """-> (stream, raw, marks): ``assemble_lz4`` plus one SeqMark per
    sequence.  ``terminator`` forces (True) or drops (False) the final
    literals-only sequence; by default it is written iff ``tail`` is
    not empty."""
    stream, raw, marks = bytearray(), bytearray(), []
    for lits, offset, mlen in seqs:
        assert mlen >= 4 and 0 < offset <= 0xFFFF
        token = len(stream)
        dlit = len(raw)
        stream.append((min(len(lits), 15) << 4) | min(mlen - 4, 15))
        if len(lits) >= 15:
            _lsic(stream, len(lits) - 15)
        stream += lits
        raw += lits
        assert offset <= len(raw), "assembled offset reaches before 0"
        off = len(stream)
        stream.append(offset & 0xFF)
        stream.append(offset >> 8)
        mext = None
        if mlen - 4 >= 15:
            mext = len(stream)
            _lsic(stream, mlen - 19)
        marks.append(SeqMark(token, off, mext, dlit, len(raw)))
        for _ in range(mlen):
            raw.append(raw[-offset])
    if terminator if terminator is not None else bool(tail):
        stream.append(min(len(tail), 15) << 4)
        if len(tail) >= 15:
            _lsic(stream, len(tail) - 15)
        stream += tail
        raw += tail
    else:
        assert not tail
    return bytes(stream), bytes(raw), marks


def assemble_lz4(seqs, tail: bytes = b"", terminator: bool = None
                 ) -> Tuple[bytes, bytes]:
    """Encode ``seqs`` = [(literals, offset, mlen), ...] and the final
    literals ``tail`` as one LZ4 block -> (stream, raw).  Writes token,
    LSIC extension bytes, literals and the little-endian offset; raw is
    built one byte at a time, independently of lz4py."""
    stream, raw, _ = assemble_lz4_marks(seqs, tail, terminator)
    return stream, raw


def classify_sequences(seqs) -> List[Tuple[str, str]]:
    """The branch of lz4_decode_kernel each sequence takes: (literal
    class, match class), names from SEQ_CLASSES."""
    out = []
    for lits, offset, mlen in seqs:
        lit = "lit_short" if len(lits) <= 64 else "lit_loop"
        if offset >= mlen:
            match = "match_single" if mlen <= 64 else "match_loop"
        else:
            done = rounds = 0
            while done < mlen:
                done += min(mlen - done, done + offset)
                rounds += 1
            match = "match_doubling_2" if rounds == 2 else \
                "match_doubling_3plus"
        out.append((lit, match))
    return out


def _match_off_spec(idx: int, offset: int):
    """One match per MATCH_LENS at a fixed offset, behind a literal
    prefix of 272 + idx >= 257 bytes.  Each further match follows 1, 2
    or 3 literals, chosen (first hit of a depth-first search that tries
    the three lengths in a rotating order) so that within the block the
    matches start at every residue of dpos mod 16, and so mod 4."""
    rng = random.Random(0x0FF5E7 + offset)
    n_match = len(MATCH_LENS)

    def search(j, dpos, seen, runs):
        if len(seen) == 16:
            # the rest keeps rotating through 1, 2, 3
            return runs + [1 + (k + idx) % 3 for k in range(j, n_match)]
        if n_match - j < 16 - len(seen):
            return None
        for t in range(3):
            nlit = 1 + (j + idx + t) % 3
            at = dpos + nlit
            found = search(j + 1, at + MATCH_LENS[j], seen | {at % 16},
                           runs + [nlit])
            if found:
                return found
        return None

    first = 272 + idx
    runs = search(1, first + MATCH_LENS[0], {first % 16}, [first])
    assert runs is not None and set(runs[1:]) == {1, 2, 3}
    seqs = [(rng.randbytes(nlit), offset, mlen)
            for nlit, mlen in zip(runs, MATCH_LENS)]
    return seqs, rng.randbytes(1 + idx % 5)


def _match_rel_spec():
    rng = random.Random(0x4E1)
    seqs, first = [], True
    for mlen in REL_LENS:
        for delta in (-1, 0, 1):
            nlit = 136 if first else 1 + len(seqs) % 3
            seqs.append((rng.randbytes(nlit), mlen + delta, mlen))
            first = False
    return seqs, rng.randbytes(2)


def _lit_runs_spec():
    rng = random.Random(0x117)
    seqs, dpos = [], 0
    for run in LIT_RUNS:
        dpos += run
        seqs.append((rng.randbytes(run), rng.randint(1, min(dpos, 300)), 4))
        dpos += 4
    return seqs, rng.randbytes(3)


def _chain_spec(seed: int, n_seq: int, zero_lit: bool, max_mlen: int,
                tail_len: int):
    """An 8-byte literal prefix with a match, then ``n_seq`` sequences
    of 0 (``zero_lit``) or 1..3 literals and a match of 4..max_mlen
    bytes at a random legal offset."""
    rng = random.Random(seed)
    seqs, dpos = [], 0
    for i in range(n_seq + 1):
        nlit = 8 if i == 0 else 0 if zero_lit else 1 + i % 3
        dpos += nlit
        mlen = rng.randint(4, max_mlen)
        seqs.append((rng.randbytes(nlit), rng.randint(1, dpos), mlen))
        dpos += mlen
    return seqs, rng.randbytes(tail_len)


def _zero_lit_chain_spec():
    return _chain_spec(0x2E80, 309, True, 12, 5)


def _zero_lit_chain_short_spec():
    # 100 four-byte matches: the longest chain that fits 448 raw bytes
    return _chain_spec(0x2E81, 100, True, 4, 3)


def _ordinary_chain_spec():
    return _chain_spec(0x0DD, 210, False, 10, 4)


def _ends_on_match_spec():
    rng = random.Random(0xE0D)
    return [(rng.randbytes(21), 7, 9), (rng.randbytes(2), 30, 70),
            (b"", 3, 33)], b""


def _small_mix_spec():
    """Every match class in under 448 raw bytes."""
    rng = random.Random(0x5A11)
    return [(rng.randbytes(70), 3, 70),      # lit_loop, doubling 3+
            (rng.randbytes(2), 100, 64),     # single
            (rng.randbytes(1), 150, 100),    # loop
            (rng.randbytes(3), 60, 100),     # doubling 2
            (b"", 1, 19)], rng.randbytes(7)


def assembled_specs():
    """(name, seqs, tail, terminator) behind assembled_decode_blocks."""
    specs = []
    for idx, offset in enumerate(MATCH_OFFSETS):
        specs.append(("match_off%d" % offset,
                      *_match_off_spec(idx, offset), None))
    specs.append(("match_rel", *_match_rel_spec(), None))
    specs.append(("lit_runs", *_lit_runs_spec(), None))
    specs.append(("zero_lit_chain", *_zero_lit_chain_spec(), None))
    specs.append(("ends_on_match", *_ends_on_match_spec(), None))
    specs.append(("empty", [], b"", None))
    specs.append(("token_only", [], b"", True))
    return specs


def assembled_decode_blocks() -> List[Tuple[str, bytes, bytes]]:
    """(name, stream, raw), at most 4096 raw bytes each:

    * ``match_off<O>`` — for each O in MATCH_OFFSETS one match per
      MATCH_LENS (token nibble 15 and extension ``00`` at 19, ``ff 00``
      at 274, ``ff ff 00`` at 529);
    * ``match_rel`` — offset == mlen - 1, mlen, mlen + 1 for REL_LENS;
    * ``lit_runs`` — literal runs of LIT_RUNS bytes (extensions ``00``
      at 15, ``ff 00`` at 270, ``ff ff 00`` at 525), each followed by a
      minimum match;
    * ``zero_lit_chain`` — 309 consecutive sequences without literals;
    * ``ends_on_match`` — no trailing literals;
    * ``empty`` — no stream at all; ``token_only`` — the stream ``00``."""
    return [(name, *assemble_lz4(seqs, tail, term))
            for name, seqs, tail, term in assembled_specs()]


def far_reach(rung: int) -> Tuple[bytes, bytes, bytes]:
    """-> (stream, raw, bad_stream).  ``rung - 68`` literals, then one
    68-byte match with offset == dpos, the farthest legal reach: it
    reads dst[0], ends on dst[rung - 1] and on the end of the stream.
    ``bad_stream`` has offset == dpos + 1."""
    rng = random.Random(0xFA2 ^ rung)
    stream, raw, marks = assemble_lz4_marks(
        [(rng.randbytes(rung - 68), rung - 68, 68)])
    bad = bytearray(stream)
    bad[marks[0].off:marks[0].off + 2] = (rung - 67).to_bytes(2, "little")
    return stream, raw, bytes(bad)


def small_decode_blocks() -> List[Tuple[str, bytes, bytes]]:
    """Good blocks of at most 448 raw bytes for the slot-reuse launch."""
    rng = random.Random(0x7121)
    return [
        ("tiny5", *assemble_lz4([], rng.randbytes(5))),
        ("small_mix", *assemble_lz4(*_small_mix_spec())),
        ("zero_lit_chain_short",
         *assemble_lz4(*_zero_lit_chain_short_spec())),
        ("ends_on_match", *assemble_lz4(*_ends_on_match_spec())),
        ("empty", b"", b""),
    ]


def _deep_edits(chain: str, seqs, tail, ks
                ) -> List[Tuple[str, bytes, int, int]]:
    stream, raw, marks = assemble_lz4_marks(seqs, tail)
    out = []
    for k in ks:
        m = marks[k]
        tag = "%s_k%d_" % (chain, k)
        zero = bytearray(stream)
        zero[m.off:m.off + 2] = b"\0\0"
        out.append((tag + "off0", bytes(zero), len(raw), ERR_OFFSET))
        far = bytearray(stream)
        far[m.off:m.off + 2] = (m.dpos + 1).to_bytes(2, "little")
        out.append((tag + "off_gt_dpos", bytes(far), len(raw), ERR_OFFSET))
        out.append((tag + "cut_offset", stream[:m.off + 1], len(raw),
                    ERR_TRUNC))
        # the same chain with a 274-byte match (extension ``ff 00``) at
        # k, cut between the two extension bytes
        long_seqs = list(seqs)
        long_seqs[k] = (seqs[k][0], seqs[k][1], 274)
        l_stream, l_raw, l_marks = assemble_lz4_marks(long_seqs, tail)
        assert l_stream[l_marks[k].mext:l_marks[k].mext + 2] == b"\xff\x00"
        out.append((tag + "cut_mlen_ext", l_stream[:l_marks[k].mext + 1],
                    len(l_raw), ERR_TRUNC))
        out.append((tag + "match_over_out", stream, m.dpos + 1,
                    ERR_OVERFLOW))
    out.append((chain + "_mismatch", stream, len(raw) + 1, ERR_MISMATCH))
    assert tail
    out.append((chain + "_lit_over_out", stream, len(raw) - 1,
                ERR_OVERFLOW))
    return out


def deep_malformed_cases() -> List[Tuple[str, bytes, int, int]]:
    """(name, stream, out_len, expected kernel status): one edit at
    sequence k of ``zero_lit_chain`` and of a 211-sequence chain of
    ordinary literal+match sequences, for k in DEEP_K and the last
    sequence, so the error is met after the producer/consumer ring has
    filled (k = 63, 64, 65) or wrapped several times (last).  Codes
    follow the check order of lz4_decode.hip: offset TRUNC, match-length
    TRUNC, OFFSET, match OVERFLOW inside the sequence; literal OVERFLOW
    on the final literals; MISMATCH once the whole stream is parsed."""
    out = []
    for chain, (seqs, tail) in (("zero_lit", _zero_lit_chain_spec()),
                                ("ordinary", _ordinary_chain_spec())):
        out += _deep_edits(chain, seqs, tail, DEEP_K + (len(seqs) - 1,))
    return out


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


def _mismatches(names, status, codes):
    return [(n, s, c) for n, s, c in zip(names, status, codes) if s != c]


def check_assembled(raw_cap: int, pc: bool) -> None:
    """Every assembled block in one launch: all OK, payloads exact,
    guard bytes intact."""
    blocks = assembled_decode_blocks()
    names = [b[0] for b in blocks]
    streams = [b[1] for b in blocks]
    raws = [b[2] for b in blocks]
    assert any(sum(map(len, streams[:i])) % 16 for i in range(len(streams)))
    status, got, stride = guarded_decode(
        streams, [len(r) for r in raws], raw_cap, pc)
    assert status == [OK] * len(blocks), _mismatches(
        names, status, [OK] * len(blocks))
    check_slots(got, stride, raws)


def check_deep_errors(pc: bool) -> None:
    """good, bad, good, bad, ..., good at raw_cap = 4096 with the deep
    malformed cases: exact codes, never DEADLOCK (6), bad slots
    untouched, good payloads exact."""
    good = assembled_decode_blocks()
    names, streams, out_lens, expect, codes = [], [], [], [], []
    for i, (name, stream, out_len, code) in enumerate(
            deep_malformed_cases()):
        g_name, g_stream, g_raw = good[i % len(good)]
        names += [g_name, name]
        streams += [g_stream, stream]
        out_lens += [len(g_raw), out_len]
        expect += [g_raw, b""]
        codes += [OK, code]
    names.append(good[-1][0])
    streams.append(good[-1][1])
    out_lens.append(len(good[-1][2]))
    expect.append(good[-1][2])
    codes.append(OK)
    status, got, stride = guarded_decode(streams, out_lens, 4096, pc)
    assert 6 not in status, _mismatches(names, status, codes)
    assert status == codes, _mismatches(names, status, codes)
    check_slots(got, stride, expect)


def slot_reuse_launch(grid: int, full_chain: bool):
    """-> (names, streams, out_lens, expected payloads, codes, stride)
    for ``grid + 40`` blocks decoded by ``grid`` workgroups at raw_cap =
    8192: blocks i and i + grid run back to back in one workgroup.  The
    blocks cycle through small_decode_blocks(); six pairs (i, i + grid)
    are a deep-error block and a good block, a TOOBIG block (out_len =
    8193) and a good block, and a zero-literal chain and a 5-byte
    block, each in both orders.  With ``full_chain`` the chain is
    ``zero_lit_chain`` (four ring wraps) in slots of 4096 + 64 bytes;
    without, its 100-sequence version, the longest that fits the 448
    raw bytes of a 512-byte slot."""
    small = small_decode_blocks()
    by_name = {b[0]: b for b in small}
    n = grid + 40
    entries = [(*small[i % len(small)], None, OK) for i in range(n)]

    def ok(block):
        return (*block, None, OK)

    tiny, good = ok(by_name["tiny5"]), ok(by_name["small_mix"])
    if full_chain:
        chain = ok(("zero_lit_chain",
                    *assemble_lz4(*_zero_lit_chain_spec())))
        stride = slot_stride(4096)
    else:
        chain = ok(by_name["zero_lit_chain_short"])
        stride = 512
    seqs, tail = _zero_lit_chain_short_spec()
    stream, raw, marks = assemble_lz4_marks(seqs, tail)
    bad = bytearray(stream)
    bad[marks[65].off:marks[65].off + 2] = b"\0\0"
    deep = ("deep_off0_k65", bytes(bad), b"", len(raw), ERR_OFFSET)
    toobig = ("toobig", good[1], b"", 8193, ERR_TOOBIG)
    pairs = [(deep, good), (good, deep), (toobig, good), (good, toobig),
             (chain, tiny), (tiny, chain)]
    for i, (first, second) in zip((1, 7, 13, 20, 29, 38), pairs):
        assert i + grid < n
        entries[i], entries[i + grid] = first, second
    names = [e[0] for e in entries]
    streams = [e[1] for e in entries]
    expect = [e[2] for e in entries]
    out_lens = [len(e[2]) if e[3] is None else e[3] for e in entries]
    codes = [e[4] for e in entries]
    assert all(len(p) <= stride - SLOT_SLACK for p in expect)
    return names, streams, out_lens, expect, codes, stride


def check_slot_reuse(grid: int, pc: bool, full_chain: bool) -> None:
    """One launch of slot_reuse_launch: exact status list, exact slots."""
    names, streams, out_lens, expect, codes, stride = slot_reuse_launch(
        grid, full_chain)
    status, got, stride = guarded_decode(streams, out_lens, 8192, pc,
                                         stride=stride)
    assert status == codes, _mismatches(names, status, codes)
    check_slots(got, stride, expect)
