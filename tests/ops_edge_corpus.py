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


# --------------------------------------------------------- matcher corpora
# Blocks built for single branches of lz4_compress_kernel and
# lz4_compress_screen_kernel.  Every builder draws seeded candidates and
# keeps the first one whose model trace (lz4_match_model) shows the
# feature for BOTH policies, so a table entry lost to a chance hash
# collision in the filler cannot hollow a case out; MATCHER_FEATURES
# holds the same predicates for the CPU pins.
MATCHER_RUNGS = (4096, 8192, 16384, 32768, 65536)
EXT_MISS_K = (0, 1, 63, 64, 65, 127, 128, 129)
# A match that ends on match_limit = n - 5 starts at or before
# mflimit = n - 12, so it has at least 7 bytes: k = mlen - 4 = 3 is the
# smallest case that exists (the match starts exactly at mflimit).
EXT_LIMIT_K = (3, 63, 64, 65, 127, 128, 129)
PERIODS = (2, 3, 5, 16, 17, 63, 64, 65)
FAR_D = (0, 1, 4)
DROP_STEPS = ("token", "litlen", "literals", "offset", "mlen")
# Cases whose feature depends on the block's own length: it is lost when
# the block is zero-padded to a slot, and holds where the kernel is
# given the true length (a direct launch, or the last block of a
# wrapper launch).
SHORT_PREFIXES = ("fit_", "drop_at_", "tail_", "full_minus_1")


def is_short_case(name: str) -> bool:
    return name.startswith(SHORT_PREFIXES)


def pad_slot(block: bytes, rung: int) -> bytes:
    assert len(block) <= rung
    return block + b"\0" * (rung - len(block))


def _traces(block: bytes, keep_all: bool = False):
    """-> ((greedy stream, trace), (screen stream, trace))"""
    import lz4_match_model as model

    gt, st = {}, {}
    g = model.greedy_model(block, gt, keep_all=keep_all)
    s = model.screen_model(block, st, keep_all=keep_all)
    return (g, gt), (s, st)


def _both(block: bytes, pred) -> bool:
    (_, gt), (_, st) = _traces(block)
    return pred(gt) and pred(st)


def _any_match(**want):
    def pred(trace):
        return any(all(m.get(k) == v for k, v in want.items())
                   for m in trace["matches"])
    return pred


def _feat_period(period: int):
    def pred(trace):
        m = trace["matches"]
        return bool(m) and m[0]["offset"] == period < m[0]["mlen"]
    return pred


def _feat_far(n: int, d: int):
    def pred(trace):
        m = trace["matches"]
        return bool(m) and (m[-1]["pos"], m[-1]["offset"]) == (
            n - 12 - d, n - 12 - d)
    return pred


def _feat_collide(trace) -> bool:
    # A ... B ... A: B probes A's entry, the second A probes B's, both
    # are rejected by the compare and the second A starts no match
    seen = trace["collisions"]
    chain = [(p2, r2) for p1, r1 in seen for p2, r2 in seen if r2 == p1]
    starts = {m["pos"] for m in trace["matches"]}
    return any(p2 not in starts for p2, _ in chain)


def _feat_screen_rounds(check):
    def pred(block: bytes) -> bool:
        (_, _), (_, st) = _traces(block)
        return check(st, len(block))
    return pred


def _feat_two_hits(st, n) -> bool:
    return any(len(r["cands"]) >= 2 and
               r["inserted"] == r["j"] + 1 < r["in_range"]
               for r in st["rounds"])


def _feat_last_lane(st, n) -> bool:
    return any(m["pos"] == n - 12 and m["lane"] == m["in_range"] - 1 < 63
               for m in st["matches"])


def _feat_dry_exit(st, n) -> bool:
    last = st["rounds"][-1]
    return (bool(st["matches"]) and st["drop"] is None and
            last["j"] is None and last["pos"] + 64 > n - 12 >= last["pos"])


def _feat_two_dry(st, n) -> bool:
    js = [r["j"] for r in st["rounds"][:3]]
    return len(js) == 3 and js[0] is None and js[1] is None and \
        js[2] is not None


def _feat_batch_blind(block: bytes) -> bool:
    (g, gt), (s, st) = _traces(block)
    blind = {m["pos"] for m in gt["matches"]} - \
        {m["pos"] for m in st["matches"]}
    # the match only the serial policy sees has its source in the same
    # 64-position round
    return g != s and bool(blind) and any(
        m["pos"] in blind and m["pos"] // 64 == m["src"] // 64
        for m in gt["matches"]) and not any(
        r["j"] is not None and r["pos"] <= min(blind) < r["pos"] + 64
        for r in st["rounds"])


def _fit_delta(block: bytes):
    (g, _), (s, _) = _traces(block, keep_all=True)
    return len(g) - len(block), len(s) - len(block)


def matcher_feature(name: str):
    """-> predicate(block) -> bool: the block reaches the feature the
    case ``name`` stands for, under both match models unless the case
    is about one of them.  None for cases defined by their size alone
    (``zeros_full``, ``tail_<n>``, ``full_*``), which the pins check
    directly."""
    def both(pred):
        return lambda block: _both(block, pred)

    if name.startswith("residue_"):
        return both(_any_match(pos_mod4=int(name[8]), src_mod4=int(name[9])))
    if name.startswith("ext_"):
        _, k, end = name.split("_")
        return both(_any_match(mlen=int(k) + 4, end=end))
    if name.startswith("period_"):
        return both(_feat_period(int(name[7:])))
    if name.startswith("far_"):
        return lambda block: _both(block, _feat_far(len(block),
                                                    int(name[4:])))
    if name == "collide":
        return both(_feat_collide)
    if name == "reprime_only":
        return both(_any_match(via_reprime=True))
    if name.startswith("fit_"):
        delta = {"m1": -1, "0": 0, "p1": 1}[name[4:]]
        return lambda block: 40 <= len(block) <= 120 and \
            _fit_delta(block) == (delta, delta)
    if name.startswith("drop_at_"):
        step = name[8:]
        return both(lambda trace: trace["drop"] == step)
    if name in ("lane_0", "lane_63"):
        lane = int(name[5:])
        return _feat_screen_rounds(lambda st, n: any(
            m["lane"] == lane and m["in_range"] == 64
            for m in st["matches"]))
    return {
        "last_lane_mflimit": _feat_screen_rounds(_feat_last_lane),
        "two_dry_then_hit": _feat_screen_rounds(_feat_two_dry),
        "two_hits": _feat_screen_rounds(_feat_two_hits),
        "batch_blind": _feat_batch_blind,
        "dry_exit": _feat_screen_rounds(_feat_dry_exit),
    }.get(name)


def _pick(name: str, seed: int, build, tries: int = 400) -> bytes:
    """First seeded candidate of ``build(rng)`` that reaches the feature
    of ``name``."""
    rng = random.Random(seed)
    reaches = matcher_feature(name)
    for _ in range(tries):
        block = build(rng)
        if block is not None and reaches(block):
            return block
    raise AssertionError("no %s block in %d tries" % (name, tries))


def _pick_kept(seed: int, n: int) -> bytes:
    """Seeded mixed content of ``n`` bytes that both matchers keep."""
    rng = random.Random(seed)
    while True:
        block = mixed_content(rng, n)
        (g, _), (s, _) = _traces(block)
        if g is not None and s is not None:
            return block


def _repeat_block(rng, src_at: int, pos: int, piece: bytes, n: int = None
                  ) -> bytes:
    """Random filler with ``piece`` at ``src_at`` and again at ``pos``;
    the byte behind each copy differs.  Without ``n`` a 128-byte run
    and 16 filler bytes follow the second copy, so the block is kept;
    with ``n`` the filler in front of the first copy starts with
    zeros for the same reason, where there is room."""
    if n is None:
        n = pos + len(piece) + 160
        buf = bytearray(rng.randbytes(n))
        buf[n - 144:n - 16] = b"\xEE" * 128
    else:
        buf = bytearray(rng.randbytes(n))
        if src_at > 256:
            buf[:src_at - 128] = bytes(src_at - 128)
    buf[src_at:src_at + len(piece)] = piece
    buf[pos:pos + len(piece)] = piece
    if pos + len(piece) < n:
        buf[pos + len(piece)] = buf[src_at + len(piece)] ^ 0x55
    return bytes(buf[:n])


def _residue_block(a: int, b: int):
    return lambda rng: _repeat_block(rng, 4 + b, 128 + a, rng.randbytes(11))


def _ext_miss_block(k: int):
    def build(rng):
        piece = rng.randbytes(4 + k)
        pos = 64 * ((8 + len(piece)) // 64 + 2) + 9
        return _repeat_block(rng, 8, pos, piece)
    return build


def _ext_limit_block(k: int, n: int):
    def build(rng):
        # the copy runs to the end of the block, so only match_limit
        # ends the extension after mlen = 4 + k bytes
        piece = rng.randbytes(4 + k + 5)
        pos = n - len(piece)
        return _repeat_block(rng, pos - len(piece) - 70, pos, piece, n)
    return build


def _period_block(period: int):
    def build(rng):
        pat = bytes(rng.sample(range(256), period))
        body = (pat * (300 // period + 1))[:300]
        return rng.randbytes(8) + body + rng.randbytes(16)
    return build


def _far_block(n: int, d: int):
    def build(rng):
        probe = bytes(rng.sample(range(1, 256), 8))
        buf = bytearray(n)
        buf[:8] = probe
        q = n - 12 - d
        buf[q:q + 8] = probe
        rest = [v for v in range(1, 256) if v not in probe]
        buf[q + 8:] = bytes(rng.sample(rest, n - q - 8))
        assert len(buf) == n and len(set(buf[-5:])) == 5
        return bytes(buf)
    return build


def _collide_block(rng):
    import lz4_match_model as model

    seen = {}
    while True:
        v = rng.getrandbits(32)
        other = seen.setdefault(model.hash4(v), v)
        if other != v:
            break
    a, b = v.to_bytes(4, "little"), other.to_bytes(4, "little")
    buf = bytearray(rng.randbytes(160))
    buf[8:12], buf[72:76], buf[136:140] = a, b, a
    return bytes(buf) + b"\xEE" * 128 + rng.randbytes(16)


def _reprime_block(rng):
    # M ... M[:18] Z ...: the second M is an 18-byte match, the reprime
    # inserts the 4-gram M[16:18] + Z[:2] that lies inside the skipped
    # span; the only later copy of that 4-gram finds it there
    m, z = rng.randbytes(20), rng.randbytes(8)
    tail = m[16:18] + z
    return (rng.randbytes(8) + m + rng.randbytes(56) + m[:18] + z +
            rng.randbytes(70) + tail + rng.randbytes(16))


def _fit_block(rng):
    # 64..90 literals, a match of 4..6 bytes from the block's start, a
    # final run below 15 bytes: token + extension byte + offset + final
    # token cost 5 bytes against the 4..6 the match saves
    lits, mlen, rest = rng.randint(64, 90), rng.randint(4, 6), \
        rng.randint(8, 14)
    return _repeat_block(rng, 0, lits, rng.randbytes(mlen),
                         lits + mlen + rest)


def _drop_block(step: str, rung: int):
    """One literal run long enough that its length-extension bytes push
    ``opos`` to ``cap`` at the named step of the match sequence (or of
    the final literals) behind it."""
    if step == "literals":
        return lambda rng: rng.randbytes(100)
    mlen, rest = {"token": (4, 8), "litlen": (4, 15), "offset": (4, 8),
                  "mlen": (19, 5)}[step]

    def build(rng):
        lits = 15 + 255 * rng.randint(0, 21)
        n = lits + mlen + rest
        if n > rung:
            return None
        return _repeat_block(rng, 0, lits, rng.randbytes(mlen), n)
    return build


def _last_lane_block(n: int):
    def build(rng):
        piece = rng.randbytes(12)
        return _repeat_block(rng, n - 12 - 100, n - 12, piece, n)
    return build


def _two_hits_block(rng):
    buf = bytearray(rng.randbytes(190))
    p1, p2 = rng.randbytes(12), rng.randbytes(12)
    buf[8:20], buf[24:36] = p1, p2
    buf[130:142], buf[150:162] = p1, p2
    return bytes(buf)


def _batch_blind_block(rng):
    buf = bytearray(rng.randbytes(200))
    buf[100:112] = buf[70:82]
    return bytes(buf) + b"\xEE" * 128 + rng.randbytes(16)


def _dry_exit_block(n: int):
    return lambda rng: b"\0" * (n - 196) + rng.randbytes(196)


_MATCHER_CACHE = {}


def matcher_blocks(rung: int) -> List[Tuple[str, bytes]]:
    """(name, block) inputs for both GPU matchers, each block at most
    ``rung`` bytes.  Cases that need no size exist at the 4 KiB rung
    only; ``zeros_full``, ``far_<d>``, ``drop_at_<step>``,
    ``full_minus_1`` and ``full_exact`` at every rung (``drop_at_mlen``
    needs 5.1 KiB of literals, so from 8 KiB up).

    Both matchers
    * ``residue_<a><b>`` — a match at pos % 4 == a from r % 4 == b;
    * ``ext_<k>_miss`` / ``ext_<k>_limit`` — a match of 4 + k bytes
      ended by a differing byte / by match_limit (block of ``rung``
      bytes, the copy runs to its end);
    * ``zeros_full`` — ``rung`` zero bytes;
    * ``period_<P>`` — 300 bytes of period P behind 8 random bytes;
    * ``far_<d>`` — probe at 0, zeros, the probe again at n - 12 - d;
    * ``collide`` — A ... B ... A with hash4(A) == hash4(B);
    * ``reprime_only`` — a match whose table entry only the reprime
      wrote;
    * ``fit_m1`` / ``fit_0`` / ``fit_p1`` — 40..120 bytes, the stream of
      either matcher is n - 1 / n / n + 1 bytes;
    * ``drop_at_<step>`` — dropped at that emit step;
    * ``tail_<n>`` — n equal bytes, n in 1..14;
    * ``full_minus_1`` / ``full_exact`` — rung - 1 / rung mixed bytes.

    Screen matcher (the serial model runs on them too)
    * ``lane_0`` / ``lane_63`` — the hit lane of a full round;
    * ``last_lane_mflimit`` — hit at p == mflimit, the last in-range
      lane of a partial round;
    * ``two_dry_then_hit``, ``two_hits`` (the first wins, lanes above it
      do not insert), ``batch_blind`` (the only source lies in the same
      round: the two policies differ), ``dry_exit`` (a dry round
      carries pos past mflimit)."""
    if rung in _MATCHER_CACHE:
        return list(_MATCHER_CACHE[rung])
    assert rung in MATCHER_RUNGS
    seed = 0x3A7C0 ^ rung
    out: List[Tuple[str, bytes]] = []

    def add(name, build):
        out.append((name, _pick(name, seed + len(out), build)))

    if rung == 4096:
        for a in range(4):
            for b in range(4):
                add("residue_%d%d" % (a, b), _residue_block(a, b))
        for k in EXT_MISS_K:
            add("ext_%d_miss" % k, _ext_miss_block(k))
        for k in EXT_LIMIT_K:
            add("ext_%d_limit" % k, _ext_limit_block(k, rung))
        for period in PERIODS:
            add("period_%d" % period, _period_block(period))
        add("collide", _collide_block)
        add("reprime_only", _reprime_block)
        for name in ("fit_m1", "fit_0", "fit_p1"):
            out.append((name, _pick(name, seed + len(out), _fit_block,
                                    tries=4000)))
        for n in range(1, 15):
            out.append(("tail_%d" % n, b"\x07" * n))
        add("lane_0", lambda rng: _repeat_block(rng, 8, 128,
                                                rng.randbytes(12), 220))
        add("lane_63", lambda rng: _repeat_block(rng, 8, 191,
                                                 rng.randbytes(12)))
        add("last_lane_mflimit", _last_lane_block(rung))
        add("two_dry_then_hit", lambda rng: _repeat_block(
            rng, 8, 133, rng.randbytes(12)))
        add("two_hits", _two_hits_block)
        add("batch_blind", _batch_blind_block)
        add("dry_exit", _dry_exit_block(rung))
    out.append(("zeros_full", b"\0" * rung))
    for d in FAR_D:
        add("far_%d" % d, _far_block(rung, d))
    for step in DROP_STEPS:
        if step != "mlen" or rung >= 8192:
            add("drop_at_" + step, _drop_block(step, rung))
    for name, n in (("full_minus_1", rung - 1), ("full_exact", rung)):
        out.append((name, _pick_kept(seed + len(out), n)))
    assert all(len(b) <= rung for _, b in out)
    _MATCHER_CACHE[rung] = tuple(out)
    return out


def matcher_launch(rung: int) -> Tuple[List[str], List[bytes]]:
    """-> (names, slots): the cases of one rung as the wrapper's single
    launch sees them with ``block_raw = rung``.  Every block is
    zero-padded to its slot except ``full_minus_1``, which goes last and
    stays rung - 1 bytes: the launch's ragged final block."""
    cases = matcher_blocks(rung)
    cases = [c for c in cases if c[0] != "full_minus_1"] + \
        [c for c in cases if c[0] == "full_minus_1"]
    names = [c[0] for c in cases]
    slots = [pad_slot(b, rung) for _, b in cases[:-1]] + [cases[-1][1]]
    return names, slots


SECOND_TRIP_GRID = 1 << 20     # grid cap in compress_blocks
SECOND_TRIP_SOURCES = 61
SECOND_TRIP_TOOBIG = (3, 17, 40, 63)


def second_trip_launch():
    """-> (buffer, src_off, src_len, n_blocks): 61 distinct source
    blocks of 0..48 bytes at 16-byte-aligned offsets of one small
    buffer, for one launch of ``(1 << 20) + 64`` blocks in which block i
    reads source i % 61.  The grid is capped at 1 << 20 workgroups, so
    workgroup w < 64 compresses blocks w and w + (1 << 20), and as 61 is
    odd the two read different sources.  Lengths cover 0, 12, 13 and 48
    bytes; sources 0..2 are 48 equal bytes, a 48-byte period-4 pattern
    (both kept by the serial matcher) and 48 random bytes (dropped)."""
    rng = random.Random(0x2D7219)
    lens = [48, 48, 48, 0, 12, 13] + [
        rng.randint(1, 48) for _ in range(SECOND_TRIP_SOURCES - 6)]
    blocks = []
    for i, n in enumerate(lens):
        if i == 0:
            b = b"\x11" * n
        elif i == 1:
            b = (b"shp4" * 12)[:n]
        elif i % 3 == 2:
            b = rng.randbytes(n)
        elif i % 3 == 0:
            b = bytes([rng.randrange(256)]) * n
        else:
            pat = rng.randbytes(rng.randint(1, 5))
            b = (pat * 48)[:n]
        blocks.append(b)
    assert len(set(blocks)) == len(blocks) == SECOND_TRIP_SOURCES
    buf = bytearray(SECOND_TRIP_SOURCES * 48)
    offs = [48 * i for i in range(SECOND_TRIP_SOURCES)]
    for off, b in zip(offs, blocks):
        buf[off:off + len(b)] = b
    return bytes(buf), offs, lens, SECOND_TRIP_GRID + 64


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
