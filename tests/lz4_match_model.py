"""Python models of the two GPU LZ4 match policies, and a strict block
validator.

A plain helper module (not a conftest).  Written from the comments and
code of ``lz4_compress_kernel`` and ``lz4_compress_screen_kernel`` in
``shipyard_amd/ops/csrc/lz4_compress_gpu.hip``; it shares no code with
``lz4py.compress_block``, whose dict-of-4-grams matcher follows another
policy.  Both kernels are deterministic, so each model predicts its
kernel's stream byte for byte.

Shared by both policies
    * 4096-entry table, ``hash4(v) = (v * 2654435761 mod 2**32) >> 20``
      over the little-endian 4-gram at a position; entries are
      ``pos + 1``, 0 means empty.
    * ``mflimit = n - 12``: the last position that is scanned or may
      start a match.  ``match_limit = n - 5``: a match never covers
      ``src[match_limit]`` or anything behind it.  Blocks under 13
      bytes are literals only.
    * Emission is capped at ``cap = n``: the first byte that would land
      at ``opos >= n`` drops the block, as does a stream of exactly
      ``n`` bytes.  A dropped block is ``None`` (length 0 on the GPU).

Serial policy (``greedy_model``)
    Every scanned position reads the table, then overwrites the entry
    with itself.  A hit needs ``ref - 1 < pos``, distance <= 65535 and
    equal 4-grams.  After a match of ``mlen`` bytes ``pos += mlen`` and,
    if ``pos <= mflimit``, position ``pos - 2`` is inserted (the
    reprime).

Wave-screen policy (``screen_model``)
    A round looks at positions ``pos + lane`` for lanes 0..63 that are
    ``<= mflimit``, all against the table as it stood before the round.
    ``j`` is the first lane with a hit (``ref - 1 < p`` and equal
    4-grams).  Lanes ``<= j`` insert ``max(old, p + 1)``; without a hit
    every in-range lane inserts and ``pos += 64``.  A hit is taken at
    ``pos + j`` from lane ``j``'s ``ref``; the reprime is ``max(old,
    pos - 1)`` at the hash of ``pos - 2``.

``trace``, a dict, receives:
    ``matches``     one dict per match: ``pos``, ``src``, ``pos_mod4``,
                    ``src_mod4``, ``offset``, ``mlen``, ``litlen``,
                    ``end`` ("miss" or "limit"), ``via_reprime``, and
                    for the screen ``lane`` and ``in_range``;
    ``collisions``  (pos, ref position) of table probes that passed the
                    position test but held a different 4-gram; the
                    screen lists those of lanes below ``j`` (or of every
                    in-range lane of a dry round);
    ``rounds``      screen only: ``pos``, ``in_range``, ``cands`` (all
                    lanes with a hit), ``j`` (None for a dry round),
                    ``inserted`` (number of lanes that inserted);
    ``drop``        None for a kept block, else the emit step at which
                    ``opos`` would pass ``cap``: "token", "litlen",
                    "literals", "offset" or "mlen"; "size" when every
                    byte fitted but the stream is exactly ``n`` bytes.
"""
from __future__ import annotations

HASH_SLOTS = 4096
WAVE = 64
DROP_STEPS = ("token", "litlen", "literals", "offset", "mlen")


def hash4(v: int) -> int:
    return ((v * 2654435761) & 0xFFFFFFFF) >> 20


def rd32(block: bytes, pos: int) -> int:
    return int.from_bytes(block[pos:pos + 4], "little")


class _Dropped(Exception):
    pass


class _Emitter:
    """The kernels' emit_byte / emit_len / emit_literals / emit_seq with
    their bounds checks in the kernels' order."""

    def __init__(self, block: bytes, cap):
        self.block = block
        self.cap = cap          # None: keep_all, nothing is dropped
        self.out = bytearray()
        self.drop = None

    def _byte(self, b: int, step: str) -> None:
        if self.cap is not None and len(self.out) >= self.cap:
            self.drop = step
            raise _Dropped()
        self.out.append(b)

    def _len(self, value: int, step: str) -> None:
        while value >= 255:
            self._byte(255, step)
            value -= 255
        self._byte(value, step)

    def seq(self, anchor: int, lit_end: int, offset: int, mlen: int) -> None:
        litlen = lit_end - anchor
        ml = mlen - 4 if mlen else 0
        self._byte((min(litlen, 15) << 4) | min(ml, 15), "token")
        if litlen >= 15:
            self._len(litlen - 15, "litlen")
        if self.cap is not None and len(self.out) + litlen > self.cap:
            self.drop = "literals"
            raise _Dropped()
        self.out += self.block[anchor:lit_end]
        if mlen == 0:
            return
        self._byte(offset & 0xFF, "offset")
        self._byte(offset >> 8, "offset")
        if ml >= 15:
            self._len(ml - 15, "mlen")


def _extend(block: bytes, r: int, pos: int, match_limit: int):
    mlen = 4
    while pos + mlen < match_limit and block[r + mlen] == block[pos + mlen]:
        mlen += 1
    return mlen, ("limit" if pos + mlen >= match_limit else "miss")


def _finish(em: _Emitter, n: int, trace, keep_all: bool):
    if trace is not None:
        trace["drop"] = em.drop
    if em.drop is not None:
        return None
    if not keep_all and len(em.out) >= n:
        if trace is not None:
            trace["drop"] = "size"
        return None
    return bytes(em.out)


def _new_trace(trace, screen: bool) -> None:
    if trace is None:
        return
    trace.clear()
    trace.update(matches=[], collisions=[], drop=None)
    if screen:
        trace["rounds"] = []


def greedy_model(block: bytes, trace=None, keep_all: bool = False):
    """The stream of lz4_compress_kernel (and of lz4_compress.cpp) for
    one block, or None where the block is dropped."""
    block = bytes(block)
    n = len(block)
    _new_trace(trace, False)
    em = _Emitter(block, None if keep_all else n)
    try:
        if n >= 13:
            table = [0] * HASH_SLOTS
            primed = [False] * HASH_SLOTS   # entry written by a reprime
            mflimit, match_limit = n - 12, n - 5
            anchor = pos = 0
            while pos <= mflimit:
                v = rd32(block, pos)
                h = hash4(v)
                ref, via = table[h], primed[h]
                table[h], primed[h] = (pos + 1) & 0xFFFF, False
                hit = False
                if ref != 0 and ref - 1 < pos and pos - (ref - 1) <= 65535:
                    if rd32(block, ref - 1) == v:
                        hit = True
                    elif trace is not None:
                        trace["collisions"].append((pos, ref - 1))
                if not hit:
                    pos += 1
                    continue
                r = ref - 1
                mlen, end = _extend(block, r, pos, match_limit)
                if trace is not None:
                    trace["matches"].append(dict(
                        pos=pos, src=r, pos_mod4=pos % 4, src_mod4=r % 4,
                        offset=pos - r, mlen=mlen, litlen=pos - anchor,
                        end=end, via_reprime=via))
                em.seq(anchor, pos, pos - r, mlen)
                pos += mlen
                anchor = pos
                if pos <= mflimit:
                    h = hash4(rd32(block, pos - 2))
                    table[h], primed[h] = (pos - 1) & 0xFFFF, True
            em.seq(anchor, n, 0, 0)
        else:
            em.seq(0, n, 0, 0)
    except _Dropped:
        pass
    return _finish(em, n, trace, keep_all)


def screen_model(block: bytes, trace=None, keep_all: bool = False):
    """The stream of lz4_compress_screen_kernel for one block, or None
    where the block is dropped."""
    block = bytes(block)
    n = len(block)
    _new_trace(trace, True)
    em = _Emitter(block, None if keep_all else n)
    try:
        if n >= 13:
            table = [0] * HASH_SLOTS
            primed = [False] * HASH_SLOTS
            mflimit, match_limit = n - 12, n - 5
            anchor = pos = 0
            while pos <= mflimit:
                # every lane reads the table before any lane inserts
                lanes = []          # (p, h, ref, cand)
                bumps = []          # collisions, by lane
                for lane in range(WAVE):
                    p = pos + lane
                    if p > mflimit:
                        break
                    v = rd32(block, p)
                    h = hash4(v)
                    ref = table[h]
                    cand = False
                    if ref != 0 and ref - 1 < p:
                        if rd32(block, ref - 1) == v:
                            cand = True
                        else:
                            bumps.append((lane, p, ref - 1))
                    lanes.append((p, h, ref, cand))
                cands = [i for i, rec in enumerate(lanes) if rec[3]]
                j = cands[0] if cands else WAVE
                via = primed[lanes[j][1]] if cands else False
                inserted = 0
                for lane, (p, h, _, _) in enumerate(lanes):
                    if lane > j:
                        break
                    inserted += 1
                    if p + 1 > table[h]:
                        table[h], primed[h] = p + 1, False
                if trace is not None:
                    trace["rounds"].append(dict(
                        pos=pos, in_range=len(lanes), cands=cands,
                        j=j if cands else None, inserted=inserted))
                    trace["collisions"] += [
                        (p, r) for lane, p, r in bumps if lane < j]
                if not cands:
                    pos += WAVE
                    continue
                pstar = pos + j
                rstar = lanes[j][2] - 1
                mlen, end = _extend(block, rstar, pstar, match_limit)
                if trace is not None:
                    trace["matches"].append(dict(
                        pos=pstar, src=rstar, pos_mod4=pstar % 4,
                        src_mod4=rstar % 4, offset=pstar - rstar,
                        mlen=mlen, litlen=pstar - anchor, end=end,
                        via_reprime=via, lane=j, in_range=len(lanes)))
                em.seq(anchor, pstar, pstar - rstar, mlen)
                pos = pstar + mlen
                anchor = pos
                if pos <= mflimit:
                    h = hash4(rd32(block, pos - 2))
                    if pos - 1 > table[h]:
                        table[h], primed[h] = pos - 1, True
            em.seq(anchor, n, 0, 0)
        else:
            em.seq(0, n, 0, 0)
    except _Dropped:
        pass
    return _finish(em, n, trace, keep_all)


def check_lz4_block(stream: bytes, raw: bytes) -> None:
    """Strict validation of a kept compressor stream; ValueError names
    the first broken rule.  Beyond decoding to ``raw``: every offset is
    1..65535 and reaches no further back than the decoded prefix, every
    match has at least 4 bytes, the last sequence is literals only, for
    ``len(raw) >= 13`` the last match starts at or before ``n - 12`` and
    ends at or before ``n - 5``, and the stream is shorter than ``raw``.
    """
    stream, raw = bytes(stream), bytes(raw)
    n, slen = len(raw), len(stream)
    if slen >= n:
        raise ValueError("stream of %d bytes is not shorter than raw %d"
                         % (slen, n))
    out = bytearray()
    spos = 0
    last_match = None       # (start, end) in decoded positions
    ended_on_literals = False
    while spos < slen:
        token = stream[spos]
        spos += 1
        run = token >> 4
        if run == 15:
            while True:
                if spos >= slen:
                    raise ValueError("truncated literal length")
                b = stream[spos]
                spos += 1
                run += b
                if b != 255:
                    break
        if spos + run > slen:
            raise ValueError("literals run past the stream")
        out += stream[spos:spos + run]
        spos += run
        if spos == slen:
            ended_on_literals = True
            break
        if spos + 2 > slen:
            raise ValueError("truncated offset")
        offset = stream[spos] | (stream[spos + 1] << 8)
        spos += 2
        if not 1 <= offset <= 65535:
            raise ValueError("offset %d out of 1..65535" % offset)
        if offset > len(out):
            raise ValueError("offset %d reaches before the block (dpos %d)"
                             % (offset, len(out)))
        mlen = (token & 15) + 4
        if token & 15 == 15:
            while True:
                if spos >= slen:
                    raise ValueError("truncated match length")
                b = stream[spos]
                spos += 1
                mlen += b
                if b != 255:
                    break
        if mlen < 4:
            raise ValueError("match of %d bytes" % mlen)
        start = len(out)
        for _ in range(mlen):
            out.append(out[-offset])
        last_match = (start, start + mlen)
    if not ended_on_literals:
        raise ValueError("the last sequence is not literals only")
    if bytes(out) != raw:
        raise ValueError("decodes to %d bytes that differ from raw (%d)"
                         % (len(out), n))
    if last_match is not None:
        if n < 13:
            raise ValueError("match in a block of %d bytes" % n)
        if last_match[0] > n - 12:
            raise ValueError("last match starts at %d, behind n - 12 = %d"
                             % (last_match[0], n - 12))
        if last_match[1] > n - 5:
            raise ValueError("last match ends at %d, behind n - 5 = %d"
                             % (last_match[1], n - 5))
