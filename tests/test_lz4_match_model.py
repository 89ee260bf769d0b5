"""CPU pins for tests/lz4_match_model.py and the matcher corpus.

The GPU matcher tests compare both compressor kernels byte for byte
with a Python model of their match policy.  These tests hold the other
end: every corpus case reaches the branch it is named for (asserted on
the models' traces, at the block's own length and as a zero-padded
slot, the two shapes in which the kernels see it), every kept model
stream passes a strict validator and decodes through lz4py, the serial
model equals the native CPU compressor, and the validator rejects what
it claims to reject."""
import functools
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lz4_match_model as model  # noqa: E402
import ops_edge_corpus as corpus  # noqa: E402

from shipyard_amd.data import lz4py  # noqa: E402

RUNGS = corpus.MATCHER_RUNGS


@functools.lru_cache(maxsize=None)
def _run(kind: str, block: bytes):
    trace = {}
    fn = model.greedy_model if kind == "greedy" else model.screen_model
    return fn(block, trace), trace


def _shapes(rung: int):
    """(name, bytes the kernel sees): every case at its own length, and
    every case that is not defined by its length as a padded slot."""
    out = []
    for name, block in corpus.matcher_blocks(rung):
        out.append((name, block))
        if not corpus.is_short_case(name) and len(block) < rung:
            out.append((name, corpus.pad_slot(block, rung)))
    return out


class TestMatcherCorpus:
    def test_names_at_4k(self):
        names = [n for n, _ in corpus.matcher_blocks(4096)]
        assert names == (
            ["residue_%d%d" % (a, b) for a in range(4) for b in range(4)]
            + ["ext_%d_miss" % k for k in (0, 1, 63, 64, 65, 127, 128, 129)]
            + ["ext_%d_limit" % k for k in (3, 63, 64, 65, 127, 128, 129)]
            + ["period_%d" % p for p in (2, 3, 5, 16, 17, 63, 64, 65)]
            + ["collide", "reprime_only", "fit_m1", "fit_0", "fit_p1"]
            + ["tail_%d" % n for n in range(1, 15)]
            + ["lane_0", "lane_63", "last_lane_mflimit", "two_dry_then_hit",
               "two_hits", "batch_blind", "dry_exit", "zeros_full",
               "far_0", "far_1", "far_4", "drop_at_token", "drop_at_litlen",
               "drop_at_literals", "drop_at_offset", "full_minus_1",
               "full_exact"])

    @pytest.mark.parametrize("rung", RUNGS[1:])
    def test_names_above_4k(self, rung):
        assert [n for n, _ in corpus.matcher_blocks(rung)] == [
            "zeros_full", "far_0", "far_1", "far_4", "drop_at_token",
            "drop_at_litlen", "drop_at_literals", "drop_at_offset",
            "drop_at_mlen", "full_minus_1", "full_exact"]

    @pytest.mark.parametrize("rung", RUNGS)
    def test_deterministic_and_sized(self, rung):
        a = corpus.matcher_blocks(rung)
        corpus._MATCHER_CACHE.pop(rung)
        assert a == corpus.matcher_blocks(rung)
        assert all(len(b) <= rung for _, b in a)
        names, slots = corpus.matcher_launch(rung)
        assert names[-1] == "full_minus_1" and len(slots[-1]) == rung - 1
        assert all(len(s) == rung for s in slots[:-1])
        assert sorted(names) == sorted(n for n, _ in a)

    @pytest.mark.parametrize("rung", RUNGS)
    def test_every_case_reaches_its_feature(self, rung):
        """At its own length, and for the cases not defined by their
        length also as the zero-padded slot of the wrapper launch."""
        checked = 0
        for name, seen in _shapes(rung):
            reaches = corpus.matcher_feature(name)
            if reaches is None:
                assert name.startswith(("zeros_full", "tail_", "full_"))
                continue
            assert reaches(seen), (name, len(seen))
            checked += 1
        # 58 cases with a trace feature at 4 KiB, 39 of them again as a
        # padded slot; far_<d> and drop_at_<step> above
        assert checked == (97 if rung == 4096 else 8)

    def test_residues_and_extensions(self):
        for name, seen in _shapes(4096):
            if name.startswith("residue_"):
                for kind in ("greedy", "screen"):
                    m = _run(kind, seen)[1]["matches"][0]
                    assert (m["pos"] % 4, m["src"] % 4) == (
                        int(name[8]), int(name[9])), (name, kind)
            if name.startswith("ext_"):
                k, end = int(name.split("_")[1]), name.split("_")[2]
                for kind in ("greedy", "screen"):
                    hits = [m for m in _run(kind, seen)[1]["matches"]
                            if m["mlen"] == k + 4 and m["end"] == end]
                    assert hits, (name, kind)
                    if end == "limit":
                        assert hits[0]["pos"] + k + 4 == len(seen) - 5
        # ext_3_limit starts on mflimit; ext_64_limit leaves one full
        # ballot round behind it
        blocks = dict(corpus.matcher_blocks(4096))
        m = _run("screen", blocks["ext_3_limit"])[1]["matches"][-1]
        assert m["pos"] == 4096 - 12 and m["mlen"] == 7
        m = _run("greedy", blocks["ext_64_limit"])[1]["matches"][-1]
        assert m["mlen"] - 4 == 64 and m["end"] == "limit"

    @pytest.mark.parametrize("rung", RUNGS)
    def test_zeros_full(self, rung):
        block = dict(corpus.matcher_blocks(rung))["zeros_full"]
        assert block == b"\0" * rung
        for kind, lits in (("greedy", 1), ("screen", 64)):
            stream, trace = _run(kind, block)
            (m,) = trace["matches"]
            assert (m["litlen"], m["offset"], m["end"]) == (lits, 1, "limit")
            assert m["pos"] + m["mlen"] == rung - 5
            first = corpus.parse_sequences(stream)[0]
            assert first["match_len"] == rung - 5 - lits
            if rung == 65536:
                assert len(first["match_ext"]) == 257

    @pytest.mark.parametrize("rung", RUNGS)
    @pytest.mark.parametrize("d", corpus.FAR_D)
    def test_far_offsets(self, rung, d):
        block = dict(corpus.matcher_blocks(rung))["far_%d" % d]
        assert len(block) == rung and len(set(block[-5:])) == 5
        for kind in ("greedy", "screen"):
            stream, trace = _run(kind, block)
            last = corpus.parse_sequences(stream)[-2:]
            assert last[0]["offset"] == rung - 12 - d
            assert last[0]["lit_len"] == 0
            assert trace["matches"][-1]["pos"] == rung - 12 - d
            if d == 0:
                # starts exactly on mflimit, stopped by match_limit
                assert last[0]["match_len"] == 7
                assert last[1]["lit_len"] == 5
                assert trace["matches"][-1]["end"] == "limit"
        if rung == 65536:
            assert rung - 12 - d == {0: 65524, 1: 65523, 4: 65520}[d]

    def test_collide(self):
        block = dict(corpus.matcher_blocks(4096))["collide"]
        a, b = block[8:12], block[72:76]
        assert a != b and block[136:140] == a
        assert model.hash4(int.from_bytes(a, "little")) == \
            model.hash4(int.from_bytes(b, "little"))
        for kind in ("greedy", "screen"):
            trace = _run(kind, block)[1]
            assert (72, 8) in trace["collisions"], kind
            assert (136, 72) in trace["collisions"], kind
            assert 136 not in {m["pos"] for m in trace["matches"]}, kind

    def test_reprime_only(self):
        block = dict(corpus.matcher_blocks(4096))["reprime_only"]
        for kind in ("greedy", "screen"):
            hits = [m for m in _run(kind, block)[1]["matches"]
                    if m["via_reprime"]]
            assert hits, kind
            first = _run(kind, block)[1]["matches"][0]
            # the source is two bytes in front of the first match's end
            assert hits[0]["src"] == first["pos"] + first["mlen"] - 2

    def test_exact_fit(self):
        blocks = dict(corpus.matcher_blocks(4096))
        for name, delta in (("fit_m1", -1), ("fit_0", 0), ("fit_p1", 1)):
            block = blocks[name]
            assert 40 <= len(block) <= 120
            for fn in (model.greedy_model, model.screen_model):
                kept = fn(block, keep_all=True)
                assert len(kept) == len(block) + delta, name
                assert lz4py.decompress_block(kept, len(block)) == block
                got = fn(block)
                if delta < 0:
                    assert got == kept
                else:
                    assert got is None

    @pytest.mark.parametrize("rung", RUNGS)
    def test_drop_steps(self, rung):
        blocks = dict(corpus.matcher_blocks(rung))
        steps = [s for s in model.DROP_STEPS
                 if s != "mlen" or rung >= 8192]
        assert corpus.DROP_STEPS == model.DROP_STEPS
        for step in steps:
            for kind in ("greedy", "screen"):
                stream, trace = _run(kind, blocks["drop_at_" + step])
                assert stream is None and trace["drop"] == step
        if rung == 4096:
            assert "drop_at_mlen" not in blocks

    def test_tails_and_full_blocks(self):
        for rung in RUNGS:
            blocks = dict(corpus.matcher_blocks(rung))
            assert len(blocks["full_minus_1"]) == rung - 1
            assert len(blocks["full_exact"]) == rung
            for name in ("full_minus_1", "full_exact"):
                for kind in ("greedy", "screen"):
                    assert _run(kind, blocks[name])[0] is not None
        blocks = dict(corpus.matcher_blocks(4096))
        for n in range(1, 15):
            block = blocks["tail_%d" % n]
            assert block == b"\x07" * n
            got = _run("greedy", block)[0]
            assert (got is None) == (n < 13)
            # one screen round against an empty table: literals only
            assert _run("screen", block)[0] is None

    def test_screen_cases(self):
        blocks = dict(corpus.matcher_blocks(4096))

        def rounds(name):
            return _run("screen", blocks[name])[1]["rounds"]

        def matches(name):
            return _run("screen", blocks[name])[1]["matches"]

        assert (matches("lane_0")[0]["lane"],
                matches("lane_63")[0]["lane"]) == (0, 63)
        m = matches("last_lane_mflimit")[-1]
        assert m["pos"] == 4096 - 12 and m["lane"] == m["in_range"] - 1
        assert m["in_range"] < 64
        assert [r["j"] for r in rounds("two_dry_then_hit")[:3]][:2] == \
            [None, None]
        assert rounds("two_dry_then_hit")[2]["j"] is not None
        two = [r for r in rounds("two_hits") if len(r["cands"]) >= 2][0]
        assert two["j"] == two["cands"][0]
        assert two["inserted"] == two["j"] + 1 < two["in_range"]
        # the hits on the second piece (at 150) lose that round and are
        # found again by a later one
        assert two["pos"] + two["cands"][-1] >= 150
        assert [m["pos"] // 10 for m in matches("two_hits")][:2] == [13, 15]
        last = rounds("dry_exit")[-1]
        assert last["j"] is None and last["pos"] <= 4096 - 12 < \
            last["pos"] + 64

    def test_batch_blind_separates_the_policies(self):
        block = dict(corpus.matcher_blocks(4096))["batch_blind"]
        for seen in (block, corpus.pad_slot(block, 4096)):
            g, gt = _run("greedy", seen)
            s, st = _run("screen", seen)
            assert g is not None and s is not None and g != s
            assert 100 in {m["pos"] for m in gt["matches"]}
            assert 100 not in {m["pos"] for m in st["matches"]}
            hit = [m for m in gt["matches"] if m["pos"] == 100][0]
            assert hit["src"] == 70 and 70 // 64 == 100 // 64

    def test_second_trip_launch(self):
        buf, offs, lens, n_blocks = corpus.second_trip_launch()
        assert n_blocks == (1 << 20) + 64 > corpus.SECOND_TRIP_GRID
        assert len(offs) == len(lens) == 61
        assert all(o % 16 == 0 for o in offs)
        assert all(o + n <= len(buf) for o, n in zip(offs, lens))
        assert {0, 12, 13, 48} <= set(lens) and max(lens) == 48
        srcs = [buf[o:o + n] for o, n in zip(offs, lens)]
        assert len(set(srcs)) == 61
        kept48 = [model.greedy_model(s) is not None
                  for s, n in zip(srcs, lens) if n == 48]
        assert True in kept48 and False in kept48
        # the two blocks of a workgroup read different sources
        assert all(w % 61 != (w + corpus.SECOND_TRIP_GRID) % 61
                   for w in range(64))
        assert all(t < 64 for t in corpus.SECOND_TRIP_TOOBIG)
        assert (buf, offs, lens, n_blocks) == corpus.second_trip_launch()


class TestModelStreams:
    @pytest.mark.parametrize("rung", RUNGS)
    def test_kept_streams_are_strictly_valid(self, rung):
        kept = 0
        for name, seen in _shapes(rung):
            for kind in ("greedy", "screen"):
                stream, trace = _run(kind, seen)
                if stream is None:
                    assert trace["drop"] is not None, (name, kind)
                    continue
                assert trace["drop"] is None
                model.check_lz4_block(stream, seen)
                assert lz4py.decompress_block(stream, len(seen)) == seen
                kept += 1
        assert kept >= 12

    def test_keep_all_returns_the_dropped_stream(self):
        rng = random.Random(9)
        block = rng.randbytes(300)
        for fn in (model.greedy_model, model.screen_model):
            assert fn(block) is None
            full = fn(block, keep_all=True)
            assert len(full) == 300 + 1 + 2
            assert lz4py.decompress_block(full, 300) == block


def _native():
    from shipyard_amd import ops

    if not ops.native_compress_available():
        pytest.skip("native ops library not built")
    return ops


class TestGreedyModelEqualsNativeCompressor:
    @pytest.mark.parametrize("rung", RUNGS)
    def test_matcher_corpus(self, rung):
        ops = _native()
        for name, seen in _shapes(rung):
            (got,) = ops.lz4_compress_blocks(seen, rung)
            assert got == _run("greedy", seen)[0], (name, len(seen))

    def test_compress_edge_blocks(self):
        ops = _native()
        for name, data in corpus.compress_edge_blocks(4096):
            got = ops.lz4_compress_blocks(data, 4096)
            want = [_run("greedy", b)[0]
                    for b in corpus.shard_blocks(data, 4096)]
            assert got == want, name

    @pytest.mark.parametrize("rung", RUNGS)
    @pytest.mark.parametrize("seed", [0, 1])
    def test_mixed_content(self, rung, seed):
        ops = _native()
        data = corpus.mixed_content(random.Random(0x6D0DE1 + rung + seed),
                                    3 * rung + 777)
        got = ops.lz4_compress_blocks(data, rung)
        want = [model.greedy_model(b)
                for b in corpus.shard_blocks(data, rung)]
        assert got == want
        assert any(w is not None for w in want)


class TestStrictValidator:
    HEAD = (b"abcdefgh", 8, 40)     # 48 decoded bytes, stream of 12

    def _block(self, lits, mlen, tail):
        return corpus.assemble_lz4_marks(
            [self.HEAD, (lits, 10, mlen)], tail)

    def test_accepts_the_limits(self):
        # the last match starts on n - 12 and ends on n - 5
        stream, raw, _ = self._block(b"xy", 7, b"vwxyz")
        assert len(raw) == 62
        model.check_lz4_block(stream, raw)

    def test_rejects_match_start_at_n_minus_11(self):
        stream, raw, marks = self._block(b"xy", 6, b"vwxyz")
        assert marks[1].dpos == len(raw) - 11
        assert lz4py.decompress_block(stream, len(raw)) == raw
        with pytest.raises(ValueError, match="starts at 50"):
            model.check_lz4_block(stream, raw)

    def test_rejects_match_end_at_n_minus_4(self):
        stream, raw, marks = self._block(b"xy", 9, b"wxyz")
        assert marks[1].dpos + 9 == len(raw) - 4
        assert marks[1].dpos <= len(raw) - 12
        assert lz4py.decompress_block(stream, len(raw)) == raw
        with pytest.raises(ValueError, match="ends at 59"):
            model.check_lz4_block(stream, raw)

    def test_rejects_offset_0(self):
        stream, raw, marks = self._block(b"xy", 7, b"vwxyz")
        bad = bytearray(stream)
        bad[marks[1].off:marks[1].off + 2] = b"\0\0"
        with pytest.raises(ValueError, match="offset 0"):
            model.check_lz4_block(bytes(bad), raw)

    def test_rejects_offset_beyond_the_prefix(self):
        stream, raw, marks = self._block(b"xy", 7, b"vwxyz")
        bad = bytearray(stream)
        bad[marks[1].off:marks[1].off + 2] = (51).to_bytes(2, "little")
        with pytest.raises(ValueError, match="reaches before"):
            model.check_lz4_block(bytes(bad), raw)

    def test_rejects_stream_that_ends_on_a_match(self):
        stream, raw, _ = corpus.assemble_lz4_marks(
            [self.HEAD, (b"xy", 10, 7)])
        assert lz4py.decompress_block(stream, len(raw)) == raw
        with pytest.raises(ValueError, match="not literals only"):
            model.check_lz4_block(stream, raw)

    def test_rejects_wrong_bytes_and_no_gain(self):
        stream, raw, _ = self._block(b"xy", 7, b"vwxyz")
        with pytest.raises(ValueError, match="differ from raw"):
            model.check_lz4_block(stream, raw[:-1] + b"!")
        lits = b"0123456789abcdef"
        with pytest.raises(ValueError, match="not shorter"):
            model.check_lz4_block(bytes([0xF0, 1]) + lits, lits)
