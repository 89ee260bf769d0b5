"""CPU-side pins for tests/ops_edge_corpus.py.

The GPU edge tests are only as good as their inputs: these tests assert
that every malformed stream really is malformed for the reference
decoder, and that every compressor edge input really produces the
encoding feature it is named for, so the GPU tests cannot silently lose
their edges when a builder or the reference codec changes."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_edge_corpus as corpus  # noqa: E402

from shipyard_amd.data import lz4py  # noqa: E402

BLOCK = 4096


def _edge(name, block_raw=BLOCK):
    data = dict(corpus.compress_edge_blocks(block_raw))[name]
    return data, corpus.final_block(data, block_raw)


class TestMalformedCases:
    def test_names_and_codes_cover_the_table(self):
        cases = corpus.malformed_lz4_cases()
        assert [c[0] for c in cases] == [
            "off0", "off_gt_dpos", "trunc_litlen", "trunc_offset",
            "trunc_mlen", "lit_over_stream", "lit_over_out",
            "match_over_out", "mismatch_short", "toobig"]
        assert {c[3] for c in cases} == {1, 2, 3, 4, 5}

    @pytest.mark.parametrize("raw_cap", [4096, 8192])
    def test_every_case_raises_in_reference(self, raw_cap):
        for name, stream, out_len, _ in corpus.malformed_lz4_cases(raw_cap):
            with pytest.raises(ValueError):
                lz4py.decompress_block(stream, out_len)

    def test_toobig_is_a_valid_block_with_oversized_claim(self):
        name, stream, out_len, code = corpus.malformed_lz4_cases(8192)[-1]
        assert (name, out_len, code) == ("toobig", 8193, 5)
        assert lz4py.decompress_block(stream, 64) == b"shipyard" * 8

    def test_accepted_case_decodes(self):
        _, stream, out_len, want = corpus.accepted_lz4_case()
        assert lz4py.decompress_block(stream, out_len) == want == b"xxxxx"


class TestDecodeFuzzBlocks:
    @pytest.mark.parametrize("raw_cap", [4096, 8192, 16384, 32768, 65536])
    @pytest.mark.parametrize("many_seq", [False, True])
    def test_shape_of_the_block_set(self, raw_cap, many_seq):
        blocks = corpus.decode_fuzz_blocks(raw_cap, 7, many_seq)
        assert len(blocks) == 6
        assert all(0 < len(b) <= raw_cap for b in blocks)
        assert len(blocks[-1]) % 16 != 0
        assert blocks == corpus.decode_fuzz_blocks(raw_cap, 7, many_seq)
        # the random block does not compress: in_len > out_len
        assert len(lz4py.compress_block(blocks[1])) > len(blocks[1])
        if many_seq:
            count = len(corpus.parse_sequences(
                lz4py.compress_block(blocks[4])))
            assert count > 200 and count % 16 != 0

    def test_parse_sequences_agrees_with_decoder(self):
        rng = random.Random(5)
        raw = corpus.mixed_content(rng, 20000)
        seqs = corpus.parse_sequences(lz4py.compress_block(raw))
        assert sum(s["lit_len"] + (s["match_len"] or 0)
                   for s in seqs) == len(raw)
        assert seqs[-1]["offset"] is None


class TestCompressEdgeBlocks:
    def test_deterministic_and_named(self):
        a = corpus.compress_edge_blocks(BLOCK)
        assert a == corpus.compress_edge_blocks(BLOCK)
        assert [n for n, _ in a] == [
            "zeros_790", "zeros_791", "zeros_25", "lit_14", "lit_15",
            "lit_16", "lit_269", "lit_270", "lit_271", "final_5",
            "final_12", "final_13", "final_16", "exact_multiple"]

    @pytest.mark.parametrize("n,ext", [
        (790, b"\xff\xff\xff\x00"), (791, b"\xff\xff\xff\x01"),
        (25, b"\x00")])
    def test_zero_blocks_match_extension(self, n, ext):
        data, last = _edge("zeros_%d" % n)
        assert len(data) == BLOCK + n and last == b"\0" * n
        comp = lz4py.compress_block(last)
        assert comp.startswith(b"\x1f\x00\x01\x00" + ext)
        first = corpus.parse_sequences(comp)[0]
        assert first["match_ext"] == ext
        assert first["match_len"] == n - 6  # 1 literal, last 5 literal

    @pytest.mark.parametrize("run", [14, 15, 16, 269, 270, 271])
    def test_literal_runs(self, run):
        _, last = _edge("lit_%d" % run)
        first = corpus.parse_sequences(lz4py.compress_block(last))[0]
        assert first["lit_len"] == run
        assert first["offset"] == run  # the match is the block's start
        want_ext = {14: b"", 15: b"\x00", 16: b"\x01", 269: b"\xfe",
                    270: b"\xff\x00", 271: b"\xff\x01"}[run]
        assert first["lit_ext"] == want_ext

    @pytest.mark.parametrize("n", [5, 12, 13, 16])
    def test_final_block_sizes(self, n):
        data, last = _edge("final_%d" % n)
        assert len(data) == BLOCK + n and len(last) == n
        if n < 13:
            # below MFLIMIT + 1 a block is literals only: never smaller
            assert len(lz4py.compress_block(last)) == n + 1

    def test_exact_multiple(self):
        data, last = _edge("exact_multiple")
        assert len(data) == 3 * BLOCK and len(last) == BLOCK

    @pytest.mark.parametrize("block_raw", [4096, 8192])
    def test_native_compressor_roundtrips_edges(self, block_raw):
        from shipyard_amd import ops

        if not ops.native_compress_available():
            pytest.skip("native ops library not built")
        for name, data in corpus.compress_edge_blocks(block_raw):
            blocks = ops.lz4_compress_blocks(data, block_raw)
            assert len(blocks) == (len(data) + block_raw - 1) // block_raw
            for b, comp in enumerate(blocks):
                raw = data[b * block_raw:(b + 1) * block_raw]
                if comp is None:
                    continue
                assert len(comp) < len(raw), (name, b)
                assert lz4py.decompress_block(comp, len(raw)) == raw, \
                    (name, b)
            last = corpus.final_block(data, block_raw)
            if name in ("final_5", "final_12"):
                assert blocks[-1] is None, name
            if name.startswith("zeros_"):
                # same greedy policy: the native stream carries the
                # same extension bytes the GPU matchers must emit
                assert blocks[-1] == lz4py.compress_block(last), name
            if name.startswith("lit_"):
                first = corpus.parse_sequences(blocks[-1])[0]
                assert first["lit_len"] == int(name[4:]), name


def _as_parsed(seqs, tail, terminator):
    want = [(len(lits), offset, mlen) for lits, offset, mlen in seqs]
    if terminator if terminator is not None else bool(tail):
        want.append((len(tail), None, None))
    return want


class TestAssembledBlocks:
    SPECS = corpus.assembled_specs()
    BLOCKS = corpus.assembled_decode_blocks()

    def test_names(self):
        assert [b[0] for b in self.BLOCKS] == \
            ["match_off%d" % o for o in corpus.MATCH_OFFSETS] + [
                "match_rel", "lit_runs", "zero_lit_chain", "ends_on_match",
                "empty", "token_only"]
        assert [s[0] for s in self.SPECS] == [b[0] for b in self.BLOCKS]

    def test_reference_decodes_every_block(self):
        for name, stream, raw in self.BLOCKS:
            assert lz4py.decompress_block(stream, len(raw)) == raw, name
            assert len(raw) <= 4096, name
            assert len(stream) <= 4096 + 1024 - 48, name

    def test_parse_returns_the_sequences_that_went_in(self):
        for (name, seqs, tail, term), (_, stream, raw) in zip(
                self.SPECS, self.BLOCKS):
            got = [(s["lit_len"], s["offset"], s["match_len"])
                   for s in corpus.parse_sequences(stream)]
            assert got == _as_parsed(seqs, tail, term), name
            assert sum(a + (c or 0) for a, _, c in got) == len(raw), name

    def test_marks_point_at_the_encoded_fields(self):
        name, seqs, tail, term = self.SPECS[0]
        stream, raw, marks = corpus.assemble_lz4_marks(seqs, tail, term)
        assert (stream, raw) == corpus.assemble_lz4(seqs, tail, term)
        dpos = 0
        for (lits, offset, mlen), m in zip(seqs, marks):
            assert stream[m.token] & 15 == min(mlen - 4, 15)
            assert int.from_bytes(stream[m.off:m.off + 2],
                                  "little") == offset
            assert (m.mext is None) == (mlen < 19)
            assert m.dlit == dpos and m.dpos == dpos + len(lits)
            assert raw[m.dlit:m.dpos] == lits
            dpos = m.dpos + mlen

    def test_literals_are_not_constant(self):
        for name, seqs, tail, _ in self.SPECS:
            lits = b"".join(s[0] for s in seqs) + tail
            if len(lits) >= 64:
                assert len(set(lits)) > 32, name

    def test_branch_classes(self):
        seen, by_block = set(), {}
        for name, seqs, _, _ in self.SPECS:
            classes = {c for pair in corpus.classify_sequences(seqs)
                       for c in pair}
            by_block[name] = classes
            seen |= classes
        assert seen == set(corpus.SEQ_CLASSES)
        for o in (1, 3, 5, 7):
            assert "match_doubling_3plus" in by_block["match_off%d" % o]
        assert by_block["match_rel"] >= {
            "match_single", "match_loop", "match_doubling_2"}
        assert by_block["lit_runs"] >= {"lit_short", "lit_loop"}

    def test_classes_of_known_sequences(self):
        lit = b"x" * 64
        got = corpus.classify_sequences([
            (lit, 64, 64), (lit + b"x", 65, 65), (b"", 64, 65),
            (b"", 22, 65), (b"", 21, 65), (b"", 1, 4)])
        assert got == [
            ("lit_short", "match_single"), ("lit_loop", "match_loop"),
            ("lit_short", "match_doubling_2"),
            ("lit_short", "match_doubling_2"),
            ("lit_short", "match_doubling_3plus"),
            ("lit_short", "match_doubling_3plus")]

    def test_match_off_lengths_extensions_and_residues(self):
        for name, seqs, tail, term in self.SPECS[:len(corpus.MATCH_OFFSETS)]:
            offset = int(name[len("match_off"):])
            assert len(seqs[0][0]) >= offset
            assert [s[2] for s in seqs] == list(corpus.MATCH_LENS)
            assert {s[1] for s in seqs} == {offset}
            assert all(1 <= len(s[0]) <= 3 for s in seqs[1:])
            stream, raw, marks = corpus.assemble_lz4_marks(seqs, tail, term)
            ext = {s["match_len"]: s["match_ext"]
                   for s in corpus.parse_sequences(stream)}
            assert (ext[18], ext[19], ext[274], ext[529]) == (
                b"", b"\x00", b"\xff\x00", b"\xff\xff\x00")
            # every block on its own: each residue of dpos mod 16
            assert {m.dpos % 16 for m in marks} == set(range(16)), name
            assert {len(s[0]) for s in seqs[1:]} == {1, 2, 3}, name
            assert 3000 <= len(raw) <= 3300

    def test_match_rel_and_lit_runs(self):
        spec = {s[0]: s for s in self.SPECS}
        rel = [(s[1] - s[2], s[2]) for s in spec["match_rel"][1]]
        assert rel == [(d, m) for m in corpus.REL_LENS for d in (-1, 0, 1)]
        runs = spec["lit_runs"][1]
        assert sorted(len(s[0]) for s in runs) == [
            0, 1, 14, 15, 16, 63, 64, 65, 66, 127, 128, 129, 269, 270, 271,
            525]
        assert {s[2] for s in runs} == {4}
        stream = dict((b[0], b[1]) for b in self.BLOCKS)["lit_runs"]
        ext = {s["lit_len"]: s["lit_ext"]
               for s in corpus.parse_sequences(stream)}
        assert (ext[14], ext[15], ext[270], ext[525]) == (
            b"", b"\x00", b"\xff\x00", b"\xff\xff\x00")

    def test_zero_lit_chain_and_terminal_shapes(self):
        blocks = {b[0]: b for b in self.BLOCKS}
        parsed = corpus.parse_sequences(blocks["zero_lit_chain"][1])
        assert len(parsed) > 256 and len(parsed) % 16 != 0
        zero = [s["lit_len"] == 0 for s in parsed[1:-1]]
        assert all(zero) and len(zero) >= 300 and len(zero) % 16 != 0
        assert corpus.parse_sequences(
            blocks["ends_on_match"][1])[-1]["offset"] is not None
        assert blocks["empty"][1:] == (b"", b"")
        assert blocks["token_only"][1:] == (b"\x00", b"")

    @pytest.mark.parametrize("rung", corpus.FAR_REACH_RUNGS)
    def test_far_reach(self, rung):
        stream, raw, bad = corpus.far_reach(rung)
        assert len(raw) == rung
        assert lz4py.decompress_block(stream, rung) == raw
        assert len(stream) == len(bad) <= rung + 1024 - 48
        (seq,) = corpus.parse_sequences(stream)
        assert (seq["lit_len"], seq["offset"], seq["match_len"]) == (
            rung - 68, rung - 68, 68)
        assert corpus.parse_sequences(bad)[0]["offset"] == rung - 67
        with pytest.raises(ValueError, match="bad offset"):
            lz4py.decompress_block(bad, rung)

    def test_small_blocks_fit_a_512_byte_slot(self):
        small = corpus.small_decode_blocks()
        assert any(len(raw) == 5 for _, _, raw in small)
        for name, stream, raw in small:
            assert len(raw) <= 448, name
            assert lz4py.decompress_block(stream, len(raw)) == raw, name
        chain = corpus.parse_sequences(dict(
            (b[0], b[1]) for b in small)["zero_lit_chain_short"])
        assert len(chain) > 64 and len(chain) % 16 != 0

    def test_slot_reuse_layout(self):
        for grid, full in ((3, True), (4096, False), (4096, True)):
            names, streams, out_lens, expect, codes, stride = \
                corpus.slot_reuse_launch(grid, full)
            assert len(names) == grid + 40
            pairs = [(names[i], names[i + grid])
                     for i in (1, 7, 13, 20, 29, 38)]
            chain = "zero_lit_chain" if full else "zero_lit_chain_short"
            assert pairs == [
                ("deep_off0_k65", "small_mix"),
                ("small_mix", "deep_off0_k65"), ("toobig", "small_mix"),
                ("small_mix", "toobig"), (chain, "tiny5"), ("tiny5", chain)]
            assert stride == (4160 if full else 512)
            for name, stream, out_len, raw, code in zip(
                    names, streams, out_lens, expect, codes):
                if code == corpus.OK:
                    assert lz4py.decompress_block(stream, out_len) == raw
                else:
                    assert raw == b"" and (
                        out_len == 8193 or name == "deep_off0_k65")

    def test_builders_are_deterministic(self):
        assert self.BLOCKS == corpus.assembled_decode_blocks()
        assert corpus.deep_malformed_cases() == corpus.deep_malformed_cases()
        assert corpus.far_reach(8192) == corpus.far_reach(8192)
        assert corpus.small_decode_blocks() == corpus.small_decode_blocks()


class TestDeepMalformedCases:
    CASES = corpus.deep_malformed_cases()

    def test_every_case_raises_in_reference(self):
        for name, stream, out_len, code in self.CASES:
            with pytest.raises(ValueError):
                lz4py.decompress_block(stream, out_len)
            assert out_len <= 4096 and len(stream) <= 4096 + 1024 - 48, name

    def test_cases_cover_edits_chains_and_depths(self):
        names = [c[0] for c in self.CASES]
        assert len(set(names)) == len(names) == 2 * (7 * 5 + 2)
        for chain, last in (("zero_lit", 309), ("ordinary", 210)):
            for k in corpus.DEEP_K + (last,):
                for edit in ("off0", "off_gt_dpos", "cut_offset",
                             "cut_mlen_ext", "match_over_out"):
                    assert "%s_k%d_%s" % (chain, k, edit) in names
            assert chain + "_mismatch" in names
            assert chain + "_lit_over_out" in names
        assert {c[3] for c in self.CASES} == {
            corpus.ERR_OFFSET, corpus.ERR_OVERFLOW, corpus.ERR_TRUNC,
            corpus.ERR_MISMATCH}

    def test_reference_fails_at_the_edited_sequence(self):
        """The error is deep: everything in front of sequence k is the
        intact chain and decodes in the reference, and the whole stream
        fails there with the message of the check the code stands for."""
        import re

        want = {"off0": "bad offset", "off_gt_dpos": "bad offset",
                "cut_offset": "truncated offset",
                "cut_mlen_ext": "truncated match length",
                "match_over_out": "!= declared"}
        base = {}
        for chain, spec in (("zero_lit", corpus._zero_lit_chain_spec()),
                            ("ordinary", corpus._ordinary_chain_spec())):
            base[chain] = corpus.assemble_lz4_marks(*spec)
        checked = 0
        for name, stream, out_len, code in self.CASES:
            m = re.fullmatch(r"(zero_lit|ordinary)_k(\d+)_(\w+)", name)
            if m is None:
                assert name.endswith(("_mismatch", "_lit_over_out")), name
                continue
            good, raw, marks = base[m.group(1)]
            mark = marks[int(m.group(2))]
            assert stream[:mark.token] == good[:mark.token], name
            assert lz4py.decompress_block(
                stream[:mark.token], mark.dlit) == raw[:mark.dlit], name
            with pytest.raises(ValueError, match=want[m.group(3)]):
                lz4py.decompress_block(stream, out_len)
            checked += 1
        assert checked == 2 * 7 * 5
