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
