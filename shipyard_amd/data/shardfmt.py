"""SYSHARD — the framework's packed shard/layer format.

Container layers and data shards are stored as sequences of
independently-compressed LZ4 blocks with a per-block CRC32C manifest, so
the GPU can decode and verify a whole shard in one pass
(shipyard_amd/ops: lz4_decode_blocks + crc32c_chunks).  This replaces
the reference's reliance on dockerd gzip inflate + CPU MD5
(reference cascade/cascade.py:500-571, convoy/util.py:461-508).

Layout (little-endian):
  8s  magic  b"SYSHARD1"
  u32 flags            (bit0: blocks are LZ4; 0 = all stored
                        bit1: FILTER_SHUFFLE, blocks are byte-shuffled
                        bits 8..15: shuffle element size E — 2, 4 or 8
                        with bit1, 0 without
                        bit2: FILTER_DELTA, blocks hold element deltas
                        bits 16..23: delta element size D — 2, 4 or 8
                        with bit2, 0 without
                        bit3: FILTER_BITSHUFFLE, blocks are bit-shuffled
                        bits 24..31: bitshuffle element size B — 2, 4 or
                        8 with bit3, 0 without; other bits ignored;
                        bit1 and bit3 exclude each other)
  u32 block_raw        (max raw bytes per block; 8 KiB default)
  u64 raw_size
  u32 n_blocks
  n_blocks * { u64 comp_off, u32 comp_len, u32 raw_len, u32 crc32c }
  comp bytes...

A block with comp_len == raw_len is STORED (incompressible); the GPU
decoder copies it through.  comp offsets are relative to the payload
start and 16 B aligned so uint4 paths stay aligned.

FILTER_SHUFFLE (typed numeric shards: token ids, index arrays, float
fields) byte-transposes every block before it is compressed or stored,
the filter HDF5/Blosc/Zarr put in front of their codecs.  For a block
of raw_len bytes, n_el = raw_len // E and body = n_el * E:

  filtered[j*n_el + i] = raw[i*E + j]     0 <= j < E, 0 <= i < n_el
  filtered[body:]      = raw[body:]       (raw_len % E leftover bytes)

The per-block crc32c stays the CRC of the ORIGINAL bytes: integrity is
end to end, and a reader that does not know the flag fails its CRC
check instead of returning transposed data.

FILTER_DELTA (monotone or slowly varying typed shards: document and
sample offsets, CSR row pointers, sorted ids, timestamps) stores
differences instead of values, the filter Zarr/numcodecs ``Delta`` and
Blosc2 put in front of the shuffle.  For a block of raw_len bytes,
n_el = raw_len // D; the elements are little-endian unsigned integers
and all arithmetic is mod 2^(8*D):

  d[0] = x[0]
  d[i] = x[i] - x[i-1]                    1 <= i < n_el
  filtered[n_el*D:] = raw[n_el*D:]        (raw_len % D leftover bytes)

The running value restarts at every block, so blocks stay independently
decodable.  Writers apply delta first, then shuffle if both are
requested, then LZ4 or store; readers undo them in the reverse order.
D and E are independent fields and need not be equal.  The per-block
crc32c is again that of the ORIGINAL bytes.  The filter is opt-in per
shard: data that is not monotone (uniform token ids) gets WORSE under
delta, because differences of independent values are noisier than the
values.

FILTER_BITSHUFFLE (float fields and weights, narrow-range integers:
the filter HDF5 bitshuffle and Blosc BITSHUFFLE put in front of their
codecs) transposes every block bit by bit, so that a bit position that
is nearly constant over the elements (a sign, high exponent bits, the
unused top bits of a small delta) becomes a run of equal bytes even
where it shares its byte with noisy bits.  For a block of raw_len
bytes, n_el = raw_len // B, n8 = n_el // 8 * 8, L = n8 // 8 and
body = n8 * B; elements are little-endian, and bit p of an element
(0 <= p < 8*B) is bit p % 8, counted LSB first, of its byte p // 8:

  plane p occupies filtered[p*L : (p+1)*L]              0 <= p < 8*B
  bit r (LSB first) of filtered[p*L + m] = bit p of element 8*m + r
  filtered[body:] = raw[body:]

The verbatim tail holds the n_el % 8 leftover elements and the
raw_len % B leftover bytes (a full block of a 4096-multiple block size
has none).  The per-block crc32c is that of the ORIGINAL bytes.
Writers apply delta, then bitshuffle, then shuffle, then LZ4 or store;
bitshuffle composes with delta, but bitshuffle and the byte shuffle
exclude each other (a byte shuffle of bit planes is meaningless):
asking for both, at a writer, in an index or in a header's flags, is a
ValueError.  The filter is opt-in per shard: skewed token ids pack
WORSE bit-shuffled than byte-shuffled (docs/35-gpu-data-plane.md).

Adding a filter: add a row to ``FILTERS`` at its place in the writer
order (flag bit, element-size bits, whether the device op may run in
place), a numpy body transform for ``_filter_blocks`` as its reference,
the kernel, its entry point's row in ``ops.SIGNATURES`` (the filters
share one prototype) and an ``ops`` wrapper with the arguments of
``ops.byte_shuffle``; then add the row's keyword to the writers' signatures
and to ``ShardIndex``.  Flags, header parsing, validation and the CPU
and device chains in both directions all follow from the row.  A filter
that transforms its elements in groups passes the group size to
``_filter_blocks`` as ``granule`` (bitshuffle: 8 elements; what does not
fill a group stays verbatim), and one that makes no sense together with
another gets a pair in ``EXCLUSIVE_FILTERS``, which every writer,
``validate_index`` and the header parser check.
"""
from __future__ import annotations

import io
import struct
from collections import namedtuple
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, List, Optional

from shipyard_amd.data import lz4py
from shipyard_amd.ops import FILTER_ELEM_SIZES, gf2

MAGIC = b"SYSHARD1"
HEADER = struct.Struct("<8sIIQI")
ENTRY = struct.Struct("<QIII")
# 8 KiB: the GPU decoder is serial-latency-bound per block; smaller
# blocks raise workgroups/CU (measured: 64K=4.9, 16K=35, 8K=94 GB/s).
# CRC chunk math requires >= 4 KiB and the block size to be 4 KiB-
# aligned.  Compression-window loss vs 64 KiB is a few percent.
DEFAULT_BLOCK_RAW = 8 * 1024
# GPU geometry limits (validate_index / pack_gpu): the v2 CRC kernel
# needs chunk_size % 4096 == 0 (sy_crc32c_chunks), which also keeps
# every raw offset 16 B aligned for the uint4 stores; the LZ4 kernels
# hold one block in LDS / u16 hash positions, so compressed blocks stop
# at 64 KiB.
GPU_BLOCK_ALIGN = 4096
GPU_LZ4_BLOCK_MAX = 64 * 1024
FLAG_LZ4 = 0x1


def _filter_blocks(data, block_raw: int, elem_size: int, inverse: bool,
                   body_fn, granule: int = 1) -> bytes:
    """Walk ``data`` as ``block_raw`` blocks (the last may be short):
    ``body_fn(x, elem_size, inverse)`` transforms the whole groups of
    ``granule`` elements of a batch of equally long blocks, an
    ``(n_blk, body)`` uint8 view, and the ``len % (granule *
    elem_size)`` leftover of every block is copied verbatim.  One call
    for all full blocks, one for the ragged one."""
    import numpy as np

    if elem_size not in FILTER_ELEM_SIZES:
        raise ValueError(f"elem_size={elem_size} not in {FILTER_ELEM_SIZES}")
    if block_raw <= 0:
        raise ValueError("block_raw must be positive")
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty_like(src)
    n_full, tail_len = divmod(len(src), block_raw)
    for lo, n_blk, blk_len in ((0, n_full, block_raw),
                               (n_full * block_raw, 1, tail_len)):
        if not n_blk or not blk_len:
            continue
        body = blk_len // (granule * elem_size) * (granule * elem_size)
        s = src[lo:lo + n_blk * blk_len].reshape(n_blk, blk_len)
        d = out[lo:lo + n_blk * blk_len].reshape(n_blk, blk_len)
        if body:
            d[:, :body] = body_fn(s[:, :body], elem_size, inverse)
        d[:, body:] = s[:, body:]
    return out.tobytes()


def _shuffle_body(x, E: int, inverse: bool):
    n_blk, body = x.shape
    shape = (n_blk, E, body // E) if inverse else (n_blk, body // E, E)
    return x.reshape(shape).transpose(0, 2, 1).reshape(n_blk, body)


def _delta_body(x, E: int, inverse: bool):
    import numpy as np

    dt = np.dtype(f"<u{E}")
    x = np.ascontiguousarray(x).view(dt)
    if inverse:
        y = np.cumsum(x, axis=1, dtype=dt)
    else:
        y = x.copy()
        y[:, 1:] -= x[:, :-1]
    return y.view(np.uint8)


def _bitshuffle_body(x, E: int, inverse: bool):
    import numpy as np

    n_blk, body = x.shape
    n8 = body // E
    if inverse:
        bits = np.unpackbits(x.reshape(n_blk, 8 * E, n8 // 8), axis=2,
                             bitorder="little")
    else:
        bits = np.unpackbits(x.reshape(n_blk, n8, E), axis=2,
                             bitorder="little")
    return np.packbits(bits.transpose(0, 2, 1), axis=2,
                       bitorder="little").reshape(n_blk, body)


def shuffle_blocks_numpy(data, block_raw: int, elem_size: int,
                         inverse: bool = False) -> bytes:
    """Reference byte-shuffle of ``data`` laid out as ``block_raw``
    blocks (the last may be short): per block, plane j holds byte j of
    every ``elem_size``-byte element and the ``len % elem_size``
    leftover is copied verbatim; ``inverse`` undoes it.  Vectorised:
    one transpose for all full blocks, one for the ragged block.  The
    CPU writer, the CPU reader and the tests of the device kernel
    (ops.byte_shuffle) share it."""
    return _filter_blocks(data, block_raw, elem_size, inverse, _shuffle_body)


def delta_blocks_numpy(data, block_raw: int, elem_size: int,
                       inverse: bool = False) -> bytes:
    """Reference delta filter of ``data`` laid out as ``block_raw``
    blocks (the last may be short): per block, every ``elem_size``-byte
    little-endian unsigned element but the first is replaced by its
    difference to the one before it (mod 2**(8*elem_size)) and the
    ``len % elem_size`` leftover is copied verbatim; ``inverse`` sums
    the differences up again.  Vectorised: one shifted subtract (or one
    ``np.cumsum`` in the unsigned dtype) for all full blocks, one for
    the ragged block.  The CPU writer, the CPU reader and the tests of
    the device kernel (ops.delta_filter) share it."""
    return _filter_blocks(data, block_raw, elem_size, inverse, _delta_body)


def bitshuffle_blocks_numpy(data, block_raw: int, elem_size: int,
                            inverse: bool = False) -> bytes:
    """Reference bit-shuffle of ``data`` laid out as ``block_raw``
    blocks (the last may be short): per block, the whole groups of 8
    ``elem_size``-byte little-endian elements are bit-transposed, so
    that plane p holds bit p of every element, 8 consecutive elements
    per byte, LSB first; what does not fill a group of 8 elements is
    copied verbatim; ``inverse`` undoes it.  Vectorised: one
    ``unpackbits`` / transpose / ``packbits`` for all full blocks, one
    for the ragged block.  The CPU writer, the CPU reader and the tests
    of the device kernel (ops.bit_shuffle) share it."""
    return _filter_blocks(data, block_raw, elem_size, inverse,
                          _bitshuffle_body, granule=8)


@dataclass(frozen=True)
class Filter:
    """One row of FILTERS: everything the format code knows about a
    block filter."""
    kwarg: str         # keyword / ShardIndex attribute with its element size
    flag_name: str     # the header flag, for messages
    flag: int          # flags bit that turns the filter on
    shift: int         # flags bits shift..shift+7 hold the element size
    sizes: tuple       # element sizes the filter takes
    numpy_fn: Callable  # reference: (data, block_raw, elem, inverse) -> bytes
    op: str            # shipyard_amd.ops function with the same arguments
    in_place: bool     # the op may run with dst == src


# in writer order; readers undo them in reverse
FILTERS = (
    Filter("delta_elem", "FILTER_DELTA", 0x4, 16, FILTER_ELEM_SIZES,
           delta_blocks_numpy, "delta_filter", in_place=True),
    Filter("bitshuffle_elem", "FILTER_BITSHUFFLE", 0x8, 24,
           FILTER_ELEM_SIZES, bitshuffle_blocks_numpy, "bit_shuffle",
           in_place=False),
    Filter("shuffle_elem", "FILTER_SHUFFLE", 0x2, 8, FILTER_ELEM_SIZES,
           shuffle_blocks_numpy, "byte_shuffle", in_place=False),
)

# pairs of filter keywords that may not both be on
EXCLUSIVE_FILTERS = (("bitshuffle_elem", "shuffle_elem"),)


def _check_exclusive(what: str, elems: dict) -> None:
    for a, b in EXCLUSIVE_FILTERS:
        if elems.get(a, 0) and elems.get(b, 0):
            raise ValueError(
                f"{what}: {a}={elems[a]} and {b}={elems[b]} exclude "
                "each other, at most one of them may be non-zero")


def _filter_elems(what: str, given) -> dict:
    """``{keyword: element size}`` of every filter (0: off), in writer
    order, from a mapping that holds them under their keyword names (a
    writer's ``locals()``, a ShardIndex's ``vars()``).  ValueError in
    ``what``'s name for a size the filter does not take, or for two
    filters on that exclude each other."""
    elems = {}
    for f in FILTERS:
        elem = given.get(f.kwarg, 0)
        if elem != 0 and elem not in f.sizes:
            raise ValueError(
                f"{what}: {f.kwarg}={elem} must be 0 (no filter) "
                f"or one of {f.sizes}")
        elems[f.kwarg] = int(elem)
    _check_exclusive(what, elems)
    return elems


def _active(elems: dict) -> list:
    """(filter, element size) of the filters that are on, writer order;
    a keyword that ``elems`` lacks means that its filter is off."""
    return [(f, elems[f.kwarg]) for f in FILTERS if elems.get(f.kwarg, 0)]


def filter_flags(elems: dict) -> int:
    """The flags bits a writer sets for these element sizes."""
    flags = 0
    for f, elem in _active(elems):
        flags |= f.flag | (elem << f.shift)
    return flags


def filter_elems_from_flags(flags: int) -> dict:
    """Element size of every filter named by a header's flags word; 0
    where the filter's bit is clear (its element-size bits are then
    ignored like every other unknown bit).  ValueError when a filter is
    on with an element size it does not take, or when two filters are
    on that exclude each other."""
    elems = {}
    for f in FILTERS:
        elem = (flags >> f.shift) & 0xFF if flags & f.flag else 0
        if flags & f.flag and elem not in f.sizes:
            raise ValueError(
                f"SYSHARD flags {flags:#x}: {f.flag_name} with element "
                f"size {elem}, must be one of {f.sizes}")
        elems[f.kwarg] = elem
    _check_exclusive(f"SYSHARD flags {flags:#x}", elems)
    return elems


def filter_chain_numpy(data, block_raw: int, elems: dict,
                       inverse: bool = False):
    """Apply every active filter to ``data`` on the CPU in writer order,
    or undo them in the reverse order with ``inverse``."""
    steps = _active(elems)
    for f, elem in (reversed(steps) if inverse else steps):
        data = f.numpy_fn(data, block_raw, elem, inverse)
    return data


def filter_chain_device(t, block_raw: int, elems: dict):
    """Writer side on the device: every active filter in order, each
    into a freshly allocated tensor; rebinding ``t`` drops the
    intermediate before it.  The tensor passed in is never written."""
    import torch

    from shipyard_amd import ops

    for f, elem in _active(elems):
        dst = torch.empty_like(t)
        getattr(ops, f.op)(t, dst, block_raw, elem)
        t = dst
    return t


def unfilter_chain_device(src, block_raw: int, elems: dict, borrowed: bool):
    """Reader side on the device: undo the active filters in reverse
    order and return the tensor that holds the result.  ``borrowed``
    says that ``src`` is (a view of) the caller's payload, which is
    never written (with no filter on, ``src`` itself comes back).  A
    step gets a newly allocated destination when its source is borrowed
    or its filter cannot run in place; otherwise it runs in place."""
    import torch

    from shipyard_amd import ops

    for f, elem in reversed(_active(elems)):
        dst = src if f.in_place and not borrowed else torch.empty_like(src)
        getattr(ops, f.op)(src, dst, block_raw, elem, inverse=True)
        src, borrowed = dst, False
    return src


@dataclass
class BlockEntry:
    comp_off: int
    comp_len: int
    raw_len: int
    crc32c: int

    @property
    def stored(self) -> bool:
        return self.comp_len == self.raw_len


ENTRY_DT = None  # numpy structured dtype for the block table (lazy)


def _entry_dt():
    global ENTRY_DT
    if ENTRY_DT is None:
        import numpy as np

        ENTRY_DT = np.dtype([("comp_off", "<u8"), ("comp_len", "<u4"),
                             ("raw_len", "<u4"), ("crc", "<u4")])
        assert ENTRY_DT.itemsize == ENTRY.size
    return ENTRY_DT


class ShardIndex:
    """Parsed shard index.  The block table is held as numpy column
    arrays (comp_off/comp_len/raw_len/crc) so million-block shards
    decode without per-block python; `.blocks` materializes the
    BlockEntry view lazily for tests/CPU paths.  ``shuffle_elem`` is
    the FILTER_SHUFFLE element size and ``delta_elem`` the FILTER_DELTA
    one, ``bitshuffle_elem`` the FILTER_BITSHUFFLE one (0: that filter
    is off)."""

    def __init__(self, block_raw: int, raw_size: int, payload_off: int,
                 table=None, blocks: List[BlockEntry] = None, *,
                 shuffle_elem: int = 0, delta_elem: int = 0,
                 bitshuffle_elem: int = 0):
        import numpy as np

        self.block_raw = block_raw
        self.raw_size = raw_size
        self.payload_off = payload_off
        self.shuffle_elem = shuffle_elem
        self.delta_elem = delta_elem
        self.bitshuffle_elem = bitshuffle_elem
        if table is None:
            blocks = blocks or []
            table = np.zeros(len(blocks), dtype=_entry_dt())
            for i, b in enumerate(blocks):
                table[i] = (b.comp_off, b.comp_len, b.raw_len, b.crc32c)
        self.table = table
        self._blocks = blocks

    @property
    def n_blocks(self) -> int:
        return len(self.table)

    @property
    def blocks(self) -> List[BlockEntry]:
        if self._blocks is None:
            self._blocks = [
                BlockEntry(int(r["comp_off"]), int(r["comp_len"]),
                           int(r["raw_len"]), int(r["crc"]))
                for r in self.table]
        return self._blocks

    def raw_offs(self):
        """Cumulative raw offset per block (numpy int64)."""
        import numpy as np

        out = np.zeros(len(self.table), dtype=np.int64)
        np.cumsum(self.table["raw_len"][:-1], out=out[1:])
        return out

    def select_blocks(self, offs, lens):
        """Sorted unique ids (numpy int64) of the blocks that hold at
        least one byte of the raw-space byte ranges
        ``[offs[i], offs[i] + lens[i])``.  A range of length 0 selects
        nothing.  ValueError for a negative offset or length and for a
        range that ends past ``raw_size``.  Vectorized,
        O(n_ranges + n_blocks): every block but the last holds exactly
        ``block_raw`` bytes, so the block of a byte is a division, and
        the union of the block intervals is a prefix sum over +1/-1
        marks at their ends."""
        offs, lens = _as_ranges(offs, lens, self.raw_size)
        return _select_blocks(offs, lens, int(self.block_raw),
                              self.n_blocks)


def _align16(n: int) -> int:
    return (n + 15) & ~15


def _to_device(arr, device, view=None):
    """A numpy column as a tensor on ``device``; ``view`` reinterprets
    it (torch.from_numpy takes no unsigned type wider than a byte, so a
    uint32 column travels as its int32 view)."""
    import numpy as np
    import torch

    t = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    return t if view is None else t.view(view)


def _compress_span(args):
    """Worker: compress blocks [lo, hi) of a span of raw bytes."""
    span, block_raw, lo_off = args
    out = []
    for boff in range(0, len(span), block_raw):
        raw = span[boff:boff + block_raw]
        comp = lz4py.compress_block(raw)
        if len(comp) >= len(raw):
            comp = raw
        out.append(comp)
    return lo_off, out


def pack(data: bytes, block_raw: int = DEFAULT_BLOCK_RAW,
         compress: bool = True, workers: Optional[int] = None,
         shuffle_elem: int = 0, delta_elem: int = 0,
         bitshuffle_elem: int = 0) -> bytes:
    """Pack raw bytes into SYSHARD format (CPU writer).

    `shuffle_elem` (2, 4 or 8; 0 = off) byte-shuffles every block over
    elements of that size before it is compressed or stored
    (FILTER_SHUFFLE, see the module docstring); the CRCs stay those of
    the original bytes.

    `delta_elem` (2, 4 or 8; 0 = off) first replaces the elements of
    that size by their differences inside every block (FILTER_DELTA),
    ahead of the shuffle; meant for monotone data such as offsets,
    sorted ids and timestamps, and opt-in because it makes other data
    compress worse.

    `bitshuffle_elem` (2, 4 or 8; 0 = off) bit-transposes every block
    over elements of that size (FILTER_BITSHUFFLE), after the delta and
    instead of the byte shuffle (ValueError with `shuffle_elem` also
    non-zero); meant for float weights and fields and for delta-coded
    offsets, and opt-in because skewed token ids compress worse.

    `workers`: block compression is embarrassingly parallel (blocks are
    independent LZ4 streams); None = serial, 0 = one per CPU.  The
    replicator/mover pass workers=0 so layer packing scales with cores
    (the pure-python compressor does ~12 MB/s per core)."""
    elems = _filter_elems("pack", locals())
    crcs = gf2.crc32c_chunks_numpy(data, block_raw)
    n_raw = len(data)
    if data:
        # from here on `data` is what the payload holds: filtered bytes
        data = filter_chain_numpy(data, block_raw, elems)
    comps: List[bytes] = []
    if compress and data:
        # native multi-threaded compressor when the ops library is
        # built (CPU-only entry point — no GPU needed); python fallback
        try:
            from shipyard_amd import ops

            nat = ops.lz4_compress_blocks(data, block_raw)
            comps = [c if c is not None else
                     data[i * block_raw:(i + 1) * block_raw]
                     for i, c in enumerate(nat)]
        except Exception:
            comps = []
    if not comps and compress and data and workers is not None:
        import concurrent.futures as _cf
        import os as _os

        n_workers = workers or _os.cpu_count() or 4
        n_blocks = (len(data) + block_raw - 1) // block_raw
        per_span = max((n_blocks + n_workers - 1) // n_workers, 1)
        spans = [(data[i * per_span * block_raw:
                       (i + 1) * per_span * block_raw], block_raw,
                  i * per_span * block_raw)
                 for i in range((n_blocks + per_span - 1) // per_span)]
        with _cf.ProcessPoolExecutor(max_workers=n_workers) as pool:
            for _, blocks_out in sorted(
                    pool.map(_compress_span, spans)):
                comps.extend(blocks_out)
    elif not comps:
        for boff in range(0, len(data), block_raw):
            raw = data[boff:boff + block_raw]
            comp = lz4py.compress_block(raw) if compress else raw
            if not compress or len(comp) >= len(raw):
                comp = raw  # stored
            comps.append(comp)
    blocks: List[BlockEntry] = []
    payload = io.BytesIO()
    off = 0
    for bi, comp in enumerate(comps):
        raw_len = min(block_raw, n_raw - bi * block_raw)
        crc = crcs[bi] if bi < len(crcs) else 0
        blocks.append(BlockEntry(off, len(comp), raw_len, crc))
        payload.write(comp)
        pad = _align16(len(comp)) - len(comp)
        payload.write(b"\x00" * pad)
        off += len(comp) + pad
    flags = (FLAG_LZ4 if compress else 0) | filter_flags(elems)
    hdr = HEADER.pack(MAGIC, flags, block_raw, n_raw, len(blocks))
    table = b"".join(ENTRY.pack(b.comp_off, b.comp_len, b.raw_len, b.crc32c)
                     for b in blocks)
    return hdr + table + payload.getvalue()


def gpu_block_raw_ok(block_raw: int) -> bool:
    """True when the GPU writer can author shards at this block size."""
    return (0 < block_raw <= GPU_LZ4_BLOCK_MAX
            and block_raw % GPU_BLOCK_ALIGN == 0)


def pack_gpu(data, block_raw: int = DEFAULT_BLOCK_RAW,
             shuffle_elem: int = 0, delta_elem: int = 0,
             bitshuffle_elem: int = 0) -> bytes:
    """GPU SYSHARD writer: block compression (ops GPU matcher) +
    per-block CRC32C both run on the MI355X; the host only assembles
    header/table around the copied-back payload.  ``data``: bytes or a
    uint8 CUDA tensor.  Default matcher is the wave-screen (v2);
    SHIPYARD_LZ4C_SCREEN=0 selects the serial-greedy matcher whose
    output is bit-identical to the CPU ``pack()``.

    ``block_raw`` must be a multiple of 4096 and at most 65536
    (ValueError otherwise, before anything touches the device); the CPU
    ``pack()`` takes any block size.

    ``shuffle_elem`` (2, 4 or 8; 0 = off) applies FILTER_SHUFFLE: the
    CRCs are taken from the original tensor, ops.byte_shuffle writes
    the filtered copy (one more raw-sized buffer in HBM), and both the
    matcher and the stored-block gather read that copy.  Output equals
    ``pack(..., shuffle_elem=...)`` under the same matcher rule.

    ``delta_elem`` (2, 4 or 8; 0 = off) applies FILTER_DELTA ahead of
    the shuffle: ops.delta_filter writes the differences into a new
    buffer (a tensor passed in stays untouched), and with both filters
    on ops.byte_shuffle reads that buffer, which is freed as soon as
    the shuffled copy exists.  Output equals
    ``pack(..., delta_elem=...)`` under the same matcher rule.

    ``bitshuffle_elem`` (2, 4 or 8; 0 = off) applies FILTER_BITSHUFFLE
    in the byte shuffle's place (ValueError with both non-zero):
    ops.bit_shuffle writes the bit planes into a new buffer, after the
    delta when that is on too.  Output equals
    ``pack(..., bitshuffle_elem=...)`` under the same matcher rule."""
    if not gpu_block_raw_ok(block_raw):
        raise ValueError(
            f"pack_gpu: block_raw={block_raw} must be a multiple of "
            f"{GPU_BLOCK_ALIGN} and at most {GPU_LZ4_BLOCK_MAX}")
    elems = _filter_elems("pack_gpu", locals())
    flags = FLAG_LZ4 | filter_flags(elems)
    import numpy as np
    import torch

    from shipyard_amd import ops

    if isinstance(data, (bytes, bytearray, memoryview)):
        raw = bytes(data)
        n = len(raw)
        if n:
            # pinned staging: one host copy into page-locked memory,
            # then a fast async H2D (a pageable bytearray H2D forces
            # the driver through an internal staging copy anyway)
            pin = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            pin.numpy()[:] = np.frombuffer(raw, dtype=np.uint8)
            t = pin.to("cuda", non_blocking=True)
        else:
            t = torch.empty(0, dtype=torch.uint8, device="cuda")
    else:
        t = data
        n = t.numel()
        raw = None
    if n == 0:
        return HEADER.pack(MAGIC, flags, block_raw, 0, 0)
    # device-side CRC of every block (raw_cap chunks; ragged tail ok)
    crcs = np.asarray(ops.crc32c_chunks(t, chunk_size=block_raw)
                      .numpy(), dtype=np.uint32)
    # the payload holds filtered bytes; the CRCs above do not
    t = filter_chain_device(t, block_raw, elems)
    d_out, stride, lens = ops.lz4_compress_blocks_gpu(t, block_raw)
    lens_np = lens.numpy().view(np.uint32)
    n_blocks = (n + block_raw - 1) // block_raw

    # vectorized assembly: compaction happens ON DEVICE (gather_copy)
    # into the exact payload layout, then ONE D2H — the original
    # per-block python loop + full-slot D2H was 30x slower than the
    # compression kernel itself
    raw_lens = np.minimum(
        np.full(n_blocks, block_raw, dtype=np.uint64),
        n - np.arange(n_blocks, dtype=np.uint64) * block_raw
    ).astype(np.uint32)
    stored = lens_np == 0
    comp_lens = np.where(stored, raw_lens, lens_np).astype(np.uint64)
    padded = (comp_lens + 15) & ~np.uint64(15)
    offs = np.zeros(n_blocks, dtype=np.uint64)
    if n_blocks > 1:
        offs[1:] = np.cumsum(padded)[:-1]
    total = int(padded.sum())
    d_payload = torch.zeros(max(total, 1), dtype=torch.uint8,
                            device=t.device)  # zero pad bytes

    dev = t.device
    comp_idx = np.nonzero(~stored)[0]
    if len(comp_idx):
        ops.gather_copy(
            d_out,
            _to_device((comp_idx.astype(np.uint64) * stride).view(np.int64),
                       dev),
            d_payload, _to_device(offs[comp_idx].view(np.int64), dev),
            _to_device(lens_np[comp_idx].view(np.int32), dev, torch.uint32))
    st_idx = np.nonzero(stored)[0]
    if len(st_idx):
        ops.gather_copy(
            t,
            _to_device((st_idx.astype(np.uint64) * block_raw).view(np.int64),
                       dev),
            d_payload, _to_device(offs[st_idx].view(np.int64), dev),
            _to_device(raw_lens[st_idx].view(np.int32), dev, torch.uint32))
    # D2H straight into pinned memory; the final join is then the
    # ONLY host-side copy of the payload
    pout = torch.empty(max(total, 1), dtype=torch.uint8,
                       pin_memory=True)
    pout[:total].copy_(d_payload[:total], non_blocking=True)
    torch.cuda.synchronize()

    table_arr = np.empty(n_blocks, dtype=_entry_dt())
    table_arr["comp_off"] = offs
    table_arr["comp_len"] = comp_lens.astype(np.uint32)
    table_arr["raw_len"] = raw_lens
    table_arr["crc"] = crcs[:n_blocks]
    hdr = HEADER.pack(MAGIC, flags, block_raw, n, n_blocks)
    return b"".join((hdr, table_arr.tobytes(),
                     memoryview(pout.numpy())[:total]))


def pack_auto(data: bytes, block_raw: int = DEFAULT_BLOCK_RAW,
              workers: Optional[int] = None,
              gpu_threshold: int = 1 << 20,
              shuffle_elem: int = 0, delta_elem: int = 0,
              bitshuffle_elem: int = 0) -> bytes:
    """Author a SYSHARD on the GPU when one is present and the
    payload is large enough to amortize the H2D hop; CPU writer
    otherwise.  Both outputs are valid shards that every reader
    decodes; with SHIPYARD_LZ4C_SCREEN=0 the GPU matcher emits the
    CPU matcher's exact bytes (the default wave-screen matcher is
    ~equal ratio but not bit-identical — decode-side parity measured
    in profiles/data_plane_r02.md).  Block sizes the GPU writer cannot
    handle (see ``pack_gpu``) always take the CPU writer.
    ``shuffle_elem``, ``delta_elem`` and ``bitshuffle_elem`` go to
    whichever writer is picked."""
    elems = _filter_elems("pack_auto", locals())
    if len(data) >= gpu_threshold and gpu_block_raw_ok(block_raw):
        try:
            import torch

            use_gpu = torch.cuda.is_available()
        except Exception:
            use_gpu = False
        if use_gpu:
            return pack_gpu(data, block_raw=block_raw, **elems)
    return pack(data, block_raw=block_raw, workers=workers, **elems)


ShardHeader = namedtuple("ShardHeader", "block_raw raw_size n_blocks elems")


def parse_header(buf) -> ShardHeader:
    """The fixed header at the start of ``buf``; ``elems`` is the
    {filter keyword: element size} of its flags.  ValueError for a short
    buffer, a wrong magic or a filter flag with a bad element size."""
    if len(buf) < HEADER.size:
        raise ValueError("buffer shorter than the SYSHARD header")
    magic, flags, block_raw, raw_size, n_blocks = HEADER.unpack_from(buf, 0)
    if magic != MAGIC:
        raise ValueError("not a SYSHARD file")
    return ShardHeader(block_raw, raw_size, n_blocks,
                       filter_elems_from_flags(flags))


def index_from_table(hdr: ShardHeader, buf, offset: int = 0,
                     payload_off: int = 0) -> ShardIndex:
    """The index of a shard with header ``hdr`` whose block table starts
    at ``buf[offset]`` (numpy view of ``buf``, no per-block python)."""
    import numpy as np

    if len(buf) - offset < hdr.n_blocks * ENTRY.size:
        raise ValueError("buffer shorter than the SYSHARD block table")
    table = np.frombuffer(buf, dtype=_entry_dt(), count=hdr.n_blocks,
                          offset=offset)
    return ShardIndex(block_raw=hdr.block_raw, raw_size=hdr.raw_size,
                      payload_off=payload_off, table=table, **hdr.elems)


def read_index(buf: bytes) -> ShardIndex:
    hdr = parse_header(buf)
    return index_from_table(hdr, buf, HEADER.size,
                            HEADER.size + hdr.n_blocks * ENTRY.size)


def validate_index(idx: ShardIndex, payload_len: int,
                   for_gpu: bool = True) -> None:
    """Check a block table against the format rules before any of its
    numbers is used as an offset.  Raises ValueError naming the rule.

    The table arrives from an object store or a peer; the GPU reader
    hands comp_off/comp_len/raw_len straight to kernels as device
    offsets, so every rule here is a bounds or alignment precondition of
    gather_copy / lz4_decode_blocks / crc32c_chunks:

    * n_blocks == ceil(raw_size / block_raw) (0 blocks iff raw_size 0)
    * raw_len == block_raw except the last block (1..block_raw)
    * sum(raw_len) == raw_size
    * 1 <= comp_len <= raw_len
    * comp_off % 16 == 0
    * comp_off + comp_len <= payload_len (no uint64 wrap)
    * for_gpu: block_raw % 4096 == 0, and block_raw <= 65536 when any
      block is compressed (stored-only shards may use larger blocks)
    * shuffle_elem is 0, 2, 4 or 8 (ops.byte_shuffle takes no other)
    * delta_elem is 0, 2, 4 or 8 (ops.delta_filter takes no other)
    * bitshuffle_elem is 0, 2, 4 or 8 (ops.bit_shuffle takes no other),
      and bitshuffle_elem and shuffle_elem are not both non-zero

    O(n_blocks) vectorized numpy; ``unpack_cpu`` stays permissive and
    does not call this."""
    import numpy as np

    t = idx.table
    n = len(t)
    block_raw = int(idx.block_raw)
    raw_size = int(idx.raw_size)
    payload_len = int(payload_len)
    if block_raw <= 0:
        raise ValueError("shard index: block_raw must be positive")
    _filter_elems("shard index", vars(idx))
    want =(raw_size + block_raw - 1) // block_raw
    if n != want:
        raise ValueError(
            f"shard index: n_blocks={n} but ceil(raw_size/block_raw)="
            f"{want} (raw_size={raw_size}, block_raw={block_raw})")
    if for_gpu and block_raw % GPU_BLOCK_ALIGN:
        raise ValueError(
            f"shard index: block_raw={block_raw} is not a multiple of "
            f"{GPU_BLOCK_ALIGN} (GPU reader)")
    if n == 0:
        return
    raw_len = t["raw_len"]
    comp_len = t["comp_len"]
    comp_off = t["comp_off"]
    if (raw_len[:-1] != block_raw).any():
        raise ValueError("shard index: inner block raw_len != block_raw")
    if not 1 <= int(raw_len[-1]) <= block_raw:
        raise ValueError(
            f"shard index: final raw_len={int(raw_len[-1])} outside "
            f"1..{block_raw}")
    total = int(raw_len.sum(dtype=np.uint64))
    if total != raw_size:
        raise ValueError(
            f"shard index: sum(raw_len)={total} != raw_size={raw_size}")
    if (comp_len == 0).any() or (comp_len > raw_len).any():
        raise ValueError("shard index: comp_len outside 1..raw_len")
    if (comp_off & np.uint64(15)).any():
        raise ValueError("shard index: comp_off not 16-byte aligned")
    # comp_off + comp_len <= payload_len without forming the uint64 sum
    # (a comp_off near 2^64 would wrap it): compare the room behind
    # each offset instead
    plen = np.uint64(payload_len)
    room = plen - np.minimum(comp_off, plen)
    if (comp_off > plen).any() or (comp_len > room).any():
        raise ValueError(
            "shard index: comp_off + comp_len beyond the payload "
            f"({payload_len} bytes; truncated or corrupt)")
    if for_gpu and block_raw > GPU_LZ4_BLOCK_MAX \
            and (comp_len != raw_len).any():
        raise ValueError(
            f"shard index: block_raw={block_raw} > {GPU_LZ4_BLOCK_MAX} "
            "with compressed blocks (GPU reader)")


def unpack_cpu(buf: bytes, verify: bool = True) -> bytes:
    """CPU reference reader (tests + CPU-only hosts)."""
    idx = read_index(buf)
    elems = _filter_elems("shard index", vars(idx))
    out = io.BytesIO()
    for b in idx.blocks:
        comp = buf[idx.payload_off + b.comp_off:
                   idx.payload_off + b.comp_off + b.comp_len]
        raw = comp if b.stored else lz4py.decompress_block(comp, b.raw_len)
        # one block per call: any block_raw >= raw_len keeps it whole
        raw = filter_chain_numpy(raw, max(len(raw), 1), elems, inverse=True)
        if verify and gf2.crc32c(raw) != b.crc32c:
            raise ValueError("CRC mismatch in shard block")
        out.write(raw)
    data = out.getvalue()
    if len(data) != idx.raw_size:
        raise ValueError("shard size mismatch")
    return data



def _stored_contiguous(idx) -> bool:
    """True when every block is stored AND the payload layout equals the
    raw layout (comp_off == cumulative raw offset) — then the payload IS
    the decoded data and no per-block copies are needed.  This is the
    common case for incompressible shards packed with compress=False
    (block sizes that are 16 B multiples keep offsets aligned)."""
    import numpy as np

    t = idx.table
    if len(t) == 0:
        return True
    if not (t["comp_len"] == t["raw_len"]).all():
        return False
    if (t["raw_len"][:-1] % 16).any():  # inner blocks must stay aligned
        return False
    acc = np.zeros(len(t), dtype=np.uint64)
    np.cumsum(t["raw_len"][:-1], out=acc[1:])  # == aligned offs here
    return bool((t["comp_off"] == acc).all())


def _verify_crcs_device(t, block_raw: int, want_crc, ids=None) -> None:
    """CRC32C of every ``block_raw`` chunk of the device tensor ``t``
    (one kernel) against the numpy uint32 column ``want_crc``.
    ValueError naming the first 8 bad chunks: their positions, or
    ``ids[position]`` when the chunks are selected blocks of a shard."""
    import numpy as np
    import torch

    from shipyard_amd import ops

    crcs = ops.crc32c_chunks(t, chunk_size=block_raw)
    # crc32c_chunks finishes the GF(2) combine on the host and returns
    # a CPU tensor; compare there (one vectorized op, no python lists)
    want = torch.from_numpy(
        np.ascontiguousarray(want_crc).view(np.int32).copy())
    eq = crcs.view(torch.int32).cpu() == want
    if not bool(eq.all().item()):
        bad = np.flatnonzero(~eq.numpy())
        if ids is not None:
            bad = ids[bad]
        raise ValueError(f"GPU CRC mismatch in blocks {bad[:8].tolist()}")


def _launch_block_decode(d_comp, comp_off, comp_len, raw_len, out, out_off,
                         block_raw: int, dev) -> None:
    """Decode the blocks described by four equally long numpy columns
    from ``d_comp`` into ``out`` at ``out_off`` (int64): one gather_copy
    for the stored ones (comp_len == raw_len), one lz4_decode_blocks for
    the others.  Shared by the whole-shard reader, where the columns are
    the table and its raw offsets, and the range reader, where they are
    the selected rows and their scratch slots."""
    import numpy as np
    import torch

    from shipyard_amd import ops

    stored = comp_len == raw_len
    if stored.any():
        ops.gather_copy(
            d_comp, _to_device(comp_off[stored].astype(np.int64), dev),
            out, _to_device(out_off[stored], dev),
            _to_device(raw_len[stored].view(np.int32), dev, torch.uint32))
    lz4 = ~stored
    if lz4.any():
        status = ops.lz4_decode_blocks(
            d_comp,
            _to_device(comp_off[lz4].astype(np.int64), dev),
            _to_device(comp_len[lz4].view(np.int32), dev, torch.uint32),
            out,
            _to_device(out_off[lz4], dev),
            _to_device(raw_len[lz4].view(np.int32), dev, torch.uint32),
            raw_cap=block_raw)
        if not ops.lz4_all_ok(status):
            raise ValueError(
                f"GPU LZ4 decode failed: status={status.cpu().tolist()}")


def _decode_blocks(d_comp, idx: ShardIndex, dev):
    """Gather the stored blocks and LZ4-decode the others into a new
    raw_size tensor (still filtered when the shard has filters)."""
    import torch

    t = idx.table
    out = torch.empty(idx.raw_size, dtype=torch.uint8, device=dev)
    _launch_block_decode(d_comp, t["comp_off"], t["comp_len"], t["raw_len"],
                         out, idx.raw_offs(), idx.block_raw, dev)
    return out


def decode_device(d_comp, idx: ShardIndex, device, verify: bool = True):
    """Decode an uploaded shard payload in HBM: batched gather-copy for
    stored blocks + wave-cooperative LZ4 for compressed ones + chunked
    CRC verify.  All host work is vectorized (numpy column arrays) —
    O(1) python regardless of block count.

    The table is validated first (``validate_index`` against
    ``d_comp.numel()``): a bad table raises ValueError before a tensor
    is made or a kernel launched.

    The shard's filters are undone by ``unfilter_chain_device`` and the
    CRCs are taken after it, over the unfiltered bytes the table's CRCs
    describe.  Its source is the decode target, or on the
    stored-contiguous fast path the payload itself, which is never
    aliased or modified: a filtered shard's output is then a new tensor
    and ``d_comp``'s base must be 16-byte aligned.  Un-delta runs in
    place on anything but the payload, unshuffle and un-bitshuffle
    never do, so the peak HBM use on top of the payload is 1x raw for
    delta alone and 2x raw when shuffle or bitshuffle is on."""
    validate_index(idx, d_comp.numel(), for_gpu=True)

    import torch

    if len(idx.table) == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    borrowed = _stored_contiguous(idx)
    if borrowed:
        src = d_comp[:idx.raw_size]
    else:
        src = _decode_blocks(d_comp, idx, device)
    out = unfilter_chain_device(
        src, idx.block_raw, _filter_elems("shard index", vars(idx)),
        borrowed)
    if verify:
        _verify_crcs_device(out[:idx.raw_size].contiguous(), idx.block_raw,
                            idx.table["crc"])
    return out


# ------------------------------------------------------------ range reads
def _as_ranges(offs, lens, raw_size: int):
    """``offs``/``lens`` as two equally long 1-D numpy int64 arrays,
    checked against ``raw_size``.  ValueError names the first bad
    range."""
    import numpy as np

    offs = np.ascontiguousarray(offs, dtype=np.int64).reshape(-1)
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    if len(offs) != len(lens):
        raise ValueError(
            f"ranges: {len(offs)} offsets but {len(lens)} lengths")
    raw_size = int(raw_size)
    # off + len <= raw_size without forming a sum that could wrap
    bad = (offs < 0) | (lens < 0) | (offs > raw_size)
    bad |= lens > raw_size - np.minimum(offs, raw_size)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(
            f"ranges: range {i} (offset {int(offs[i])}, length "
            f"{int(lens[i])}) is negative or ends past raw_size="
            f"{raw_size}")
    return offs, lens


def _select_blocks(offs, lens, block_raw: int, n_blocks: int):
    import numpy as np

    if block_raw <= 0:
        raise ValueError("shard index: block_raw must be positive")
    live = lens > 0
    first = offs[live] // block_raw
    last = (offs[live] + lens[live] - 1) // block_raw
    if len(last) and int(last.max()) >= n_blocks:
        raise ValueError(
            f"shard index: a range ends in block {int(last.max())} but "
            f"the table has {n_blocks} blocks")
    # +1 where an interval of blocks opens, -1 behind its last block
    mark = np.bincount(first, minlength=n_blocks + 1) - \
        np.bincount(last + 1, minlength=n_blocks + 1)
    return np.nonzero(np.cumsum(mark[:n_blocks]) > 0)[0].astype(np.int64)


def _scratch_offsets(offs, lens, sel, block_raw: int, n_blocks: int):
    """Where every range starts in the compact buffer that holds
    selected block ``sel[k]`` at ``k * block_raw`` (numpy int64).  A
    range that spans several blocks selected all of them, and ``sel`` is
    sorted, so they are neighbours in the buffer too and the range is
    contiguous there.  An empty range gets 0."""
    import numpy as np

    if not len(sel):
        return np.zeros(len(offs), dtype=np.int64)
    slot = np.full(n_blocks, -1, dtype=np.int64)
    slot[sel] = np.arange(len(sel), dtype=np.int64)
    # an empty range at raw_size may name the block behind the last one
    blk = np.minimum(offs // block_raw, n_blocks - 1)
    return np.where(lens > 0, slot[blk] * block_raw + offs % block_raw, 0)


def read_ranges_cpu(buf: bytes, offs, lens, verify: bool = True) -> bytes:
    """CPU reference of the range readers: the raw-space byte ranges
    ``[offs[i], offs[i] + lens[i])`` of the shard in ``buf``,
    concatenated in the caller's order.  Only the blocks that hold a
    byte of a range (``ShardIndex.select_blocks``) are decoded, have
    their filters undone (one ``filter_chain_numpy`` call on the compact
    buffer of selected blocks) and, with ``verify``, their CRC checked:
    a corrupt block that no range touches goes unnoticed."""
    import numpy as np

    idx = read_index(buf)
    elems = _filter_elems("shard index", vars(idx))
    offs, lens = _as_ranges(offs, lens, idx.raw_size)
    block_raw = int(idx.block_raw)
    sel = _select_blocks(offs, lens, block_raw, idx.n_blocks)
    if not len(sel):
        return b""
    t = idx.table[sel]
    if (t["raw_len"][:-1] != block_raw).any() or \
            not 1 <= int(t["raw_len"][-1]) <= block_raw:
        raise ValueError("shard index: inner block raw_len != block_raw")
    compact = bytearray((len(sel) - 1) * block_raw + int(t["raw_len"][-1]))
    for k, (coff, clen, rlen) in enumerate(zip(
            t["comp_off"].tolist(), t["comp_len"].tolist(),
            t["raw_len"].tolist())):
        comp = buf[idx.payload_off + coff:idx.payload_off + coff + clen]
        raw = comp if clen == rlen else lz4py.decompress_block(comp, rlen)
        if len(raw) != rlen:
            raise ValueError("shard size mismatch")
        compact[k * block_raw:k * block_raw + rlen] = raw
    # the ragged final block of the shard, if selected, is last: the
    # compact buffer is a regular block_raw buffer for the filters
    data = filter_chain_numpy(bytes(compact), block_raw, elems, inverse=True)
    if verify:
        crcs = np.asarray(gf2.crc32c_chunks_numpy(data, block_raw),
                          dtype=np.uint32)
        bad = sel[crcs != t["crc"]]
        if len(bad):
            raise ValueError(
                f"CRC mismatch in shard blocks {bad[:8].tolist()}")
    src = _scratch_offsets(offs, lens, sel, block_raw, idx.n_blocks)
    return b"".join(data[s:s + n]
                    for s, n in zip(src.tolist(), lens.tolist()))


def _check_rows(lens, row_stride: int, fill: int) -> None:
    """The output arguments of a range read against its (checked)
    lengths; ValueError before anything is read, made or launched."""
    import numpy as np

    if int(row_stride) < 0:
        raise ValueError(f"row_stride={row_stride} must not be negative")
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"fill={fill} is not a byte value")
    if row_stride and len(lens) and int(lens.max()) > row_stride:
        i = int(np.argmax(lens > row_stride))
        raise ValueError(
            f"ranges: range {i} has {int(lens[i])} bytes, more than "
            f"row_stride={row_stride}")


def _decode_selected(d_comp, idx: ShardIndex, sel, comp_off, offs, lens,
                     device, verify: bool):
    """The first half of a device range read, shared by the byte path
    (``_decode_ranges``) and the typed path (``_decode_rows``): decode
    the selected blocks ``sel`` (at least one) into a compact scratch
    tensor, undo the filters, verify.  Returns the scratch and, as a
    device int64 tensor, the byte offset in it of every range
    (``_scratch_offsets``)."""
    import numpy as np
    import torch

    block_raw = int(idx.block_raw)
    t = idx.table[sel]
    scratch = torch.empty(
        (len(sel) - 1) * block_raw + int(t["raw_len"][-1]),
        dtype=torch.uint8, device=device)
    _launch_block_decode(
        d_comp, comp_off, t["comp_len"], t["raw_len"], scratch,
        np.arange(len(sel), dtype=np.int64) * block_raw, block_raw, device)
    scratch = unfilter_chain_device(
        scratch, block_raw, _filter_elems("shard index", vars(idx)),
        borrowed=False)
    if verify:
        _verify_crcs_device(scratch, block_raw, t["crc"], ids=sel)
    src_off = _scratch_offsets(offs, lens, sel, block_raw, idx.n_blocks)
    return scratch, _to_device(src_off, device)


def _decode_ranges(d_comp, idx: ShardIndex, sel, comp_off, offs, lens,
                   device, verify: bool, row_stride: int, fill: int):
    """The device side of a range read, shared by
    ``decode_ranges_device`` and ``ShardStager.stage_ranges``: decode,
    unfilter, verify (``_decode_selected``), gather.  ``sel`` are the
    selected block ids and ``comp_off`` where their payload starts in
    ``d_comp`` (the table's column for a full payload, rebased offsets
    for a partial one); ``offs``/``lens`` are checked numpy int64
    arrays, the index is validated and ``_check_rows`` has passed."""
    import numpy as np
    import torch

    from shipyard_amd import ops

    n = len(offs)
    row_stride = int(row_stride)
    if n == 0:
        return torch.empty((0, row_stride) if row_stride else 0,
                           dtype=torch.uint8, device=device)
    if row_stride:
        out = torch.full((n, row_stride), int(fill), dtype=torch.uint8,
                         device=device)
        dst_off = np.arange(n, dtype=np.int64) * row_stride
    else:
        out = torch.empty(int(lens.sum()), dtype=torch.uint8, device=device)
        dst_off = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=dst_off[1:])
    if not len(sel):
        return out  # nothing but empty ranges
    scratch, src_off = _decode_selected(d_comp, idx, sel, comp_off, offs,
                                        lens, device, verify)
    ops.gather_ranges(scratch, src_off, _to_device(lens, device),
                      out.view(-1), _to_device(dst_off, device))
    return out


def decode_ranges_device(d_comp, idx: ShardIndex, offs, lens, device,
                         verify: bool = True, row_stride: int = 0,
                         fill: int = 0):
    """Random-access read of an uploaded shard payload in HBM: the
    raw-space byte ranges ``[offs[i], offs[i] + lens[i])``, decoding
    only the blocks that hold a byte of them.

    ``d_comp`` is the full payload on the device, as for
    ``decode_device``.  The table is validated first (``validate_index``
    against ``d_comp.numel()``), then the ranges are checked against
    ``raw_size`` and ``row_stride``; each failure is a ValueError raised
    before a tensor is made or a kernel launched.

    The selected blocks (``ShardIndex.select_blocks``) are decoded into
    a compact scratch tensor, selected block ``k`` at ``k * block_raw``:
    one gather_copy for the stored ones, one lz4_decode_blocks for the
    others.  The ids are sorted, so the shard's short final block, if
    selected, is last, and the scratch is a regular ``block_raw`` buffer
    for ``unfilter_chain_device`` and, with ``verify``, for
    ``crc32c_chunks``, whose result is compared with the selected rows'
    CRCs (a mismatch is a ValueError that names the shard's block ids).
    Only those blocks are verified: a corrupt block that no range
    touches goes unnoticed.  ``ops.gather_ranges`` then cuts the ranges
    out of the scratch; the byte at raw offset ``r`` is at
    ``slot(r // block_raw) * block_raw + r % block_raw`` there.

    ``row_stride == 0``: a 1-D uint8 tensor of ``sum(lens)`` bytes, the
    ranges in the caller's order.  ``row_stride > 0``: a
    ``[n, row_stride]`` uint8 tensor, row ``i`` holding range ``i``
    followed by ``fill`` bytes (ValueError if a range is longer).  No
    ranges: an empty tensor and no launch.  All host work is vectorized
    numpy, whatever the number of ranges and blocks.

    Peak HBM on top of the payload, with S selected blocks and
    R = sum(lens): ``S * block_raw + R`` with no filter or delta alone,
    ``2 * S * block_raw + R`` when shuffle or bitshuffle is on."""
    validate_index(idx, d_comp.numel(), for_gpu=True)
    offs, lens = _as_ranges(offs, lens, idx.raw_size)
    _check_rows(lens, row_stride, fill)
    sel = _select_blocks(offs, lens, int(idx.block_raw), idx.n_blocks)
    return _decode_ranges(d_comp, idx, sel, idx.table["comp_off"][sel],
                          offs, lens, device, verify, row_stride, fill)


# -------------------------------------------------------------- row reads
def _row_types(src_dtype, out_dtype, pad):
    """The type arguments of a row read: (source element bytes, numpy
    source dtype, numpy output dtype, pad as an int).  ``out_dtype`` is
    anything that names int32 or int64 (a numpy or torch dtype, a
    string).  ValueError for an unknown type, a conversion that does not
    keep every value (``u4`` into int32) and a pad outside
    ``out_dtype``."""
    import numpy as np

    from shipyard_amd import ops

    try:
        out = np.dtype(out_dtype)
    except TypeError:
        try:  # torch.int32 and its like
            out = np.dtype(str(out_dtype).rpartition(".")[2])
        except TypeError:
            out = None
    if out not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError(
            f"rows: out_dtype={out_dtype!r} must be int32 or int64")
    size, signed = ops.widen_sizes(src_dtype, 8 * out.itemsize)
    pad = ops.check_widen_pad(pad, 8 * out.itemsize)
    return size, np.dtype(f"<{'i' if signed else 'u'}{size}"), out, pad


def _as_rows(starts, counts, size: int, raw_size: int, row_elems: int):
    """``starts``/``counts``, in elements of ``size`` bytes, as two
    equally long 1-D numpy int64 arrays, checked against ``raw_size``
    and ``row_elems``.  ValueError names the first bad row."""
    import numpy as np

    if int(row_elems) < 0:
        raise ValueError(f"row_elems={row_elems} must not be negative")
    starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(starts) != len(counts):
        raise ValueError(
            f"rows: {len(starts)} starts but {len(counts)} counts")
    # (start + count) * size <= raw_size without a product or a sum that
    # could wrap: count the elements that can be addressed
    n_el = int(raw_size) // size
    bad = (starts < 0) | (counts < 0) | (starts > n_el)
    bad |= counts > n_el - np.minimum(starts, n_el)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(
            f"rows: row {i} (start {int(starts[i])}, count "
            f"{int(counts[i])}) is negative or ends past the {n_el} "
            f"elements of {size} bytes in raw_size={int(raw_size)}")
    if len(counts) and int(counts.max()) > row_elems:
        i = int(np.argmax(counts > row_elems))
        raise ValueError(
            f"rows: row {i} has {int(counts[i])} elements, more than "
            f"row_elems={row_elems}")
    return starts, counts


def read_rows_cpu(buf: bytes, starts, counts, src_dtype, out_dtype,
                  row_elems: int, pad: int, verify: bool = True):
    """CPU reference of the row readers: a numpy ``[n, row_elems]``
    array of ``out_dtype`` (int32 or int64) whose row ``i`` holds the
    ``counts[i]`` elements of type ``src_dtype`` (``u1``, ``u2``,
    ``i2``, ``u4``, ``i4``, little-endian) that start at element
    ``starts[i]`` of the shard in ``buf``, followed by ``pad``.  All
    units are elements of ``src_dtype``; bytes of ``raw_size`` behind
    the last whole element cannot be addressed.  Built on
    ``read_ranges_cpu`` (only touched blocks are decoded and verified)
    and ``astype``.  Each bad argument is a ValueError, see
    ``decode_rows_device``."""
    import numpy as np

    idx = read_index(buf)
    size, src_np, out_np, pad = _row_types(src_dtype, out_dtype, pad)
    starts, counts = _as_rows(starts, counts, size, idx.raw_size, row_elems)
    data = read_ranges_cpu(buf, starts * size, counts * size, verify=verify)
    out = np.full((len(starts), int(row_elems)), pad, dtype=out_np)
    # the ranges come back concatenated in row order, as the mask walks
    live = np.arange(int(row_elems))[None, :] < counts[:, None]
    out[live] = np.frombuffer(data, dtype=src_np).astype(out_np)
    return out


def _decode_rows(d_comp, idx: ShardIndex, sel, comp_off, starts, counts,
                 device, verify: bool, src_dtype, out_np, row_elems: int,
                 pad: int):
    """The device side of a row read, shared by ``decode_rows_device``
    and ``ShardStager.stage_rows``: ``_decode_selected`` as for a range
    read, then ``ops.gather_widen``.  ``starts``/``counts`` are checked
    numpy int64 arrays in elements, the index is validated and
    ``_row_types`` has passed."""
    import numpy as np
    import torch

    from shipyard_amd import ops

    n = len(starts)
    out = torch.empty((n, int(row_elems)),
                      dtype=getattr(torch, out_np.name), device=device)
    if n == 0:
        return out
    size = ops.widen_sizes(src_dtype, 8 * out_np.itemsize)[0]
    if len(sel):
        scratch, src_off = _decode_selected(
            d_comp, idx, sel, comp_off, starts * size, counts * size,
            device, verify)
    else:  # nothing but empty rows: nothing to decode, all of it pad
        scratch = torch.empty(0, dtype=torch.uint8, device=device)
        src_off = _to_device(np.zeros(n, dtype=np.int64), device)
    ops.gather_widen(scratch, src_off, _to_device(counts, device), out,
                     src_dtype, pad)
    return out


def decode_rows_device(d_comp, idx: ShardIndex, starts, counts, device,
                       src_dtype, out_dtype, row_elems: int, pad: int,
                       verify: bool = True):
    """Typed random-access read of an uploaded shard payload in HBM: a
    ``[n, row_elems]`` device tensor of ``out_dtype`` (int32 or int64)
    whose row ``i`` holds the ``counts[i]`` elements of type
    ``src_dtype`` (``u1``, ``u2``, ``i2``, ``u4``, ``i4``,
    little-endian) that start at element ``starts[i]`` of the raw data,
    zero- or sign-extended, followed by ``pad``: a batch for an
    embedding lookup and a loss, padded with a token id or an
    ``ignore_index``.  All units are elements of ``src_dtype``, which
    keeps every row aligned to its element in the scratch (``block_raw``
    is a multiple of 4096); a ``raw_size`` that is no multiple of the
    element size is fine, its trailing bytes cannot be addressed.

    Everything up to the last step is ``decode_ranges_device``'s: the
    table is validated, the blocks that hold an element of a row are
    selected, decoded into the compact scratch, unfiltered and, with
    ``verify``, CRC-checked (only those blocks).  ``ops.gather_widen``
    then writes the whole output in one launch: data widened, padding
    filled, nothing pre-filled and no pass over the output afterwards.

    Each of these is a ValueError raised before a tensor is made or a
    kernel launched, naming the first bad row: unequal lengths of
    ``starts`` and ``counts``, a negative value, a row that ends past
    the last whole element of ``raw_size``, ``counts[i] > row_elems``,
    ``row_elems < 0``, an unknown ``src_dtype`` or ``out_dtype``, a
    conversion that does not keep every value (``u4`` into int32) and a
    ``pad`` that ``out_dtype`` cannot hold.  No rows: an empty
    ``[0, row_elems]`` tensor and no launch.  Rows that are all empty:
    a tensor of ``pad``, written by the kernel, and nothing is decoded.

    Peak HBM on top of the payload is that of ``decode_ranges_device``
    with R = ``n * row_elems * out_dtype.itemsize`` and S selected
    blocks: ``S * block_raw + R`` with no filter or delta alone,
    ``2 * S * block_raw + R`` when shuffle or bitshuffle is on."""
    validate_index(idx, d_comp.numel(), for_gpu=True)
    size, _, out_np, pad = _row_types(src_dtype, out_dtype, pad)
    starts, counts = _as_rows(starts, counts, size, idx.raw_size, row_elems)
    sel = _select_blocks(starts * size, counts * size, int(idx.block_raw),
                         idx.n_blocks)
    return _decode_rows(d_comp, idx, sel, idx.table["comp_off"][sel],
                        starts, counts, device, verify, src_dtype, out_np,
                        row_elems, pad)


# ----------------------------------------------------------- packed reads
def plan_packed_rows(counts, row_elems: int):
    """Where every sample of a packed read goes: ``(row, col, n_rows)``,
    two numpy int64 arrays as long as ``counts`` and the number of rows
    used.  Next-fit in the caller's order: sample ``i`` goes directly
    behind sample ``i - 1`` in the same row if it still fits
    (``col + counts[i] <= row_elems``) and opens the next row at column
    0 otherwise.  An empty sample takes the cursor's place and no
    space; no samples at all give ``n_rows == 0``.  ValueError, naming
    the first bad sample, for ``row_elems < 0``, a negative count and a
    sample longer than a row.  The readers take ``row``/``col`` as
    plain arguments: a caller with a better bin-packer brings its own
    plan."""
    import numpy as np

    row_elems = int(row_elems)
    if row_elems < 0:
        raise ValueError(f"row_elems={row_elems} must not be negative")
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    bad = (counts < 0) | (counts > row_elems)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(
            f"packed: sample {i} has {int(counts[i])} elements, which is "
            f"negative or more than row_elems={row_elems}")
    row = np.empty(len(counts), dtype=np.int64)
    col = np.empty(len(counts), dtype=np.int64)
    r = c = 0
    for i, n in enumerate(counts.tolist()):
        if c + n > row_elems:
            r, c = r + 1, 0
        row[i], col[i] = r, c
        c += n
    return row, col, (r + 1 if len(counts) else 0)


def _as_packed(starts, counts, row, col, n_rows: int, size: int,
               raw_size: int, row_elems: int):
    """The plan of a packed read, checked: ``starts``/``counts`` as
    ``_as_rows`` gives them, ``row``/``col`` as numpy int64 arrays of
    their length.  ValueError names the first bad sample in the
    caller's order (of two samples that overlap, the later one)."""
    import numpy as np

    starts, counts = _as_rows(starts, counts, size, raw_size, row_elems)
    row = np.ascontiguousarray(row, dtype=np.int64).reshape(-1)
    col = np.ascontiguousarray(col, dtype=np.int64).reshape(-1)
    if len(row) != len(starts) or len(col) != len(starts):
        raise ValueError(
            f"packed: {len(starts)} starts and counts but {len(row)} rows "
            f"and {len(col)} columns")
    n_rows, row_elems = int(n_rows), int(row_elems)
    if n_rows < 0:
        raise ValueError(f"n_rows={n_rows} must not be negative")
    for bad, what in (
            ((row < 0) | (row >= n_rows),
             f"a row outside the {n_rows} rows"),
            (col < 0, "a negative column"),
            (col > row_elems - counts,
             f"a last column behind row_elems={row_elems}")):
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(
                f"packed: sample {i} (row {int(row[i])}, column "
                f"{int(col[i])}, count {int(counts[i])}) has {what}")
    order, dst_start, _ = _packed_lists(counts, row, col, row_elems)
    if len(order) > 1:
        ends = dst_start + counts[order]
        # the sample that reaches furthest among those sorted before k
        reach = np.maximum.accumulate(ends)[:-1]
        hit = np.flatnonzero(dst_start[1:] < reach)
        if len(hit):
            holder = np.flatnonzero(np.concatenate(([True], ends[1:] >
                                                    reach)))
            # of every overlapping pair the later sample in caller order
            other = order[holder[np.searchsorted(holder, hit, "right") - 1]]
            later = np.maximum(order[hit + 1], other)
            k = int(np.argmin(later))
            i = int(later[k])
            j = int(min(order[hit[k] + 1], other[k]))
            raise ValueError(
                f"packed: sample {i} (row {int(row[i])}, columns "
                f"{int(col[i])}..{int(col[i] + counts[i]) - 1}) overlaps "
                f"sample {j} (columns {int(col[j])}.."
                f"{int(col[j] + counts[j]) - 1})")
    return starts, counts, row, col


def _packed_lists(counts, row, col, row_elems: int):
    """The non-empty samples of a packed plan in destination order
    (stable, by ``row * row_elems + col``): their indices in the
    caller's order, their flat destination starts and their labels
    (1 + the number of non-empty samples of the same row at a smaller
    column), as numpy int64, int64 and int32 arrays."""
    import numpy as np

    live = np.flatnonzero(counts > 0)
    key = row[live] * int(row_elems) + col[live]
    by_dst = np.argsort(key, kind="stable")
    order, dst_start = live[by_dst], key[by_dst]
    rows = row[order]
    labels = np.arange(len(order)) - np.searchsorted(rows, rows, "left") + 1
    return order, dst_start, labels.astype(np.int32)


def read_packed_cpu(buf: bytes, starts, counts, row, col, n_rows: int,
                    src_dtype, out_dtype, row_elems: int, pad: int,
                    verify: bool = True):
    """CPU reference of the packed readers: numpy arrays
    ``(tokens, segment_ids, positions)`` of shape ``[n_rows, row_elems]``,
    ``tokens`` of ``out_dtype`` (int32 or int64) and the other two
    int32.  Sample ``i``, the ``counts[i]`` elements of type
    ``src_dtype`` from element ``starts[i]`` of the shard in ``buf``,
    lands widened at ``tokens[row[i], col[i]:col[i] + counts[i]]``;
    there ``positions`` counts from 0 and ``segment_ids`` holds the
    sample's label, 1 + the number of non-empty samples of the same row
    at a smaller column.  Every other element holds ``pad`` in
    ``tokens`` and 0 in the other two.  Built on ``read_ranges_cpu``
    (only touched blocks are decoded and verified).  Each bad argument
    is a ValueError, see ``decode_packed_device``."""
    import numpy as np

    idx = read_index(buf)
    size, src_np, out_np, pad = _row_types(src_dtype, out_dtype, pad)
    starts, counts, row, col = _as_packed(
        starts, counts, row, col, n_rows, size, idx.raw_size, row_elems)
    shape = (int(n_rows), int(row_elems))
    tokens = np.full(shape, pad, dtype=out_np)
    segment_ids = np.zeros(shape, dtype=np.int32)
    positions = np.zeros(shape, dtype=np.int32)
    order, dst_start, labels = _packed_lists(counts, row, col, row_elems)
    if len(order):
        n = counts[order]
        data = read_ranges_cpu(buf, starts[order] * size, n * size,
                               verify=verify)
        # the ranges come back concatenated in destination order
        first = np.cumsum(n) - n
        within = np.arange(int(n.sum())) - np.repeat(first, n)
        at = np.repeat(dst_start, n) + within
        tokens.reshape(-1)[at] = np.frombuffer(data, dtype=src_np)
        segment_ids.reshape(-1)[at] = np.repeat(labels, n)
        positions.reshape(-1)[at] = within
    return tokens, segment_ids, positions


def _decode_packed(d_comp, idx: ShardIndex, sel, comp_off, starts, counts,
                   row, col, n_rows: int, device, verify: bool, src_dtype,
                   out_np, row_elems: int, pad: int):
    """The device side of a packed read, shared by
    ``decode_packed_device`` and ``ShardStager.stage_packed``: the
    non-empty samples in destination order (``_packed_lists``),
    ``_decode_selected`` for their byte ranges, then one
    ``ops.gather_pack`` launch.  The plan is checked (``_as_packed``),
    the index is validated and ``_row_types`` has passed."""
    import numpy as np
    import torch

    from shipyard_amd import ops

    shape = (int(n_rows), int(row_elems))
    tokens = torch.empty(shape, dtype=getattr(torch, out_np.name),
                         device=device)
    segment_ids = torch.empty(shape, dtype=torch.int32, device=device)
    positions = torch.empty(shape, dtype=torch.int32, device=device)
    if shape[0] == 0 or shape[1] == 0:
        return tokens, segment_ids, positions
    size = ops.widen_sizes(src_dtype, 8 * out_np.itemsize)[0]
    order, dst_start, labels = _packed_lists(counts, row, col, row_elems)
    n = counts[order]
    if len(sel):
        scratch, src_off = _decode_selected(
            d_comp, idx, sel, comp_off, starts[order] * size, n * size,
            device, verify)
    else:  # nothing but empty samples: nothing to decode, all of it pad
        scratch = torch.empty(0, dtype=torch.uint8, device=device)
        src_off = _to_device(np.zeros(0, dtype=np.int64), device)
    ops.gather_pack(scratch, src_off, _to_device(n, device),
                    _to_device(dst_start, device),
                    _to_device(labels, device), tokens, segment_ids,
                    positions, src_dtype, pad)
    return tokens, segment_ids, positions


def decode_packed_device(d_comp, idx: ShardIndex, starts, counts, row, col,
                         n_rows: int, device, src_dtype, out_dtype,
                         row_elems: int, pad: int, verify: bool = True):
    """Packed typed read of an uploaded shard payload in HBM: several
    samples per row instead of one sample and its padding.  Returns
    device tensors ``(tokens, segment_ids, positions)`` of shape
    ``[n_rows, row_elems]``, ``tokens`` of ``out_dtype`` (int32 or
    int64), the other two int32.

    Sample ``i`` is the ``counts[i]`` elements of type ``src_dtype``
    from element ``starts[i]`` of the raw data (units and types as for
    ``decode_rows_device``).  It lands, widened, at
    ``tokens[row[i], col[i]:col[i] + counts[i]]``.  There ``positions``
    is ``0 .. counts[i] - 1``, position ids that restart at every
    sample, and ``segment_ids`` is the sample's label: 1 + the number
    of non-empty samples of the same row at a smaller column, so
    ``segment_ids[r, a] == segment_ids[r, b] != 0`` is the
    block-diagonal attention mask.  An empty sample appears nowhere and
    takes no label.  Every element that no sample covers, a gap inside
    a row as well as its tail, holds ``pad`` in ``tokens`` and 0 in the
    other two.  Samples come in any order and may repeat or overlap in
    the source, not in the destination.  ``plan_packed_rows`` makes a
    next-fit ``row``/``col``/``n_rows``; any other plan that passes the
    checks will do.

    Everything up to the last step is ``decode_rows_device``'s: the
    table is validated, the blocks that hold an element of a sample are
    selected, decoded into the compact scratch, unfiltered and, with
    ``verify``, CRC-checked (only those blocks).  The non-empty samples
    are stable-sorted by destination on the host and ``ops.gather_pack``
    writes all three outputs in one launch, nothing pre-filled.

    Each of these is a ValueError raised before a tensor is made or a
    kernel launched, naming the first bad sample in the caller's order:
    everything ``decode_rows_device`` checks for ``starts``/``counts``,
    the types and ``pad``; unequal lengths of the four sequences;
    ``n_rows < 0``; a ``row[i]`` outside ``0 .. n_rows - 1``;
    ``col[i] < 0``; ``col[i] + counts[i] > row_elems``; two non-empty
    samples of one row that overlap (named: the later one in the
    caller's order).  ``n_rows == 0`` or ``row_elems == 0``: empty
    tensors and no launch.  Samples that are all empty: ``pad`` and
    zeros, written by the kernel, and nothing is decoded.

    Peak HBM on top of the payload is that of ``decode_rows_device``
    with R = ``n_rows * row_elems * (out_dtype.itemsize + 8)``."""
    validate_index(idx, d_comp.numel(), for_gpu=True)
    size, _, out_np, pad = _row_types(src_dtype, out_dtype, pad)
    starts, counts, row, col = _as_packed(
        starts, counts, row, col, n_rows, size, idx.raw_size, row_elems)
    sel = _select_blocks(starts * size, counts * size, int(idx.block_raw),
                         idx.n_blocks)
    return _decode_packed(d_comp, idx, sel, idx.table["comp_off"][sel],
                          starts, counts, row, col, n_rows, device, verify,
                          src_dtype, out_np, row_elems, pad)


# ------------------------------------------------------------- row writes
def _narrow_types(dst_dtype):
    """(element bytes, numpy dtype, smallest value, largest value) of a
    row writer's destination type; ValueError for an unknown one."""
    import numpy as np

    from shipyard_amd import ops

    size, signed = ops.narrow_sizes(dst_dtype)
    bits = 8 * size
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else \
        (0, (1 << bits) - 1)
    return size, np.dtype(f"<{'i' if signed else 'u'}{size}"), lo, hi


def _row_start(counts, n: int, row_elems: int):
    """``counts`` (a host sequence, a numpy array or a tensor, which is
    copied to the host) checked against the ``[n, row_elems]`` batch
    they describe, as their exclusive prefix sum: a numpy int64 array of
    ``n + 1`` entries.  ValueError names the first bad row."""
    import numpy as np

    if hasattr(counts, "detach"):  # a tensor: one D2H when on a device
        counts = counts.detach().cpu().numpy()
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(counts) != n:
        raise ValueError(f"rows: {len(counts)} counts for {n} rows")
    bad = (counts < 0) | (counts > row_elems)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(
            f"rows: row {i} has count {int(counts[i])}, must be 0.."
            f"{row_elems} (row_elems)")
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=row_start[1:])
    return row_start


def _stream_row(row_start, index: int) -> int:
    """The row that holds stream element ``index``: the last one that
    starts at or before it (rows in front of it that start there too
    are empty)."""
    import numpy as np

    return int(np.searchsorted(row_start, index, side="right")) - 1


def _misfit_error(row_start, index: int, value: int, dst_dtype, lo: int,
                  hi: int) -> ValueError:
    """The error of both row writers for the value at stream index
    ``index``, the first one that ``dst_dtype`` cannot represent."""
    row = _stream_row(row_start, index)
    return ValueError(
        f"rows: row {row}, column {index - int(row_start[row])} holds "
        f"{value}, which {dst_dtype} ({lo}..{hi}) cannot represent")


def narrow_rows_numpy(rows, counts, dst_dtype):
    """CPU reference of the row writers: the live prefix of every row of
    the ``[n, T]`` int32 or int64 array ``rows`` (``counts[i]`` elements
    of row ``i``; what lies behind them is padding and is never looked
    at) as one dense stream of little-endian ``dst_dtype`` elements
    (``u1``, ``u2``, ``i2``, ``u4``, ``i4``).  Returns ``(bytes,
    row_start)``: ``row_start`` is the exclusive prefix sum of the
    counts, a numpy int64 array of ``n + 1`` entries in elements, so row
    ``i`` is elements ``row_start[i]:row_start[i + 1]`` of the stream
    and ``row_start[:-1]``, ``np.diff(row_start)`` are the ``starts``
    and ``counts`` of the row readers.

    ValueError for ``rows`` that is not a 2-D int32/int64 array, an
    unknown ``dst_dtype``, counts of another length than ``n`` or
    outside ``0..T`` (the first bad row is named), and for a live value
    that ``dst_dtype`` cannot represent: the first one in stream order,
    with its row, column and value."""
    import numpy as np

    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.dtype not in (np.dtype(np.int32),
                                            np.dtype(np.int64)):
        raise ValueError(
            "rows: the batch must be a 2-D int32 or int64 array, not "
            f"{rows.ndim}-D {rows.dtype}")
    _, dst_np, lo, hi = _narrow_types(dst_dtype)
    n, row_elems = rows.shape
    row_start = _row_start(counts, n, row_elems)
    live = np.arange(row_elems)[None, :] < np.diff(row_start)[:, None]
    vals = rows[live]  # row-major: stream order
    bad = (vals < lo) | (vals > hi)
    if bad.any():
        e = int(np.argmax(bad))
        raise _misfit_error(row_start, e, int(vals[e]), dst_dtype, lo, hi)
    return vals.astype(dst_np).tobytes(), row_start


def narrow_rows_device(rows, counts, dst_dtype):
    """``narrow_rows_numpy`` on the GPU: ``rows`` is an ``[n, T]`` int32
    or int64 CUDA tensor, the stream comes back as a uint8 CUDA tensor
    of ``row_start[n] * S`` bytes next to the numpy ``row_start``.
    Streams of several batches can be concatenated (their ``row_start``
    shifted) and handed to ``pack_gpu``.

    ``counts`` may be a host sequence, a numpy array or a device tensor
    (one D2H); they are checked on the host as in ``narrow_rows_numpy``
    before anything is launched.  Then the prefix sum is uploaded,
    ``ops.compact_narrow`` makes one launch, and its status word is read
    back, the one synchronise of the call.  A live value that
    ``dst_dtype`` cannot represent raises the ValueError of
    ``narrow_rows_numpy``, same first offender and same text; padding
    columns are never loaded.  A ``rows`` that is not contiguous is
    copied first."""
    import torch

    from shipyard_amd import ops

    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or \
            rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            "rows: the batch must be a 2-D int32 or int64 tensor")
    if not rows.is_cuda:
        raise ValueError(f"rows: the batch is on {rows.device}, not on a "
                         "GPU (narrow_rows_numpy is the CPU path)")
    size, _, lo, hi = _narrow_types(dst_dtype)
    n, row_elems = rows.shape
    row_start = _row_start(counts, n, row_elems)
    total = int(row_start[n])
    stream = torch.empty(total * size, dtype=torch.uint8, device=rows.device)
    if total == 0:
        return stream, row_start
    clean = (1 << 63) - 1
    status = torch.full((1,), clean, dtype=torch.int64, device=rows.device)
    rows = rows.contiguous()
    ops.compact_narrow(rows, _to_device(row_start, rows.device), stream,
                       dst_dtype, status)
    first = int(status.item())  # the synchronise
    if first != clean:
        row = _stream_row(row_start, first)
        value = int(rows[row, first - int(row_start[row])].item())
        raise _misfit_error(row_start, first, value, dst_dtype, lo, hi)
    return stream, row_start


def pack_rows(rows, counts, dst_dtype, block_raw: int = DEFAULT_BLOCK_RAW,
              shuffle_elem: int = 0, delta_elem: int = 0,
              bitshuffle_elem: int = 0, workers: Optional[int] = None):
    """Author a typed shard from a padded batch on the CPU:
    ``narrow_rows_numpy`` followed by ``pack``.  Returns ``(shard bytes,
    row_start)``; the shard's raw data is the stream of ``dst_dtype``
    elements, and ``read_rows_cpu`` / ``ShardStager.stage_rows`` with
    ``starts = row_start[:-1]``, ``counts = np.diff(row_start)`` and the
    batch's pad give the batch back.  The offsets travel as a shard of
    their own: ``pack(row_start.tobytes(), delta_elem=8,
    bitshuffle_elem=8)``.  The filter keywords and ``workers`` are
    ``pack``'s (``shuffle_elem`` of the element size suits token
    ids)."""
    elems = _filter_elems("pack_rows", locals())
    stream, row_start = narrow_rows_numpy(rows, counts, dst_dtype)
    return pack(stream, block_raw=block_raw, workers=workers,
                **elems), row_start


def pack_rows_gpu(rows, counts, dst_dtype,
                  block_raw: int = DEFAULT_BLOCK_RAW, shuffle_elem: int = 0,
                  delta_elem: int = 0, bitshuffle_elem: int = 0):
    """``pack_rows`` on the GPU for an ``[n, T]`` CUDA tensor:
    ``narrow_rows_device`` followed by ``pack_gpu`` on the stream, which
    never leaves HBM in between.  ``block_raw`` and the filter keywords
    are ``pack_gpu``'s and are checked before anything touches the
    device.  Output equals ``pack_gpu`` of ``narrow_rows_numpy``'s
    stream byte for byte."""
    if not gpu_block_raw_ok(block_raw):
        raise ValueError(
            f"pack_rows_gpu: block_raw={block_raw} must be a multiple of "
            f"{GPU_BLOCK_ALIGN} and at most {GPU_LZ4_BLOCK_MAX}")
    elems = _filter_elems("pack_rows_gpu", locals())
    stream, row_start = narrow_rows_device(rows, counts, dst_dtype)
    return pack_gpu(stream, block_raw=block_raw, **elems), row_start


def pack_rows_auto(rows, counts, dst_dtype,
                   block_raw: int = DEFAULT_BLOCK_RAW,
                   workers: Optional[int] = None,
                   gpu_threshold: int = 1 << 20, shuffle_elem: int = 0,
                   delta_elem: int = 0, bitshuffle_elem: int = 0):
    """``pack_rows`` wherever the batch is.  A CUDA tensor is narrowed
    on its device and written by ``pack_rows_gpu`` (by the CPU writer
    from the copied-back stream when ``block_raw`` is one that the GPU
    writer does not take).  A host batch is narrowed by
    ``narrow_rows_numpy`` and its stream goes to ``pack_auto``, whose
    rules decide: the GPU writer when a GPU is present, the stream
    reaches ``gpu_threshold`` bytes and ``block_raw`` suits it, the CPU
    writer otherwise."""
    elems = _filter_elems("pack_rows_auto", locals())
    if getattr(rows, "is_cuda", False):
        if gpu_block_raw_ok(block_raw):
            return pack_rows_gpu(rows, counts, dst_dtype,
                                 block_raw=block_raw, **elems)
        stream, row_start = narrow_rows_device(rows, counts, dst_dtype)
        return pack(stream.cpu().numpy().tobytes(), block_raw=block_raw,
                    workers=workers, **elems), row_start
    stream, row_start = narrow_rows_numpy(rows, counts, dst_dtype)
    return pack_auto(stream, block_raw=block_raw, workers=workers,
                     gpu_threshold=gpu_threshold, **elems), row_start


def unpack_gpu(buf: bytes, device=None, verify: bool = True):
    """GPU reader: upload payload once, LZ4-decode all blocks on the
    MI355X, CRC32C-verify the decoded bytes, return a uint8 CUDA tensor.

    This is the cascade-analogue/stager hot path: NVMe -> pinned host ->
    HBM (hipMemcpyAsync under torch) -> wave-cooperative decode -> chunk
    CRC — no CPU inflate, no CPU hash.
    """
    import torch

    dev = device or torch.device("cuda", torch.cuda.current_device())
    idx = read_index(buf)
    payload = buf[idx.payload_off:]
    if not payload:
        # frombuffer rejects 0-length buffers.  Only the empty shard may
        # have no payload: a shard cut at the end of its table raises
        # here instead of coming back as an empty tensor.
        validate_index(idx, 0, for_gpu=True)
        return torch.empty(0, dtype=torch.uint8, device=dev)
    d_comp = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(
        dev, non_blocking=True)
    return decode_device(d_comp, idx, dev, verify=verify)


def pack_file(src: Path, dst: Path, block_raw: int = DEFAULT_BLOCK_RAW,
              compress: bool = True, shuffle_elem: int = 0,
              delta_elem: int = 0, bitshuffle_elem: int = 0) -> ShardIndex:
    data = Path(src).read_bytes()
    packed = pack(data, block_raw=block_raw, compress=compress,
                  **_filter_elems("pack_file", locals()))
    Path(dst).write_bytes(packed)
    return read_index(packed)
