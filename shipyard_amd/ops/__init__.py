"""shipyard_amd.ops — HIP data-plane kernels (gfx950/MI355X) + bindings.

The framework's native hot paths: chunked CRC32C, LZ4
block decode, SHA-256 page digests.  The library is loaded via ctypes and
driven with raw device pointers from torch tensors on the current torch
HIP stream.

Contract: on a machine with a GPU these ops REQUIRE the compiled
``libshipyardops.so`` and raise ``OpsUnavailableError`` if it is missing —
there is no silent eager fallback on the GPU path.  On CPU-only machines
(`torch.cuda.is_available()` is False) the CPU reference implementations
in :mod:`shipyard_amd.ops.gf2` / :mod:`shipyard_amd.data.integrity` are
the supported path.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

from . import gf2

# device-side GF(2) operator cache: (kind, chunk, n_chains, device) ->
# tensor (the wrapper is called once per staged file; rebuilding the
# 32x32 operators host-side each call costs more than the kernel at
# 4 TB/s).  The v2 operator set has log2(256 * n_chains) levels of
# shift-by-(chunk / (256 * n_chains)) * 2^k, so the chain count is part
# of the key; the v3 set is geometry-fixed (n_chains == 0 there).
_MAT_CACHE: dict = {}


def _cached_mats(kind: str, chunk_size: int, device, n_chains: int = 0):
    import torch

    if kind == "coal":
        n_chains = 0
    elif n_chains <= 0:
        raise ValueError("v2 CRC operators need the launch's chain count")
    key = (kind, chunk_size, n_chains, str(device))
    t = _MAT_CACHE.get(key)
    if t is None:
        if kind == "coal":
            vals = gf2.coalesced_matrices()
        else:
            vals = gf2.level_matrices(chunk_size, 256 * n_chains)
        t = torch.tensor(vals, dtype=torch.int64).to(
            torch.uint32).to(device)
        _MAT_CACHE[key] = t
    return t

_LIB_PATH = Path(__file__).resolve().parent / "libshipyardops.so"
_lib: Optional[ctypes.CDLL] = None


class OpsUnavailableError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def is_built() -> bool:
    return _LIB_PATH.exists()


_P, _STR = ctypes.c_void_p, ctypes.c_char_p
_U32, _U64 = ctypes.c_uint32, ctypes.c_uint64
_INT, _I64 = ctypes.c_int, ctypes.c_int64

_LZ4_DECODE = (_P, _P, _P, _P, _P, _P, _P, _U32, _U32, _P)
_LZ4_COMPRESS_GPU = (_P, _P, _P, _P, _U64, _P, _U32, _U32, _P)
_BLOCK_FILTER = (_P, _P, _U64, _U32, _U32, _INT, _P)

# C entry point -> argument types, one row per ``SY_EXPORT int sy_*``
# prototype in csrc/ (every one returns int; hipStream_t is a pointer).
# _load() applies it, _call() relies on it to convert plain ints, and
# tests/test_ops_bindings.py compares it with the prototypes.
SIGNATURES = {
    "sy_crc32c_chunks": (_P, _U64, _U32, _P, _P, _U64, _U32, _P),
    "sy_crc32c_chunks_coal": (_P, _U64, _U32, _P, _P, _U64, _P),
    "sy_sha256_pages": (_P, _U64, _U32, _P, _U64, _P),
    "sy_lz4_decode_blocks": _LZ4_DECODE,
    "sy_lz4_decode_blocks_pc": _LZ4_DECODE,
    "sy_lz4_compress_blocks_gpu": _LZ4_COMPRESS_GPU,
    "sy_lz4_compress_blocks_gpu2": _LZ4_COMPRESS_GPU,
    "sy_lz4_compress_blocks": (_STR, _U64, _U32, _P, _U64, _P, _U32, _INT),
    "sy_gather_copy": (_P, _P, _P, _P, _P, _U32, _P),
    "sy_gather_range_pieces": (_P, _P, _P, _P, _U32, _P),
    "sy_gather_ranges": (_P, _U64, _P, _P, _P, _P, _P, _U32, _P),
    "sy_gather_widen": (_P, _P, _P, _P, _U32, _U32, _U32, _INT, _U32, _I64,
                        _P),
    "sy_compact_narrow": (_P, _P, _P, _P, _U32, _U32, _U32, _U32, _INT, _P),
    "sy_gather_pack": (_P, _P, _P, _P, _P, _P, _P, _P, _U32, _U64, _U32, _INT,
                       _U32, _I64, _P),
    "sy_byte_shuffle": _BLOCK_FILTER,
    "sy_delta_filter": _BLOCK_FILTER,
    "sy_bit_shuffle": _BLOCK_FILTER,
    "sy_stage_file": (_STR, _P, _U64, _U64, _U64, _INT, _P,
                      ctypes.POINTER(ctypes.c_double)),
}


def _load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise OpsUnavailableError(
            f"HIP ops library missing: {_LIB_PATH}. "
            "Build it with `python -m shipyard_amd.ops.build` "
            "(hipcc cross-compiles for gfx950 without a GPU)."
        )
    # ORDER MATTERS (found on hardware): dlopen'ing the kernel library
    # BEFORE the HIP runtime is initialized (e.g. the CPU compressor
    # entry point running first) registers its code objects into an
    # uninitialized runtime, and later kernel launches fail with
    # hipErrorNoDevice even though torch's own kernels run.  Force
    # torch's HIP init first whenever a device exists.
    try:
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass  # CPU-only host: the CPU entry points need no runtime
    lib = ctypes.CDLL(str(_LIB_PATH))
    for entry, argtypes in SIGNATURES.items():
        fn = getattr(lib, entry)
        fn.restype = ctypes.c_int
        fn.argtypes = list(argtypes)
    _lib = lib
    return lib


def _stream() -> ctypes.c_void_p:
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}")


def _call(entry: str, *args, stream: bool = True) -> int:
    """Call the C entry point ``entry`` of the library ``_load()`` gives
    at this moment.  A tensor (anything with ``data_ptr()``) and a numpy
    array go as the address of their first byte; a pointer plus an
    offset is passed as an explicit ``ctypes.c_void_p``; ints and bytes
    are left to the entry point's ``argtypes``.  With ``stream`` the
    current torch stream is appended as the last argument.  RuntimeError
    naming ``entry`` for a non-zero return code; returns it (0)
    otherwise."""
    fn = getattr(_load(), entry)
    conv = []
    for a in args:
        if type(a) is not int:  # this runs once per launch: ints are cheap
            data_ptr = getattr(a, "data_ptr", None)
            if data_ptr is not None:
                a = _P(data_ptr())
            elif hasattr(a, "ctypes"):
                a = _P(a.ctypes.data)
        conv.append(a)
    if stream:
        conv.append(_stream())
    rc = fn(*conv)
    _check(rc, entry)
    return rc


def _check_aligned16(t, what: str, where: str = "", advice: str = "") -> None:
    """ValueError unless the base pointer of tensor ``t``, which the
    message calls ``what``, is a multiple of 16 (the kernels walk it
    with uint4 accesses)."""
    if t.data_ptr() % 16:
        raise ValueError(
            f"{what} base pointer must be 16-byte aligned{where} (tensor "
            f"storage offset {t.storage_offset()}){advice}")


_CLONE_IT = "; pass an aligned view or .clone() it"


def _check_index_tensors(op: str, src, named) -> None:
    """The index tensors of a gather, ``named`` as (tensor, name) pairs:
    each int64, contiguous 1-D and on ``src``'s device, or ValueError in
    ``op``'s name."""
    import torch

    for t, which in named:
        if t.dtype != torch.int64:
            raise ValueError(f"{op}: {which} must be int64, not {t.dtype}")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError(
                f"{op}: {which} must be a contiguous 1-D tensor")
        if t.device != src.device:
            raise ValueError(
                f"{op}: {which} is on {t.device}, src on {src.device}")


def _check_u8_device(t, what: str) -> None:
    """Input contract of the kernels that walk a tensor with uint4
    accesses from its base: uint8, contiguous, CUDA, and a base pointer
    that is 16-byte aligned.  A contiguous view such as ``buf[1:]``
    meets everything but the last and would fault or tear on the
    device, so misalignment is a ValueError raised before any launch
    (checked ahead of the device assert so the rule is testable on
    hosts without a GPU)."""
    import torch

    assert t.dtype == torch.uint8 and t.is_contiguous(), what
    _check_aligned16(t, f"{what}:", advice=_CLONE_IT)
    assert t.is_cuda, what


def crc32c_chunks_coal_raw(data, chunk_size: int = 256 * 1024):
    """v3 coalesced-tile CRC kernel (experimental): RAW per-chunk CRCs
    for a tensor whose length is an exact multiple of chunk_size
    (chunk_size % 32768 == 0).  See crc32c.hip v3 notes.

    ``data``: contiguous uint8 CUDA tensor whose base pointer is
    16-byte aligned (ValueError otherwise, before launch)."""
    import torch

    _check_u8_device(data, "crc32c_chunks_coal_raw")
    n = data.numel()
    if chunk_size % 32768 or n % chunk_size:
        raise ValueError("coalesced CRC needs chunk%32768==0 and "
                         "full chunks")
    n_chunks = n // chunk_size
    out = torch.empty(n_chunks, dtype=torch.uint32, device=data.device)
    _call("sy_crc32c_chunks_coal", data, n, chunk_size,
          _cached_mats("coal", chunk_size, data.device), out, n_chunks)
    return out.cpu()


def crc32c_chunks(data, chunk_size: int = 256 * 1024, finish: bool = True):
    """CRC32C of each ``chunk_size`` slice of a uint8 CUDA tensor.

    Returns a CPU torch.uint32 tensor of per-chunk CRCs (standard
    init/final-xor applied when ``finish``).  MI355X-native replacement
    for the reference's CPU-side file hashing (convoy/util.py:461-508).

    ``data`` must be contiguous with a 16-byte-aligned base pointer
    (both kernels load uint4 from the base); a misaligned view raises
    ValueError before launch.
    """
    import torch

    _check_u8_device(data, "crc32c_chunks")
    n = data.numel()
    n_chunks = (n + chunk_size - 1) // chunk_size
    out = torch.empty(n_chunks, dtype=torch.uint32, device=data.device)
    n_full = n // chunk_size
    # v3 coalesced-tile kernel for the full-chunk prefix (4.2 TB/s vs
    # v2's 2.7 at 256 KiB chunks — profiles/data_plane_r02.md); v2
    # handles the ragged tail chunk via its front-pad semantics.  Both
    # emit identical RAW CRCs.
    use_v3 = chunk_size % 32768 == 0 and n_full > 0 and \
        os.environ.get("SHIPYARD_CRC_V3", "1") != "0"
    if use_v3:
        _call("sy_crc32c_chunks_coal", data, n_full * chunk_size, chunk_size,
              _cached_mats("coal", chunk_size, data.device), out, n_full)
    if not use_v3 or n_chunks > n_full:
        start = n_full if use_v3 else 0
        # resolved once: the cached operators and the launch agree
        n_chains = gf2.pick_crc_chains(chunk_size)
        _call("sy_crc32c_chunks",
              ctypes.c_void_p(data.data_ptr() + start * chunk_size),
              n - start * chunk_size, chunk_size,
              _cached_mats("v2", chunk_size, data.device, n_chains),
              ctypes.c_void_p(out.data_ptr() + start * 4),
              n_chunks - start, n_chains)
    raw = out.cpu()
    if not finish:
        return raw
    full = gf2.matvec(list(gf2.zero_shift_operator(chunk_size)), 0xFFFFFFFF)
    tail_len = n - (n_chunks - 1) * chunk_size
    tail = gf2.matvec(list(gf2.zero_shift_operator(tail_len)), 0xFFFFFFFF)
    import numpy as np

    rawnp = raw.numpy().astype(np.uint32)
    finnp = rawnp ^ np.uint32(full) ^ np.uint32(0xFFFFFFFF)
    if n_chunks:
        finnp[-1] = rawnp[-1] ^ np.uint32(tail) ^ np.uint32(0xFFFFFFFF)
    fin = torch.from_numpy(finnp.copy())
    return fin


def crc32c_file_digest(data, chunk_size: int = 256 * 1024) -> int:
    """Whole-buffer CRC32C via GPU chunk CRCs + host GF(2) combine."""
    raw = crc32c_chunks(data, chunk_size, finish=False).numpy()
    n = data.numel()
    acc = 0
    pos = 0
    for i, r in enumerate(raw.astype("uint32").tolist()):
        clen = min(chunk_size, n - pos)
        acc = gf2.combine_raw(acc, int(r), clen)
        pos += clen
    return gf2.finish(acc, n)


def lz4_compress_blocks_gpu(data, block_raw: int,
                            screen: bool = None):
    """GPU LZ4 block compression: one wave per block.  Two matchers:

    * screen=False — v1, the CPU greedy policy exactly (byte-identical
      streams; the testing baseline);
    * screen=True — v2 wave-screen: 64 positions per LDS round trip
      with deterministic atomicMax inserts (valid LZ4, slightly
      different stream; faster).

    Default comes from SHIPYARD_LZ4C_SCREEN (unset -> v2 screen: on
    text it matches v1 within ~2% ratio and speed, on incompressible
    content it is ~19x faster to give up, which dominates mixed
    real-world shards).  ``data``
    is a uint8 CUDA tensor; returns (slotted uint8 CUDA tensor,
    stride, uint32 lens CPU tensor) — lens[b] == 0 means
    incompressible (store raw).  The staging loop loads uint4 from
    ``data``'s base: it must be contiguous and 16-byte aligned
    (ValueError before launch otherwise).  Every block starts at a
    multiple of ``block_raw``, so ``block_raw`` must be a positive
    multiple of 16 for the same reason (ValueError as well)."""
    if screen is None:
        screen = os.environ.get("SHIPYARD_LZ4C_SCREEN", "1") == "1"

    import torch

    if block_raw <= 0 or block_raw % 16:
        raise ValueError(
            f"lz4_compress_blocks_gpu: block_raw must be a positive "
            f"multiple of 16 (uint4 staging loads), got {block_raw}")
    _check_u8_device(data, "lz4_compress_blocks_gpu")
    n = data.numel()
    n_blocks = (n + block_raw - 1) // block_raw
    if n_blocks == 0:
        return None, 0, None
    import numpy as np

    offs = np.arange(n_blocks, dtype=np.uint64) * block_raw
    lens_in = np.minimum(
        np.full(n_blocks, block_raw, dtype=np.uint64),
        n - offs).astype(np.uint32)
    d_off = torch.from_numpy(offs.view(np.int64)).to(data.device)
    d_len = torch.from_numpy(lens_in.view(np.int32)).to(data.device)
    stride = block_raw  # emit caps at raw size (else stored)
    d_out = torch.empty(n_blocks * stride, dtype=torch.uint8,
                        device=data.device)
    d_lens = torch.zeros(n_blocks, dtype=torch.int32,
                         device=data.device)
    _call("sy_lz4_compress_blocks_gpu2" if screen
          else "sy_lz4_compress_blocks_gpu",
          data, d_off, d_len, d_out, stride, d_lens, n_blocks, block_raw)
    return d_out, stride, d_lens.cpu()


def lz4_compress_blocks(data: bytes, block_raw: int,
                        threads: int = 0):
    """CPU multi-threaded LZ4 block compression (native authoring path
    for SYSHARD).  Returns a list with one entry per block: compressed
    bytes, or None where the block is incompressible (store raw).
    Host-only — needs no GPU, just the built library."""
    import numpy as np

    n_blocks = (len(data) + block_raw - 1) // block_raw
    if n_blocks == 0:
        return []
    stride = block_raw + block_raw // 255 + 32
    dst = np.empty(n_blocks * stride, dtype=np.uint8)
    lens = np.zeros(n_blocks, dtype=np.uint32)
    _call("sy_lz4_compress_blocks", data, len(data), block_raw, dst, stride,
          lens, n_blocks, threads, stream=False)
    out = []
    for b in range(n_blocks):
        ln = int(lens[b])
        out.append(bytes(dst[b * stride:b * stride + ln].tobytes())
                   if ln else None)
    return out


def native_compress_available() -> bool:
    try:
        return hasattr(_load(), "sy_lz4_compress_blocks")
    except Exception:
        return False


def gather_copy(src, src_off, dst, dst_off, lens):
    """Batched device gather-copy (stored shard blocks): one workgroup
    per block, uint4 body + byte tail.  src_off/dst_off int64 byte
    offsets (src 16 B aligned by the format), lens uint32."""
    n = src_off.numel()
    if n == 0:
        return
    _call("sy_gather_copy", src, src_off, dst, dst_off, lens, n)


def gather_ranges(src, src_off, lens, dst, dst_off):
    """Ragged device gather: for every ``i``,
    ``dst[dst_off[i]:dst_off[i]+lens[i]] = src[src_off[i]:src_off[i]+lens[i]]``.

    ``src`` and ``dst`` are contiguous uint8 CUDA tensors on one device;
    ``src_off``, ``lens`` and ``dst_off`` are int64 tensors of equal
    length on that device.  Any byte alignment on either side (the
    tensors' base pointers included), any length (0 too), ranges in any
    order; source ranges may overlap or repeat.  A wrong dtype or device
    of an offset tensor, or unequal lengths, is a ValueError raised
    before any launch; no ranges at all is a no-op without a launch.

    The caller guarantees, and nothing checks, that
    * the destination ranges do not overlap each other,
    * ``dst`` does not overlap ``src``,
    * every range lies inside its tensor: the numbers are on the
      device, and looking at them here would cost a synchronise
      (``shardfmt.decode_ranges_device`` checks its ranges on the host,
      where they come from).

    Three launches, no host sync: the piece count of every range, its
    prefix sum (``torch.cumsum``), and the gather, whose waves split the
    bytes and not the ranges between them (gather_ranges.hip)."""
    import torch

    for t, which in ((src, "src"), (dst, "dst")):
        assert t.dtype == torch.uint8 and t.is_contiguous(), \
            f"gather_ranges: {which}"
    _check_index_tensors("gather_ranges", src, (
        (src_off, "src_off"), (lens, "lens"), (dst_off, "dst_off")))
    n = lens.numel()
    if src_off.numel() != n or dst_off.numel() != n:
        raise ValueError(
            f"gather_ranges: {src_off.numel()} source offsets, {n} "
            f"lengths and {dst_off.numel()} destination offsets")
    if n >= 1 << 32:
        raise ValueError("gather_ranges: at most 2**32 - 1 ranges")
    assert src.is_cuda and dst.is_cuda and src.device == dst.device, \
        "gather_ranges: CUDA tensors on one device"
    if n == 0:
        return
    pieces = torch.empty(n, dtype=torch.int64, device=src.device)
    _call("sy_gather_range_pieces", dst, dst_off, lens, pieces, n)
    cum = torch.cumsum(pieces, 0)
    _call("sy_gather_ranges", src, src.numel(), src_off, lens, dst, dst_off,
          cum, n)


# source element types of gather_widen: name -> (bytes, signed), all
# little-endian
WIDEN_SRC_DTYPES = {"u1": (1, False), "u2": (2, False), "i2": (2, True),
                    "u4": (4, False), "i4": (4, True)}
# the kernel finds a lane's row with 32-bit arithmetic on column + 256
WIDEN_MAX_ROW_ELEMS = (1 << 31) - 257


def widen_sizes(src_dtype, dst_bits: int) -> tuple:
    """(source element bytes, signed) of a ``gather_widen`` source type
    for a destination of ``dst_bits`` (32 or 64) bit signed integers.
    ValueError for an unknown type and for ``u4`` into 32 bits, the one
    pair that cannot keep every value."""
    if src_dtype not in WIDEN_SRC_DTYPES:
        raise ValueError(
            f"gather_widen: src_dtype={src_dtype!r} is not one of "
            f"{sorted(WIDEN_SRC_DTYPES)}")
    size, signed = WIDEN_SRC_DTYPES[src_dtype]
    if 8 * size - signed > dst_bits - 1:
        raise ValueError(
            f"gather_widen: {src_dtype} does not fit int{dst_bits} (only "
            "value-preserving conversions)")
    return size, signed


def check_widen_pad(pad, dst_bits: int) -> int:
    """``pad`` as a Python int; ValueError unless it is an integer that
    an int``dst_bits`` holds."""
    import operator

    try:
        pad = operator.index(pad)
    except TypeError:
        raise ValueError(f"gather_widen: pad={pad!r} is not an integer")
    if not -(1 << (dst_bits - 1)) <= pad < 1 << (dst_bits - 1):
        raise ValueError(
            f"gather_widen: pad={pad} does not fit int{dst_bits}")
    return pad


def gather_widen(src, src_off, counts, dst, src_dtype: str, pad: int):
    """Typed row gather: for every row ``i`` of the ``[n, T]`` tensor
    ``dst``, ``dst[i, :counts[i]]`` receives the ``counts[i]`` elements
    of type ``src_dtype`` that start at byte ``src_off[i]`` of ``src``,
    zero-extended (``u1``, ``u2``, ``u4``) or sign-extended (``i2``,
    ``i4``), and ``dst[i, counts[i]:]`` receives ``pad``.

    ``src`` is a contiguous uint8 CUDA tensor whose base pointer is a
    multiple of the source element size S; ``src_off`` (int64, bytes,
    multiples of S) and ``counts`` (int64, elements, 0..T) are 1-D
    tensors of length n on its device; ``dst`` is a contiguous 2-D
    ``torch.int32`` or ``torch.int64`` tensor, whose base may be any
    multiple of its element size (a view at +4 or +8 inside an
    allocation is fine).  Only value-preserving conversions: every type
    into int64, all but ``u4`` into int32 (``i4`` is a copy).  Rows in
    any order; source rows may overlap or repeat.

    One launch (gather_widen.hip): every element of ``dst`` is written
    exactly once, so the caller does not pre-fill it, no byte outside
    ``dst`` is written, and only the bytes of the rows are loaded.

    A ``src`` that is not contiguous uint8, a wrong dtype or device of
    an index tensor or of ``dst``, tensors that are not on a GPU,
    unequal lengths, ``n != dst.shape[0]``, an unknown or forbidden
    conversion, a ``pad`` that ``dst.dtype`` cannot hold and a ``src``
    base that is no multiple of S are each a ValueError raised before
    any launch;
    ``n == 0`` or ``T == 0`` is a no-op without a launch.

    The caller guarantees, and nothing checks, that every row lies
    inside ``src``, that ``0 <= counts[i] <= T`` and that ``dst`` does
    not overlap ``src``: the numbers are on the device, and looking at
    them here would cost a synchronise (``shardfmt.decode_rows_device``
    checks its rows on the host, where they come from)."""
    import torch

    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError(
            "gather_widen: src must be a contiguous uint8 tensor")
    if dst.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            f"gather_widen: dst must be int32 or int64, not {dst.dtype}")
    if dst.dim() != 2 or not dst.is_contiguous():
        raise ValueError("gather_widen: dst must be a contiguous [n, T] "
                         "tensor")
    dst_size = dst.element_size()
    size, signed = widen_sizes(src_dtype, 8 * dst_size)
    pad = check_widen_pad(pad, 8 * dst_size)
    if src.data_ptr() % size:
        raise ValueError(
            f"gather_widen: src base pointer must be a multiple of the "
            f"{size}-byte element (tensor storage offset "
            f"{src.storage_offset()})")
    _check_index_tensors("gather_widen", src, (
        (src_off, "src_off"), (counts, "counts")))
    n, row_elems = dst.shape
    if src_off.numel() != counts.numel() or counts.numel() != n:
        raise ValueError(
            f"gather_widen: {src_off.numel()} source offsets and "
            f"{counts.numel()} counts for {n} rows of dst")
    if n >= 1 << 32 or row_elems > WIDEN_MAX_ROW_ELEMS:
        raise ValueError(
            "gather_widen: at most 2**32 - 1 rows of at most "
            f"{WIDEN_MAX_ROW_ELEMS} elements")
    if dst.device != src.device:
        raise ValueError(
            f"gather_widen: dst is on {dst.device}, src on {src.device}")
    if not src.is_cuda:
        raise ValueError(
            f"gather_widen: src and dst are on {src.device}, not on a GPU")
    if n == 0 or row_elems == 0:
        return
    _call("sy_gather_widen", src, src_off, counts, dst, n, row_elems, size,
          int(signed), dst_size, pad)


GATHER_PACK_MAX_SEGMENTS = (1 << 31) - 1


def gather_pack(src, src_off, counts, dst_start, labels, tokens,
                segment_ids, positions, src_dtype: str, pad: int):
    """Packed typed gather: several source runs per row of a batch, with
    the two tensors that say which run an element belongs to.  For every
    segment ``i`` of the m given, with ``e = dst_start[i]`` an index into
    the flattened ``[n, T]`` outputs and ``c = counts[i]``:
    ``tokens.view(-1)[e:e + c]`` receives the ``c`` elements of type
    ``src_dtype`` that start at byte ``src_off[i]`` of ``src``,
    zero-extended (``u1``, ``u2``, ``u4``) or sign-extended (``i2``,
    ``i4``); ``segment_ids.view(-1)[e:e + c]`` receives ``labels[i]``
    and ``positions.view(-1)[e:e + c]`` receives ``0, 1, ..., c - 1``.
    Every element that no segment covers, in front of the first one, in
    a gap or behind the last one, receives ``pad`` in ``tokens`` and 0
    in the other two.  A segment may run across a row end.

    ``src`` is a contiguous uint8 CUDA tensor whose base pointer is a
    multiple of the source element size S; ``src_off`` (int64, bytes,
    multiples of S), ``counts`` (int64, elements, all > 0) and
    ``dst_start`` (int64, flat elements) are 1-D tensors of length m on
    its device and ``labels`` is an int32 one; ``tokens`` is a
    contiguous 2-D ``torch.int32`` or ``torch.int64`` tensor and
    ``segment_ids`` and ``positions`` are contiguous ``torch.int32``
    tensors of its shape, all three with a 16-byte-aligned base (fresh
    tensors are; the kernel stores whole uint4s from the base and has no
    path for an unaligned head).  Only value-preserving conversions, as
    for ``gather_widen``.  Source runs may overlap or repeat.

    One launch (gather_pack.hip) and no host sync: every element of the
    three outputs is written exactly once, so the caller does not
    pre-fill them, nothing outside them is written, and of ``src`` only
    the bytes of the segments are loaded.

    A ``src`` that is not contiguous uint8, a wrong dtype, shape or
    device of a list or of an output, a non-contiguous tensor, tensors
    that are not on a GPU, lists of unequal lengths, an unknown or
    forbidden conversion, a ``pad`` that ``tokens.dtype`` cannot hold, a
    ``src`` base that is no multiple of S, an output base that is no
    multiple of 16 and more than ``GATHER_PACK_MAX_SEGMENTS``
    (2**31 - 1) segments are each a ValueError raised before any
    launch.  ``n * T == 0`` is a no-op without a launch; ``m == 0`` is
    legal and writes an all-pad output.

    The caller guarantees, and nothing checks, that ``dst_start``
    ascends with ``dst_start[i] + counts[i] <= dst_start[i + 1]``, that
    ``0 < counts[i] < 2**31`` and the last segment ends inside ``n * T``,
    that every segment lies inside ``src``, and that no output overlaps
    ``src`` or another output: the numbers are on the device, and
    looking at them here would cost a synchronise
    (``shardfmt.decode_packed_device`` checks its plan on the host,
    where it comes from)."""
    import torch

    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError(
            "gather_pack: src must be a contiguous uint8 tensor")
    if tokens.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            f"gather_pack: tokens must be int32 or int64, not {tokens.dtype}")
    if tokens.dim() != 2 or not tokens.is_contiguous():
        raise ValueError("gather_pack: tokens must be a contiguous [n, T] "
                         "tensor")
    for t, which in ((segment_ids, "segment_ids"), (positions, "positions")):
        if t.dtype != torch.int32:
            raise ValueError(
                f"gather_pack: {which} must be int32, not {t.dtype}")
        if t.shape != tokens.shape or not t.is_contiguous():
            raise ValueError(
                f"gather_pack: {which} must be a contiguous tensor of "
                f"tokens' shape {tuple(tokens.shape)}, not {tuple(t.shape)}")
    dst_size = tokens.element_size()
    size, signed = widen_sizes(src_dtype, 8 * dst_size)
    pad = check_widen_pad(pad, 8 * dst_size)
    if src.data_ptr() % size:
        raise ValueError(
            f"gather_pack: src base pointer must be a multiple of the "
            f"{size}-byte element (tensor storage offset "
            f"{src.storage_offset()})")
    _check_index_tensors("gather_pack", src, (
        (src_off, "src_off"), (counts, "counts"), (dst_start, "dst_start")))
    if labels.dtype != torch.int32:
        raise ValueError(
            f"gather_pack: labels must be int32, not {labels.dtype}")
    if labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError("gather_pack: labels must be a contiguous 1-D tensor")
    if labels.device != src.device:
        raise ValueError(
            f"gather_pack: labels is on {labels.device}, src on {src.device}")
    m = counts.numel()
    if src_off.numel() != m or dst_start.numel() != m or labels.numel() != m:
        raise ValueError(
            f"gather_pack: {src_off.numel()} source offsets, {m} counts, "
            f"{dst_start.numel()} destination starts and {labels.numel()} "
            "labels")
    if m > GATHER_PACK_MAX_SEGMENTS:
        raise ValueError(
            f"gather_pack: at most {GATHER_PACK_MAX_SEGMENTS} segments")
    for t, which in ((tokens, "tokens"), (segment_ids, "segment_ids"),
                     (positions, "positions")):
        if t.device != src.device:
            raise ValueError(
                f"gather_pack: {which} is on {t.device}, src on {src.device}")
        _check_aligned16(t, f"gather_pack: {which}", advice=_CLONE_IT)
    if not src.is_cuda:
        raise ValueError(
            f"gather_pack: src and the outputs are on {src.device}, not on "
            "a GPU")
    if tokens.numel() == 0:
        return
    _call("sy_gather_pack", src, src_off, counts, dst_start, labels, tokens,
          segment_ids, positions, m, tokens.numel(), size, int(signed),
          dst_size, pad)


def narrow_sizes(dst_dtype) -> tuple:
    """(destination element bytes, signed) of a ``compact_narrow``
    destination type, one of ``WIDEN_SRC_DTYPES``; ValueError for
    anything else."""
    if dst_dtype not in WIDEN_SRC_DTYPES:
        raise ValueError(
            f"compact_narrow: dst_dtype={dst_dtype!r} is not one of "
            f"{sorted(WIDEN_SRC_DTYPES)}")
    return WIDEN_SRC_DTYPES[dst_dtype]


def compact_narrow(src, row_start, dst, dst_dtype: str, status):
    """Typed row compaction, the inverse of ``gather_widen``: the live
    prefix of every row of the ``[n, T]`` tensor ``src`` as one dense
    little-endian stream of ``dst_dtype`` elements.  Element
    ``row_start[i] + c`` of the stream, for
    ``c < row_start[i + 1] - row_start[i]``, is ``src[i, c]`` reduced to
    its low S bytes (S the size of ``dst_dtype``).

    ``src`` is a contiguous 2-D ``torch.int32`` or ``torch.int64`` CUDA
    tensor, whose base may be any multiple of its element size;
    ``row_start`` is the exclusive prefix sum of the rows' live counts,
    a contiguous 1-D int64 tensor of ``n + 1`` entries on ``src``'s
    device (``row_start[0] == 0``, ``row_start[n]`` the total);
    ``dst`` is a contiguous uint8 tensor on that device whose base is
    16-byte aligned; ``dst_dtype`` is one of ``WIDEN_SRC_DTYPES``
    (``u1``, ``u2``, ``i2``, ``u4``, ``i4``; ``i4`` from int32 is a
    plain compaction); ``status`` is an int64 tensor of one element on
    the device that the caller has set to ``INT64_MAX``
    (``2**63 - 1``).

    One launch (compact_narrow.hip) with no host sync, the total is read
    on the device: every byte of ``dst[:total * S]`` is written exactly
    once, no byte behind it is written, only live elements are loaded
    (what the padding columns hold does not matter), and ``status``
    receives the smallest stream index whose value ``dst_dtype`` cannot
    represent (it keeps ``INT64_MAX`` when all fit).  A value that does
    not fit is still stored, truncated; the caller is expected to read
    ``status`` and discard the stream.

    A ``src`` that is not a contiguous 2-D int32/int64 CUDA tensor, an
    unknown ``dst_dtype``, a ``row_start`` of another dtype, shape,
    length or device, a ``dst`` that is not contiguous uint8, is on
    another device or is not 16-byte aligned, a ``status`` that is not
    int64[1] on the device, ``n >= 2**32`` and
    ``T > WIDEN_MAX_ROW_ELEMS`` are each a ValueError raised before any
    launch; ``n == 0`` or ``T == 0`` is a no-op without a launch.

    The caller guarantees, and nothing checks, that ``row_start``
    ascends from 0 in steps of at most T, that ``dst`` holds
    ``row_start[n] * S`` bytes and that it does not overlap ``src``:
    the numbers are on the device, and looking at them here would cost
    a synchronise (``shardfmt.narrow_rows_device`` builds ``row_start``
    from counts it has checked on the host)."""
    import torch

    if src.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            f"compact_narrow: src must be int32 or int64, not {src.dtype}")
    if src.dim() != 2 or not src.is_contiguous():
        raise ValueError("compact_narrow: src must be a contiguous [n, T] "
                         "tensor")
    if not src.is_cuda:
        raise ValueError(
            f"compact_narrow: src is on {src.device}, not on a GPU")
    size, signed = narrow_sizes(dst_dtype)
    _check_index_tensors("compact_narrow", src, ((row_start, "row_start"),))
    n, row_elems = src.shape
    if row_start.numel() != n + 1:
        raise ValueError(
            f"compact_narrow: {row_start.numel()} entries of row_start "
            f"for {n} rows of src, must be {n + 1}")
    if dst.dtype != torch.uint8 or not dst.is_contiguous():
        raise ValueError(
            "compact_narrow: dst must be a contiguous uint8 tensor")
    if dst.device != src.device:
        raise ValueError(
            f"compact_narrow: dst is on {dst.device}, src on {src.device}")
    _check_aligned16(dst, "compact_narrow: dst", advice=_CLONE_IT)
    if status.dtype != torch.int64 or status.numel() != 1 or \
            status.device != src.device:
        raise ValueError(
            "compact_narrow: status must be one int64 on src's device, not "
            f"{status.numel()} of {status.dtype} on {status.device}")
    if n >= 1 << 32 or row_elems > WIDEN_MAX_ROW_ELEMS:
        raise ValueError(
            "compact_narrow: at most 2**32 - 1 rows of at most "
            f"{WIDEN_MAX_ROW_ELEMS} elements")
    if n == 0 or row_elems == 0:
        return
    _call("sy_compact_narrow", src, row_start, dst, status, n, row_elems,
          src.element_size(), size, int(signed))


FILTER_ELEM_SIZES = (2, 4, 8)
FILTER_BLOCK_ALIGN = 4096


def _block_filter(name: str, entry: str, allow_in_place: bool, src, dst,
                  block_raw: int, elem_size: int, inverse: bool) -> None:
    """Argument rules and launch shared by the SYSHARD block filters:
    the op ``name`` bound to the C entry point ``entry``, which takes
    ``dst`` being ``src`` itself only with ``allow_in_place``.  Every
    ValueError comes ahead of the device assert."""
    import torch

    for t, which in ((src, "src"), (dst, "dst")):
        assert t.dtype == torch.uint8 and t.is_contiguous(), \
            f"{name}: {which}"
        _check_aligned16(t, f"{name}: {which}", advice=_CLONE_IT)
    n = src.numel()
    if dst.numel() != n:
        raise ValueError(f"{name}: src has {n} bytes but dst {dst.numel()}")
    in_place = allow_in_place and src.data_ptr() == dst.data_ptr()
    if n and not in_place and src.data_ptr() < dst.data_ptr() + n and \
            dst.data_ptr() < src.data_ptr() + n:
        raise ValueError(
            f"{name}: src and dst overlap " +
            ("partially (in place means the same base and length)"
             if allow_in_place else "(this filter cannot run in place)"))
    if elem_size not in FILTER_ELEM_SIZES:
        raise ValueError(
            f"{name}: elem_size={elem_size} not in {FILTER_ELEM_SIZES}")
    if not 0 < block_raw < (1 << 32) or block_raw % FILTER_BLOCK_ALIGN:
        raise ValueError(
            f"{name}: block_raw={block_raw} must be a positive "
            f"multiple of {FILTER_BLOCK_ALIGN} below 2**32")
    assert src.is_cuda and dst.is_cuda and src.device == dst.device, \
        f"{name}: CUDA tensors on one device"
    if n == 0:
        return
    _call(entry, src, dst, n, block_raw, elem_size, int(bool(inverse)))


def byte_shuffle(src, dst, block_raw: int, elem_size: int,
                 inverse: bool = False):
    """SYSHARD byte-shuffle filter on the device: ``dst`` receives
    ``src`` with every ``block_raw`` block (the last one may be short)
    byte-transposed over ``elem_size``-byte elements — plane j of a
    block holds byte j of each of its elements, the ``len % elem_size``
    leftover is copied verbatim.  ``inverse=True`` undoes it.  The byte
    layout is ``shardfmt.shuffle_blocks_numpy``'s.

    ``src``/``dst``: contiguous uint8 CUDA tensors of equal numel whose
    base pointers are 16-byte aligned and whose byte ranges do not
    overlap; ``elem_size`` in {2, 4, 8}; ``block_raw`` a positive
    multiple of 4096 below 2**32.  Each violation is a ValueError raised
    before any launch (and ahead of the device assert, so the rules are
    testable on hosts without a GPU)."""
    _block_filter("byte_shuffle", "sy_byte_shuffle", False, src, dst,
                  block_raw, elem_size, inverse)


def delta_filter(src, dst, block_raw: int, elem_size: int,
                 inverse: bool = False):
    """SYSHARD delta filter on the device: ``dst`` receives ``src`` with
    every ``block_raw`` block (the last one may be short) turned into
    differences of its ``elem_size``-byte little-endian unsigned
    elements mod 2**(8*elem_size) — ``d[0] = x[0]``,
    ``d[i] = x[i] - x[i-1]``, restarting at every block, the
    ``len % elem_size`` leftover copied verbatim.  ``inverse=True`` sums
    them up again (one inclusive scan per block).  The byte layout is
    ``shardfmt.delta_blocks_numpy``'s.

    ``src``/``dst``: contiguous uint8 CUDA tensors of equal numel whose
    base pointers are 16-byte aligned.  ``dst`` may be ``src`` itself
    (same base, same length: the filter then runs in place, in either
    direction); any other overlap of the byte ranges is a ValueError.
    ``elem_size`` in {2, 4, 8}; ``block_raw`` a positive multiple of 4096
    below 2**32.  Each violation is a ValueError raised before any
    launch (and ahead of the device assert, so the rules are testable
    on hosts without a GPU).

    One workgroup decodes one block from start to end, so a buffer of a
    few very large blocks uses only a few CUs."""
    _block_filter("delta_filter", "sy_delta_filter", True, src, dst,
                  block_raw, elem_size, inverse)


def bit_shuffle(src, dst, block_raw: int, elem_size: int,
                inverse: bool = False):
    """SYSHARD bit-shuffle filter on the device: ``dst`` receives
    ``src`` with every ``block_raw`` block (the last one may be short)
    bit-transposed over ``elem_size``-byte little-endian elements —
    plane p of a block holds bit p of each of its elements, 8
    consecutive elements per byte, LSB first; what does not fill a
    group of 8 elements (only in a ragged final block) is copied
    verbatim.  ``inverse=True`` undoes it.  The byte layout is
    ``shardfmt.bitshuffle_blocks_numpy``'s.

    ``src``/``dst``: contiguous uint8 CUDA tensors of equal numel whose
    base pointers are 16-byte aligned and whose byte ranges do not
    overlap (the filter does not run in place); ``elem_size`` in
    {2, 4, 8}; ``block_raw`` a positive multiple of 4096 below 2**32.
    Each violation is a ValueError raised before any launch (and ahead
    of the device assert, so the rules are testable on hosts without a
    GPU)."""
    _block_filter("bit_shuffle", "sy_bit_shuffle", False, src, dst,
                  block_raw, elem_size, inverse)


def _env_atoi(name: str, default: int) -> int:
    """The value common.h's sy_env_atoi (getenv + atoi) gives for
    ``name`` in lz4_decode.hip."""
    e = os.environ.get(name)
    if e is None:
        return default
    try:
        return int(e)
    except ValueError:
        return 0


def _lz4_staged_by_env() -> bool:
    """True when the environment sends sy_lz4_decode_blocks to a kernel
    instantiation that stages the stream with uint4 loads (STAGE=1)."""
    return _env_atoi("SY_LZ4_NOSTAGE", 1) == 0 or \
        _env_atoi("SY_LZ4_SKIP", 0) in (1, 2)


def lz4_decode_blocks(comp, in_off, in_len, out, out_off, out_len,
                      raw_cap: int = 64 * 1024, pc: bool = None):
    """Decode independent LZ4 blocks on the GPU.

    All tensors are CUDA: ``comp``/``out`` uint8, ``in_off``/``out_off``
    int64 (byte offsets; out offsets 16 B aligned), ``in_len``/``out_len``
    uint32.  ``raw_cap`` is the max raw block size (selects the LDS
    geometry: smaller blocks -> more workgroups/CU -> more latency
    hiding; the decoder is serial per block).  Returns a CUDA uint32
    status tensor (0 == OK per block).

    ``out``'s base pointer must be 16-byte aligned (the decoded block
    is streamed out with uint4 stores at ``out + out_off``); a
    misaligned view raises ValueError before launch.  ``in_off`` may
    always be unaligned.  ``comp``'s base may be unaligned only on the
    default path, which parses the stream bytewise; the producer/
    consumer path (``pc``) and the staged path (SY_LZ4_NOSTAGE=0, and
    the SY_LZ4_SKIP probes) round the *offset* down to 16 and load
    uint4 from ``comp + offset``, so there a misaligned ``comp`` base
    raises ValueError before launch as well.
    """
    import torch

    _check_aligned16(out, "lz4_decode_blocks: out")
    if pc is None:
        pc = os.environ.get("SHIPYARD_LZ4_PC", "0") == "1"
    if pc or _lz4_staged_by_env():
        _check_aligned16(
            comp, "lz4_decode_blocks: comp",
            where=" on the producer/consumer and staged paths")
    n_blocks = in_off.numel()
    status = torch.empty(n_blocks, dtype=torch.uint32, device=comp.device)
    _call("sy_lz4_decode_blocks_pc" if pc else "sy_lz4_decode_blocks",
          comp, in_off, in_len, out, out_off, out_len, status, n_blocks,
          raw_cap)
    return status


def lz4_all_ok(status) -> bool:
    """True iff every block decoded cleanly (uint32 reductions are not
    implemented on CUDA in torch, so check on host)."""
    import torch

    return bool((status.cpu().to(torch.int64) == 0).all().item())


def sha256_pages(data, page_size: int = 4096):
    """SHA-256 digest of each page of a uint8 CUDA tensor -> (n_pages, 32).

    ``data`` must be contiguous with a 16-byte-aligned base pointer
    (message words are loaded as uint4); a misaligned view raises
    ValueError before launch."""
    import torch

    _check_u8_device(data, "sha256_pages")
    n = data.numel()
    n_pages = (n + page_size - 1) // page_size
    out = torch.empty((n_pages, 32), dtype=torch.uint8, device=data.device)
    _call("sy_sha256_pages", data, n, page_size, out, n_pages)
    return out


def stage_file_native(path, dst, file_off: int = 0,
                      n_bytes: int = None, staging_mb: int = 64,
                      use_direct: bool = True) -> float:
    """Native C++ staging pipeline: pread (O_DIRECT when possible) ->
    pinned ring -> hipMemcpyAsync into the uint8 CUDA tensor ``dst``.
    Returns pipeline seconds."""
    lib = _load()
    if n_bytes is None:
        n_bytes = os.path.getsize(path) - file_off
    assert dst.numel() >= n_bytes
    secs = ctypes.c_double(0.0)
    # its own error text, and the stream is not the last argument
    rc = lib.sy_stage_file(
        str(path).encode(), dst.data_ptr(), file_off, n_bytes,
        staging_mb << 20, int(use_direct), _stream(), ctypes.byref(secs))
    if rc != 0:
        raise RuntimeError(f"sy_stage_file failed rc={rc} "
                           f"({os.strerror(-rc) if rc < 0 else 'hip'})")
    return secs.value


def require_native() -> None:
    """Fail loudly when running on a GPU box without the compiled ops."""
    import torch

    if torch.cuda.is_available():
        _load()
