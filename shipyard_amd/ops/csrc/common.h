// Common helpers for shipyard_amd HIP kernels (gfx950 / MI355X only).
//
// These kernels implement the framework's data-plane hot paths — the
// MI355X-native equivalent of the reference's delegated native work
// (container layer decompress in dockerd, MD5/SHA256 integrity in
// convoy/util.py:461-508, blobxfer chunk hashing).  See SURVEY.md §2.5.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#define SY_EXPORT extern "C" __attribute__((visibility("default")))

// Error contract: every entry point returns a hipError_t-compatible int
// (0 == success).  Kernel-level data errors (corrupt LZ4 stream, bounds)
// are reported through per-item status words, not the return code.
static inline int sy_check(hipError_t e) { return static_cast<int>(e); }

// wave64 is the CDNA scheduling quantum; hard-code 64 per the CDNA4 guide.
#ifndef SY_WAVE
#define SY_WAVE 64
#endif

// Integer knob from the environment with C atoi semantics (leading
// integer, 0 for garbage); `unset` when the variable is absent.  Callers
// keep the result in a function-local static so each variable is read
// once per process.  ops._env_atoi mirrors this in Python.
static inline int sy_env_atoi(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}

// Host side of the LZ4 kernels (lz4_decode.hip, lz4_compress_gpu.hip):
// each kernel is compiled for a ladder of RAWCAP rungs (LDS bytes per
// block, so occupancy).  Calls f(std::integral_constant<int, CAP>{}) for
// the smallest CAP >= raw_cap and returns its result; CAPS ascend.
// Returns -22 (EINVAL) when raw_cap is above the top rung: f is not
// called and nothing is launched.
template <int... CAPS, class F>
static inline int sy_dispatch_rung(uint32_t raw_cap, F&& f) {
  int rc = -22;
  (void)((raw_cap <= static_cast<uint32_t>(CAPS) &&
          ((rc = f(std::integral_constant<int, CAPS>{})), true)) ||
         ...);
  return rc;
}

// Host side of the SYSHARD block filters (byte_shuffle.hip,
// delta_filter.hip, bit_shuffle.hip): one launch walks a buffer of block_raw-sized blocks
// whose last block may be short.

// What the exported wrappers accept: blocks made of whole 4 KiB tiles,
// elements of 2, 4 or 8 bytes.
static inline bool sy_filter_args_ok(uint32_t block_raw, uint32_t elem_size) {
  return block_raw != 0 && block_raw % 4096 == 0 &&
         (elem_size == 2 || elem_size == 4 || elem_size == 8);
}

struct SyBlockSplit {
  uint64_t n_full;    // blocks of exactly block_raw bytes
  uint32_t tail_len;  // bytes of the ragged final block, 0 if none
};

static inline SyBlockSplit sy_block_split(uint64_t n_bytes,
                                          uint32_t block_raw) {
  const uint64_t n_full = n_bytes / block_raw;
  return {n_full, static_cast<uint32_t>(n_bytes - n_full * block_raw)};
}

// capped grid + grid-stride loop: 32 workgroups per CU's worth
static inline uint32_t sy_capped_grid(uint64_t n_work) {
  const uint32_t cap = 8192;
  return n_work < cap ? static_cast<uint32_t>(n_work) : cap;
}
