// Byte-shuffle (byte-transpose) filter for typed SYSHARD blocks (gfx950).
//
// SYSHARD's FILTER_SHUFFLE stores each block of raw_len bytes, seen as
// n_el = raw_len / E elements of E bytes, plane by plane:
//   filtered[j*n_el + i] = raw[i*E + j]   (0 <= j < E, 0 <= i < n_el)
// with the raw_len % E leftover bytes copied verbatim.  LZ4 then finds
// the redundancy of typed data (always-zero high bytes of token ids)
// that it cannot see in the interleaved form.  One launch covers a
// whole buffer of regular blocks in either direction; the ragged final
// block is part of the same launch.  (Reference analogue: none.)
//
// Tile: 4 KiB of raw bytes = T = 4096/E elements; 256 threads x 16 B.
// A full block is block_raw/4096 tiles (block_raw % 4096 == 0), so no
// block is ever held whole in LDS and block_raw is unbounded.  On the
// raw side a tile is 4096 contiguous bytes, on the filtered side E runs
// of T bytes at plane stride n_el; n_el and T are both multiples of
// 512, so every run starts 16 B aligned and BOTH global sides are one
// uint4 per lane, consecutive lanes on consecutive 16 B (a wave covers
// whole 1 KiB raw spans, or 1 KiB / 512 B / 256 B plane runs for
// E = 2 / 4 / 8 at T = 2048 / 1024 / 512).
//
// LDS: the tile is always kept in the FILTERED layout (plane j at
// j*T), UNROLL = 4 tiles per workgroup pass so four uint4 loads per
// lane are in flight before the first LDS access: 16 KiB per
// workgroup.  The kernels compile to 65-67 VGPRs, so 7 workgroups
// (7 waves/SIMD, 112 of the CU's 160 KiB LDS) are resident per CU.
// The transposition is split: a 16-byte in-register permutation turns
// a lane's 16/E elements into E pieces of P = 16/E bytes (one per
// plane), and LDS moves pieces between lanes.
//   * wide side (ds_read_b128 / ds_write_b128): lane t at byte 16*t —
//     linear, consecutive lanes on consecutive 16 B slots, conflict-free
//     in every lane group.
//   * narrow side, one instruction per plane j: lane t at j*T + P*t.
//     The 64 lanes of one instruction cover 64*P contiguous bytes
//     (E=2: ds_*_b64 over 512 B, E=4: ds_*_b32 over 256 B, E=8:
//     ds_*_u16/b16 over 128 B), so inside any lane group no two lanes
//     touch different dwords of one bank; for E=8 lanes 2k and 2k+1
//     share a dword (same address: a broadcast on the read side, at
//     worst the 2-way store case that costs nothing extra on
//     ds_write_b32-class stores).  The compiler pairs two planes into
//     one ds_{read,write}2st64 for E=2 and E=4; each half of such a
//     pair is one of the contiguous accesses above.  No padding or
//     swizzle is needed because neither side ever walks LDS with a
//     power-of-two stride across lanes.
// LDS traffic is 16 B + E narrow ops per 16 B moved; even E=8 (eight
// 4-cycle stores per KiB per wave) leaves the LDS several times faster
// than HBM can feed it, so the kernel is expected to be memory-bound.
//
// Ragged final block (any length 1..block_raw-1): n_el is arbitrary,
// plane starts are unaligned, so it takes a byte-granular path that
// walks the RAW index (divisions by the constant E only).  Every index
// it forms is < tail_len, so nothing outside [0, n_bytes) is touched.

#include "shuffle_tile.h"

namespace {

template <int E, bool INVERSE>
__global__ __launch_bounds__(kThreads) void byte_shuffle_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint64_t n_tiles, uint32_t tiles_per_block, uint32_t block_raw,
    uint64_t tail_off, uint32_t tail_len, uint64_t n_work_full,
    uint64_t n_work) {
  constexpr uint32_t T = kTileBytes / E;    // elements (= plane bytes) per tile
  constexpr uint32_t LPP = kThreads / E;    // lanes per plane run (T / 16)
  __shared__ __attribute__((aligned(16))) uint8_t lds[kUnroll * kTileBytes];

  const uint32_t t = threadIdx.x;
  const uint32_t n_el = block_raw / E;
  // this lane's 16 B on the filtered side: plane t/LPP, byte 16*(t%LPP)
  // of its run (plane * n_el < block_raw, so 32 bits hold it)
  const uint32_t flt_lane = (t / LPP) * n_el + 16u * (t % LPP);
  const uint32_t raw_lane = 16u * t;  // also the lane's 16 B in an LDS tile

  for (uint64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    if (w < n_work_full) {
      // kUnroll consecutive tiles; one division per pass, then a carry.
      // Tile bases are workgroup-uniform (scalar registers); the lane
      // parts raw_lane / flt_lane are loop-invariant.
      const uint64_t tile0 = w * kUnroll;
      uint64_t blk = tile0 / tiles_per_block;
      uint32_t ti = static_cast<uint32_t>(tile0 - blk * tiles_per_block);
      uint64_t raw_base[kUnroll];  // tile start on the raw side
      uint64_t flt_base[kUnroll];  // tile start inside plane 0
      bool live[kUnroll];
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        live[u] = tile0 + u < n_tiles;
        const uint64_t base = blk * block_raw;
        raw_base[u] = base + static_cast<uint64_t>(ti) * kTileBytes;
        flt_base[u] = base + static_cast<uint64_t>(ti) * T;
        if (++ti == tiles_per_block) {
          ti = 0;
          ++blk;
        }
      }
      vec4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u)
        if (live[u])
          v[u] = *reinterpret_cast<const vec4*>(
              INVERSE ? src + flt_base[u] + flt_lane
                      : src + raw_base[u] + raw_lane);
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        if (live[u]) {
          uint8_t* tile = lds + u * kTileBytes;
          if constexpr (INVERSE) {
            *reinterpret_cast<lds_u4*>(tile + raw_lane) = v[u];
          } else {
            const uint32_t raw[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t pm[4];
            permute16<E, false>(raw, pm);
            lds_put_pieces<E>(tile, t, pm);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        if (live[u]) {
          const uint8_t* tile = lds + u * kTileBytes;
          if constexpr (INVERSE) {
            uint32_t pm[4], raw[4];
            lds_get_pieces<E>(tile, t, pm);
            permute16<E, true>(pm, raw);
            *reinterpret_cast<vec4*>(dst + raw_base[u] + raw_lane) =
                vec4{raw[0], raw[1], raw[2], raw[3]};
          } else {
            *reinterpret_cast<vec4*>(dst + flt_base[u] + flt_lane) =
                *reinterpret_cast<const lds_u4*>(tile + raw_lane);
          }
        }
      }
      __syncthreads();  // the next pass overwrites the tiles
    } else {
      // ragged final block, 4 KiB of raw index per pass, byte-granular
      const uint32_t r_el = tail_len / E;
      const uint32_t body = r_el * E;
      const uint32_t k0 =
          static_cast<uint32_t>(w - n_work_full) * kTileBytes;
      const uint32_t k1 =
          tail_len - k0 < kTileBytes ? tail_len : k0 + kTileBytes;
      const uint8_t* s = src + tail_off;
      uint8_t* d = dst + tail_off;
      for (uint32_t k = k0 + t; k < k1; k += kThreads) {
        // k is a raw index; its filtered twin is (k%E)*r_el + k/E
        const uint32_t f = k < body ? (k % E) * r_el + k / E : k;
        if constexpr (INVERSE)
          d[k] = s[f];
        else
          d[f] = s[k];
      }
    }
  }
}

template <int E>
int launch(const uint8_t* src, uint8_t* dst, uint64_t n_bytes,
           uint32_t block_raw, int inverse, hipStream_t stream) {
  const auto [n_full, tail_len] = sy_block_split(n_bytes, block_raw);
  const uint32_t tiles_per_block = block_raw / kTileBytes;
  const uint64_t n_tiles = n_full * tiles_per_block;
  const uint64_t n_work_full = (n_tiles + kUnroll - 1) / kUnroll;
  const uint64_t n_work =
      n_work_full + (tail_len + kTileBytes - 1) / kTileBytes;
  const uint32_t grid = sy_capped_grid(n_work);
  const uint64_t tail_off = n_full * block_raw;
  if (inverse)
    hipLaunchKernelGGL((byte_shuffle_kernel<E, true>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_tiles,
                       tiles_per_block, block_raw, tail_off, tail_len,
                       n_work_full, n_work);
  else
    hipLaunchKernelGGL((byte_shuffle_kernel<E, false>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_tiles,
                       tiles_per_block, block_raw, tail_off, tail_len,
                       n_work_full, n_work);
  return sy_check(hipGetLastError());
}

}  // namespace

// d_src / d_dst: 16 B aligned, non-overlapping, n_bytes each.  Block b
// is [b*block_raw, min((b+1)*block_raw, n_bytes)).  inverse == 0
// shuffles (raw -> filtered), nonzero unshuffles.
SY_EXPORT int sy_byte_shuffle(const void* d_src, void* d_dst,
                              uint64_t n_bytes, uint32_t block_raw,
                              uint32_t elem_size, int inverse,
                              hipStream_t stream) {
  if (!sy_filter_args_ok(block_raw, elem_size))
    return sy_check(hipErrorInvalidValue);
  if (n_bytes == 0) return 0;
  const uint8_t* s = static_cast<const uint8_t*>(d_src);
  uint8_t* d = static_cast<uint8_t*>(d_dst);
  switch (elem_size) {
    case 2: return launch<2>(s, d, n_bytes, block_raw, inverse, stream);
    case 4: return launch<4>(s, d, n_bytes, block_raw, inverse, stream);
    default: return launch<8>(s, d, n_bytes, block_raw, inverse, stream);
  }
}
