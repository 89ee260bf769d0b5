// Bit-shuffle (bit-transpose) filter for typed SYSHARD blocks (gfx950).
//
// SYSHARD's FILTER_BITSHUFFLE stores each block of raw_len bytes, seen
// as n_el = raw_len / B little-endian elements of B bytes, bit plane by
// bit plane.  With n8 = n_el / 8 * 8, L = n8 / 8 and body = n8 * B:
//   plane p is filtered[p*L, (p+1)*L)                     (0 <= p < 8*B)
//   bit r (LSB first) of filtered[p*L + m] = bit p of element 8*m + r
//   filtered[body:] = raw[body:]
// where bit p of an element is bit p % 8 of its byte p / 8.  A sign or
// exponent bit that is nearly constant over the elements becomes a run
// of equal bytes that LZ4 can remove although it shares its byte with
// mantissa bits.  One launch covers a whole buffer of regular blocks in
// either direction; the ragged final block is part of the same launch.
// (Reference analogue: none.)
//
// Tile: 4 KiB of raw bytes = T = 4096/B elements; 256 threads x 16 B,
// UNROLL = 4 tiles per workgroup pass, as in byte_shuffle.hip.  A full
// block is block_raw/4096 tiles, so no block is held whole in LDS and
// block_raw is unbounded.  On the raw side a tile is 4096 contiguous
// bytes; on the filtered side it is 8*B runs of TP = T/8 bytes (256 /
// 128 / 64 B for B = 2 / 4 / 8), one per plane, at plane stride
// L = block_raw/(8*B).  L and TP are multiples of 64, so every run
// starts 16 B aligned and BOTH global sides are one uint4 per lane.  On
// the filtered side lane t takes 16 B of plane t/(TP/16): 16 / 8 / 4
// consecutive lanes cover one run, so a wave instruction touches 4 / 8 /
// 16 runs.  Coalescing on that side is what the format allows: the runs
// of the consecutive tiles of one block are adjacent in every plane, and
// the four tiles of a pass are consecutive, so for B = 8 at the 8 KiB
// default (a plane is 128 B, a tile's run half of it) the two halves of
// each 128 B line come from two uint4 instructions of the same
// workgroup issued back to back; at 4 KiB blocks a plane is one 64 B
// run and every 128 B line is shared by two planes.  Larger blocks give
// up to 4 adjacent runs (256 B for B = 8) per pass, at a plane stride
// that is a larger power of two.  Measured on the MI355X
// (docs/35-gpu-data-plane.md): 0.98-1.01 of the device copy rate,
// except B = 8 at 64 KiB blocks (64 B runs 1 KiB apart) at 0.91.
//
// Transposition, forward (inverse: the same steps backwards):
//  1. raw -> byte planes, shuffle_tile.h: a 16-byte in-register
//     permutation, then one narrow LDS store per byte plane j to
//     j*T + (16/B)*t.  The tile in LDS now holds byte j of its elements
//     at [j*T, (j+1)*T).
//  2. bit transpose, 2 tasks per thread: a task is 32 B of a byte
//     plane = byte j of 32 consecutive elements = four 8x8 bit
//     matrices.  It reads them with two ds_read_b128, transposes each
//     64-bit word in registers with the three-round masked swap
//     (7, 14, 28), which leaves in byte q of word i the plane byte
//     8*j+q of elements 8*(m0+i)..+7, and turns the four words with two
//     4x4 byte transposes into one dword per plane: bytes m0..m0+3 of
//     plane 8*j+q.  After a barrier (the stores go where other tasks
//     read) eight ds_write_b32 put them at j*T + q*TP + m0: the tile is
//     now in its filtered layout, plane p at p*TP, in the same LDS.
//     Region j of the tile holds byte plane j before and bit planes
//     8*j..8*j+7 after, so the step is local to T bytes.
//  3. ds_read_b128 at 16*t, global store to plane t/(TP/16).
// No ballot and no per-bit loop: 12 bit-matrix rounds and 16 byte
// merges of 32-bit VALU work per 32 bytes.
//
// LDS accesses and banks (lane groups per MI355X: 2 x 32 lanes for the
// 4- and 8-byte accesses, 16 lanes for ds_read_b128, 8 lanes for
// ds_write_b128):
//   * 16*t wide accesses (steps 1/3): linear, conflict-free.
//   * step 1 narrow accesses: byte_shuffle.hip's reasoning, unchanged.
//   * step 2 wide side, 32 B lane stride: lanes i and i+8 of a
//     ds_read_b128 group (i and i+4 of a ds_write_b128 group) meet on a
//     bank, a 2-way conflict on 2 of the ~14 LDS instructions of a task.
//   * step 2 narrow side: consecutive lanes take consecutive dwords of
//     one plane run (TP/4 = 64 / 32 / 16 lanes per run).  For B = 2 and
//     4 a 32-lane group stays inside one run: conflict-free.  For B = 8
//     lanes l and l+16 sit in regions 512 B apart, the same bank: 2-way,
//     free on the ds_write_b32 side (forward), 2 extra LDS cycles per
//     ds_read_b32 on the inverse side.
// Per 4 KiB tile that is about 24 wave-level LDS instructions of at most
// 13 cycles, against roughly 800 cycles in which HBM moves the tile's
// 8 KiB at the copy rate, so the kernel is expected to stay
// memory-bound; it has three barriers per pass where byte_shuffle has
// two.
//
// Resources (hipcc -O3, gfx950): 16 KiB LDS per workgroup; the six
// kernels take 60-61 VGPRs and 53-68 SGPRs, no scratch, so the register
// file allows 8 waves per SIMD and the 32-wave cap gives 8 workgroups
// (128 of the CU's 160 KiB LDS) resident per CU.
//
// Ragged final block (any length 1..block_raw-1): L is arbitrary and
// plane starts are unaligned, so it takes a byte-granular path.  Every
// thread owns whole destination bytes: forward it walks the FILTERED
// index and gathers one bit from each of 8 raw bytes, inverse it walks
// the RAW index and gathers one bit from each of 8 plane bytes; no byte
// is written by two threads.  Every index it forms is < tail_len, so
// nothing outside [0, n_bytes) is touched.

#include "shuffle_tile.h"

namespace {

// step 2 works on 32 B of a byte plane per task
constexpr uint32_t kTaskBytes = 32;
constexpr uint32_t kTasksPerTile = kTileBytes / kTaskBytes;
constexpr uint32_t kTasks = kUnroll * kTasksPerTile / kThreads;
static_assert(kTasks * kThreads == kUnroll * kTasksPerTile &&
              kThreads % kTasksPerTile == 0, "tasks divide evenly");

// 8x8 bit-matrix transpose of a 64-bit word (row = byte, LSB first on
// both axes); its own inverse
__device__ __forceinline__ uint64_t transpose8x8(uint64_t x) {
  uint64_t s;
  s = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
  x ^= s ^ (s << 7);
  s = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
  x ^= s ^ (s << 14);
  s = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
  x ^= s ^ (s << 28);
  return x;
}

// 4x4 byte transpose: byte i of o[q] = byte q of a[i]; its own inverse
__device__ __forceinline__ void transpose4x4(const uint32_t (&a)[4],
                                             uint32_t (&o)[4]) {
  const uint32_t l01 = (a[0] & 0x00ff00ffu) | ((a[1] & 0x00ff00ffu) << 8);
  const uint32_t h01 = ((a[0] >> 8) & 0x00ff00ffu) | (a[1] & 0xff00ff00u);
  const uint32_t l23 = (a[2] & 0x00ff00ffu) | ((a[3] & 0x00ff00ffu) << 8);
  const uint32_t h23 = ((a[2] >> 8) & 0x00ff00ffu) | (a[3] & 0xff00ff00u);
  o[0] = (l01 & 0xffffu) | (l23 << 16);
  o[1] = (h01 & 0xffffu) | (h23 << 16);
  o[2] = (l01 >> 16) | (l23 & 0xffff0000u);
  o[3] = (h01 >> 16) | (h23 & 0xffff0000u);
}

// four 64-bit words (byte planes side: w[2i], w[2i+1] = word i) <->
// eight plane dwords (w[q] = bytes m0..m0+3 of plane q); its own inverse
// up to the order of the two stages
template <bool INVERSE>
__device__ __forceinline__ void transpose_task(uint32_t (&w)[8]) {
  if constexpr (!INVERSE) {
    uint32_t lo[4], hi[4], olo[4], ohi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t y = transpose8x8(
          static_cast<uint64_t>(w[2 * i]) |
          (static_cast<uint64_t>(w[2 * i + 1]) << 32));
      lo[i] = static_cast<uint32_t>(y);
      hi[i] = static_cast<uint32_t>(y >> 32);
    }
    transpose4x4(lo, olo);
    transpose4x4(hi, ohi);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w[q] = olo[q];
      w[4 + q] = ohi[q];
    }
  } else {
    const uint32_t plo[4] = {w[0], w[1], w[2], w[3]};
    const uint32_t phi[4] = {w[4], w[5], w[6], w[7]};
    uint32_t lo[4], hi[4];
    transpose4x4(plo, lo);
    transpose4x4(phi, hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t y = transpose8x8(
          static_cast<uint64_t>(lo[i]) |
          (static_cast<uint64_t>(hi[i]) << 32));
      w[2 * i] = static_cast<uint32_t>(y);
      w[2 * i + 1] = static_cast<uint32_t>(y >> 32);
    }
  }
}

template <int B, bool INVERSE>
__global__ __launch_bounds__(kThreads) void bit_shuffle_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint64_t n_tiles, uint32_t tiles_per_block, uint32_t block_raw,
    uint64_t tail_off, uint32_t tail_len, uint64_t n_work_full,
    uint64_t n_work) {
  constexpr uint32_t T = kTileBytes / B;  // elements (= byte-plane bytes) per tile
  constexpr uint32_t TP = T / 8;          // bit-plane bytes per tile
  constexpr uint32_t LPP = TP / 16;       // lanes per bit-plane run
  __shared__ __attribute__((aligned(16))) uint8_t lds[kUnroll * kTileBytes];

  const uint32_t t = threadIdx.x;
  const uint32_t plane_len = block_raw / (8 * B);  // L of a full block
  // this lane's 16 B on the filtered side: plane t/LPP, byte 16*(t%LPP)
  // of its run (plane * L < block_raw, so 32 bits hold it)
  const uint32_t flt_lane = (t / LPP) * plane_len + 16u * (t % LPP);
  const uint32_t raw_lane = 16u * t;  // also the lane's 16 B in an LDS tile
  // step 2: task k of this lane is 32 B at bp_off of tile 2*k + t/128;
  // its plane dwords sit at ft_off + q*TP of the same tile
  const uint32_t bp_off = kTaskBytes * (t % kTasksPerTile);
  const uint32_t ft_off = (bp_off & ~(T - 1)) + (bp_off & (T - 1)) / 8;
  uint8_t* const task_tile = lds + (t / kTasksPerTile) * kTileBytes;
  constexpr uint32_t kTaskStride = (kThreads / kTasksPerTile) * kTileBytes;

  for (uint64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    if (w < n_work_full) {
      // kUnroll consecutive tiles; one division per pass, then a carry.
      // Tile bases are workgroup-uniform (scalar registers); the lane
      // parts raw_lane / flt_lane are loop-invariant.
      const uint64_t tile0 = w * kUnroll;
      uint64_t blk = tile0 / tiles_per_block;
      uint32_t ti = static_cast<uint32_t>(tile0 - blk * tiles_per_block);
      uint64_t raw_base[kUnroll];  // tile start on the raw side
      uint64_t flt_base[kUnroll];  // start of the tile's run in plane 0
      bool live[kUnroll];
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        live[u] = tile0 + u < n_tiles;
        const uint64_t base = blk * block_raw;
        raw_base[u] = base + static_cast<uint64_t>(ti) * kTileBytes;
        flt_base[u] = base + static_cast<uint64_t>(ti) * TP;
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
      // step 1 (forward) / filtered tile as it is (inverse) into LDS
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        if (live[u]) {
          uint8_t* tile = lds + u * kTileBytes;
          if constexpr (INVERSE) {
            *reinterpret_cast<lds_u4*>(tile + raw_lane) = v[u];
          } else {
            const uint32_t raw[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t pm[4];
            permute16<B, false>(raw, pm);
            lds_put_pieces<B>(tile, t, pm);
          }
        }
      }
      __syncthreads();
      // step 2: read, barrier, transpose, write back into the same
      // tile.  The tiles of a partial pass that are not live hold
      // leftovers; transposing them touches LDS only.
      uint32_t task[kTasks][8];
#pragma unroll
      for (int k = 0; k < static_cast<int>(kTasks); ++k) {
        const uint8_t* tile = task_tile + k * kTaskStride;
        if constexpr (INVERSE) {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            task[k][q] =
                *reinterpret_cast<const lds_u32*>(tile + ft_off + q * TP);
        } else {
          const vec4 a = *reinterpret_cast<const lds_u4*>(tile + bp_off);
          const vec4 b = *reinterpret_cast<const lds_u4*>(tile + bp_off + 16);
          task[k][0] = a.x, task[k][1] = a.y, task[k][2] = a.z;
          task[k][3] = a.w, task[k][4] = b.x, task[k][5] = b.y;
          task[k][6] = b.z, task[k][7] = b.w;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < static_cast<int>(kTasks); ++k) {
        uint8_t* tile = task_tile + k * kTaskStride;
        transpose_task<INVERSE>(task[k]);
        if constexpr (INVERSE) {
          *reinterpret_cast<lds_u4*>(tile + bp_off) =
              vec4{task[k][0], task[k][1], task[k][2], task[k][3]};
          *reinterpret_cast<lds_u4*>(tile + bp_off + 16) =
              vec4{task[k][4], task[k][5], task[k][6], task[k][7]};
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            *reinterpret_cast<lds_u32*>(tile + ft_off + q * TP) = task[k][q];
        }
      }
      __syncthreads();
      // step 3 (forward) / step 1 backwards (inverse) out of LDS
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        if (live[u]) {
          const uint8_t* tile = lds + u * kTileBytes;
          if constexpr (INVERSE) {
            uint32_t pm[4], raw[4];
            lds_get_pieces<B>(tile, t, pm);
            permute16<B, true>(pm, raw);
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
      // ragged final block, 4 KiB of destination index per pass
      const uint32_t r_len = tail_len / (8 * B);  // its plane length L
      const uint32_t body = r_len * 8 * B;
      const uint32_t k0 =
          static_cast<uint32_t>(w - n_work_full) * kTileBytes;
      const uint32_t k1 =
          tail_len - k0 < kTileBytes ? tail_len : k0 + kTileBytes;
      const uint8_t* s = src + tail_off;
      uint8_t* d = dst + tail_off;
      for (uint32_t k = k0 + t; k < k1; k += kThreads) {
        uint32_t out;
        if (k >= body) {
          out = s[k];
        } else if constexpr (INVERSE) {
          // k is a raw index: byte jb of element el = 8*m + r; its bit c
          // is bit r of byte m of plane 8*jb + c
          const uint32_t el = k / B, jb = k % B;
          const uint32_t m = el / 8, r = el % 8;
          const uint8_t* f = s + 8 * jb * r_len + m;
          out = 0;
#pragma unroll
          for (uint32_t c = 0; c < 8; ++c)
            out |= ((f[c * r_len] >> r) & 1u) << c;
        } else {
          // k is a filtered index: byte m of plane p; its bit r is bit
          // p%8 of byte p/8 of element 8*m + r
          const uint32_t p = k / r_len, m = k - p * r_len;
          const uint8_t* e = s + 8 * m * B + p / 8;
          out = 0;
#pragma unroll
          for (uint32_t r = 0; r < 8; ++r)
            out |= ((e[r * B] >> (p % 8)) & 1u) << r;
        }
        d[k] = static_cast<uint8_t>(out);
      }
    }
  }
}

template <int B>
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
    hipLaunchKernelGGL((bit_shuffle_kernel<B, true>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_tiles,
                       tiles_per_block, block_raw, tail_off, tail_len,
                       n_work_full, n_work);
  else
    hipLaunchKernelGGL((bit_shuffle_kernel<B, false>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_tiles,
                       tiles_per_block, block_raw, tail_off, tail_len,
                       n_work_full, n_work);
  return sy_check(hipGetLastError());
}

}  // namespace

// d_src / d_dst: 16 B aligned, non-overlapping, n_bytes each.  Block b
// is [b*block_raw, min((b+1)*block_raw, n_bytes)).  inverse == 0
// bit-shuffles (raw -> filtered), nonzero undoes it.
SY_EXPORT int sy_bit_shuffle(const void* d_src, void* d_dst,
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
