// Delta filter for monotone typed SYSHARD blocks (gfx950).
//
// SYSHARD's FILTER_DELTA stores each block of raw_len bytes, seen as
// n_el = raw_len / E little-endian unsigned elements of E bytes, as
// differences mod 2^(8E):
//   d[0] = x[0];  d[i] = x[i] - x[i-1]   (1 <= i < n_el)
// with the raw_len % E leftover bytes copied verbatim.  The running
// value restarts at every block, so blocks stay independent.  Offsets,
// row pointers, sorted ids and timestamps turn into small numbers whose
// high byte planes FILTER_SHUFFLE + LZ4 then remove.  One launch covers
// a whole buffer of regular blocks in either direction; the ragged
// final block is part of the same launch.  (Reference analogue: none.)
//
// Decomposition: ONE workgroup (256 threads, 4 waves) owns a block from
// its first byte to its last and walks it in passes of kUnroll = 4 tiles
// of 4 KiB; lane t holds bytes [16t, 16t+16) of each tile, so every
// global access of a full block is one uint4 per lane, consecutive lanes
// on consecutive 16 B.  No workgroup ever waits for another one: there
// is no look-back flag and nothing that a stalled neighbour could hang.
// The price is that the blocks, not the bytes, are the unit of
// parallelism: a shard of a few giant blocks (stored-only shards may use
// any block_raw) decodes on a few CUs, each block serially, pass after
// pass.  At the format's 8..64 KiB blocks a 256 MiB buffer has 4096 to
// 32768 of them, several per resident workgroup.
//
// Inverse (inclusive scan mod 2^(8E)), three levels per pass:
//   1. in lane: serial scan of the lane's 16/E elements per tile;
//   2. in wave: a 6-step shuffle scan (__shfl_up) of the lane totals,
//      the four tiles of a pass as four independent chains;
//   3. across the 4 waves: lane 63 of each wave puts its wave total of
//      each tile into LDS, one barrier, then every thread reads the 16
//      totals (same address in all lanes: broadcast reads) and adds up
//      what lies in front of it.
// The workgroup's running carry (the block's prefix up to this pass)
// lives in a register that every thread updates identically from those
// 16 totals.  E = 8 uses uint64_t arithmetic throughout (v_add_co /
// v_addc pairs), so carries cross the 32-bit halves.
//
// Forward: an element-wise subtract with one neighbour read.  The
// neighbour is never re-read from memory: inside a lane it is the
// previous register, between lanes a shuffle, between waves and tiles
// the same LDS slots as above (each wave's last element), between
// passes a register (prev_last).
//
// In place (src == dst): each pass loads all its bytes before the
// barrier and stores after it, a lane stores exactly the 16 bytes it
// loaded, passes and blocks touch disjoint bytes, and the forward
// predecessor comes from registers/LDS as described, so both directions
// run in place.  The pointers are deliberately not __restrict__.
//
// LDS: 2 (pass parity) x 4 tiles x 4 waves x E bytes <= 256 B per
// workgroup.  The parity double-buffer makes one barrier per pass
// enough: a wave can write the slots of pass p+2 only after passing the
// barrier of pass p+1, which every wave reaches after its reads of
// pass p.  Registers: 16 for the pass's data plus scan temporaries; the
// kernels compile to 44-51 VGPRs (8 workgroups = 8 waves/SIMD per CU),
// the E = 8 inverse to 68 (7 per CU); LDS is no limit and nothing
// spills.  Arithmetic per 16 B is a few dozen VALU
// ops and 6 * E/4-dword shuffles per tile; the kernel is expected to be
// memory-bound with the inverse somewhat below a plain copy because
// every pass ends in load -> scan -> barrier -> store with no overlap
// inside a workgroup (other resident workgroups cover it).
//
// Ragged final block (any length 1..block_raw-1): same code with
// RAGGED = true.  Its start is 16 B aligned (block_raw % 4096 == 0), so
// every lane slot that lies wholly inside body = n_el * E still moves
// as one uint4; the single slot that straddles body moves element by
// element (loads and stores at off + k*E with off + (k+1)*E <= body),
// slots past body move nothing, and thread 0 copies the < E leftover
// bytes [body, len).  Every index formed is < len, so nothing outside
// [0, n_bytes) is touched.

#include "common.h"

namespace {

constexpr uint32_t kTileBytes = 4096;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / SY_WAVE;
constexpr uint32_t kUnroll = 4;
constexpr uint32_t kPassBytes = kUnroll * kTileBytes;

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));

// a lane's 16 bytes <-> its 16/E elements; compile-time indices only,
// so the arrays stay in registers
template <typename T>
__device__ __forceinline__ void unpack16(const vec4 v,
                                         T (&e)[16 / sizeof(T)]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      e[2 * d] = static_cast<T>(w[d]);
      e[2 * d + 1] = static_cast<T>(w[d] >> 16);
    }
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int d = 0; d < 4; ++d) e[d] = w[d];
  } else {
#pragma unroll
    for (int d = 0; d < 2; ++d)
      e[d] = static_cast<uint64_t>(w[2 * d]) |
             (static_cast<uint64_t>(w[2 * d + 1]) << 32);
  }
}

template <typename T>
__device__ __forceinline__ vec4 pack16(const T (&e)[16 / sizeof(T)]) {
  uint32_t w[4];
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      w[d] = static_cast<uint32_t>(e[2 * d]) |
             (static_cast<uint32_t>(e[2 * d + 1]) << 16);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = e[d];
  } else {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      w[2 * d] = static_cast<uint32_t>(e[d]);
      w[2 * d + 1] = static_cast<uint32_t>(e[d] >> 32);
    }
  }
  return vec4{w[0], w[1], w[2], w[3]};
}

// value of lane (l - delta); lanes l < delta get their own value back
template <typename T>
__device__ __forceinline__ T shfl_up_t(T x, uint32_t delta) {
  if constexpr (sizeof(T) == 8) {
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(x), delta);
    const uint32_t hi = __shfl_up(static_cast<uint32_t>(x >> 32), delta);
    return static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32);
  } else {
    return static_cast<T>(__shfl_up(static_cast<uint32_t>(x), delta));
  }
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < SY_WAVE; d <<= 1) {
    const T y = shfl_up_t<T>(x, d);
    if (lane >= d) x = static_cast<T>(x + y);
  }
  return x;
}

// One block [s, s + len) -> [d, d + len), s and d 16 B aligned.  xch is
// the workgroup's exchange array, par the running pass parity.
template <typename T, bool INVERSE, bool RAGGED>
__device__ __forceinline__ void filter_block(
    const uint8_t* s, uint8_t* d, uint32_t len,
    T (&xch)[2][kUnroll][kWaves], uint32_t& par) {
  constexpr uint32_t E = sizeof(T);
  constexpr int N = 16 / E;
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t % SY_WAVE;
  const uint32_t wave = t / SY_WAVE;
  const uint32_t body = RAGGED ? len / E * E : len;

  T carry = 0;      // INVERSE: sum of every element in front of this pass
  T prev_last = 0;  // forward: the element in front of this pass

  // counted in passes: off0 += kPassBytes would wrap for a body within
  // one pass of 2^32
  const uint32_t n_pass = static_cast<uint32_t>(
      (static_cast<uint64_t>(body) + kPassBytes - 1) / kPassBytes);
  for (uint32_t pass = 0; pass < n_pass; ++pass) {
    const uint32_t off0 = pass * kPassBytes;
    T e[kUnroll][N];
    bool live[kUnroll];     // workgroup-uniform: the tile has elements
    uint32_t loff[kUnroll];  // this lane's 16 B inside the block
#pragma unroll
    for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
      const uint32_t tile = off0 + u * kTileBytes;
      live[u] = tile < body;
      loff[u] = tile + 16u * t;
    }
    // every load of the pass before anything else
#pragma unroll
    for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
      if (!live[u]) {
#pragma unroll
        for (int k = 0; k < N; ++k) e[u][k] = 0;
        continue;
      }
      if (!RAGGED || loff[u] + 16u <= body) {
        unpack16<T>(*reinterpret_cast<const vec4*>(s + loff[u]), e[u]);
      } else {
        // the slot that straddles body, or one past it: absent elements
        // read as 0 (they add nothing and are never stored)
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const uint32_t o = loff[u] + k * E;
          e[u][k] = o + E <= body ? *reinterpret_cast<const T*>(s + o) : T(0);
        }
      }
    }

    // stores come only after the pass's barrier, tile by tile
    auto store_tile = [&](int u, const T (&out)[N]) {
      if (!live[u]) return;
      if (!RAGGED || loff[u] + 16u <= body) {
        *reinterpret_cast<vec4*>(d + loff[u]) = pack16<T>(out);
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const uint32_t o = loff[u] + k * E;
          if (o + E <= body) *reinterpret_cast<T*>(d + o) = out[k];
        }
      }
    };
    if constexpr (INVERSE) {
      T tot[kUnroll], incl[kUnroll];
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        tot[u] = 0;
        incl[u] = 0;
        if (!live[u]) continue;
#pragma unroll
        for (int k = 1; k < N; ++k)
          e[u][k] = static_cast<T>(e[u][k] + e[u][k - 1]);
        tot[u] = e[u][N - 1];
        incl[u] = wave_inclusive_scan<T>(tot[u], lane);
      }
      if (lane == SY_WAVE - 1) {
#pragma unroll
        for (int u = 0; u < static_cast<int>(kUnroll); ++u)
          xch[par][u][wave] = incl[u];  // 0 for a tile that is not live
      }
      __syncthreads();
      T base = carry;
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        T in_front = base;  // + the waves of this tile in front of mine
#pragma unroll
        for (int w = 0; w < static_cast<int>(kWaves); ++w) {
          const T ws = xch[par][u][w];
          if (static_cast<uint32_t>(w) < wave)
            in_front = static_cast<T>(in_front + ws);
          base = static_cast<T>(base + ws);
        }
        const T add = static_cast<T>(in_front + incl[u] - tot[u]);
        T out[N];
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = static_cast<T>(e[u][k] + add);
        store_tile(u, out);
      }
      carry = base;
    } else {
      T from_lane[kUnroll];
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        const T last = live[u] ? e[u][N - 1] : T(0);
        from_lane[u] = shfl_up_t<T>(last, 1);
        if (lane == SY_WAVE - 1) xch[par][u][wave] = last;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < static_cast<int>(kUnroll); ++u) {
        T pred = from_lane[u];
        if (lane == 0) {
          if (wave > 0)
            pred = xch[par][u][wave - 1];
          else
            pred = u == 0 ? prev_last : xch[par][u > 0 ? u - 1 : 0][kWaves - 1];
        }
        T out[N];
        out[0] = static_cast<T>(e[u][0] - pred);
#pragma unroll
        for (int k = 1; k < N; ++k)
          out[k] = static_cast<T>(e[u][k] - e[u][k - 1]);
        store_tile(u, out);
      }
      // only a block's final pass has tiles that are not live, and
      // nothing reads prev_last after it
      prev_last = xch[par][kUnroll - 1][kWaves - 1];
    }
    par ^= 1u;
  }
  if constexpr (RAGGED) {
    // len % E leftover bytes, verbatim
    if (t == 0)
      for (uint32_t o = body; o < len; ++o) d[o] = s[o];
  }
}

template <typename T, bool INVERSE>
__global__ __launch_bounds__(kThreads) void delta_filter_kernel(
    const uint8_t* src, uint8_t* dst, uint64_t n_full, uint32_t block_raw,
    uint32_t tail_len, uint64_t n_work) {
  __shared__ T xch[2][kUnroll][kWaves];
  uint32_t par = 0;
  for (uint64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const uint64_t off = w * block_raw;
    if (w < n_full)
      filter_block<T, INVERSE, false>(src + off, dst + off, block_raw, xch,
                                      par);
    else
      filter_block<T, INVERSE, true>(src + off, dst + off, tail_len, xch,
                                     par);
  }
}

template <typename T>
int launch(const uint8_t* src, uint8_t* dst, uint64_t n_bytes,
           uint32_t block_raw, int inverse, hipStream_t stream) {
  const auto [n_full, tail_len] = sy_block_split(n_bytes, block_raw);
  const uint64_t n_work = n_full + (tail_len ? 1 : 0);
  const uint32_t grid = sy_capped_grid(n_work);  // grid-stride over blocks
  if (inverse)
    hipLaunchKernelGGL((delta_filter_kernel<T, true>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_full, block_raw,
                       tail_len, n_work);
  else
    hipLaunchKernelGGL((delta_filter_kernel<T, false>), dim3(grid),
                       dim3(kThreads), 0, stream, src, dst, n_full, block_raw,
                       tail_len, n_work);
  return sy_check(hipGetLastError());
}

}  // namespace

// d_src / d_dst: 16 B aligned, n_bytes each, either the same buffer
// (in place) or non-overlapping.  Block b is
// [b*block_raw, min((b+1)*block_raw, n_bytes)).  inverse == 0 takes
// differences (raw -> filtered), nonzero sums them up again.
SY_EXPORT int sy_delta_filter(const void* d_src, void* d_dst,
                              uint64_t n_bytes, uint32_t block_raw,
                              uint32_t elem_size, int inverse,
                              hipStream_t stream) {
  if (!sy_filter_args_ok(block_raw, elem_size))
    return sy_check(hipErrorInvalidValue);
  if (n_bytes == 0) return 0;
  const uint8_t* s = static_cast<const uint8_t*>(d_src);
  uint8_t* d = static_cast<uint8_t*>(d_dst);
  switch (elem_size) {
    case 2:
      return launch<uint16_t>(s, d, n_bytes, block_raw, inverse, stream);
    case 4:
      return launch<uint32_t>(s, d, n_bytes, block_raw, inverse, stream);
    default:
      return launch<uint64_t>(s, d, n_bytes, block_raw, inverse, stream);
  }
}
