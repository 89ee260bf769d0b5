// Device leaves shared by the tile-transposing SYSHARD block filters
// (byte_shuffle.hip, bit_shuffle.hip): a 4 KiB raw tile, 256 threads x
// 16 B, moves between its raw form (element-major) and its byte-plane
// form (plane j at j*T, T = 4096/E: byte j of each of the tile's T
// elements) by a 16-byte in-register permutation plus one narrow LDS
// access per plane.  Bank-conflict reasoning: byte_shuffle.hip's header.
#pragma once

#include "common.h"

namespace {

constexpr uint32_t kTileBytes = 4096;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kUnroll = 4;

// native vectors (not the HIP structs): a struct copy through a
// may_alias type takes the register array's address and spills it
typedef uint32_t vec4 __attribute__((ext_vector_type(4)));
typedef uint32_t vec2 __attribute__((ext_vector_type(2)));
typedef vec4 __attribute__((may_alias)) lds_u4;
typedef vec2 __attribute__((may_alias)) lds_u2;
typedef uint32_t __attribute__((may_alias)) lds_u32;
typedef uint16_t __attribute__((may_alias)) lds_u16;

// 16-byte permutation between a lane's raw bytes (element-major,
// byte e*E + j) and its piece-major form (byte j*P + e).  All indices
// are compile-time, the arrays stay in registers.
template <int E, bool TO_RAW>
__device__ __forceinline__ void permute16(const uint32_t (&in)[4],
                                          uint32_t (&out)[4]) {
  constexpr int P = 16 / E;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t acc = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = d * 4 + b;
      const int s = TO_RAW ? ((k % E) * P + k / E) : ((k % P) * E + k / P);
      acc |= ((in[s >> 2] >> ((s & 3) * 8)) & 0xffu) << (b * 8);
    }
    out[d] = acc;
  }
}

// piece j of a lane (bytes [j*P, j*P+P) of its piece-major registers)
// <-> LDS at plane j, lane offset P*t
template <int E>
__device__ __forceinline__ void lds_put_pieces(uint8_t* tile, uint32_t t,
                                               const uint32_t (&pm)[4]) {
  constexpr uint32_t T = kTileBytes / E;
  if constexpr (E == 2) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      *reinterpret_cast<lds_u2*>(tile + j * T + 8 * t) =
          vec2{pm[2 * j], pm[2 * j + 1]};
  } else if constexpr (E == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<lds_u32*>(tile + j * T + 4 * t) = pm[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      *reinterpret_cast<lds_u16*>(tile + j * T + 2 * t) =
          static_cast<uint16_t>(pm[j >> 1] >> ((j & 1) * 16));
  }
}

template <int E>
__device__ __forceinline__ void lds_get_pieces(const uint8_t* tile,
                                               uint32_t t,
                                               uint32_t (&pm)[4]) {
  constexpr uint32_t T = kTileBytes / E;
  if constexpr (E == 2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const vec2 v = *reinterpret_cast<const lds_u2*>(tile + j * T + 8 * t);
      pm[2 * j] = v.x;
      pm[2 * j + 1] = v.y;
    }
  } else if constexpr (E == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pm[j] = *reinterpret_cast<const lds_u32*>(tile + j * T + 4 * t);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo =
          *reinterpret_cast<const lds_u16*>(tile + (2 * j) * T + 2 * t);
      const uint32_t hi =
          *reinterpret_cast<const lds_u16*>(tile + (2 * j + 1) * T + 2 * t);
      pm[j] = lo | (hi << 16);
    }
  }
}

}  // namespace
