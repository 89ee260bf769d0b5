// Typed row compaction for SYSHARD authoring (gfx950): the inverse of
// gather_widen.hip.
//
// A tokeniser or a filter pass hands over what a row read produces: a
// contiguous [n, T] batch of int32 or int64 of which row i is live in
// its first counts[i] columns and padding behind them.  A typed shard
// wants the live elements alone, one after the other, as little-endian
// u1, u2, i2, u4 or i4.  row_start is the exclusive prefix sum of the
// counts (n + 1 entries, row_start[n] = total), so element
// row_start[i] + c of the stream is src[i, c] for c < counts[i], reduced
// to its low S bytes.  One launch writes every byte of dst[0, total*S)
// exactly once and nothing behind it, loads live elements only (a
// padding column is never loaded, so never range-checked, and no byte
// outside src is touched), and leaves in *status the smallest stream
// index whose value the destination type cannot hold.  dst must not
// overlap src (the caller's promise).  (Reference analogue: none.)
//
// Geometry.  dst is 16 B aligned and is cut into SLOTS of 16 B; a slot
// holds EPS = 16 / S stream elements, whose sources are a CHUNK of
// C = EPS * W bytes where they lie in one row (W: 4 or 8, the source
// width; C is 16 to 128).  Lane l of a wave takes slot 64*step + l, so
// a wave's store is 1 KiB of consecutive aligned uint4s.
//
// Work split: by destination bytes.  The grid is fixed and every wave
// reads total = row_start[n] on the device (no host sync), takes an
// equal run of consecutive steps, finds the row of its first element
// with one binary search in row_start and then walks forward; all of
// that is wave-uniform and lives in SGPRs.
//
//   * UNIFORM step: all 64 slots lie inside one row.  Every lane loads
//     its chunk and stores a uint4.  The chunks of one step have the
//     same address mod 16 (C is a multiple of 16), so the load width is
//     picked by a scalar branch: 16 B loads when the chunk is 16 B
//     aligned, else 8 B, else (an int32 row with odd T, or a view at +1
//     element) 4 B.  A load is never rounded to a wider boundary.
//   * PER-LANE step (a row ends inside the wave's 1 KiB, which for
//     short rows is every step; also the last step of the stream): the
//     wave finds the row of the step's last element, and each lane
//     finds its own row between the two with a binary search.  A slot
//     inside one row goes as above with the lane's own load width; a
//     slot that crosses a row end is built element by element, each
//     element that leaves the row looking its row up (runs of empty
//     rows of any length cost one search); the partial last slot of the
//     stream stores its elements one by one.
//
// Range check.  Every loaded element gives a word that is zero iff the
// value survives the narrowing; a chunk ORs them, so clean data costs
// one OR per element and one test per chunk.  A lane keeps the smallest
// stream index that failed; before a wave leaves it reduces the 64
// lanes with shuffles, and if any lane had a misfit (one ballot, a
// scalar branch) lane 0 issues one 64-bit atomic min on *status.  A
// misfit is stored truncated like every other value.
//
// No LDS, no barrier, no communication between waves but that atomic.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see
// the note at compact_narrow_kernel.

#include "common.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWavesPerGroup = kThreads / SY_WAVE;
constexpr uint32_t kSlot = 16;  // bytes per store
// 8 workgroups of 4 waves on each of the 256 CUs; a small stream leaves
// most of them with nothing (they read row_start[n] and leave)
constexpr uint32_t kGrid = 2048;
constexpr uint64_t kClean = 0x7FFFFFFFFFFFFFFFull;  // INT64_MAX

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));
typedef uint32_t vec2 __attribute__((ext_vector_type(2)));

// C bytes at p, a multiple of LW, in loads of LW bytes
template <int C, int LW>
__device__ __forceinline__ void load_words(const uint8_t* p,
                                           uint32_t (&w)[C / 4]) {
#pragma unroll
  for (int i = 0; i < C / LW; ++i) {
    if constexpr (LW == 16) {
      const vec4 v = *reinterpret_cast<const vec4*>(p + 16 * i);
      w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z,
            w[4 * i + 3] = v.w;
    } else if constexpr (LW == 8) {
      const vec2 v = *reinterpret_cast<const vec2*>(p + 8 * i);
      w[2 * i] = v.x, w[2 * i + 1] = v.y;
    } else {
      w[i] = *reinterpret_cast<const uint32_t*>(p + 4 * i);
    }
  }
}

// The C bytes at p in the widest loads that `addr`, the low bits of p's
// address, allows (passed apart so that a caller whose alignment is
// wave-uniform gets scalar branches).  p is a multiple of W.
template <int C, int W>
__device__ __forceinline__ void load_chunk(const uint8_t* p, uint32_t addr,
                                           uint32_t (&w)[C / 4]) {
  if ((addr & 15u) == 0)
    load_words<C, 16>(p, w);
  else if (W == 8 || (addr & 7u) == 0)
    load_words<C, 8>(p, w);
  else
    load_words<C, 4>(p, w);
}

// Zero iff the W-byte two's complement value {hi, lo} (hi unused for
// W == 4) is representable in S bytes, SIGNED or not.
template <int W, int S, bool SIGNED>
__device__ __forceinline__ uint32_t misfit(uint32_t lo, uint32_t hi) {
  if constexpr (S == 4) {
    if constexpr (W == 8)
      return SIGNED ? hi ^ static_cast<uint32_t>(static_cast<int32_t>(lo) >> 31)
                    : hi;
    else
      return SIGNED ? 0u : lo >> 31;
  } else if constexpr (SIGNED) {  // S == 2
    const int32_t s = static_cast<int16_t>(lo);
    const uint32_t low = static_cast<uint32_t>(s) ^ lo;
    return W == 8 ? low | (hi ^ static_cast<uint32_t>(s >> 31)) : low;
  } else {
    const uint32_t low = lo >> (8 * S);
    return W == 8 ? low | hi : low;
  }
}

// element j of a slot's 16 bytes; the elements come in order, j from 0
template <int S>
__device__ __forceinline__ void put(uint32_t (&o)[4], int j, uint32_t lo) {
  if constexpr (S == 4) {
    o[j] = lo;
  } else if constexpr (S == 2) {
    if (j % 2 == 0)
      o[j / 2] = lo & 0xFFFFu;
    else
      o[j / 2] |= lo << 16;
  } else {
    if (j % 4 == 0)
      o[j / 4] = lo & 0xFFu;
    else
      o[j / 4] |= (lo & 0xFFu) << (8 * (j % 4));
  }
}

__device__ __forceinline__ void store16(uint8_t* p, const uint32_t (&o)[4]) {
  vec4 v;
  v.x = o[0], v.y = o[1], v.z = o[2], v.w = o[3];
  *reinterpret_cast<vec4*>(p) = v;
}

// A slot whose EPS elements are the chunk at p: load, check, narrow and
// store.  e0 is the stream index of its first element.
template <int W, int S, bool SIGNED>
__device__ __forceinline__ void slot_from_chunk(const uint8_t* p,
                                                uint32_t addr, uint8_t* to,
                                                uint64_t e0, uint64_t& bad) {
  constexpr int EPS = kSlot / S;
  constexpr int C = EPS * W;
  uint32_t w[C / 4], o[4];
  load_chunk<C, W>(p, addr, w);
  uint32_t any = 0;
#pragma unroll
  for (int j = 0; j < EPS; ++j) {
    const uint32_t lo = w[j * (W / 4)];
    const uint32_t hi = W == 8 ? w[j * (W / 4) + W / 4 - 1] : 0u;
    any |= misfit<W, S, SIGNED>(lo, hi);
    put<S>(o, j, lo);
  }
  store16(to, o);
  if (any) {  // rare: which element was it
    uint32_t first = 0;
#pragma unroll
    for (int j = EPS - 1; j >= 0; --j) {
      const uint32_t lo = w[j * (W / 4)];
      const uint32_t hi = W == 8 ? w[j * (W / 4) + W / 4 - 1] : 0u;
      if (misfit<W, S, SIGNED>(lo, hi)) first = j;
    }
    bad = e0 + first < bad ? e0 + first : bad;
  }
}

// Smallest r in [lo, hi] with row_start[r + 1] > e; the caller
// guarantees row_start[hi + 1] > e and row_start[lo] <= e.
__device__ __forceinline__ uint32_t row_search(
    const int64_t* __restrict__ row_start, uint32_t lo, uint32_t hi,
    uint64_t e) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (static_cast<uint64_t>(row_start[static_cast<uint64_t>(mid) + 1]) > e)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The same for a row at or after `lo` that is expected to be near:
// doubling strides until a row ends behind e, then the binary search.
// e < row_start[n].
__device__ __forceinline__ uint32_t row_forward(
    const int64_t* __restrict__ row_start, uint32_t n, uint32_t lo,
    uint64_t e) {
  uint64_t hi = lo, stride = 1;
  while (static_cast<uint64_t>(row_start[hi + 1]) <= e) {
    lo = static_cast<uint32_t>(hi + 1);
    stride *= 2;
    hi = hi + stride < n ? hi + stride : n - 1;  // row_start[n] > e
  }
  return row_search(row_start, lo, static_cast<uint32_t>(hi), e);
}

// one element of the stream, e, which lies in row r (from rs): loaded,
// checked; returns its low dword
template <int W, int S, bool SIGNED>
__device__ __forceinline__ uint32_t take_elem(const uint8_t* __restrict__ src,
                                              uint32_t T, uint32_t r,
                                              uint64_t rs, uint64_t e,
                                              uint64_t& bad) {
  const uint8_t* p = src + (static_cast<uint64_t>(r) * T + (e - rs)) * W;
  uint32_t lo, hi = 0;
  if constexpr (W == 8) {
    const vec2 v = *reinterpret_cast<const vec2*>(p);
    lo = v.x, hi = v.y;
  } else {
    lo = *reinterpret_cast<const uint32_t*>(p);
  }
  if (misfit<W, S, SIGNED>(lo, hi)) bad = e < bad ? e : bad;
  return lo;
}

// The lane's slot of a step in which a row ends (or the stream): the
// step's elements lie in rows r_first .. r_last.
template <int W, int S, bool SIGNED>
__device__ __forceinline__ void slot_per_lane(
    uint64_t e0, const uint8_t* __restrict__ src,
    const int64_t* __restrict__ row_start, uint8_t* __restrict__ dst,
    uint64_t total, uint32_t T, uint32_t r_first, uint32_t r_last,
    uint64_t& bad) {
  constexpr int EPS = kSlot / S;
  if (e0 >= total) return;  // behind the last slot
  uint32_t r = row_search(row_start, r_first, r_last, e0);
  uint64_t rs = static_cast<uint64_t>(row_start[r]);
  uint64_t re = static_cast<uint64_t>(row_start[static_cast<uint64_t>(r) + 1]);
  uint8_t* to = dst + e0 * S;
  if (e0 + EPS <= re) {  // re <= total: a whole slot inside one row
    const uint8_t* p = src + (static_cast<uint64_t>(r) * T + (e0 - rs)) * W;
    slot_from_chunk<W, S, SIGNED>(
        p, static_cast<uint32_t>(reinterpret_cast<uint64_t>(p)), to, e0, bad);
    return;
  }
  if (e0 + EPS <= total) {  // a whole slot across a row end
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < EPS; ++j) {
      const uint64_t e = e0 + j;
      if (e >= re) {  // e <= the step's last element, which r_last holds
        r = row_search(row_start, r + 1, r_last, e);
        rs = static_cast<uint64_t>(row_start[r]);
        re = static_cast<uint64_t>(row_start[static_cast<uint64_t>(r) + 1]);
      }
      put<S>(o, j, take_elem<W, S, SIGNED>(src, T, r, rs, e, bad));
    }
    store16(to, o);
    return;
  }
  // the partial last slot of the stream: the elements that exist, one
  // store each
#pragma unroll 1
  for (uint64_t e = e0; e < total; ++e) {
    if (e >= re) {
      r = row_search(row_start, r + 1, r_last, e);
      rs = static_cast<uint64_t>(row_start[r]);
      re = static_cast<uint64_t>(row_start[static_cast<uint64_t>(r) + 1]);
    }
    const uint32_t lo = take_elem<W, S, SIGNED>(src, T, r, rs, e, bad);
    uint8_t* out = dst + e * S;
    if constexpr (S == 4)
      *reinterpret_cast<uint32_t*>(out) = lo;
    else if constexpr (S == 2)
      *reinterpret_cast<uint16_t*>(out) = static_cast<uint16_t>(lo);
    else
      *out = static_cast<uint8_t>(lo);
  }
}

// Resources on gfx950 (kernel-resource-usage), over the ten
// instantiations: 28 to 64 VGPRs, at most 74 SGPRs and occupancy 8
// waves per SIMD, so the 2048 workgroups of the grid are all resident
// at once (8 per CU); int64 -> u1, whose chunk is 128 B per lane, takes
// 80 VGPRs and runs at 6 waves per SIMD.  No scratch, no LDS.
template <int W, int S, bool SIGNED>
__global__ __launch_bounds__(kThreads) void compact_narrow_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ row_start,
    uint8_t* __restrict__ dst, int64_t* __restrict__ status, uint32_t n,
    uint32_t T) {
  constexpr uint32_t EPS = kSlot / S;
  constexpr uint32_t C = EPS * W;
  constexpr uint32_t kStepElems = SY_WAVE * EPS;
  const uint32_t lane = threadIdx.x % SY_WAVE;
  // the wave id in an SGPR, so that all that follows from it is scalar
  const uint32_t wave = __builtin_amdgcn_readfirstlane(
      blockIdx.x * kWavesPerGroup + threadIdx.x / SY_WAVE);
  const uint64_t total = static_cast<uint64_t>(row_start[n]);
  const uint64_t n_slots = (total + EPS - 1) / EPS;
  const uint64_t n_steps = (n_slots + SY_WAVE - 1) / SY_WAVE;
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerGroup;
  const uint64_t per_wave = (n_steps + n_waves - 1) / n_waves;
  uint64_t step = wave * per_wave;
  const uint64_t step_end =
      step + per_wave < n_steps ? step + per_wave : n_steps;
  if (step >= step_end) return;

  const uint64_t sb = reinterpret_cast<uint64_t>(src);
  uint64_t bad = kClean;
  // e: the step's first element, which lies in row r = [rs, re)
  uint64_t e = step * kStepElems;  // < total: the step has a slot
  uint32_t r = row_search(row_start, 0, n - 1, e);
  uint64_t rs = static_cast<uint64_t>(row_start[r]);
  uint64_t re = static_cast<uint64_t>(row_start[static_cast<uint64_t>(r) + 1]);
  while (true) {
    const uint64_t e0 = e + lane * EPS;
    if (e + kStepElems <= re) {
      // all of the step inside row r
      const uint64_t at = (static_cast<uint64_t>(r) * T + (e - rs)) * W;
      slot_from_chunk<W, S, SIGNED>(src + at + lane * C,
                                    static_cast<uint32_t>(sb + at),
                                    dst + e0 * S, e0, bad);
    } else {
      const uint64_t e_last =
          (e + kStepElems < total ? e + kStepElems : total) - 1;
      const uint32_t r_last = row_forward(row_start, n, r, e_last);
      slot_per_lane<W, S, SIGNED>(e0, src, row_start, dst, total, T, r,
                                  r_last, bad);
      if (r_last != r) {
        r = r_last;
        rs = static_cast<uint64_t>(row_start[r]);
        re = static_cast<uint64_t>(
            row_start[static_cast<uint64_t>(r) + 1]);
      }
    }
    if (++step >= step_end) break;
    e += kStepElems;  // < total: there is a next step
    if (e >= re) {
      r = row_forward(row_start, n, r, e);
      rs = static_cast<uint64_t>(row_start[r]);
      re = static_cast<uint64_t>(row_start[static_cast<uint64_t>(r) + 1]);
    }
  }

  // the wave's smallest misfit; nothing but the ballot on clean data
  if (__ballot(bad != kClean) == 0) return;
#pragma unroll
  for (int d = SY_WAVE / 2; d > 0; d /= 2) {
    const uint64_t other = __shfl_xor(static_cast<unsigned long long>(bad), d);
    bad = other < bad ? other : bad;
  }
  if (lane == 0)
    __hip_atomic_fetch_min(status, static_cast<int64_t>(bad),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int W, int S, bool SIGNED>
int launch(const void* d_src, const int64_t* d_row_start, void* d_dst,
           int64_t* d_status, uint32_t n, uint32_t T, hipStream_t stream) {
  hipLaunchKernelGGL((compact_narrow_kernel<W, S, SIGNED>), dim3(kGrid),
                     dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(d_src), d_row_start,
                     static_cast<uint8_t*>(d_dst), d_status, n, T);
  return sy_check(hipGetLastError());
}

}  // namespace

// The stream of the live elements of src, an [n, T] batch of src_size
// (4 or 8) byte signed integers: element row_start[i] + c of dst, for
// c < row_start[i + 1] - row_start[i], is the low dst_size (1, 2 or 4)
// bytes of src[i, c].  row_start has n + 1 ascending entries from 0 with
// steps of at most T; dst is 16 B aligned and holds row_start[n] *
// dst_size bytes; src's base is a multiple of src_size.  *d_status,
// which the caller sets to INT64_MAX, receives the smallest stream
// index whose value dst_size bytes, read as dst_signed says, cannot
// hold.  -22 (EINVAL) for other sizes and for a signed 1-byte type.
SY_EXPORT int sy_compact_narrow(const void* d_src, const int64_t* d_row_start,
                                void* d_dst, int64_t* d_status, uint32_t n,
                                uint32_t T, uint32_t src_size,
                                uint32_t dst_size, int dst_signed,
                                hipStream_t stream) {
  if (src_size != 4 && src_size != 8) return -22;
  if (T >= 0x7FFFFF00u) return -22;
  if (n == 0 || T == 0) return 0;
  const bool wide = src_size == 8;
#define SY_NARROW(S, SIGNED)                                              \
  (wide ? launch<8, S, SIGNED>(d_src, d_row_start, d_dst, d_status, n, T, \
                               stream)                                    \
        : launch<4, S, SIGNED>(d_src, d_row_start, d_dst, d_status, n, T, \
                               stream))
  switch (dst_size) {
    case 1:
      return dst_signed ? -22 : SY_NARROW(1, false);
    case 2:
      return dst_signed ? SY_NARROW(2, true) : SY_NARROW(2, false);
    case 4:
      return dst_signed ? SY_NARROW(4, true) : SY_NARROW(4, false);
    default:
      return -22;
  }
#undef SY_NARROW
}
