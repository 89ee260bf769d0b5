// Packed row gather for random-access SYSHARD reads (gfx950).
//
// gather_widen.hip writes one source run per output row and pads behind
// it.  A packed read puts several samples into one row: m SEGMENTS, each
// counts[i] > 0 little-endian source elements (u1, u2, i2, u4 or i4) at
// src + src_off[i], land at flat element dst_start[i] of an [n, T] batch
// of int32 or int64 (`tokens`), zero- or sign-extended.  Two int32
// tensors of the same shape go with it: `segment_ids` holds labels[i]
// over the segment's elements and `positions` 0, 1, ... counts[i] - 1.
// An element that no segment covers (before the first one, in a gap,
// behind the last one) holds pad in tokens and 0 in the other two.  The
// segments ascend and do not overlap in the destination:
// dst_start[i] + counts[i] <= dst_start[i + 1], the last one ends inside
// n * T; in the source they may overlap or repeat.  One launch writes
// every element of the three outputs exactly once and nothing else, and
// loads no byte of src outside the segments.  No output may overlap src
// or another output (the caller's promise; nothing here checks it).
// (Reference analogue: none.)
//
// Geometry.  The three outputs are 16 B aligned.  The flat elements are
// cut into GROUPS of 4: a group is one uint4 of segment_ids, one of
// positions and one (int32) or two (int64) of tokens, and its sources
// are a CHUNK of C = 4 * S bytes where they lie in one segment.  Lane l
// of a wave takes group 64*step + l, so a wave's stores are consecutive
// aligned uint4s in each of the three streams.  The last group of n * T
// may be partial; it stores its elements one by one.
//
// Work split: by destination.  A fixed grid of waves takes equal runs of
// consecutive steps.  The segment of element e is the last i with
// dst_start[i] <= e (none: pad); e is data iff e - dst_start[i] <
// counts[i].  A wave binary-searches dst_start once for the first
// element of its run and then walks forward; the segment it is in, its
// four list entries and the start of the next one live in SGPRs.
//
//   * UNIFORM step: 64 whole groups and no segment starts behind the
//     step's first element.  If the segment's data covers all of the
//     step, every lane loads its chunk and stores; the chunks of one
//     segment have the same address mod C, so the load width is picked
//     by a scalar branch, and two such steps in a row go as a pair, the
//     loads of both ahead of the first store.  If the step lies wholly
//     behind the data (or before the first segment), the lanes store pad
//     and zeros and nothing is loaded.
//   * PER-LANE step (a segment starts or its data ends inside the step,
//     which for short samples is every step; also the last step of a
//     buffer that is no multiple of 256 elements): the wave finds the
//     segment of the step's last element with a doubling search, and
//     each lane binary-searches between the two for the segment of its
//     group's first element.  A group inside one segment's data goes as
//     above with the lane's own load width, a group inside one gap is
//     pad; any other group is built element by element, moving on to the
//     next segment where it starts (segments are at least one element
//     long, so one step forward per element is enough).
//
// Source loads are as wide as the chunk's address allows and never wider
// than the chunk: C bytes when the address is a multiple of C, else
// halves, down to single elements (an element is always S-aligned: src's
// base and every src_off are multiples of S).  No load is rounded down
// or up to a wider boundary, a chunk is loaded only where all four of
// its elements are data of one segment, and a single element only where
// it is data: with segments that lie inside src no byte outside
// [src, src + numel) is touched, and none outside the segments.  The
// lists are read at indices 0 .. m - 1 only.
//
// No LDS, no barrier, no communication between waves.  Resources
// (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see the note at
// gather_pack_kernel.

#include "common.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWavesPerGroup = kThreads / SY_WAVE;
constexpr uint32_t kGroup = 4;  // elements per lane and step
constexpr uint32_t kStepElems = SY_WAVE * kGroup;
// 8 workgroups of 4 waves on each of the 256 CUs
constexpr uint32_t kGrid = 2048;
// "no next segment": above every flat index
constexpr uint64_t kNever = ~0ull;

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));
typedef uint32_t vec2 __attribute__((ext_vector_type(2)));

// W bytes at p, a multiple of W, into byte AT of the chunk image w
template <int W, int AT>
__device__ __forceinline__ void load_part(const uint8_t* p,
                                          uint32_t (&w)[4]) {
  if constexpr (W == 16) {
    const vec4 v = *reinterpret_cast<const vec4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else if constexpr (W == 8) {
    const vec2 v = *reinterpret_cast<const vec2*>(p);
    w[AT / 4] = v.x, w[AT / 4 + 1] = v.y;
  } else if constexpr (W == 4) {
    w[AT / 4] = *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (W == 2) {
    w[AT / 4] |= static_cast<uint32_t>(*reinterpret_cast<const uint16_t*>(p))
                 << (8 * (AT % 4));
  } else {
    w[AT / 4] |= static_cast<uint32_t>(*p) << (8 * (AT % 4));
  }
}

template <int C, int W, int I = 0>
__device__ __forceinline__ void load_parts(const uint8_t* p,
                                           uint32_t (&w)[4]) {
  if constexpr (I < C / W) {
    load_part<W, I * W>(p + I * W, w);
    load_parts<C, W, I + 1>(p, w);
  }
}

// The C bytes at p into w (zeroed by the caller), in loads of the widest
// W <= C that divides `addr`, the low bits of p's address (passed apart
// so that a caller whose alignment is wave-uniform gets scalar branches).
template <int C, int S, int W = C>
__device__ __forceinline__ void load_chunk(const uint8_t* p, uint32_t addr,
                                           uint32_t (&w)[4]) {
  if constexpr (W == S) {
    load_parts<C, W>(p, w);
  } else {
    if ((addr & (W - 1)) == 0)
      load_parts<C, W>(p, w);
    else
      load_chunk<C, S, W / 2>(p, addr, w);
  }
}

// low dword of element J of a chunk image, extended to 32 bits
template <int S, bool SIGNED, int J>
__device__ __forceinline__ uint32_t chunk_elem(const uint32_t (&w)[4]) {
  if constexpr (S == 4) {
    return w[J];
  } else if constexpr (S == 2) {
    const uint32_t v = (w[J / 2] >> (16 * (J % 2))) & 0xFFFFu;
    return SIGNED ? static_cast<uint32_t>(
                        static_cast<int32_t>(static_cast<int16_t>(v)))
                  : v;
  } else {
    return (w[0] >> (8 * J)) & 0xFFu;
  }
}

// one element at p, extended to 32 bits
template <int S, bool SIGNED>
__device__ __forceinline__ uint32_t load_elem(const uint8_t* p) {
  if constexpr (S == 4) {
    return *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (S == 2) {
    if constexpr (SIGNED)
      return static_cast<uint32_t>(
          static_cast<int32_t>(*reinterpret_cast<const int16_t*>(p)));
    else
      return *reinterpret_cast<const uint16_t*>(p);
  } else {
    return *p;
  }
}

// the dword above `lo` of a D == 8 element
template <bool SIGNED>
__device__ __forceinline__ uint32_t high_of(uint32_t lo) {
  return SIGNED ? static_cast<uint32_t>(static_cast<int32_t>(lo) >> 31) : 0u;
}

__device__ __forceinline__ void store16(void* p, uint32_t a, uint32_t b,
                                        uint32_t c, uint32_t d) {
  vec4 v;
  v.x = a, v.y = b, v.z = c, v.w = d;
  *reinterpret_cast<vec4*>(p) = v;
}

// The three outputs and the pad, as every store helper needs them.
struct Out {
  uint8_t* tokens;
  int32_t* segment_ids;
  int32_t* positions;
  uint32_t pad_lo, pad_hi;
};

// A whole group at flat element e0: the low dwords t of its tokens
// (SIGNED says how a D == 8 element gets its high dword; a pad element
// takes pad_hi instead where its bit of `pads` is set), labels g and
// positions q.
template <int D, bool SIGNED>
__device__ __forceinline__ void store_group(const Out& out, uint64_t e0,
                                            const uint32_t (&t)[4],
                                            const uint32_t (&g)[4],
                                            const uint32_t (&q)[4],
                                            uint32_t pads) {
  uint8_t* to = out.tokens + e0 * D;
  if constexpr (D == 4) {
    store16(to, t[0], t[1], t[2], t[3]);
  } else {
    uint32_t h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      h[j] = (pads >> j) & 1u ? out.pad_hi : high_of<SIGNED>(t[j]);
    store16(to, t[0], h[0], t[1], h[1]);
    store16(to + 16, t[2], h[2], t[3], h[3]);
  }
  store16(out.segment_ids + e0, g[0], g[1], g[2], g[3]);
  store16(out.positions + e0, q[0], q[1], q[2], q[3]);
}

// A whole group of data: the chunk at p, which is element `at` of a
// segment labelled `label`.
template <int S, int D, bool SIGNED>
__device__ __forceinline__ void data_group(const Out& out, uint64_t e0,
                                           const uint32_t (&w)[4],
                                           uint32_t at, uint32_t label) {
  const uint32_t t[4] = {chunk_elem<S, SIGNED, 0>(w),
                         chunk_elem<S, SIGNED, 1>(w),
                         chunk_elem<S, SIGNED, 2>(w),
                         chunk_elem<S, SIGNED, 3>(w)};
  const uint32_t g[4] = {label, label, label, label};
  const uint32_t q[4] = {at, at + 1, at + 2, at + 3};
  store_group<D, SIGNED>(out, e0, t, g, q, 0u);
}

// A whole group of pad.
template <int D>
__device__ __forceinline__ void pad_group(const Out& out, uint64_t e0) {
  const uint32_t t[4] = {out.pad_lo, out.pad_lo, out.pad_lo, out.pad_lo};
  const uint32_t z[4] = {0u, 0u, 0u, 0u};
  store_group<D, false>(out, e0, t, z, z, 0xFu);
}

// The four lists; entry r of them is a segment, r in [0, m).
struct Lists {
  const int64_t* src_off;
  const int64_t* counts;
  const int64_t* dst_start;
  const int32_t* labels;
  uint32_t m;
};

// One segment, or with r == -1 the stretch in front of the first one
// (no data): [start, start + count) is data, `next` the start of the
// segment behind it (kNever: none).
struct Seg {
  int64_t r;
  uint64_t start, count, next;
  int64_t off;
  uint32_t label;
};

__device__ __forceinline__ Seg load_seg(const Lists& ls, int64_t r) {
  Seg s;
  s.r = r;
  s.start = 0, s.count = 0, s.off = 0, s.label = 0;
  if (r >= 0) {
    s.start = static_cast<uint64_t>(ls.dst_start[r]);
    s.count = static_cast<uint64_t>(ls.counts[r]);
    s.off = ls.src_off[r];
    s.label = static_cast<uint32_t>(ls.labels[r]);
  }
  s.next = r + 1 < static_cast<int64_t>(ls.m)
               ? static_cast<uint64_t>(ls.dst_start[r + 1])
               : kNever;
  return s;
}

// Largest r in [lo, hi] with dst_start[r] <= e; lo itself is known to
// qualify (or is -1, which always does) and is never read.
__device__ __forceinline__ int64_t seg_search(
    const int64_t* __restrict__ dst_start, int64_t lo, int64_t hi,
    uint64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;  // lo < mid <= hi
    if (static_cast<uint64_t>(dst_start[mid]) <= e)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The same over [lo, m) for a segment that is expected to be near lo:
// doubling strides until a segment starts behind e, then the binary
// search.
__device__ __forceinline__ int64_t seg_forward(
    const int64_t* __restrict__ dst_start, uint32_t m, int64_t lo,
    uint64_t e) {
  int64_t hi, stride = 1;
  while (true) {
    const int64_t cand = lo + stride;
    if (cand >= static_cast<int64_t>(m)) {
      hi = static_cast<int64_t>(m) - 1;
      break;
    }
    if (static_cast<uint64_t>(dst_start[cand]) > e) {
      hi = cand - 1;
      break;
    }
    lo = cand;
    stride *= 2;
  }
  return seg_search(dst_start, lo, hi, e);
}

// The lane's group of a per-lane step, whatever it holds; the step's
// elements lie in segments r_first .. r_last (r_first may be -1).
template <int S, int D, bool SIGNED>
__device__ __forceinline__ void group_per_lane(
    uint64_t e0, const uint8_t* __restrict__ src, const Lists& ls,
    const Out& out, uint64_t n_elems, int64_t r_first, int64_t r_last) {
  constexpr int C = kGroup * S;
  if (e0 >= n_elems) return;  // behind the last group
  Seg s = load_seg(ls, seg_search(ls.dst_start, r_first, r_last, e0));
  const bool whole = e0 + kGroup <= n_elems;
  if (whole && e0 + kGroup <= s.start + s.count) {
    // all of it data of one segment (start <= e0)
    const uint64_t at = e0 - s.start;
    const uint8_t* p = src + s.off + at * S;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    load_chunk<C, S>(p, static_cast<uint32_t>(reinterpret_cast<uint64_t>(p)),
                     w);
    data_group<S, D, SIGNED>(out, e0, w, static_cast<uint32_t>(at), s.label);
    return;
  }
  if (whole && e0 >= s.start + s.count && e0 + kGroup <= s.next) {
    pad_group<D>(out, e0);  // all of it in one gap
    return;
  }
  // element by element: data ends or a segment starts inside the group,
  // or it is the partial last group of the buffer
  uint32_t t[4], g[4], q[4], pads = 0;
#pragma unroll
  for (int j = 0; j < static_cast<int>(kGroup); ++j) {
    const uint64_t e = e0 + j;
    t[j] = out.pad_lo, g[j] = 0u, q[j] = 0u;
    if (e < n_elems) {
      if (e >= s.next) s = load_seg(ls, s.r + 1);  // starts at e exactly
      const uint64_t at = e - s.start;
      if (at < s.count) {
        t[j] = load_elem<S, SIGNED>(src + s.off + at * S);
        g[j] = s.label;
        q[j] = static_cast<uint32_t>(at);
      } else {
        pads |= 1u << j;
      }
    }
  }
  if (whole) {
    store_group<D, SIGNED>(out, e0, t, g, q, pads);
    return;
  }
  // the partial last group: the elements that exist, one store each
#pragma unroll
  for (int j = 0; j < static_cast<int>(kGroup) - 1; ++j) {
    const uint64_t e = e0 + j;
    if (e >= n_elems) break;
    uint32_t* tok = reinterpret_cast<uint32_t*>(out.tokens + e * D);
    tok[0] = t[j];
    if constexpr (D == 8)
      tok[1] = (pads >> j) & 1u ? out.pad_hi : high_of<SIGNED>(t[j]);
    out.segment_ids[e] = static_cast<int32_t>(g[j]);
    out.positions[e] = static_cast<int32_t>(q[j]);
  }
}

// Resources on gfx950 (kernel-resource-usage): see docs/35-gpu-data-plane.md,
// "Packed row reads"; no scratch, no LDS in any of the nine
// instantiations.
template <int S, int D, bool SIGNED>
__global__ __launch_bounds__(kThreads) void gather_pack_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
    const int64_t* __restrict__ counts, const int64_t* __restrict__ dst_start,
    const int32_t* __restrict__ labels, uint8_t* __restrict__ tokens,
    int32_t* __restrict__ segment_ids, int32_t* __restrict__ positions,
    uint32_t m, uint64_t n_elems, uint32_t pad_lo, uint32_t pad_hi) {
  constexpr uint32_t C = kGroup * S;
  const uint32_t lane = threadIdx.x % SY_WAVE;
  // the wave id in an SGPR, so that all that follows from it is scalar
  const uint32_t wave = __builtin_amdgcn_readfirstlane(
      blockIdx.x * kWavesPerGroup + threadIdx.x / SY_WAVE);
  const uint64_t n_steps = (n_elems + kStepElems - 1) / kStepElems;
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerGroup;
  const uint64_t per_wave = (n_steps + n_waves - 1) / n_waves;
  uint64_t step = wave * per_wave;
  const uint64_t step_end =
      step + per_wave < n_steps ? step + per_wave : n_steps;
  if (step >= step_end) return;

  const Lists ls = {src_off, counts, dst_start, labels, m};
  const Out out = {tokens, segment_ids, positions, pad_lo, pad_hi};
  const uint64_t sb = reinterpret_cast<uint64_t>(src);
  // e: the step's first element (< n_elems: the step has a group); s:
  // the segment it lies in, the last one that starts at or before it
  uint64_t e = step * kStepElems;
  Seg s = load_seg(
      ls, seg_search(dst_start, -1, static_cast<int64_t>(m) - 1, e));
  while (true) {
    const uint64_t e0 = e + lane * kGroup;
    uint32_t took = 1;  // steps done in this round
    const uint64_t data_end = s.start + s.count;
    if (e + kStepElems <= n_elems && s.next >= e + kStepElems &&
        data_end >= e + kStepElems) {
      // 64 whole groups, all of them data of segment s
      const uint64_t at = e - s.start;
      const uint8_t* p = src + s.off + (at + lane * kGroup) * S;
      const uint32_t addr = static_cast<uint32_t>(sb + s.off + at * S);
      const uint32_t pos = static_cast<uint32_t>(at) + lane * kGroup;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (step + 1 < step_end && data_end >= e + 2 * kStepElems &&
          e + 2 * kStepElems <= n_elems) {
        // the next step is all data of s too: both steps' loads go out
        // before the first store
        uint32_t w2[4] = {0u, 0u, 0u, 0u};
        load_chunk<C, S>(p, addr, w);
        load_chunk<C, S>(p + SY_WAVE * C, addr, w2);  // 64 * C: same mod C
        data_group<S, D, SIGNED>(out, e0, w, pos, s.label);
        data_group<S, D, SIGNED>(out, e0 + kStepElems, w2, pos + kStepElems,
                                 s.label);
        took = 2;
      } else {
        load_chunk<C, S>(p, addr, w);
        data_group<S, D, SIGNED>(out, e0, w, pos, s.label);
      }
    } else if (e + kStepElems <= n_elems && s.next >= e + kStepElems &&
               data_end <= e) {
      pad_group<D>(out, e0);  // 64 whole groups of one gap
    } else {
      const uint64_t e_last =
          (e + kStepElems < n_elems ? e + kStepElems : n_elems) - 1;
      const int64_t r_last = seg_forward(dst_start, m, s.r, e_last);
      group_per_lane<S, D, SIGNED>(e0, src, ls, out, n_elems, s.r, r_last);
      if (r_last != s.r) s = load_seg(ls, r_last);
    }
    step += took;
    if (step >= step_end) break;
    e += took * kStepElems;  // < n_elems: there is a next step
    if (s.next <= e) s = load_seg(ls, seg_forward(dst_start, m, s.r, e));
  }
}

template <int S, int D, bool SIGNED>
int launch(const void* d_src, const int64_t* d_src_off,
           const int64_t* d_counts, const int64_t* d_dst_start,
           const int32_t* d_labels, void* d_tokens, int32_t* d_segment_ids,
           int32_t* d_positions, uint32_t m, uint64_t n_elems, int64_t pad,
           hipStream_t stream) {
  const uint64_t per_group = static_cast<uint64_t>(kThreads) * kGroup;
  const uint64_t groups = (n_elems + per_group - 1) / per_group;
  const uint64_t bits = static_cast<uint64_t>(pad);
  hipLaunchKernelGGL((gather_pack_kernel<S, D, SIGNED>),
                     dim3(groups < kGrid ? static_cast<uint32_t>(groups)
                                         : kGrid),
                     dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(d_src), d_src_off, d_counts,
                     d_dst_start, d_labels, static_cast<uint8_t*>(d_tokens),
                     d_segment_ids, d_positions, m, n_elems,
                     static_cast<uint32_t>(bits),
                     static_cast<uint32_t>(bits >> 32));
  return sy_check(hipGetLastError());
}

}  // namespace

// For every segment i < m: tokens[dst_start[i] + c] = element c of the
// counts[i] elements of src_size bytes at src + src_off[i], zero-extended
// or (src_signed) sign-extended to dst_size bytes, segment_ids[...] =
// labels[i], positions[...] = c; every other of the n_elems elements:
// pad, 0, 0.  The three outputs are 16 B aligned; src's base and every
// src_off are multiples of src_size; counts[i] > 0, dst_start ascends
// with dst_start[i] + counts[i] <= dst_start[i + 1] and the last segment
// ends inside n_elems; every segment lies inside src; m < 2^31.  -22
// (EINVAL) for sizes outside {1, 2, 4} -> {4, 8}, a signed 1-byte
// source, unsigned 4 -> 4, which loses values, m >= 2^31 and a
// misaligned output.
SY_EXPORT int sy_gather_pack(const void* d_src, const int64_t* d_src_off,
                             const int64_t* d_counts,
                             const int64_t* d_dst_start,
                             const int32_t* d_labels, void* d_tokens,
                             int32_t* d_segment_ids, int32_t* d_positions,
                             uint32_t m, uint64_t n_elems, uint32_t src_size,
                             int src_signed, uint32_t dst_size, int64_t pad,
                             hipStream_t stream) {
  if (dst_size != 4 && dst_size != 8) return -22;
  if (m >= 0x80000000u) return -22;
  if ((reinterpret_cast<uint64_t>(d_tokens) |
       reinterpret_cast<uint64_t>(d_segment_ids) |
       reinterpret_cast<uint64_t>(d_positions)) & 15u)
    return -22;
  if (n_elems == 0) return 0;
  const bool wide = dst_size == 8;
#define SY_PACK_AS(S, D, SIGNED)                                           \
  launch<S, D, SIGNED>(d_src, d_src_off, d_counts, d_dst_start, d_labels, \
                       d_tokens, d_segment_ids, d_positions, m, n_elems,  \
                       pad, stream)
#define SY_PACK(S, SIGNED) \
  (wide ? SY_PACK_AS(S, 8, SIGNED) : SY_PACK_AS(S, 4, SIGNED))
  switch (src_size) {
    case 1:
      return src_signed ? -22 : SY_PACK(1, false);
    case 2:
      return src_signed ? SY_PACK(2, true) : SY_PACK(2, false);
    case 4:
      if (!wide)  // a copy; only the signed reading keeps every value
        return src_signed ? SY_PACK_AS(4, 4, false) : -22;
      return src_signed ? SY_PACK_AS(4, 8, true) : SY_PACK_AS(4, 8, false);
    default:
      return -22;
  }
#undef SY_PACK
#undef SY_PACK_AS
}
