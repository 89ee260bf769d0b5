// Typed row gather for random-access SYSHARD reads (gfx950).
//
// A row read wants the decoded scratch as a [n, T] batch of int32 or
// int64: row i holds the counts[i] little-endian source elements (u1,
// u2, i2, u4 or i4) at src + src_off[i], zero- or sign-extended, and
// then T - counts[i] copies of a pad value.  gather_ranges.hip delivers
// bytes padded with one byte value, so a pad id such as 50256 or -100
// took a fill, the gather, a widening pass and a masked overwrite.  Here
// the destination is a regular buffer of n*T*D bytes, every element of
// it either data or pad, and one launch writes each of its bytes exactly
// once and reads the source bytes of each row once (a byte that several
// rows share is read once for each of them).  Rows in any order, source
// rows that overlap or repeat, counts of 0.  dst must not overlap src (the
// caller's promise; nothing here checks it).  (Reference analogue: none.)
//
// Geometry.  dst is cut into SLOTS of 16 B at absolute 16 B boundaries;
// dst's base is a multiple of D but maybe not of 16, so the first and the
// last slot of the buffer may be partial.  A slot holds EPS = 16 / D
// elements; element e of the buffer is row e / T, column e % T.  Lane l
// of a wave takes slot 64*step + l, so a wave's store is 1 KiB of
// consecutive aligned uint4s.
//
// Work split: by destination bytes.  A fixed grid of waves takes equal
// runs of consecutive steps.  A wave divides once (64 bits) to find the
// row and column of its first element and then moves on by adding, with
// one 32-bit division per step; all of that is wave-uniform.
//
//   * UNIFORM step: all 64 slots lie inside one row.  The row's src_off
//     and counts are scalar loads, kept while the wave stays in the row;
//     two steps in a row that are both all data go as a pair, the loads
//     of both ahead of the first store.  If the row's data covers all of the
//     step, every lane loads its EPS source elements (a CHUNK of
//     C = EPS * S bytes) and stores a uint4; the chunks of one row have
//     the same address mod C, so the load width below is picked by a
//     scalar branch.  If the step lies wholly in the row's padding, the
//     lanes store the pad pattern and nothing is loaded.  Only the one
//     step that holds the end of the row's data goes the lanes' way.
//   * PER-LANE step (a row ends inside the wave's 1 KiB, which for small
//     T is every step; also the partial slots): the lane divides (32
//     bits) to find the row and column of its slot, loads that row's
//     src_off and counts itself, and builds its 16 bytes element by
//     element where the slot crosses a row or the end of the row's data.
//     A partial slot stores its elements one by one.
//
// Source loads are as wide as the chunk's address allows and never wider
// than the chunk: C bytes when the address is a multiple of C, else
// halves, down to single elements (an element is always S-aligned: src's
// base and every src_off are multiples of S).  No load is ever rounded
// down or up to a wider boundary, so no byte in front of a row's first
// element or behind its last one is touched, and with rows that lie
// inside src none outside [src, src + numel).
//
// No LDS, no barrier, no communication between waves.  Resources
// (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see the note at
// gather_widen_kernel.

#include "common.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWavesPerGroup = kThreads / SY_WAVE;
constexpr uint32_t kSlot = 16;  // bytes per store
// 8 workgroups of 4 waves on each of the 256 CUs
constexpr uint32_t kGrid = 2048;

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

// The C bytes at p into w, in loads of the widest W <= C that divides
// `addr`, the low bits of p's address (passed apart so that a caller
// whose alignment is wave-uniform gets scalar branches).
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

// element j of a slot's 16 bytes
template <int D>
__device__ __forceinline__ void put(uint32_t (&o)[4], int j, uint32_t lo,
                                    uint32_t hi) {
  if constexpr (D == 4) {
    o[j] = lo;
  } else {
    o[2 * j] = lo;
    o[2 * j + 1] = hi;
  }
}

template <int S, int D, bool SIGNED, int J = 0>
__device__ __forceinline__ void widen_chunk(const uint32_t (&w)[4],
                                            uint32_t (&o)[4]) {
  if constexpr (J < 16 / D) {
    const uint32_t lo = chunk_elem<S, SIGNED, J>(w);
    put<D>(o, J, lo, high_of<SIGNED>(lo));
    widen_chunk<S, D, SIGNED, J + 1>(w, o);
  }
}

__device__ __forceinline__ void store16(uint8_t* p, const uint32_t (&o)[4]) {
  vec4 v;
  v.x = o[0], v.y = o[1], v.z = o[2], v.w = o[3];
  *reinterpret_cast<vec4*>(p) = v;
}

// What a wave knows about its step: element `ebase` of the buffer is
// row `row`, column `col`; the step's first slot starts at element
// `e_first` (negative in the first slot of a dst that is not 16 B
// aligned, and then ebase is 0).
struct Step {
  int64_t e_first;
  uint64_t ebase;
  uint64_t row;
  uint32_t col;
};

// The lane's slot of a step, whatever it holds.
template <int S, int D, bool SIGNED>
__device__ __forceinline__ void slot_per_lane(
    const Step& st, uint32_t lane, const uint8_t* __restrict__ src,
    const int64_t* __restrict__ src_off, const int64_t* __restrict__ counts,
    uint8_t* __restrict__ dst, uint64_t n_elems, uint32_t T, uint32_t pad_lo,
    uint32_t pad_hi) {
  constexpr int EPS = kSlot / D;
  constexpr int C = EPS * S;
  const int64_t e0 = st.e_first + static_cast<int64_t>(lane) * EPS;
  if (e0 >= static_cast<int64_t>(n_elems)) return;  // behind the last slot
  if (e0 >= 0 && e0 + EPS <= static_cast<int64_t>(n_elems)) {
    // a whole slot: one uint4 store
    const uint32_t d =
        st.col + static_cast<uint32_t>(static_cast<uint64_t>(e0) - st.ebase);
    const uint32_t q = d / T;
    uint64_t r = st.row + q;
    uint32_t c = d - q * T;
    uint32_t cnt = static_cast<uint32_t>(counts[r]);
    const uint8_t* from = src + src_off[r];
    uint32_t o[4];
    if (c + EPS <= cnt) {  // cnt <= T: one row, all of it data
      const uint8_t* p = from + static_cast<uint64_t>(c) * S;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      load_chunk<C, S>(
          p, static_cast<uint32_t>(reinterpret_cast<uint64_t>(p)), w);
      widen_chunk<S, D, SIGNED>(w, o);
    } else {
#pragma unroll
      for (int j = 0; j < EPS; ++j) {
        if (c == T) {  // the next row (c < T on entry)
          c = 0;
          ++r;
          cnt = static_cast<uint32_t>(counts[r]);
          from = src + src_off[r];
        }
        uint32_t lo = pad_lo, hi = pad_hi;
        if (c < cnt) {
          lo = load_elem<S, SIGNED>(from + static_cast<uint64_t>(c) * S);
          hi = high_of<SIGNED>(lo);
        }
        put<D>(o, j, lo, hi);
        ++c;
      }
    }
    store16(dst + e0 * D, o);
    return;
  }
  // a partial slot (the first or the last of the buffer): the elements
  // that exist, one store each
  for (int j = 0; j < EPS; ++j) {
    const int64_t e = e0 + j;
    if (e < 0 || e >= static_cast<int64_t>(n_elems)) continue;
    const uint32_t d =
        st.col + static_cast<uint32_t>(static_cast<uint64_t>(e) - st.ebase);
    const uint32_t q = d / T;
    const uint64_t r = st.row + q;
    const uint32_t c = d - q * T;
    uint32_t lo = pad_lo, hi = pad_hi;
    if (c < static_cast<uint32_t>(counts[r])) {
      lo = load_elem<S, SIGNED>(src + src_off[r] +
                                static_cast<uint64_t>(c) * S);
      hi = high_of<SIGNED>(lo);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + e * D);
    out[0] = lo;
    if constexpr (D == 8) out[1] = hi;
  }
}

// Resources on gfx950 (kernel-resource-usage), over the nine
// instantiations: at most 28 VGPRs and 51 SGPRs, no scratch, no LDS,
// occupancy 8 waves per SIMD, so the 2048 workgroups of a full grid are
// all resident at once (8 per CU).
template <int S, int D, bool SIGNED>
__global__ __launch_bounds__(kThreads) void gather_widen_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
    const int64_t* __restrict__ counts, uint8_t* __restrict__ dst, uint32_t n,
    uint32_t T, uint32_t pad_lo, uint32_t pad_hi) {
  constexpr uint32_t EPS = kSlot / D;
  constexpr uint32_t C = EPS * S;
  constexpr uint32_t kStepElems = SY_WAVE * EPS;
  const uint32_t lane = threadIdx.x % SY_WAVE;
  // the wave id in an SGPR, so that all that follows from it is scalar
  const uint32_t wave = __builtin_amdgcn_readfirstlane(
      blockIdx.x * kWavesPerGroup + threadIdx.x / SY_WAVE);
  const uint64_t db = reinterpret_cast<uint64_t>(dst);
  const uint32_t lead_bytes = static_cast<uint32_t>(db) & (kSlot - 1);
  const uint64_t n_elems = static_cast<uint64_t>(n) * T;
  const uint64_t n_slots = (lead_bytes + n_elems * D + kSlot - 1) / kSlot;
  const uint64_t n_steps = (n_slots + SY_WAVE - 1) / SY_WAVE;
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerGroup;
  const uint64_t per_wave = (n_steps + n_waves - 1) / n_waves;
  uint64_t step = wave * per_wave;
  const uint64_t step_end =
      step + per_wave < n_steps ? step + per_wave : n_steps;
  if (step >= step_end) return;

  Step st;
  st.e_first = static_cast<int64_t>(step * kStepElems) -
               static_cast<int64_t>(lead_bytes / D);
  st.ebase = st.e_first < 0 ? 0 : static_cast<uint64_t>(st.e_first);
  st.row = st.ebase / T;  // ebase < n_elems: the step has a slot
  st.col = static_cast<uint32_t>(st.ebase - st.row * T);
  const uint32_t pad[4] = {pad_lo, D == 4 ? pad_lo : pad_hi, pad_lo,
                           D == 4 ? pad_lo : pad_hi};
  const uint64_t sb = reinterpret_cast<uint64_t>(src);

  // the row whose counts / src_off the wave holds (SGPRs): a row of
  // many steps is looked up once
  uint64_t held = ~0ull;
  uint32_t cnt = 0;
  int64_t off = 0;
  while (step < step_end) {
    uint32_t took = 1;  // steps done in this round
    bool lanes = true;
    // a step of whole slots (e_first >= 0 makes ebase == e_first) ...
    if (st.e_first >= 0 &&
        st.ebase + kStepElems <= n_elems &&
        static_cast<uint64_t>(st.col) + kStepElems <= T) {
      // ... that lies inside one row
      if (st.row != held) {
        held = st.row;
        cnt = static_cast<uint32_t>(counts[st.row]);
        off = src_off[st.row];
      }
      uint8_t* to = dst + (st.ebase + lane * EPS) * D;
      if (cnt >= st.col + kStepElems) {
        const uint64_t at = static_cast<uint64_t>(st.col) * S;
        const uint8_t* p = src + off + at + lane * C;
        const uint32_t addr = static_cast<uint32_t>(sb + off + at);
        uint32_t w[4] = {0u, 0u, 0u, 0u}, o[4];
        if (step + 1 < step_end && cnt >= st.col + 2 * kStepElems &&
            st.ebase + 2 * kStepElems <= n_elems) {
          // the next step is all data of this row too (cnt <= T): both
          // steps' loads go out before the first store
          uint32_t w2[4] = {0u, 0u, 0u, 0u}, o2[4];
          load_chunk<C, S>(p, addr, w);
          load_chunk<C, S>(p + SY_WAVE * C, addr, w2);  // 64 * C: same mod C
          widen_chunk<S, D, SIGNED>(w, o);
          widen_chunk<S, D, SIGNED>(w2, o2);
          store16(to, o);
          store16(to + SY_WAVE * kSlot, o2);
          took = 2;
        } else {
          load_chunk<C, S>(p, addr, w);
          widen_chunk<S, D, SIGNED>(w, o);
          store16(to, o);
        }
        lanes = false;
      } else if (cnt <= st.col) {
        store16(to, pad);
        lanes = false;
      }
    }
    if (lanes)
      slot_per_lane<S, D, SIGNED>(st, lane, src, src_off, counts, dst,
                                  n_elems, T, pad_lo, pad_hi);
    // the next round's first element, as row and column
    step += took;
    const int64_t next = st.e_first + took * kStepElems;  // > 0
    uint32_t d = st.col + static_cast<uint32_t>(
                              static_cast<uint64_t>(next) - st.ebase);
    if (d >= T) {
      const uint32_t q = d / T;
      st.row += q;
      d -= q * T;
    }
    st.col = d;
    st.e_first = next;
    st.ebase = static_cast<uint64_t>(next);
  }
}

template <int S, int D, bool SIGNED>
int launch(const void* d_src, const int64_t* d_src_off,
           const int64_t* d_counts, void* d_dst, uint32_t n, uint32_t T,
           int64_t pad, hipStream_t stream) {
  const uint64_t lead = reinterpret_cast<uint64_t>(d_dst) & (kSlot - 1);
  const uint64_t n_slots =
      (lead + static_cast<uint64_t>(n) * T * D + kSlot - 1) / kSlot;
  const uint64_t groups = (n_slots + kThreads - 1) / kThreads;
  const uint64_t bits = static_cast<uint64_t>(pad);
  hipLaunchKernelGGL((gather_widen_kernel<S, D, SIGNED>),
                     dim3(groups < kGrid ? static_cast<uint32_t>(groups)
                                         : kGrid),
                     dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(d_src), d_src_off, d_counts,
                     static_cast<uint8_t*>(d_dst), n, T,
                     static_cast<uint32_t>(bits),
                     static_cast<uint32_t>(bits >> 32));
  return sy_check(hipGetLastError());
}

}  // namespace

// dst[i, :counts[i]] = the counts[i] elements of src_size bytes at
// src + src_off[i], zero-extended or (src_signed) sign-extended to
// dst_size bytes; dst[i, counts[i]:] = pad.  dst is [n, T], its base a
// multiple of dst_size; src's base and every src_off are multiples of
// src_size; 0 <= counts[i] <= T < 2^31 - 256; every row lies inside
// src.  -22 (EINVAL) for sizes outside {1, 2, 4} -> {4, 8}, a signed
// 1-byte source and unsigned 4 -> 4, which loses values.
SY_EXPORT int sy_gather_widen(const void* d_src, const int64_t* d_src_off,
                              const int64_t* d_counts, void* d_dst,
                              uint32_t n, uint32_t T, uint32_t src_size,
                              int src_signed, uint32_t dst_size, int64_t pad,
                              hipStream_t stream) {
  if (dst_size != 4 && dst_size != 8) return -22;
  if (T >= 0x7FFFFF00u) return -22;
  if (n == 0 || T == 0) return 0;
  const bool wide = dst_size == 8;
#define SY_WIDEN(S, SIGNED)                                                  \
  (wide ? launch<S, 8, SIGNED>(d_src, d_src_off, d_counts, d_dst, n, T, pad, \
                               stream)                                       \
        : launch<S, 4, SIGNED>(d_src, d_src_off, d_counts, d_dst, n, T, pad, \
                               stream))
  switch (src_size) {
    case 1:
      return src_signed ? -22 : SY_WIDEN(1, false);
    case 2:
      return src_signed ? SY_WIDEN(2, true) : SY_WIDEN(2, false);
    case 4:
      if (!wide)  // a copy; only the signed reading keeps every value
        return src_signed ? launch<4, 4, false>(d_src, d_src_off, d_counts,
                                                d_dst, n, T, pad, stream)
                          : -22;
      return src_signed ? launch<4, 8, true>(d_src, d_src_off, d_counts,
                                             d_dst, n, T, pad, stream)
                        : launch<4, 8, false>(d_src, d_src_off, d_counts,
                                              d_dst, n, T, pad, stream);
    default:
      return -22;
  }
#undef SY_WIDEN
}
