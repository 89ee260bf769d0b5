// Ragged range gather for random-access SYSHARD reads (gfx950).
//
// A range read decodes the blocks that cover the requested byte ranges
// into a scratch buffer and then has to cut the ranges out of it: range
// i is len[i] bytes at src + src_off[i] and goes to dst + dst_off[i].  A
// sample starts and ends at any byte and lands in a packed batch at any
// byte, so neither side is 16 B aligned and the two sides are not
// aligned to each other; gather_copy.hip, which casts both sides to
// uint4 and gives every block a workgroup, cannot do it.  This kernel
// takes any alignment, any length (0 included), ranges in any order and
// source ranges that overlap or repeat.  Destination ranges must not
// overlap each other and dst must not overlap src (the caller's
// promise; nothing here checks it).  (Reference analogue: none.)
//
// Geometry.  All alignment is taken on absolute addresses, so the
// tensors' own base pointers may be misaligned too.  For range i let
// D0 = dst + dst_off[i], D1 = D0 + len[i], S0 = src + src_off[i] and
// A0 = D0 rounded down to 16.  The range is cut into PIECES: piece k is
// the destination window [A0 + k*4096, A0 + (k+1)*4096) clipped to
// [D0, D1).  A window is 256 SLOTS of 16 B, each 16 B aligned in dst.
// One WAVE copies one piece in up to four steps of 64 slots (1 KiB),
// lane l on slot 64*u + l, all loads of the piece issued before its
// first store and with no branch between them (a lane whose slot does
// not move as a uint4 loads a slot that does and drops the result; a
// branch around each load would make the compiler wait for one load
// before it issues the next).
//
//   * A slot that lies wholly inside [D0, D1) is one uint4 store.
//   * Its 16 source bytes start at A + (S0 - D0), which is
//     m = (S0 - D0) mod 16 bytes past a 16 B boundary, the same m for
//     every slot of the range.  m == 0 (equal misalignment on both
//     sides): one aligned uint4 load, a straight copy.  Otherwise: the
//     two aligned uint4 loads that cover the bytes, and the 16 bytes
//     are cut out of those 8 dwords in registers, dword k of the result
//     being v_alignbyte(w[k+q+1], w[k+q], m%4) with q = m/4.  m is
//     uniform over the wave, so q selects one of four compile-time
//     register patterns by a scalar branch; nothing is indexed at run
//     time.
//   * The first and last slot of a range (where [D0, D1) covers only
//     part of the 16 B) are written byte by byte, each byte predicated
//     on D0 <= address < D1 and loaded from exactly its source byte.
//   * An aligned source load may reach up to 15 bytes in front of S0 or
//     31 bytes past the slot's last source byte.  Inside the tensor
//     that is harmless, but the first and last range of src must not
//     make it leave [src, src + src_bytes): a slot whose aligned loads
//     do not lie wholly inside the tensor takes the byte path as well.
//
// Why the source is the re-aligned side: a store that is not 16 B
// aligned, or narrower than 16 B, makes the memory system merge partial
// lines, while a load that is shifted against its consumer only has to
// be fetched as the two aligned neighbours, which hit the same or the
// next cache line that the adjacent lane fetches anyway.  The second
// load costs L1 bandwidth, not HBM traffic.  So the stores are the
// aligned, full-width side and the shift is paid in a few VALU
// instructions per 16 B (4 v_alignbyte_b32).
//
// Work split: by bytes, not by range.  sy_gather_range_pieces writes
// the piece count of every range (0 for an empty one); the caller turns
// it into an inclusive prefix sum `cum` on the device (torch.cumsum).
// The gather kernel is launched with a fixed grid of kGrid workgroups
// of 4 waves; it reads the piece total cum[n-1] on the device (no host
// sync), and wave w takes the contiguous run of ceil(total / n_waves)
// pieces that starts at w times that number.  It finds the range of its
// first piece with one binary search in `cum` and then walks forward: a
// piece after the last one of its range belongs to the next range that
// has pieces.  So a single 256 MiB range (65536 pieces) spreads over
// every wave of the chip, and 100k ranges of 200 bytes cost one wave
// step each, several thousand waves wide, and not a workgroup each.
// Everything that picks the piece (wave id, range, offsets, m) is
// wave-uniform and lives in SGPRs; `cum` and the three offset arrays
// are read with scalar loads.
//
// No LDS, no barrier, no communication between waves.  Resources
// (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see the note
// at gather_ranges_kernel.

#include "common.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWavesPerGroup = kThreads / SY_WAVE;
constexpr uint32_t kSlot = 16;                       // bytes per store
constexpr uint32_t kStepBytes = SY_WAVE * kSlot;     // 1 KiB: a wave's store
constexpr uint32_t kSteps = 4;                       // loads in flight
constexpr uint32_t kPieceBytes = kSteps * kStepBytes;  // 4 KiB
// 8 workgroups of 4 waves on each of the 256 CUs: a full chip of
// resident waves for a large gather, and a launch of mostly empty
// workgroups (they read cum[n-1] and leave) for a small one
constexpr uint32_t kGrid = 2048;

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));

// The kernel computes with absolute addresses (alignment is a property
// of the address, not of an offset into a tensor).  A pointer made from
// an integer would be a generic one and cost flat_* instructions; these
// say that it is global memory.  `base` is wave-uniform (an SGPR pair)
// and `off` the lane's 32-bit offset, the addressing form that needs
// one VGPR per access.
#define SY_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ vec4 load16(uint64_t base, uint32_t off) {
  return *reinterpret_cast<const SY_GLOBAL vec4*>(
      reinterpret_cast<const SY_GLOBAL uint8_t*>(base) + off);
}
__device__ __forceinline__ void store16(uint64_t base, uint32_t off,
                                        const vec4 v) {
  *reinterpret_cast<SY_GLOBAL vec4*>(
      reinterpret_cast<SY_GLOBAL uint8_t*>(base) + off) = v;
}
__device__ __forceinline__ void copy_byte(uint64_t to, uint64_t from,
                                          uint32_t off) {
  reinterpret_cast<SY_GLOBAL uint8_t*>(to)[off] =
      reinterpret_cast<const SY_GLOBAL uint8_t*>(from)[off];
}

// pieces of one range whose destination starts at absolute address d0
__device__ __forceinline__ uint64_t piece_count(uint64_t d0, int64_t len) {
  if (len <= 0) return 0;
  return ((d0 & (kSlot - 1)) + static_cast<uint64_t>(len) + kPieceBytes - 1) /
         kPieceBytes;
}

__global__ __launch_bounds__(kThreads) void gather_range_pieces_kernel(
    const uint8_t* dst, const int64_t* __restrict__ dst_off,
    const int64_t* __restrict__ lens, int64_t* __restrict__ pieces,
    uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t d0 = reinterpret_cast<uint64_t>(dst) +
                      static_cast<uint64_t>(dst_off[i]);
  pieces[i] = static_cast<int64_t>(piece_count(d0, lens[i]));
}

// the 16 bytes that start Q*4 + r bytes into the 32 bytes {lo, hi}
template <int Q>
__device__ __forceinline__ vec4 realign(const vec4 lo, const vec4 hi,
                                        uint32_t r) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  vec4 o;
  o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q + 0], r);
  o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r);
  o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r);
  o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r);
  return o;
}

// min(max(x, 0), cap) of a difference of addresses taken as signed
__device__ __forceinline__ uint32_t clamp_off(uint64_t x, uint32_t cap) {
  const int64_t v = static_cast<int64_t>(x);
  return v < 0 ? 0u : v > static_cast<int64_t>(cap) ? cap
                                                    : static_cast<uint32_t>(v);
}

// Wave-uniform description of one piece: the window [win, win + 4 KiB)
// of dst and what of it moves how.  A slot is named by its offset o in
// the window.
struct Piece {
  uint64_t win;   // destination window, 16 B aligned
  uint64_t swin;  // slot o loads from swin + o (16 B aligned)
  uint64_t from;  // byte x of the window comes from from + x
  uint32_t r_lo, r_hi;  // the range inside the window: bytes [r_lo, r_hi)
  uint32_t v_lo, v_hi;  // slot o moves as one uint4 iff
                        // v_lo <= o && o + 16 <= v_hi
};

// d0/d1: the range in dst; delta = S0 - D0 (mod 2^64), m = delta % 16;
// [sb, se) the source tensor; load_bytes: 16 for m == 0, else 32.
__device__ __forceinline__ Piece make_piece(uint64_t win, uint64_t d0,
                                            uint64_t d1, uint64_t delta,
                                            uint32_t m, uint64_t sb,
                                            uint64_t se,
                                            uint32_t load_bytes) {
  Piece pc;
  pc.win = win;
  pc.swin = win + delta - m;
  pc.from = win + delta;
  pc.r_lo = clamp_off(d0 - win, kPieceBytes);
  pc.r_hi = clamp_off(d1 - win, kPieceBytes);
  // the source tensor on the scale of o: loads of slot o cover
  // [o, o + load_bytes) and must lie in [s_lo, s_hi)
  const uint32_t s_lo = clamp_off(sb - pc.swin, kPieceBytes);
  const uint32_t s_hi = clamp_off(se - pc.swin, kPieceBytes + load_bytes);
  const uint32_t over = load_bytes - kSlot;
  const uint32_t s_top = s_hi > over ? s_hi - over : 0u;
  pc.v_lo = pc.r_lo > s_lo ? pc.r_lo : s_lo;
  pc.v_hi = pc.r_hi < s_top ? pc.r_hi : s_top;
  return pc;
}

// The uint4 part of a piece: STEPS steps of 64 slots.  ALIGNED: m == 0;
// Q = m / 4 otherwise, r = m % 4.  The caller guarantees that `safe` is
// a slot that moves as a uint4.  Every lane loads in every step, with
// no branch between the loads, so that all 2 * STEPS of them are in
// flight together: a lane whose slot does not move as a uint4 loads
// slot `safe` instead (in bounds, on a line that another lane fetches
// anyway) and throws the result away.  Only the stores are predicated.
// FULL: every slot of the window moves as a uint4 (each inner piece of
// a long range), nothing is predicated at all.
template <bool ALIGNED, int Q, int STEPS, bool FULL>
__device__ __forceinline__ void copy_slots(const Piece& pc, uint32_t r,
                                           uint32_t safe, uint32_t lane) {
  vec4 lo[STEPS], hi[STEPS];
  bool vec[STEPS];
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {
    const uint32_t o = lane * kSlot + u * kStepBytes;
    vec[u] = FULL || (o >= pc.v_lo && o + kSlot <= pc.v_hi);
    const uint32_t ol = vec[u] ? o : safe;
    lo[u] = load16(pc.swin, ol);
    if constexpr (!ALIGNED) hi[u] = load16(pc.swin, ol + kSlot);
  }
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {
    const uint32_t o = lane * kSlot + u * kStepBytes;
    vec4 v;
    if constexpr (ALIGNED)
      v = lo[u];
    else
      v = realign<Q>(lo[u], hi[u], r);
    if (vec[u]) store16(pc.win, o, v);
  }
}

template <bool ALIGNED, int Q>
__device__ __forceinline__ void copy_piece(uint64_t win, uint64_t d0,
                                           uint64_t d1, uint64_t delta,
                                           uint32_t m, uint64_t sb,
                                           uint64_t se, uint32_t lane) {
  const Piece pc =
      make_piece(win, d0, d1, delta, m, sb, se, ALIGNED ? kSlot : 2 * kSlot);
  // first slot that moves as a uint4, if there is one
  const uint32_t safe = (pc.v_lo + kSlot - 1) & ~(kSlot - 1);
  if (safe + kSlot <= pc.v_hi) {
    if (pc.v_lo == 0 && pc.v_hi == kPieceBytes) {
      copy_slots<ALIGNED, Q, kSteps, true>(pc, m & 3u, safe, lane);
      return;  // and no byte is left
    }
    // a short range (or the end of a long one) takes one step
    if (pc.v_hi <= kStepBytes)
      copy_slots<ALIGNED, Q, 1, false>(pc, m & 3u, safe, lane);
    else
      copy_slots<ALIGNED, Q, kSteps, false>(pc, m & 3u, safe, lane);
  }
  // What is left: the head and tail slots of the range, and slots whose
  // aligned loads would leave the source tensor.  Byte by byte, inside
  // [r_lo, r_hi) only, each byte from exactly its source byte.  At most
  // a few slots of a range; the wave skips the loop when the uint4
  // slots covered all of the range that is in the window, and the loop
  // is kept rolled up so that it costs the bulk path no registers.
  if (pc.v_lo == 0 && pc.v_hi == pc.r_hi && pc.r_hi % kSlot == 0) return;
#pragma unroll 1
  for (uint32_t o = lane * kSlot; o < pc.r_hi; o += kStepBytes) {
    if (o >= pc.v_lo && o + kSlot <= pc.v_hi) continue;
#pragma unroll 1
    for (uint32_t x = o; x < o + kSlot; ++x)
      if (x >= pc.r_lo && x < pc.r_hi) copy_byte(pc.win, pc.from, x);
  }
}

// smallest r with cum[r] > p; the caller guarantees p < cum[n-1]
__device__ __forceinline__ uint32_t range_of_piece(
    const int64_t* __restrict__ cum, uint32_t n, uint64_t p) {
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (static_cast<uint64_t>(cum[mid]) > p)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// Resources on gfx950 (kernel-resource-usage): 58 VGPRs, 80 SGPRs, no
// scratch, no LDS, occupancy 8 waves per SIMD, so the 2048 workgroups
// of the grid are all resident at once (8 per CU).
__global__ __launch_bounds__(kThreads) void gather_ranges_kernel(
    const uint8_t* src, uint64_t src_bytes,
    const int64_t* __restrict__ src_off, const int64_t* __restrict__ lens,
    uint8_t* dst, const int64_t* __restrict__ dst_off,
    const int64_t* __restrict__ cum, uint32_t n) {
  const uint32_t lane = threadIdx.x % SY_WAVE;
  // the wave id in an SGPR, so that all that follows from it is scalar
  const uint32_t wave = __builtin_amdgcn_readfirstlane(
      blockIdx.x * kWavesPerGroup + threadIdx.x / SY_WAVE);
  const uint64_t total = static_cast<uint64_t>(cum[n - 1]);
  const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kWavesPerGroup;
  const uint64_t per_wave = (total + n_waves - 1) / n_waves;
  uint64_t p = wave * per_wave;
  const uint64_t p_end = p + per_wave < total ? p + per_wave : total;
  if (p >= p_end) return;

  const uint64_t sb = reinterpret_cast<uint64_t>(src);
  const uint64_t se = sb + src_bytes;
  uint32_t r = range_of_piece(cum, n, p);
  while (true) {
    // pieces [first, last) belong to range r, and first <= p < last
    const uint64_t first = r ? static_cast<uint64_t>(cum[r - 1]) : 0;
    const uint64_t last = static_cast<uint64_t>(cum[r]);
    const uint64_t stop = last < p_end ? last : p_end;
    const uint64_t d0 = reinterpret_cast<uint64_t>(dst) +
                        static_cast<uint64_t>(dst_off[r]);
    const uint64_t d1 = d0 + static_cast<uint64_t>(lens[r]);
    const uint64_t delta =
        sb + static_cast<uint64_t>(src_off[r]) - d0;
    const uint32_t m = static_cast<uint32_t>(delta) & (kSlot - 1);
    const uint64_t a0 = d0 & ~static_cast<uint64_t>(kSlot - 1);
    for (; p < stop; ++p) {
      const uint64_t win = a0 + (p - first) * kPieceBytes;
      if (m == 0) {
        copy_piece<true, 0>(win, d0, d1, delta, m, sb, se, lane);
      } else {
        switch (m >> 2) {  // wave-uniform
          case 0:
            copy_piece<false, 0>(win, d0, d1, delta, m, sb, se, lane);
            break;
          case 1:
            copy_piece<false, 1>(win, d0, d1, delta, m, sb, se, lane);
            break;
          case 2:
            copy_piece<false, 2>(win, d0, d1, delta, m, sb, se, lane);
            break;
          default:
            copy_piece<false, 3>(win, d0, d1, delta, m, sb, se, lane);
            break;
        }
      }
    }
    if (p >= p_end) return;
    // p == cum[r]: the next range that has pieces; after a run of empty
    // ranges, search instead of walking them one by one
    ++r;
    if (static_cast<uint64_t>(cum[r]) == p) r = range_of_piece(cum, n, p);
  }
}

}  // namespace

// d_pieces[i] = number of 4 KiB destination pieces of range i (0 for
// len <= 0).  The caller's inclusive prefix sum of it is sy_gather_ranges'
// d_cum.
SY_EXPORT int sy_gather_range_pieces(const void* d_dst,
                                     const int64_t* d_dst_off,
                                     const int64_t* d_lens, int64_t* d_pieces,
                                     uint32_t n, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(gather_range_pieces_kernel,
                     dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, static_cast<const uint8_t*>(d_dst), d_dst_off,
                     d_lens, d_pieces, n);
  return sy_check(hipGetLastError());
}

// dst[dst_off[i] .. +lens[i]) = src[src_off[i] .. +lens[i]) for i < n.
// src_bytes is the size of the source tensor: no load leaves
// [d_src, d_src + src_bytes).  Every range must lie inside its tensor.
SY_EXPORT int sy_gather_ranges(const void* d_src, uint64_t src_bytes,
                               const int64_t* d_src_off,
                               const int64_t* d_lens, void* d_dst,
                               const int64_t* d_dst_off, const int64_t* d_cum,
                               uint32_t n, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(gather_ranges_kernel, dim3(kGrid), dim3(kThreads), 0,
                     stream, static_cast<const uint8_t*>(d_src), src_bytes,
                     d_src_off, d_lens, static_cast<uint8_t*>(d_dst),
                     d_dst_off, d_cum, n);
  return sy_check(hipGetLastError());
}
