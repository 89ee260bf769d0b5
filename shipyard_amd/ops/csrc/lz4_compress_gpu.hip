// GPU LZ4 block compressor for MI355X (gfx950).
//
// SYSHARD authoring on the GPU: the CPU matcher
// (lz4_compress.cpp, 262 MB/s on 8 cores) becomes one wave per block
// with the SAME greedy policy — 12-bit hash table, insert-per-scan,
// skip-and-reprime — so the emitted stream is BYTE-IDENTICAL to the
// CPU compressor's (tested), just authored at GPU rate.  Parallelism
// follows the decoder's occupancy law: many independent blocks, one
// serial match loop per wave, with the wave's 64 lanes used for the
// two data-parallel pieces (match extension compare via ballot,
// literal/stream copies).
//
// Memory layout (measured in this order): a global-src draft put 4
// serial BYTE loads per scanned position on the match-loop chain
// (13-21 GB/s); staging the source block into LDS and reading
// unaligned 32-bit words as two aligned ds_read_b32 + v_alignbit cut
// the per-position chain to ~1 LDS round trip.  The emitted stream
// goes STRAIGHT to global — append-only, never re-read, fire-and-
// forget writes off the serial chain.  LDS = RAWCAP src + 8 KiB
// table.
//
// Output: slotted buffer (blk * stride) + out_lens[blk] = compressed
// size, or 0 when not smaller than raw (caller stores the block raw —
// same contract as the CPU entry point).
//
// Two kernels, the serial greedy matcher (lz4_compress_kernel) and the
// wave-screen matcher (lz4_compress_screen_kernel), share the staging,
// table clear, unaligned read and match extension below and the host
// dispatch; each keeps its matcher loop and its own copy of the emit
// lambdas (see the note there).

#include "common.h"

namespace {

constexpr uint32_t kHashSlots = 4096;

__device__ __forceinline__ uint32_t hash4(uint32_t v) {
  return (v * 2654435761u) >> 20;  // 12-bit table
}

// unaligned 32-bit read from the LDS copy: two aligned words +
// funnel shift (v_alignbit) — ONE LDS round trip on the chain
// instead of four serial byte loads
__device__ __forceinline__ uint32_t lds_rd32(const uint8_t* sbuf,
                                             uint32_t off) {
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(sbuf);
  const uint32_t lo = sw[off >> 2], hi = sw[(off >> 2) + 1];
  const uint32_t sh = (off & 3u) * 8u;
  return sh ? ((lo >> sh) | (hi << (32u - sh))) : lo;
}

// stage the source block into LDS (coalesced 16 B/lane).  The uint4
// loads need data + in_off 16-byte aligned: the wrapper passes an
// aligned base and in_off = blk * block_raw, and rejects a block_raw
// that is not a positive multiple of 16; a caller of the C entry
// points owes the same.  The ragged tail copies bytewise so the last
// block never reads past the input tensor.
__device__ __forceinline__ void stage_block(uint8_t* sbuf,
                                            const uint8_t* gsrc, uint32_t n,
                                            int lane) {
  const uint4* g4 = reinterpret_cast<const uint4*>(gsrc);
  uint4* s4 = reinterpret_cast<uint4*>(sbuf);
  const uint32_t nfull = n >> 4;
  for (uint32_t i = lane; i < nfull; i += SY_WAVE) s4[i] = g4[i];
  for (uint32_t i = (nfull << 4) + lane; i < n; i += SY_WAVE)
    sbuf[i] = gsrc[i];
}

// clear the hash table (64 lanes x 64 entries); T is uint16_t in the
// serial matcher, uint32_t (for atomicMax) in the screen matcher
template <class T>
__device__ __forceinline__ void clear_table(T* ht, int lane) {
  for (uint32_t i = lane; i < kHashSlots; i += SY_WAVE) ht[i] = 0;
}

// wave-parallel match extension: 64 B compared per ballot round.
// The 4-byte match at src[r] / src[pos] is already known; returns the
// full match length, which stops short of match_limit.
__device__ __forceinline__ uint32_t extend_match(const uint8_t* src,
                                                 uint32_t r, uint32_t pos,
                                                 uint32_t match_limit,
                                                 int lane) {
  uint32_t mlen = 4;
  for (;;) {
    const uint32_t i = mlen + (uint32_t)lane;
    const bool ok = (pos + i < match_limit) && src[r + i] == src[pos + i];
    const uint64_t mask = __ballot(ok);
    const uint32_t run =
        (~mask == 0ull) ? 64u : (uint32_t)(__ffsll((long long)~mask) - 1);
    mlen += run;
    if (run < 64u) break;
  }
  return mlen;
}

// Serial greedy matcher: the CPU policy exactly, one scanned position
// per LDS round trip.
template <int RAWCAP>
__global__ __launch_bounds__(SY_WAVE) void lz4_compress_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ in_off,
    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
    uint64_t stride, uint32_t* __restrict__ out_lens, uint32_t n_blocks) {
  __shared__ uint16_t ht[kHashSlots];
  __shared__ uint8_t sbuf[RAWCAP + 16];

  const int lane = threadIdx.x;
  const uint8_t* src = sbuf;

  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const uint32_t n = in_len[blk];
    if (n > (uint32_t)RAWCAP) {  // host routes by raw_cap; belt+braces
      if (lane == 0) out_lens[blk] = 0;
      continue;
    }
    stage_block(sbuf, data + in_off[blk], n, lane);
    clear_table(ht, lane);
    __builtin_amdgcn_s_waitcnt(0);

    uint32_t opos = 0;
    bool fail = false;
    uint8_t* dstbuf = out + (uint64_t)blk * stride;
    const uint32_t cap = n;  // emit caps at raw size (else stored)

    // emit helpers run in UNIFORM control flow (every lane computes
    // the same scalar state; same-address same-value LDS writes are
    // benign, but we predicate on lane 0 to keep LDS traffic down).
    // They stay lambdas over kernel locals, one copy per kernel: as
    // methods of a shared struct the compiler keeps opos/fail in
    // vector registers and the 8 KiB and 64 KiB rows measured slower.
    auto emit_byte = [&](uint8_t b) {
      if (opos >= cap) { fail = true; return; }
      if (lane == 0) dstbuf[opos] = b;
      ++opos;
    };
    auto emit_len = [&](uint32_t len) {
      while (len >= 255 && !fail) {
        emit_byte(255);
        len -= 255;
      }
      if (!fail) emit_byte((uint8_t)len);
    };
    auto emit_literals = [&](uint32_t anchor, uint32_t litlen) {
      if (opos + litlen > cap) { fail = true; return; }
      for (uint32_t i = lane; i < litlen; i += SY_WAVE) {
        dstbuf[opos + i] = src[anchor + i];
      }
      opos += litlen;
    };
    auto emit_seq = [&](uint32_t anchor, uint32_t lit_end,
                        uint32_t offset, uint32_t mlen) {
      const uint32_t litlen = lit_end - anchor;
      const uint32_t ml = mlen ? mlen - 4 : 0;
      emit_byte((uint8_t)(((litlen < 15 ? litlen : 15) << 4) |
                          (ml < 15 ? ml : 15)));
      if (!fail && litlen >= 15) emit_len(litlen - 15);
      if (!fail) emit_literals(anchor, litlen);
      if (fail || mlen == 0) return;
      emit_byte((uint8_t)(offset & 0xFF));
      emit_byte((uint8_t)(offset >> 8));
      if (!fail && ml >= 15) emit_len(ml - 15);
    };
    if (n >= 13) {
      const uint32_t mflimit = n - 12;
      const uint32_t match_limit = n - 5;
      uint32_t anchor = 0, pos = 0;
      while (pos <= mflimit && !fail) {
        const uint32_t h = hash4(lds_rd32(sbuf, pos));
        const uint32_t ref = (uint32_t)ht[h];  // pos+1 encoding
        ht[h] = (uint16_t)(pos + 1);
        if (ref != 0 && ref - 1 < pos && pos - (ref - 1) <= 65535 &&
            lds_rd32(sbuf, ref - 1) == lds_rd32(sbuf, pos)) {
          const uint32_t r = ref - 1;
          const uint32_t mlen = extend_match(src, r, pos, match_limit, lane);
          emit_seq(anchor, pos, pos - r, mlen);
          pos += mlen;
          anchor = pos;
          // re-prime inside the skipped span (matches CPU matcher)
          if (pos <= mflimit)
            ht[hash4(lds_rd32(sbuf, pos - 2))] = (uint16_t)(pos - 1);
        } else {
          ++pos;
        }
      }
      if (!fail) emit_seq(anchor, n, 0, 0);
    } else {
      emit_seq(0, n, 0, 0);
    }

    const uint32_t clen = (!fail && opos < n) ? opos : 0;
    if (lane == 0) out_lens[blk] = clen;
    __builtin_amdgcn_s_waitcnt(0);
  }
}

// ---------------------------------------------------------------------
// v2 "wave-screen" matcher: instead of one serial LDS round trip per
// scanned position, the wave screens 64 positions at once — parallel
// rd32 + hash + table gather, ballot for the first candidate — then
// inserts the scanned span with ds atomicMax (deterministic: max ==
// most-recent position regardless of write order).  Match extension
// and emission are the shared wave code above.  Semantics: a valid
// greedy-LZ4 stream, but NOT byte-identical to v1 — candidates whose
// source lies inside the current 64-position batch are invisible
// (their inserts land after the screen), so some short-range matches
// shift by a batch.  The stream is deterministic all the same: tests
// compare it byte for byte with a Python model of this policy
// (tests/lz4_match_model.py), as they do the serial matcher's.
// ---------------------------------------------------------------------
template <int RAWCAP>
__global__ __launch_bounds__(SY_WAVE) void lz4_compress_screen_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ in_off,
    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
    uint64_t stride, uint32_t* __restrict__ out_lens, uint32_t n_blocks) {
  __shared__ uint32_t ht[kHashSlots];  // u32 for atomicMax
  __shared__ uint8_t sbuf[RAWCAP + 16];

  const int lane = threadIdx.x;
  const uint8_t* src = sbuf;

  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const uint32_t n = in_len[blk];
    if (n > (uint32_t)RAWCAP) {  // host routes by raw_cap; belt+braces
      if (lane == 0) out_lens[blk] = 0;
      continue;
    }
    stage_block(sbuf, data + in_off[blk], n, lane);
    clear_table(ht, lane);
    __builtin_amdgcn_s_waitcnt(0);

    uint32_t opos = 0;
    bool fail = false;
    uint8_t* dstbuf = out + (uint64_t)blk * stride;
    const uint32_t cap = n;  // emit caps at raw size (else stored)

    // emit helpers run in UNIFORM control flow (every lane computes
    // the same scalar state; same-address same-value LDS writes are
    // benign, but we predicate on lane 0 to keep LDS traffic down).
    // They stay lambdas over kernel locals, one copy per kernel: as
    // methods of a shared struct the compiler keeps opos/fail in
    // vector registers and the 8 KiB and 64 KiB rows measured slower.
    auto emit_byte = [&](uint8_t b) {
      if (opos >= cap) { fail = true; return; }
      if (lane == 0) dstbuf[opos] = b;
      ++opos;
    };
    auto emit_len = [&](uint32_t len) {
      while (len >= 255 && !fail) {
        emit_byte(255);
        len -= 255;
      }
      if (!fail) emit_byte((uint8_t)len);
    };
    auto emit_literals = [&](uint32_t anchor, uint32_t litlen) {
      if (opos + litlen > cap) { fail = true; return; }
      for (uint32_t i = lane; i < litlen; i += SY_WAVE) {
        dstbuf[opos + i] = src[anchor + i];
      }
      opos += litlen;
    };
    auto emit_seq = [&](uint32_t anchor, uint32_t lit_end,
                        uint32_t offset, uint32_t mlen) {
      const uint32_t litlen = lit_end - anchor;
      const uint32_t ml = mlen ? mlen - 4 : 0;
      emit_byte((uint8_t)(((litlen < 15 ? litlen : 15) << 4) |
                          (ml < 15 ? ml : 15)));
      if (!fail && litlen >= 15) emit_len(litlen - 15);
      if (!fail) emit_literals(anchor, litlen);
      if (fail || mlen == 0) return;
      emit_byte((uint8_t)(offset & 0xFF));
      emit_byte((uint8_t)(offset >> 8));
      if (!fail && ml >= 15) emit_len(ml - 15);
    };
    if (n >= 13) {
      const uint32_t mflimit = n - 12;
      const uint32_t match_limit = n - 5;
      uint32_t anchor = 0, pos = 0;
      while (pos <= mflimit && !fail) {
        // ---- screen 64 positions in one parallel round trip ----
        const uint32_t p = pos + (uint32_t)lane;
        const bool in_range = p <= mflimit;
        uint32_t v = 0, h = 0, ref = 0;
        bool cand = false;
        if (in_range) {
          v = lds_rd32(sbuf, p);
          h = hash4(v);
          ref = ht[h];
          cand = ref != 0 && ref - 1 < p && lds_rd32(sbuf, ref - 1) == v;
        }
        const uint64_t mask = __ballot(cand);
        const uint32_t j = mask ? (uint32_t)(__ffsll((long long)mask)
                                             - 1) : 64u;
        // insert the scanned span (positions pos..pos+min(j,63)):
        // atomicMax == latest position wins, order-independent
        if (in_range && (uint32_t)lane <= j) {
          atomicMax(&ht[h], p + 1);
        }
        if (!mask) {
          pos += SY_WAVE;
          continue;
        }
        const uint32_t pstar = pos + j;
        const uint32_t rstar = __shfl(ref, (int)j) - 1;
        const uint32_t mlen =
            extend_match(src, rstar, pstar, match_limit, lane);
        emit_seq(anchor, pstar, pstar - rstar, mlen);
        pos = pstar + mlen;
        anchor = pos;
        if (pos <= mflimit) {  // reprime like the serial matcher
          atomicMax(&ht[hash4(lds_rd32(sbuf, pos - 2))], pos - 1);
        }
      }
      if (!fail) emit_seq(anchor, n, 0, 0);
    } else {
      emit_seq(0, n, 0, 0);
    }

    const uint32_t clen = (!fail && opos < n) ? opos : 0;
    if (lane == 0) out_lens[blk] = clen;
    __builtin_amdgcn_s_waitcnt(0);
  }
}

// Kernel families for the shared host entry: rung -> instantiation.
struct SerialMatcher {
  template <int CAP>
  static auto kernel() { return lz4_compress_kernel<CAP>; }
};
struct ScreenMatcher {
  template <int CAP>
  static auto kernel() { return lz4_compress_screen_kernel<CAP>; }
};

template <class Family>
int compress_blocks(const void* d_data, const uint64_t* d_in_off,
                    const uint32_t* d_in_len, void* d_out, uint64_t stride,
                    uint32_t* d_out_lens, uint32_t n_blocks,
                    uint32_t raw_cap, hipStream_t stream) {
  // nothing to compress: success without a launch, whatever raw_cap is
  if (n_blocks == 0) return 0;
  const uint32_t grid = n_blocks < (1u << 20) ? n_blocks : (1u << 20);
  // raw_cap > 64 KiB is -22: the serial matcher's table holds u16
  // positions, and neither family has a larger rung.
  return sy_dispatch_rung<4 * 1024, 8 * 1024, 16 * 1024, 32 * 1024,
                          64 * 1024>(raw_cap, [&](auto cap) {
    hipLaunchKernelGGL(Family::template kernel<decltype(cap)::value>(),
                       dim3(grid), dim3(SY_WAVE), 0, stream,
                       static_cast<const uint8_t*>(d_data), d_in_off,
                       d_in_len, static_cast<uint8_t*>(d_out), stride,
                       d_out_lens, n_blocks);
    return sy_check(hipGetLastError());
  });
}

}  // namespace

SY_EXPORT int sy_lz4_compress_blocks_gpu(
    const void* d_data, const uint64_t* d_in_off, const uint32_t* d_in_len,
    void* d_out, uint64_t stride, uint32_t* d_out_lens, uint32_t n_blocks,
    uint32_t raw_cap, hipStream_t stream) {
  return compress_blocks<SerialMatcher>(d_data, d_in_off, d_in_len, d_out,
                                        stride, d_out_lens, n_blocks,
                                        raw_cap, stream);
}

SY_EXPORT int sy_lz4_compress_blocks_gpu2(
    const void* d_data, const uint64_t* d_in_off, const uint32_t* d_in_len,
    void* d_out, uint64_t stride, uint32_t* d_out_lens, uint32_t n_blocks,
    uint32_t raw_cap, hipStream_t stream) {
  return compress_blocks<ScreenMatcher>(d_data, d_in_off, d_in_len, d_out,
                                        stride, d_out_lens, n_blocks,
                                        raw_cap, stream);
}
