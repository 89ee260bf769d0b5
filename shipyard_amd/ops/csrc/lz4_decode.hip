// LZ4 block decompression for MI355X (gfx950) — v3.
//
// Role in the framework: the cascade-analogue image replicator and the
// shard stager store container layers / data shards as sequences of
// independently-compressed LZ4 blocks (raw block format, <= 64 KiB raw
// per block).  The reference delegates layer decompress to dockerd
// (reference cascade/cascade.py:500-571); here decode runs on the GPU so
// a layer goes NVMe -> pinned host -> HBM (hipMemcpyAsync) -> decoded in
// HBM without a CPU inflate pass.
//
// Design history (measured on MI355X):
//   v1: lane-0 parse + ds_bpermute broadcasts      -> 4.7 GB/s
//   v2: uniform-lane parse + register byte window  -> 5.0 GB/s
//   The bound was never the broadcasts: LZ4 decode is a serial
//   dependency chain per block, and every literal-copy global load was
//   a COLD HBM/L2 miss (~600 cycles) sitting on that chain.
//   v3: stage the whole compressed block into LDS up front with one
//   coalesced wave-wide copy (streams at full bandwidth, off the
//   critical path), then parse + copy entirely LDS->LDS (~64-cycle
//   dependent accesses).
//   v4 (round 2, DEFAULT): drop the src staging — parse straight from
//   global.  The stream is read once sequentially so its lines stay
//   L1-hot (v1's cold-miss problem was its RANDOM literal reads, not
//   sequential parse reads), and halving the LDS footprint doubles
//   resident blocks/CU: +23-75% measured across geometries
//   (8 KiB synthetic 111 -> 163 GB/s; real text 8 KiB 88 -> 129).
//
// Geometry (default, v4): one wave (64 lanes) per block, parsing the
// compressed stream straight from global memory; LDS = RAWCAP bytes of
// decoded output only.  RAWCAP is the smallest compiled rung
// (4/8/16/32/64 KiB) that holds the caller's raw_cap; SYSHARD defaults
// to 8 KiB blocks, so the 8 KiB rung is the one that normally runs
// (about 9 workgroups per CU, table below).  Throughput comes from
// block parallelism; the framework's SYSHARD format stores
// incompressible blocks raw ("stored"), which bypass this kernel
// entirely via device memcpy.
// The v3 staged geometry (SY_LZ4_NOSTAGE=0, the SY_LZ4_SKIP probes and
// the producer/consumer kernel) adds RAWCAP + 1 KiB of LDS for the
// staged input (compressed blocks may slightly exceed raw size for
// incompressible data): at 64 KiB that is one workgroup per CU.
//
// Match copies use the doubling schedule: round r copies
// n = min(remaining, done+offset) bytes at read stride -(done+offset)
// (a multiple of `offset` by induction), so the periodic pattern is
// preserved and every read lands in a completed round.

#include "common.h"

namespace {

// RAWCAP instantiations (measured, 1 GiB synthetic, ratio ~0.9):
//   64 KiB -> 1 workgroup/CU  ->  4.9 GB/s
//   32 KiB -> 2               -> 12.7
//   16 KiB -> 4               -> 35.2
//    8 KiB -> 9               -> 94.2
// The decoder is a serial dependency chain per block; occupancy (more
// concurrent blocks per CU) is the throughput lever.  SYSHARD defaults
// to 8 KiB blocks (compression-window loss is a few %% vs 64 KiB).

enum : uint32_t {
  SY_LZ4_OK = 0,
  SY_LZ4_ERR_OFFSET = 1,
  SY_LZ4_ERR_OVERFLOW = 2,
  SY_LZ4_ERR_TRUNC = 3,
  SY_LZ4_ERR_MISMATCH = 4,
  SY_LZ4_ERR_TOOBIG = 5,
};

// s_waitcnt immediate: lgkmcnt(0) only (vmcnt/expcnt unconstrained)
constexpr int kWaitLgkm0 = 0xC07F;

// ---- leaves shared by the single-wave and producer/consumer kernels ----

// Length extension: add 255-run bytes to `len` until one is < 255.
// Sets `st` to SY_LZ4_ERR_TRUNC when the stream ends first.
__device__ __forceinline__ void read_len_ext(const uint8_t* src,
                                             uint32_t& pos, uint32_t slen,
                                             uint32_t& len, uint32_t& st) {
  uint8_t b;
  do {
    if (pos >= slen) { st = SY_LZ4_ERR_TRUNC; break; }
    b = src[pos++];
    len += b;
  } while (b == 255);
}

// Longest stream a staged kernel accepts in an sbuf of `src_buf` bytes.
// -48: staging copies the 16B-aligned enclosing region (up to +15
// head, +15 tail rounding) — keep the last sbuf slot unwritten
__device__ __forceinline__ constexpr uint32_t stage_max_slen(int src_buf) {
  return (uint32_t)src_buf - 48;
}

// Stage a compressed block into LDS, coalesced 16 B per thread over NT
// threads.  Copies the 16B-aligned enclosing region so loads stay
// aligned; returns `srcoff`, where the stream starts inside sbuf.  The
// caller orders the LDS writes before its first parse read.
template <int NT>
__device__ __forceinline__ uint32_t stage_in(uint8_t* sbuf,
                                             const uint8_t* comp,
                                             uint64_t abase, uint32_t slen,
                                             int tid) {
  const uint64_t astart = abase & ~15ull;
  const uint32_t srcoff = (uint32_t)(abase - astart);
  const uint32_t stage_bytes = srcoff + slen;
  const uint4* g4 = reinterpret_cast<const uint4*>(comp + astart);
  uint4* s4 = reinterpret_cast<uint4*>(sbuf);
  const uint32_t n16 = (stage_bytes + 15) >> 4;
  for (uint32_t i = tid; i < n16; i += NT) s4[i] = g4[i];
  return srcoff;
}

// Stream a decoded block LDS -> HBM, coalesced 16 B per thread over NT
// threads, byte tail last.  `g` is 16B-aligned (out_off contract).
template <int NT>
__device__ __forceinline__ void stream_out(uint8_t* g, const uint8_t* dst,
                                           uint32_t rawlen, int tid) {
  const uint32_t n16 = rawlen >> 4;
  const uint4* s4 = reinterpret_cast<const uint4*>(dst);
  uint4* g4 = reinterpret_cast<uint4*>(g);
  for (uint32_t i = tid; i < n16; i += NT) g4[i] = s4[i];
  for (uint32_t i = (n16 << 4) + tid; i < rawlen; i += NT) g[i] = dst[i];
}

// PROBE: 0 = real decode; 1 = skip literal copies; 2 = skip match
// copies (both produce WRONG output — perf attribution only, selected
// via SY_LZ4_SKIP for experiments).
// STAGE: 1 = stage the compressed block into LDS (v3); 0 = parse
// straight from global memory (the stream is read once, sequentially,
// so its lines stay hot in the wave's L1) — the ~9 KiB LDS saved per
// WG roughly doubles resident blocks/CU, and occupancy is the
// measured throughput lever.  A/B via SY_LZ4_NOSTAGE=1.
template <int RAWCAP, int PROBE = 0, int STAGE = 1>
__global__ __launch_bounds__(SY_WAVE) void lz4_decode_kernel(
    const uint8_t* __restrict__ comp, const uint64_t* __restrict__ in_off,
    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
    const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_len,
    uint32_t* __restrict__ status, uint32_t n_blocks) {
  constexpr int kSrcBuf = STAGE ? RAWCAP + 1024 : 16;
  __shared__ uint8_t dst[RAWCAP];
  __shared__ uint8_t sbuf[kSrcBuf];

  const int lane = threadIdx.x;

  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const uint64_t abase = in_off[blk];
    const uint32_t slen = in_len[blk];
    const uint32_t rawlen = out_len[blk];
    uint32_t st = SY_LZ4_OK;

    if ((STAGE && slen > stage_max_slen(kSrcBuf)) ||
        rawlen > (uint32_t)RAWCAP) {
      if (lane == 0) status[blk] = SY_LZ4_ERR_TOOBIG;
      continue;
    }

    {
      // STAGE: parse from the LDS copy (src = sbuf + srcoff), else
      // straight from global.  NOTE (measured): a
      // 16 B register-window fetch for header bytes is 45% SLOWER than
      // these per-byte LDS reads — at 9+ waves/CU the read latency is
      // TLP-hidden and the window's extraction VALU + refill join the
      // serial chain instead.
      const uint8_t* src = comp + abase;
      if (STAGE) {
        src = sbuf + stage_in<SY_WAVE>(sbuf, comp, abase, slen, lane);
        // all lanes' vm loads -> lds writes must land before parsing
        __builtin_amdgcn_s_waitcnt(0);
      }

      // Uniform parse state (identical in every lane; LDS byte reads
      // of the same address broadcast).
      uint32_t pos = 0;
      uint32_t dpos = 0;
      for (;;) {
        if (pos >= slen) {
          if (dpos != rawlen) st = SY_LZ4_ERR_MISMATCH;
          break;
        }
        const uint32_t token = src[pos++];
        uint32_t litlen = token >> 4;
        if (litlen == 15) {
          read_len_ext(src, pos, slen, litlen, st);
          if (st != SY_LZ4_OK) break;
        }
        if (dpos + litlen > rawlen || pos + litlen > slen) {
          st = SY_LZ4_ERR_OVERFLOW;
          break;
        }

        // ---- cooperative literal copy: LDS sbuf -> LDS dst ----
        // (byte-granular; funnel-shift wide copies measured 15-20%
        // SLOWER overall — typical runs are 5-30 B and the head/word/
        // tail fragmentation costs more than 4 B/lane saves.)
        // Short-run fast path: typical literal runs fit one wave, so
        // a predicated single copy drops the loop back-edge from the
        // serial chain (round-2 instruction-economy lever).
        if (PROBE != 1) {
          if (litlen <= (uint32_t)SY_WAVE) {
            if ((uint32_t)lane < litlen) dst[dpos + lane] = src[pos + lane];
          } else {
            for (uint32_t i = lane; i < litlen; i += SY_WAVE) {
              dst[dpos + i] = src[pos + i];
            }
          }
        }
        pos += litlen;
        dpos += litlen;
        if (pos == slen) {
          if (dpos != rawlen) st = SY_LZ4_ERR_MISMATCH;
          break;
        }

        if (pos + 2 > slen) { st = SY_LZ4_ERR_TRUNC; break; }
        const uint32_t offset =
            (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
        pos += 2;
        uint32_t mlen = (token & 0xFu) + 4;
        if ((token & 0xFu) == 15) {
          read_len_ext(src, pos, slen, mlen, st);
          if (st != SY_LZ4_OK) break;
        }
        if (offset == 0 || offset > dpos) { st = SY_LZ4_ERR_OFFSET; break; }
        if (dpos + mlen > rawlen) { st = SY_LZ4_ERR_OVERFLOW; break; }

        // all prior LDS writes (this sequence's literals, earlier
        // matches) must be visible before match reads; between rounds
        // the same wait orders round i -> i+1.  The LAST round needs
        // no wait: the next sequence's literal copy only WRITES (to
        // disjoint, higher dst addresses), and its own pre-match wait
        // re-orders before any read.
        __builtin_amdgcn_s_waitcnt(kWaitLgkm0);

        // ---- cooperative match copy, doubling over overlap ----
        // Fast path: a non-overlapping match (offset >= mlen) is one
        // round by construction, and when it also fits one wave the
        // predicated copy skips the doubling machinery entirely.
        if (PROBE != 2) {
          if (offset >= mlen) {
            if (mlen <= (uint32_t)SY_WAVE) {
              if ((uint32_t)lane < mlen)
                dst[dpos + lane] = dst[dpos + lane - offset];
            } else {
              for (uint32_t i = lane; i < mlen; i += SY_WAVE) {
                dst[dpos + i] = dst[dpos + i - offset];
              }
            }
          } else {
            uint32_t done = 0;
            while (done < mlen) {
              const uint32_t dist = done + offset;  // multiple of offset
              const uint32_t n = min(mlen - done, dist);
              for (uint32_t i = lane; i < n; i += SY_WAVE) {
                dst[dpos + done + i] = dst[dpos + done + i - dist];
              }
              done += n;
              if (done < mlen) __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
            }
          }
        }
        dpos += mlen;
      }
    }

    if (lane == 0) status[blk] = st;
    if (st == SY_LZ4_OK) {
      __builtin_amdgcn_s_waitcnt(0);
      stream_out<SY_WAVE>(out + out_off[blk], dst, rawlen, lane);
    }
    __builtin_amdgcn_s_waitcnt(0);
  }
}

}  // namespace

SY_EXPORT int sy_lz4_decode_blocks(const void* d_comp, const uint64_t* d_in_off,
                                   const uint32_t* d_in_len, void* d_out,
                                   const uint64_t* d_out_off,
                                   const uint32_t* d_out_len,
                                   uint32_t* d_status, uint32_t n_blocks,
                                   uint32_t raw_cap, hipStream_t stream) {
  // nothing to decode: success without a launch, whatever raw_cap is
  if (n_blocks == 0) return 0;
  // Grid cap (SY_LZ4_GRID overrides; 0 or unset = default).
  // DVFS-warmed sweep on real
  // content at 4 KiB blocks: cap 2048 -> 47 GB/s, 4096 -> 74,
  // 6144 -> 82, 8192 -> 90.5 (and 8 KiB blocks scale the same) —
  // monotone in resident+queued workgroups (8192 -> 197, 16384 -> 216,
  // 32768 -> 229 GB/s synthetic 4 KiB) — hardware dispatch of queued
  // workgroups beats grid-striding; effectively uncapped by default.
  static const uint32_t grid_env = (uint32_t)sy_env_atoi("SY_LZ4_GRID", 0);
  const uint32_t grid_cap = grid_env ? grid_env : 1u << 22;
  const uint32_t grid = n_blocks < grid_cap ? n_blocks : grid_cap;
  // v4 DEFAULT: parse straight from global memory (no LDS src
  // staging).  The compressed stream is read once sequentially so its
  // lines stay L1-hot, and the ~9-66 KiB LDS saved per WG doubles
  // resident blocks/CU — measured +23-75% across geometries
  // (profiles/data_plane_r02.md).  SY_LZ4_NOSTAGE=0 forces the v3
  // staged path back for A/B.
  static const bool stage = sy_env_atoi("SY_LZ4_NOSTAGE", 1) == 0;
  // Perf-attribution probes (WRONG OUTPUT; experiments only):
  // SY_LZ4_SKIP=1|2 takes effect only for raw_cap <= 8 KiB, where it
  // runs the staged 8 KiB instantiation whatever SY_LZ4_NOSTAGE says.
  // Any other value or a larger raw_cap is the normal path.
  static const int probe_env = sy_env_atoi("SY_LZ4_SKIP", 0);
  const int probe = raw_cap <= 8 * 1024 ? probe_env : 0;
  const bool probing = probe == 1 || probe == 2;

  auto launch = [&](auto* kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(SY_WAVE), 0, stream,
                       static_cast<const uint8_t*>(d_comp), d_in_off,
                       d_in_len, static_cast<uint8_t*>(d_out), d_out_off,
                       d_out_len, d_status, n_blocks);
    return sy_check(hipGetLastError());
  };
  // raw_cap > 64 KiB is -22 under every environment setting.  A probe
  // asks for exactly 8 KiB, which lands on the 8 KiB rung.
  return sy_dispatch_rung<4 * 1024, 8 * 1024, 16 * 1024, 32 * 1024,
                          64 * 1024>(
      probing ? 8 * 1024 : raw_cap, [&](auto cap) {
        constexpr int CAP = decltype(cap)::value;
        if constexpr (CAP == 8 * 1024) {
          if (probe == 1) return launch(lz4_decode_kernel<CAP, 1, 1>);
          if (probe == 2) return launch(lz4_decode_kernel<CAP, 2, 1>);
        }
        return stage ? launch(lz4_decode_kernel<CAP, 0, 1>)
                     : launch(lz4_decode_kernel<CAP, 0, 0>);
      });
}

namespace {

// ---------------------------------------------------------------------
// Producer/consumer variant: one 128-thread workgroup (2 waves) per
// block.  Wave 0 parses the sequence stream into an LDS record ring;
// wave 1 executes literal/match copies.  The two serial dependency
// chains (parse: dependent LDS byte reads; copy: LDS round trips +
// lgkm waits) overlap instead of interleaving, targeting ~2x per
// block at unchanged LDS footprint (occupancy is LDS-bound).
// All spins are bounded: a protocol bug yields SY_LZ4_ERR_DEADLOCK,
// never a wedged GPU.
// ---------------------------------------------------------------------

constexpr uint32_t SY_LZ4_ERR_DEADLOCK = 6;
constexpr int kRingSz = 64;  // records; power of two
constexpr uint32_t kBatch = 16;  // records per counter publish (r2)
constexpr uint32_t kSpinLimit = 1u << 27;

struct SeqRec {
  uint32_t lit_src;   // comp offset of literal bytes (rel. to src)
  uint32_t lit_len;
  uint32_t offset;    // 0 == literals-only terminator
  uint32_t mlen;
};

template <int RAWCAP>
__global__ __launch_bounds__(2 * SY_WAVE) void lz4_decode_pc_kernel(
    const uint8_t* __restrict__ comp, const uint64_t* __restrict__ in_off,
    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
    const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_len,
    uint32_t* __restrict__ status, uint32_t n_blocks) {
  constexpr int kSrcBuf = RAWCAP + 1024;
  __shared__ uint8_t dst[RAWCAP];
  __shared__ uint8_t sbuf[kSrcBuf];
  __shared__ SeqRec ring[kRingSz];
  __shared__ uint32_t ctl[4];  // [0]=produced [1]=consumed [2]=status [3]=nseq

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  volatile uint32_t* vctl = ctl;

  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const uint64_t abase = in_off[blk];
    const uint32_t slen = in_len[blk];
    const uint32_t rawlen = out_len[blk];

    if (slen > stage_max_slen(kSrcBuf) || rawlen > (uint32_t)RAWCAP) {
      if (tid == 0) status[blk] = SY_LZ4_ERR_TOOBIG;
      __syncthreads();
      continue;
    }

    // ---- stage compressed block into LDS (both waves) ----
    const uint32_t srcoff =
        stage_in<2 * SY_WAVE>(sbuf, comp, abase, slen, tid);
    if (tid == 0) {
      ctl[0] = 0; ctl[1] = 0; ctl[2] = SY_LZ4_OK; ctl[3] = 0;
    }
    __syncthreads();
    const uint8_t* src = sbuf + srcoff;

    if (wave == 0) {
      // ---------------- producer: parse into the ring ----------------
      uint32_t pos = 0;
      uint32_t produced = 0;
      uint32_t st = SY_LZ4_OK;
      uint32_t dtotal = 0;  // decoded bytes accounted (bounds checks)
      for (;;) {
        if (pos >= slen) {
          if (dtotal != rawlen) st = SY_LZ4_ERR_MISMATCH;
          break;
        }
        const uint32_t token = src[pos++];
        uint32_t litlen = token >> 4;
        if (litlen == 15) {
          read_len_ext(src, pos, slen, litlen, st);
          if (st != SY_LZ4_OK) break;
        }
        if (dtotal + litlen > rawlen || pos + litlen > slen) {
          st = SY_LZ4_ERR_OVERFLOW;
          break;
        }
        const uint32_t lit_src = pos;
        pos += litlen;
        dtotal += litlen;
        uint32_t offset = 0, mlen = 0;
        if (pos != slen) {
          if (pos + 2 > slen) { st = SY_LZ4_ERR_TRUNC; break; }
          offset = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
          pos += 2;
          mlen = (token & 0xFu) + 4;
          if ((token & 0xFu) == 15) {
            read_len_ext(src, pos, slen, mlen, st);
            if (st != SY_LZ4_OK) break;
          }
          if (offset == 0 || offset > dtotal) {
            st = SY_LZ4_ERR_OFFSET;
            break;
          }
          if (dtotal + mlen > rawlen) { st = SY_LZ4_ERR_OVERFLOW; break; }
          dtotal += mlen;
        }
        // flow control: wait for ring space (lane 0 polls, broadcast)
        uint32_t spins = 0;
        uint32_t consumed;
        do {
          consumed = vctl[1];
          if (++spins > kSpinLimit) { st = SY_LZ4_ERR_DEADLOCK; break; }
          if (produced - consumed >= (uint32_t)kRingSz)
            __builtin_amdgcn_s_sleep(2);  // back off the LDS pipe
        } while (produced - consumed >= (uint32_t)kRingSz);
        if (st != SY_LZ4_OK) break;
        if (lane == 0) {
          SeqRec r;
          r.lit_src = lit_src;
          r.lit_len = litlen;
          r.offset = offset;
          r.mlen = mlen;
          ring[produced & (kRingSz - 1)] = r;
        }
        ++produced;
        // batched handoff (round-2): publish the counter every
        // kBatch records instead of per record — the per-record
        // publish (record-write wait + counter write + wait) was the
        // ~2-LDS-latency handoff that made the r1 p/c variant lose
        if (lane == 0 && (produced & (kBatch - 1)) == 0) {
          __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // records first
          ctl[0] = produced;
          __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
        }
        if (pos == slen && (dtotal == rawlen)) {
          // final literals-only sequence had offset==0 terminator
          if (offset == 0) break;
        }
        if (pos == slen) {
          if (dtotal != rawlen) st = SY_LZ4_ERR_MISMATCH;
          break;
        }
      }
      if (lane == 0) {
        if (st != SY_LZ4_OK) vctl[2] = st;
        __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // tail records land
        vctl[0] = produced;  // publish any unbatched tail
        vctl[3] = produced | 0x80000000u;  // parse done + count
        __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
      }
    } else {
      // ---------------- consumer: execute copies ---------------------
      uint32_t consumed = 0;
      uint32_t dpos = 0;
      uint32_t st = SY_LZ4_OK;
      for (;;) {
        // wait for a record or parse-done
        uint32_t spins = 0;
        uint32_t produced, done_word;
        for (;;) {
          produced = vctl[0];
          done_word = vctl[3];
          if (produced > consumed) break;
          if (done_word & 0x80000000u) break;
          if (vctl[2] != SY_LZ4_OK) break;
          if (++spins > kSpinLimit) break;
          __builtin_amdgcn_s_sleep(1);  // back off the LDS pipe
        }
        if (produced <= consumed) {
          // done/error observed with a possibly stale counter (the
          // produced read precedes the done read): re-read once so a
          // just-published tail batch is never dropped
          produced = vctl[0];
          if (produced <= consumed) {
            if (spins > kSpinLimit) st = SY_LZ4_ERR_DEADLOCK;
            break;  // parse done (or error): no more records
          }
        }
        SeqRec r = ring[consumed & (kRingSz - 1)];
        // literal copy: sbuf -> dst
        for (uint32_t i = lane; i < r.lit_len; i += SY_WAVE) {
          dst[dpos + i] = src[r.lit_src + i];
        }
        dpos += r.lit_len;
        if (r.offset) {
          __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
          uint32_t done = 0;
          while (done < r.mlen) {
            const uint32_t dist = done + r.offset;
            const uint32_t n = min(r.mlen - done, dist);
            for (uint32_t i = lane; i < n; i += SY_WAVE) {
              dst[dpos + done + i] = dst[dpos + done + i - dist];
            }
            done += n;
            __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
          }
          dpos += r.mlen;
        }
        ++consumed;
        // batched consumed publish: the producer only polls this when
        // the 64-slot ring fills, so a <=kBatch lag can never stall it
        if (lane == 0 && (consumed & (kBatch - 1)) == 0) {
          vctl[1] = consumed;
        }
      }
      if (lane == 0 && st != SY_LZ4_OK && vctl[2] == SY_LZ4_OK) {
        vctl[2] = st;
      }
    }
    __syncthreads();

    const uint32_t st = ctl[2];
    if (tid == 0) status[blk] = st;
    if (st == SY_LZ4_OK) {
      // both waves
      stream_out<2 * SY_WAVE>(out + out_off[blk], dst, rawlen, tid);
    }
    __syncthreads();
  }
}

}  // namespace

SY_EXPORT int sy_lz4_decode_blocks_pc(
    const void* d_comp, const uint64_t* d_in_off, const uint32_t* d_in_len,
    void* d_out, const uint64_t* d_out_off, const uint32_t* d_out_len,
    uint32_t* d_status, uint32_t n_blocks, uint32_t raw_cap,
    hipStream_t stream) {
  // nothing to decode: success without a launch, whatever raw_cap is
  if (n_blocks == 0) return 0;
  // fixed grid cap; SY_LZ4_GRID and the other knobs do not apply here
  const uint32_t grid = n_blocks < 4096u ? n_blocks : 4096u;
  // No 4 KiB or 32 KiB rung: those raw_caps run at 8 and 64 KiB.
  // raw_cap > 64 KiB is -22.
  return sy_dispatch_rung<8 * 1024, 16 * 1024, 64 * 1024>(
      raw_cap, [&](auto cap) {
        hipLaunchKernelGGL(lz4_decode_pc_kernel<decltype(cap)::value>,
                           dim3(grid), dim3(2 * SY_WAVE), 0, stream,
                           static_cast<const uint8_t*>(d_comp), d_in_off,
                           d_in_len, static_cast<uint8_t*>(d_out),
                           d_out_off, d_out_len, d_status, n_blocks);
        return sy_check(hipGetLastError());
      });
}
