// AllReduce (sum) of fp16 / bf16 buffers whose payload crosses xGMI in an OCP microscaling format: MXINT8 or
// MXFP4 codes with one e8m0 scale byte per block of 32 consecutive elements.  A two-shot push
// through the bulk scratch: no user buffer is mapped or read remotely.  Per block of fp32 values v,
//
//   amax = max |v_j|, e32 = amax's biased fp32 exponent field
//   mxint8: E = e32,              code_j = clamp(RNE(v_j * 2^(133 - E)), +-127),   dq_j = code_j * 2^(E - 133)
//   mxfp4:  E = max(e32 - 2, 0),  code_j = e2m1(v_j * 2^(127 - E)) (RNE, +-6),     dq_j = e2m1(code_j) * 2^(E - 127)
//
// and out = (DT) D(Q(c_0 + c_1 + ... + c_{n-1})), c_r = D(Q(x_r)), the sum in fp32 in rank order.  Every product
// is a scaling by a power of two (v_ldexp_f32, the scaled FP4 conversions): exact, and nothing a compiler could
// contract with the adds.  The own contribution passes through Q like the peers', so out depends on the inputs
// alone: the same bits on every rank, at every grid and pass split.
//
//  * Blocks over ranks: B = count / 32, S = ceil(B / n); rank q owns blocks [q S, min((q + 1) S, B)).  A pass
//    covers P blocks of every slice, workgroup b the blocks [b W, (b + 1) W) of the pass (W % 4 == 0), in every
//    slice alike, and it waits for the peers' workgroup b alone (channel b).
//  * A lane unit is 16 bytes of codes: 16 elements (32 bytes of x) in mxint8, where a block is a lane pair whose
//    amax is one DPP quad_perm move, and 32 elements (64 bytes of x), a whole block, in mxfp4.  Scale bytes of
//    four consecutive blocks are gathered into one lane (ds_bpermute, no LDS memory) and leave as a dword.
//  * The scratch holds region A and region B, n images each; an image is a run of codes (P * 32 or P * 16
//    bytes) followed by a run of scale bytes (P, padded to 16).  Every loop is uniform over the workgroup: a lane
//    past the range loads zeros and stores nothing (descriptors of exactly the range), so the lanes that share a
//    block, or gather its scale, are all live.
//  * Phase 1: for the slices rank + 1, ..., rank (mod n): plain 16-byte loads of x, Q, the codes and scales into
//    the OWNER's region A at image [rank].  Handshake.  Phase 2: the n images of the own slice out of the own
//    region A, all loads of a unit issued first; D, the sum in rank order, Q in the registers that hold the sum;
//    the result into region B, image [rank], of every rank.  Handshake.  Phase 3: the n images of the own region
//    B, D, one rounding to DT, plain stores to out.  One handshake at exit hands the scratch to whatever kernel
//    comes next (§17n has the argument; between passes and between launches of this kernel none is needed).
//  * out == x is carried: a pass reads its range of x in phase 1 and writes it in phase 3.
//    Trace stamps (of the last pass): 0 start, 1 scattered, 2 handshake, 3 reduced, 4 handshake, 5 stored, 6 end.
#include "allreduce_rmsnorm.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

constexpr int kWireInt8 = MSCCLPP_AMD_WIRE_MXINT8, kWireFp4 = MSCCLPP_AMD_WIRE_MXFP4;

struct ArQuantGeom {
  uint32_t blocks;   // B
  uint32_t slice;    // S
  uint32_t pass;     // P: blocks of a slice per pass, a multiple of 4
  uint32_t wg;       // W: blocks of a pass per workgroup, a multiple of 4
  uint32_t npasses;
  uint32_t img;      // bytes of an image
  uint64_t regionB;  // byte offset of region B in the scratch
};

template <int NV>
struct ArQuantArgs {
  Views<NV> views;
  ArQuantGeom g;
  uint64_t budget;
  uint64_t* trace;
  int nranks;
  int pad;
};
static_assert(sizeof(ArQuantArgs<kMaxRanks>) <= 4096, "in-process quantised AllReduce arguments exceed the limit");

__host__ __device__ constexpr uint32_t arqCodeBytes(int fmt) { return fmt == kWireInt8 ? 32u : 16u; }  // per block
__host__ __device__ inline uint32_t arqImageBytes(uint32_t P, int fmt) { return P * arqCodeBytes(fmt) + ((P + 15u) & ~15u); }

// Workgroup b's blocks of rank q's slice in pass ps: [*first, *first + the result).
__host__ __device__ inline uint32_t arqBlocks(const ArQuantGeom& g, uint32_t q, uint32_t ps, uint32_t b, uint32_t* first) {
  const uint64_t pEnd = (uint64_t)(ps + 1) * g.pass;
  const uint64_t lo = (uint64_t)ps * g.pass + (uint64_t)b * g.wg;
  uint64_t hi = lo + g.wg < pEnd ? lo + g.wg : pEnd;
  if (hi > g.slice) hi = g.slice;
  const uint64_t at = (uint64_t)q * g.slice + lo;
  uint64_t end = (uint64_t)q * g.slice + hi;
  if (end > g.blocks) end = g.blocks;
  *first = (uint32_t)at;
  return lo < hi && at < end ? (uint32_t)(end - at) : 0u;
}

// The value of lane t + d of the wave (t + d stays inside it wherever the result is used).
__device__ __forceinline__ uint32_t arq_lane(uint32_t v, uint32_t t, uint32_t d) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((t + d) & 63u) << 2), (int)v);
}

// What a lane holds of a unit: EPU fp32 values.
template <int FMT>
struct ArqUnit {
  static constexpr int EPU = FMT == kWireInt8 ? 16 : 32;  // elements
  static constexpr int LPB = 32 / EPU;                    // lanes per block
  static constexpr int NX = EPU / 8;                      // 16-byte units of DT elements
  float v[EPU];
};

// Q of the lane's values: the 16 bytes of codes and the block's scale byte E.
template <int FMT>
__device__ __forceinline__ u32x4 arq_quant(const ArqUnit<FMT>& a, uint32_t* Eout) {
  constexpr int EPU = ArqUnit<FMT>::EPU;
  uint32_t am = 0;
#pragma unroll
  for (int j = 0; j < EPU; ++j) {
    const uint32_t m = __builtin_bit_cast(uint32_t, a.v[j]) & 0x7fffffffu;
    am = m > am ? m : am;
  }
  if constexpr (FMT == kWireInt8) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)am, 0xb1, 0xf, 0xf, true);  // lane t ^ 1
    am = am > o ? am : o;
  }
  const uint32_t e32 = am >> 23;
  uint32_t w[4];
  if constexpr (FMT == kWireInt8) {
    const uint32_t E = e32;
    const int sh = 133 - (int)E;  // 2^(127 - E) * 64
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t p = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s = __builtin_rintf(__builtin_ldexpf(a.v[4 * i + j], sh));  // an exact product, RNE to an integer
        s = __builtin_amdgcn_fmed3f(s, -127.0f, 127.0f);
        p |= ((uint32_t)(int)s & 0xffu) << (8 * j);
      }
      w[i] = p;
    }
    *Eout = E;
  } else {
    const uint32_t E = e32 > 2u ? e32 - 2u : 0u;
    const float x = __builtin_bit_cast(float, E << 23);  // the instruction divides by 2^(its exponent field - 127)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* e = a.v + 8 * i;  // (the byte selector is an immediate)
      uint32_t p = 0;
      p = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(p, e[0], e[1], x, 0);
      p = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(p, e[2], e[3], x, 1);
      p = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(p, e[4], e[5], x, 2);
      p = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(p, e[6], e[7], x, 3);
      w[i] = p;
    }
    *Eout = E;
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// D of 16 bytes of codes under scale byte E: first == true sets the values, else they are added (one fp32 add
// per element).
template <int FMT, bool First>
__device__ __forceinline__ void arq_dequant(ArqUnit<FMT>& a, u32x4 c, uint32_t E) {
  if constexpr (FMT == kWireInt8) {
    const int sh = (int)E - 133;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int code = (int)(c[i] << (24 - 8 * j)) >> 24;  // the byte, sign-extended
        const float d = __builtin_ldexpf((float)code, sh);
        if constexpr (First) a.v[4 * i + j] = d;
        else a.v[4 * i + j] = a.v[4 * i + j] + d;
      }
  } else {
    const float x = __builtin_bit_cast(float, E << 23);
    auto put = [&](int at, auto d) {
      if constexpr (First) {
        a.v[at] = d[0];
        a.v[at + 1] = d[1];
      } else {
        a.v[at] = a.v[at] + d[0];
        a.v[at + 1] = a.v[at + 1] + d[1];
      }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // (the byte selector is an immediate)
      put(8 * i, __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c[i], x, 0));
      put(8 * i + 2, __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c[i], x, 1));
      put(8 * i + 4, __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c[i], x, 2));
      put(8 * i + 6, __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c[i], x, 3));
    }
  }
}

// The codes and the gathered scale dword of unit u into an image: rc over the range's codes, rs over its scale
// bytes rounded up to whole dwords.  Every lane of the workgroup calls it.
template <int FMT>
__device__ __forceinline__ void arq_store(__amdgpu_buffer_rsrc_t rc, __amdgpu_buffer_rsrc_t rs, uint32_t u, uint32_t t,
                                          u32x4 codes, uint32_t w) {
  constexpr uint32_t LPB = ArqUnit<FMT>::LPB;
  store16<kSystem>(rc, u * 16u, codes);
  if ((t & (4u * LPB - 1u)) == 0) store4<kSystem>(rs, u / LPB, w);  // u / LPB: the block, a multiple of 4 here
}

// The scale bytes of the four blocks that start at this lane's, low byte first (used on lanes t % (4 LPB) == 0).
template <int FMT>
__device__ __forceinline__ uint32_t arq_gather(uint32_t E, uint32_t t) {
  constexpr uint32_t LPB = ArqUnit<FMT>::LPB;
  uint32_t w = E;
  w |= arq_lane(E, t, LPB) << 8;
  w |= arq_lane(E, t, 2u * LPB) << 16;
  w |= arq_lane(E, t, 3u * LPB) << 24;
  return w;
}

// Two waves per SIMD at 512 lanes: up to 256 VGPRs (mxfp4 holds 32 sums and 8 x 4 code words per lane).
template <int DT, int FMT, int NV>
__global__ void __launch_bounds__(512) allreduceQuantKernel(ArQuantArgs<NV> a) {
  using Unit = ArqUnit<FMT>;
  constexpr uint32_t EPU = Unit::EPU, LPB = Unit::LPB, NX = Unit::NX, XB = EPU * 2u, CB = arqCodeBytes(FMT);
  const mscclppAmdRankView& v = a.views.v[NV == 1 ? 0 : blockIdx.y];
  const int rank = v.rank, n = a.nranks;
  const ArQuantGeom& g = a.g;
  const uint32_t T = blockDim.x, t = threadIdx.x, b = blockIdx.x;
  const uint32_t codeAt = b * g.wg * CB, scaleAt = g.pass * CB + b * g.wg;  // of the workgroup's range in an image
  uint8_t* scr = (uint8_t*)v.scratch;
  trace_stamp(a.trace, 0);

  for (uint32_t ps = 0; ps < g.npasses; ++ps) {
    // ---- phase 1: Q of my x for every slice, into the owner's region A at image [rank]
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
      const int q = (rank + 1 + k) % n;
      uint32_t first;
      const uint32_t nb = arqBlocks(g, (uint32_t)q, ps, b, &first);
      if (!nb) continue;
      const uint32_t nU = nb * LPB;
      const auto rx = arnorm_rsrc((const uint8_t*)v.input + (uint64_t)first * 64u, nb * 64u);
      uint8_t* image = (uint8_t*)v.peerScratch[q] + (uint64_t)rank * g.img;
      const auto rc = arnorm_rsrc(image + codeAt, nb * CB);
      const auto rs = arnorm_rsrc(image + scaleAt, (nb + 3u) & ~3u);
      for (uint32_t u0 = 0; u0 < nU; u0 += T) {
        const uint32_t u = u0 + t;
        u32x4 raw[NX];
#pragma unroll
        for (uint32_t i = 0; i < NX; ++i) raw[i] = load16<kPlain>(rx, u * XB + i * 16u);
        Unit x;
#pragma unroll
        for (uint32_t i = 0; i < NX; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            x.v[8 * i + 2 * j] = arnorm_lo<DT>(raw[i][j]);
            x.v[8 * i + 2 * j + 1] = arnorm_hi<DT>(raw[i][j]);
          }
        uint32_t E;
        const u32x4 codes = arq_quant<FMT>(x, &E);
        arq_store<FMT>(rc, rs, u, t, codes, arq_gather<FMT>(E, t));
      }
    }
    trace_stamp(a.trace, 1);
    block_handshake(v, n, rank, b, a.budget);  // every rank's image of my slice is in my region A
    trace_stamp(a.trace, 2);

    // ---- phase 2: D of the n images of my slice, the sum in rank order, Q, into everyone's region B at [rank]
    {
      uint32_t first;
      const uint32_t nb = arqBlocks(g, (uint32_t)rank, ps, b, &first);
      if (nb) {
        const uint32_t nU = nb * LPB, sLen = (nb + 3u) & ~3u;
        for (uint32_t u0 = 0; u0 < nU; u0 += T) {
          const uint32_t u = u0 + t;
          u32x4 c[kMaxRanks];
          uint32_t e[kMaxRanks];
#pragma unroll
          for (int k = 0; k < kMaxRanks; ++k)
            if (k < n) {
              const uint8_t* image = scr + (uint64_t)k * g.img;
              c[k] = load16<kSystem>(arnorm_rsrc(image + codeAt, nb * CB), u * 16u);
              e[k] = __builtin_amdgcn_raw_buffer_load_b8(arnorm_rsrc(image + scaleAt, sLen), u / LPB, 0, kSystem);
            }
          Unit s;
          arq_dequant<FMT, true>(s, c[0], e[0]);
#pragma unroll
          for (int k = 1; k < kMaxRanks; ++k)
            if (k < n) arq_dequant<FMT, false>(s, c[k], e[k]);
          uint32_t E;
          const u32x4 codes = arq_quant<FMT>(s, &E);
          const uint32_t w = arq_gather<FMT>(E, t);
#pragma unroll 1
          for (int k = 0; k < n; ++k) {
            uint8_t* image = (uint8_t*)v.peerScratch[(rank + k) % n] + g.regionB + (uint64_t)rank * g.img;
            arq_store<FMT>(arnorm_rsrc(image + codeAt, nb * CB), arnorm_rsrc(image + scaleAt, sLen), u, t, codes, w);
          }
        }
      }
    }
    trace_stamp(a.trace, 3);
    block_handshake(v, n, rank, b, a.budget);  // every owner's result image is in my region B
    trace_stamp(a.trace, 4);

    // ---- phase 3: D of my region B, one rounding to DT, out
#pragma unroll 1
    for (int q = 0; q < n; ++q) {
      uint32_t first;
      const uint32_t nb = arqBlocks(g, (uint32_t)q, ps, b, &first);
      if (!nb) continue;
      const uint32_t nU = nb * LPB;
      const uint8_t* image = scr + g.regionB + (uint64_t)q * g.img;
      const auto rc = arnorm_rsrc(image + codeAt, nb * CB);
      const auto rs = arnorm_rsrc(image + scaleAt, (nb + 3u) & ~3u);
      const auto ro = arnorm_rsrc((uint8_t*)v.output + (uint64_t)first * 64u, nb * 64u);
      for (uint32_t u0 = 0; u0 < nU; u0 += T) {
        const uint32_t u = u0 + t;
        const u32x4 c = load16<kSystem>(rc, u * 16u);
        const uint32_t E = __builtin_amdgcn_raw_buffer_load_b8(rs, u / LPB, 0, kSystem);
        Unit d;
        arq_dequant<FMT, true>(d, c, E);
#pragma unroll
        for (uint32_t i = 0; i < NX; ++i) {
          uint32_t z[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) z[j] = arnorm_pack<DT>(d.v[8 * i + 2 * j], d.v[8 * i + 2 * j + 1]);
          store16<kPlain>(ro, u * XB + i * 16u, u32x4{z[0], z[1], z[2], z[3]});
        }
      }
    }
    trace_stamp(a.trace, 5);
  }
  block_handshake(v, n, rank, b, a.budget);  // every rank is done with its region B: the scratch may change hands
  trace_stamp(a.trace, 6);
}

// A workgroup's range of x goes through one descriptor whose offsets stay below 2^32 for every lane of the last,
// partly idle, step: W * 64 + 512 * 64 bytes.
constexpr uint32_t kArqMaxWg = 1u << 25;

static uint64_t arqRegionBytes(int nranks, uint32_t P, int fmt) {
  return ((uint64_t)nranks * arqImageBytes(P, fmt) + 255) & ~255ull;
}

// 64 KiB of a rank's slice of x per workgroup, 1 .. 64: a function of (nranks, count) alone.  (Unmeasured.)
int allReduceQuantDefaultBlocks(int nranks, uint64_t count) {
  const uint64_t slice = (count / 32 + nranks - 1) / nranks * 64;
  const uint64_t want = (slice + (64u << 10) - 1) / (64u << 10);
  return (int)(want < 1 ? 1 : want > 64 ? 64 : want);
}

// The bytes of one pass over the whole buffer, enough at every grid; 0: the call is not carried.
size_t allReduceQuantScratchRequired(int nranks, size_t count, int dtype, int format) {
  if (nranks < 2 || nranks > kMaxRanks || count == 0 || count % 32 || (dtype != kF16 && dtype != kBF16) ||
      (format != kWireInt8 && format != kWireFp4) || count / 32 > 0xFFFFFFFFull)
    return 0;
  const uint64_t S = (count / 32 + nranks - 1) / nranks;
  const uint64_t P = ((S + 3) & ~3ull) + 4ull * kMaxChannels;  // W rounded up to 4 blocks in each workgroup
  if (P > 0x7FFFFFFFull / arqCodeBytes(format)) return 0;
  return (size_t)(2 * arqRegionBytes(nranks, (uint32_t)P, format));
}

// 0, or 4 / 5 with g untouched.  scratch: the smallest scratch of the views.
static int arqGeometry(int nranks, size_t count, int format, int nblocks, uint64_t scratch, ArQuantGeom* g) {
  const uint64_t B = count / 32, S = (B + nranks - 1) / nranks;
  uint64_t W = (((S + nblocks - 1) / nblocks) + 3) & ~3ull;
  const uint32_t CB = arqCodeBytes(format);
  auto need = [&](uint64_t w) { return 2 * arqRegionBytes(nranks, (uint32_t)(w * nblocks), format); };
  if (W * nblocks * CB > 0x7FFFFFFFull || need(W) > scratch) {
    // several passes: the largest W (a multiple of 4) whose two regions fit
    const uint64_t per = 2ull * nranks * nblocks * (CB + 1);
    uint64_t w = scratch / per;  // an upper bound: the padding only adds
    if (w > 0x7FFFFFFFull / ((uint64_t)nblocks * CB)) w = 0x7FFFFFFFull / ((uint64_t)nblocks * CB);
    w &= ~3ull;
    while (w && need(w) > scratch) w -= 4;
    if (!w) return 5;
    W = w;
  }
  if (W > kArqMaxWg) return 5;  // more workgroups carry it
  g->blocks = (uint32_t)B;
  g->slice = (uint32_t)S;
  g->wg = (uint32_t)W;
  g->pass = (uint32_t)(W * nblocks);
  g->npasses = (uint32_t)((S + g->pass - 1) / g->pass);
  g->img = arqImageBytes(g->pass, format);
  g->regionB = arqRegionBytes(nranks, g->pass, format);
  return 0;
}

template <int DT, int FMT>
static int launchArQuantT(const mscclppAmdRankView* views, int nviews, int nranks, const ArQuantGeom& g, int nblocks,
                          int nthreads, uint64_t budget, hipStream_t s) {
  auto fill = [&](auto& args) {
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.nranks = nranks;
    return 0;
  };
  return launchViews(allreduceQuantKernel<DT, FMT, 1>, allreduceQuantKernel<DT, FMT, kMaxRanks>, views, nviews, nblocks,
                     nthreads, s, fill);
}

// 4: invalid, nothing launched and no device touched -- a dtype other than fp16 / bf16, a count of 0 or no multiple
// of 32, nranks outside 2..8, an unknown format, a pointer that is null or not 16-byte aligned, an output that
// overlaps any input or other output otherwise than out == x of the same view, a bad launch shape; 5: a scratch
// too small for one workgroup step, a workgroup's range beyond one descriptor, or a grid that cannot be resident.
// The views' other fields (scratch, tokens, ...) are the caller's to check.
int launchAllReduceQuant(const mscclppAmdRankView* views, int nviews, int nranks, size_t count, int dtype, int format,
                         int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  if (!views || nviews < 1 || nviews > kMaxRanks || nranks < 2 || nranks > kMaxRanks) return 4;
  if (count == 0 || count % 32 || count / 32 > 0xFFFFFFFFull || (dtype != kF16 && dtype != kBF16) ||
      (format != kWireInt8 && format != kWireFp4))
    return 4;
  if (nblocks <= 0) nblocks = allReduceQuantDefaultBlocks(nranks, count);
  if (!launchShapeOk(nblocks, kMaxChannels, nthreads)) return 4;
  const size_t bytes = count * 2;
  uint64_t scratch = ~0ull;
  for (int i = 0; i < nviews; ++i) {
    const void* x = views[i].input;
    const void* o = views[i].output;
    if (!x || !o || ((uintptr_t)x | (uintptr_t)o) % 16) return 4;
    if (o != x && arNormOverlap(o, bytes, x, bytes)) return 4;
    for (int j = 0; j < i; ++j)
      if (arNormOverlap(o, bytes, views[j].input, bytes) || arNormOverlap(o, bytes, views[j].output, bytes) ||
          arNormOverlap(views[j].output, bytes, x, bytes))
        return 4;
    if (views[i].scratchBytes < scratch) scratch = views[i].scratchBytes;
  }
  ArQuantGeom g;
  if (const int rc = arqGeometry(nranks, count, format, nblocks, scratch, &g)) return rc;
  if (format == kWireInt8)
    return dtype == kF16 ? launchArQuantT<kF16, kWireInt8>(views, nviews, nranks, g, nblocks, nthreads, budget, s)
                         : launchArQuantT<kBF16, kWireInt8>(views, nviews, nranks, g, nblocks, nthreads, budget, s);
  return dtype == kF16 ? launchArQuantT<kF16, kWireFp4>(views, nviews, nranks, g, nblocks, nthreads, budget, s)
                       : launchArQuantT<kBF16, kWireFp4>(views, nviews, nranks, g, nblocks, nthreads, budget, s);
}

}  // namespace mscclpp_amd
