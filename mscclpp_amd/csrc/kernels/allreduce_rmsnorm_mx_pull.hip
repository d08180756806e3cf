// Fused AllReduce + residual add + RMSNorm whose normalised rows leave in an OCP microscaling format, MXFP8
// (e4m3) or MXFP4 (e2m1) with one e8m0 scale byte per block of 32 columns: allreduce_rmsnorm_pull.hip's two-shot
// zero-copy pull with the block quantisation behind it.  Steps 1-4 are §17i's, in §17j's order
// (so res_out, and y before it is quantised, are that kernel's bits at the same (cols, nthreads)); then, per
// block B of 32 consecutive columns of a row,
//
//   amax = max_{j in B} |y_j|            of the ROUNDED y (DT)
//   E    = max(e32(amax) - emax, 0)      e32: the biased exponent field of amax as fp32; emax = 8 (e4m3), 2 (e2m1);
//                                        one byte at scale[row][B]: the block's scale is X = 2^(E - 127)
//   q_j  = fmt(y_j * 2^(127 - E))        an exact fp32 product, rounded once (RNE), saturating at +-448 / +-6;
//                                        MXFP8: one byte at q[row][j]; MXFP4: column 2i in the low and column
//                                        2i + 1 in the high nibble of q[row][i]
//
//  * The geometry, the three handshakes, the visibility discipline and the descriptors are §17j's.  A row is
//    cols / 8 lane units: 16 bytes of x and res_out, 8 (MXFP8) or 4 (MXFP4) bytes of q; cols % 32 == 0 makes a
//    block four adjacent units -- the lanes of one quad, in one slot -- and keeps every row of q whole 16-byte
//    units in both formats.
//  * Phase 1, per row: §17j up to rstd, the prefetch of row i + 1's first batch ahead of the one barrier included.
//    Pass 2, per unit: y, packed in DT, over the registers that held zq; the lane's amax as an unsigned 16-bit
//    maximum of the sign-cleared patterns (§17k); the quad's maximum by two DPP quad_perm moves -- no LDS, no
//    second barrier; E by integer arithmetic on the exponent field; the conversion; the store, contiguous across
//    the lanes.  Lane 0 of each quad stores the block's E.
//    MXFP4 converts with v_cvt_scalef32_pk_fp4_f32 (on the GPU: RNE, saturating, the scale operand's exponent
//    field alone is read); MXFP8 multiplies by 2^(127 - E) and converts with v_cvt_pk_fp8_f32 behind §17k's clamp
//    (v_cvt_scalef32_pk_fp8_f32 gives the NaN code 0x7f above 448 where the definition saturates).
//  * Phase 2: workgroup b's range of every other slice of q (16-byte units), of the scale bytes (any length and
//    alignment: dwords where source and destination are aligned alike, bytes at the ragged ends and otherwise)
//    and, with a residual, of res_out are copied from their owners: system-scope loads, plain stores.
//  * q and scale overlap nothing; res_out == residual is carried as in §17j.  A block whose y holds a NaN or an
//    infinity has an unspecified q and E; its res_out, the other blocks and rows are as defined.
//    Trace stamps: 0 start, 1 entry handshake done, 2 own rows quantised, 3 peers' rows gathered, 4 end.
#include "allreduce_rmsnorm.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

template <int NV>
struct ArNormMxPullArgs {
  Views<NV> views;           // output: q
  const void* residual[NV];  // null on every view, or on none
  void* resOut[NV];
  const void* gamma[NV];
  uint8_t* scale[NV];
  const void* peerResOut[NV][kMaxRanks];  // rank q's res_out as this view has it mapped
  const void* peerScale[NV][kMaxRanks];   // ... and its scale bytes
  ArNormPullGeom g;
  uint64_t budget;
  uint64_t* trace;
  float eps;
  float invCols;  // 1.0f / (float)cols, computed once by the host
  int nranks;
  int pad;
};
static_assert(sizeof(ArNormMxPullArgs<kMaxRanks>) <= 4096,
              "in-process AllReduce+RMSNorm MX pull arguments exceed the kernel-argument limit");

// Four waves per SIMD (at most 128 VGPRs), as allreduceRmsNormPullKernel.
template <int DT, int UPL, int NV, int FMT>
__global__ void __launch_bounds__(512, 4) allreduceRmsNormMxPullKernel(ArNormMxPullArgs<NV> a) {
  // units whose loads are in flight together: (ranks + residual) x 4 VGPRs each
  constexpr int PB = UPL == 2 ? 2 : 1;
  constexpr uint32_t kEmax = FMT == kMxFp8 ? 8u : 2u;
  constexpr uint32_t kQShift = FMT == kMxFp8 ? 1u : 2u;  // a unit's bytes of q: 16 >> kQShift
  __shared__ uint32_t waveWords[2][8];                   // [the row's parity][wave]: 64 bytes
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const ArNormPullGeom& g = a.g;
  const uint32_t T = blockDim.x, t = threadIdx.x, b = blockIdx.x;
  const uint32_t rowBytes = g.upr * 16u, qRowBytes = rowBytes >> kQShift, sRowBytes = g.upr / 4u;
  const bool hasRes = a.residual[vi] != nullptr;
  trace_stamp(a.trace, 0);

  // The lane's units of a row: t, t + T, ...; the same slots are live in every row.  A slot past the row's
  // end loads the row's last unit, whose value is not used, and stores nothing.
  bool ok[UPL];
  uint32_t uoff[UPL];
  u32x4 gam[UPL];
  {
    const auto rgam = arnorm_rsrc(a.gamma[vi], rowBytes);
#pragma unroll
    for (int k = 0; k < UPL; ++k) {
      const uint32_t u = t + (uint32_t)k * T;
      ok[k] = u < g.upr;
      uoff[k] = (ok[k] ? u : g.upr - 1) * 16u;
      gam[k] = load16<kPlain>(rgam, uoff[k]);
    }
  }
  block_handshake(v, n, rank, b, a.budget);  // every rank's x is final
  trace_stamp(a.trace, 1);

  uint32_t row0;
  const uint32_t nrows = arNormPullRows(g, (uint32_t)rank, b, &row0);
  if (nrows) {
    const uint64_t at = (uint64_t)row0 * rowBytes;
    const uint32_t len = nrows * rowBytes;  // <= kBlkOffsetLimit (the host); q's and scale's ranges are shorter
    const auto rx = arnorm_rsrc((const uint8_t*)v.input + at, len);
    const auto rq = arnorm_rsrc((uint8_t*)v.output + (uint64_t)row0 * qRowBytes, nrows * qRowBytes);
    const auto rsc = arnorm_rsrc(a.scale[vi] + (uint64_t)row0 * sRowBytes, nrows * sRowBytes);
    const auto rres = arnorm_rsrc(hasRes ? (const uint8_t*)a.residual[vi] + at : nullptr, hasRes ? len : 0u);
    const auto rro = arnorm_rsrc(hasRes ? (uint8_t*)a.resOut[vi] + at : nullptr, hasRes ? len : 0u);
    const uint8_t* pin[kMaxRanks];  // pin[k]: rank k's x, this range
#pragma unroll
    for (int k = 0; k < kMaxRanks; ++k) pin[k] = k < n && k != rank ? (const uint8_t*)v.peerInput[k] + at : nullptr;

    u32x4 raw[PB][kMaxRanks], res[PB];
    // the loads of slots k0 .. k0 + PB - 1 of the row at byte rowOff of the range
    auto issue = [&](uint32_t rowOff, int k0) {
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const uint32_t off = rowOff + uoff[k0 + i];
#pragma unroll
        for (int k = 0; k < kMaxRanks; ++k)
          if (k < n) {
            if (k == rank)
              raw[i][k] = load16<kPlain>(rx, off);
            else
              raw[i][k] = load16<kSystem>(arnorm_rsrc(pin[k], len), off);
          }
        if (hasRes) res[i] = load16<kPlain>(rres, off);
      }
    };
    issue(0, 0);
    float sat = 448.0f;
    asm("" : "+s"(sat));  // no instruction: the bound as a register value (arnorm_sat448)
    for (uint32_t row = 0; row < nrows; ++row) {
      const uint32_t rowOff = row * rowBytes;
      u32x4 zq[UPL];  // the row packed in DT: zq up to rstd, y after it
      float ss = 0.0f;
#pragma unroll
      for (int k0 = 0; k0 < UPL; k0 += PB) {
        if (k0 > 0) issue(rowOff, k0);
#pragma unroll
        for (int i = 0; i < PB; ++i) {
          const int k = k0 + i;
          // zq of the unit, as allreduceRmsNormPullKernel: the fp32 sum over the ranks in rank order, plus the
          // residual where there is one, rounded once
          float acc[8];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t w = raw[i][0][j];
            acc[2 * j] = arnorm_lo<DT>(w);
            acc[2 * j + 1] = arnorm_hi<DT>(w);
          }
#pragma unroll
          for (int p = 1; p < kMaxRanks; ++p)
            if (p < n) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const uint32_t w = raw[i][p][j];
                acc[2 * j] = acc[2 * j] + arnorm_lo<DT>(w);
                acc[2 * j + 1] = acc[2 * j + 1] + arnorm_hi<DT>(w);
              }
            }
          if (hasRes) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t w = res[i][j];
              acc[2 * j] = fp32_value(acc[2 * j]) + arnorm_lo<DT>(w);
              acc[2 * j + 1] = fp32_value(acc[2 * j + 1]) + arnorm_hi<DT>(w);
            }
          }
          uint32_t z[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) z[j] = arnorm_pack<DT>(fp32_value(acc[2 * j]), fp32_value(acc[2 * j + 1]));
          zq[k] = u32x4{z[0], z[1], z[2], z[3]};
          if (ok[k]) {
            if (hasRes) store16<kPlain>(rro, rowOff + uoff[k], zq[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float e0 = arnorm_lo<DT>(z[j]), e1 = arnorm_hi<DT>(z[j]);
              ss = __builtin_fmaf(e0, e0, ss);
              ss = __builtin_fmaf(e1, e1, ss);
            }
          }
        }
      }
      // the next row's first batch goes out ahead of this row's barrier (all of it at UPL <= 2)
      if (row + 1 < nrows) issue(rowOff + rowBytes, 0);

      // row sum: wave butterfly, one LDS word per wave (double buffered), wave order
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1)
        ss = ss + __builtin_bit_cast(float, arnorm_xor_lane(__builtin_bit_cast(uint32_t, ss), m, t));
      uint32_t* ws = waveWords[row & 1u];
      if ((t & 63u) == 0) ws[t >> 6] = __builtin_bit_cast(uint32_t, ss);
      __syncthreads();
      float total = __builtin_bit_cast(float, ws[0]);
      for (uint32_t wv = 1; wv < T / 64; ++wv) total = total + __builtin_bit_cast(float, ws[wv]);
      const float ms = fp32_product(total, a.invCols);
      const float rstd = __builtin_amdgcn_rsqf(fp32_value(ms + a.eps));

      // pass 2, per unit: y over zq's registers, the block's amax and E, the conversion, the stores
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        // cols % 32 == 0 is upr % 4 == 0 (the host's check): the four slots of a quad, units 4 m .. 4 m + 3 of
        // the row, are all live or all dead, so every lane the quad's DPP moves read from is active here.
        if (!ok[k]) continue;
        uint32_t y[4];
        arnorm_u16x2 am2 = {0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t z = zq[k][j];
          uint32_t gw = gam[k][j];
          asm volatile("" : "+v"(gw));  // no instruction: gamma is decoded here, per row, and stays packed across rows
          const float lo = fp32_product(fp32_product(arnorm_lo<DT>(z), rstd), arnorm_lo<DT>(gw));
          const float hi = fp32_product(fp32_product(arnorm_hi<DT>(z), rstd), arnorm_hi<DT>(gw));
          y[j] = arnorm_pack<DT>(lo, hi);
          am2 = __builtin_elementwise_max(am2, __builtin_bit_cast(arnorm_u16x2, y[j] & 0x7fff7fffu));
        }
        const uint32_t am = arnorm_quad_max(am2.x > am2.y ? am2.x : am2.y);
        // E: the exponent field of amax as fp32 (an exact conversion), less emax, not below 0
        const uint32_t e32 = __builtin_bit_cast(uint32_t, arnorm_lo<DT>(am)) >> 23;
        const uint32_t E = e32 > kEmax ? e32 - kEmax : 0u;
        const uint32_t qoff = (rowOff + uoff[k]) >> kQShift;
        if constexpr (FMT == kMxFp8) {
          const float f = __builtin_bit_cast(float, (254u - E) << 23);  // 2^(127 - E): E <= 247, a normal number
          uint32_t q0 = arnorm_quant2<DT, false>(y[0], f, sat, 0u);
          uint32_t q1 = arnorm_quant2<DT, false>(y[2], f, sat, 0u);
          q0 = arnorm_quant2<DT, true>(y[1], f, sat, q0);
          q1 = arnorm_quant2<DT, true>(y[3], f, sat, q1);
          store8<kPlain>(rq, qoff, u32x2{q0, q1});
        } else {
          const float x = __builtin_bit_cast(float, E << 23);  // the instruction divides by 2^(its exponent field - 127)
          uint32_t q0 = 0u;
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y[0]), arnorm_hi<DT>(y[0]), x, 0);
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y[1]), arnorm_hi<DT>(y[1]), x, 1);
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y[2]), arnorm_hi<DT>(y[2]), x, 2);
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y[3]), arnorm_hi<DT>(y[3]), x, 3);
          store4<kPlain>(rq, qoff, q0);
        }
        if ((t & 3u) == 0)  // unit u = uoff / 16 is the first of block u / 4
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)E, rsc, row * sRowBytes + (uoff[k] >> 6), 0, kPlain);
      }
    }
  }
  trace_stamp(a.trace, 2);

  block_handshake(v, n, rank, b, a.budget);  // every peer's rows of workgroup b are stored and released
  constexpr int U = kArNormPullCopyUnits;
#pragma unroll 1
  for (int k = 1; k < n; ++k) {
    const int q = (rank + k) % n;
    uint32_t qrow0;
    const uint32_t qrows = arNormPullRows(g, (uint32_t)q, b, &qrow0);
    if (!qrows) continue;
    {  // the rows' scale bytes, a descriptor of exactly the range each: [0, head) and [head + mid, slen) by bytes,
       // the middle, where source and destination are both dword aligned, by dwords
      const uint8_t* ssc = (const uint8_t*)a.peerScale[vi][q] + (uint64_t)qrow0 * sRowBytes;
      uint8_t* dsc = a.scale[vi] + (uint64_t)qrow0 * sRowBytes;
      const uint32_t slen = qrows * sRowBytes;
      const uint32_t sa = (uint32_t)(uintptr_t)ssc & 3u, da = (uint32_t)(uintptr_t)dsc & 3u;
      const uint32_t lead = (4u - da) & 3u;
      const uint32_t head = sa != da || lead > slen ? slen : lead;
      const uint32_t mid = (slen - head) & ~3u;
      const auto rs = arnorm_rsrc(ssc, slen);
      const auto rd = arnorm_rsrc(dsc, slen);
      for (uint32_t i = t * 4u; i < mid; i += T * 4u) store4<kPlain>(rd, head + i, load4<kSystem>(rs, head + i));
      for (uint32_t i = t; i < slen - mid; i += T) {
        const uint32_t o = i < head ? i : i + mid;
        __builtin_amdgcn_raw_buffer_store_b8(__builtin_amdgcn_raw_buffer_load_b8(rs, o, 0, kSystem), rd, o, 0, kPlain);
      }
    }
    const uint64_t at = (uint64_t)qrow0 * rowBytes, qat = (uint64_t)qrow0 * qRowBytes;
    const uint32_t len = qrows * rowBytes, qlen = qrows * qRowBytes;
    // (upr % 4 == 0: qlen is whole 16-byte units, a half or a quarter of len's)
    const uint32_t nUnitsQ = qlen / 16u, nUnits = hasRes ? len / 16u : nUnitsQ;
    const auto sq = arnorm_rsrc((const uint8_t*)v.peerOutput[q] + qat, qlen);
    const auto dq = arnorm_rsrc((uint8_t*)v.output + qat, qlen);
    const auto sr = arnorm_rsrc(hasRes ? (const uint8_t*)a.peerResOut[vi][q] + at : nullptr, hasRes ? len : 0u);
    const auto dr = arnorm_rsrc(hasRes ? (uint8_t*)a.resOut[vi] + at : nullptr, hasRes ? len : 0u);
    for (uint32_t u0 = t; u0 < nUnits; u0 += T * U) {
      u32x4 wq[U], wr[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + (uint32_t)i * T;
        if (u < nUnitsQ) wq[i] = load16<kSystem>(sq, u * 16u);
        if (hasRes && u < nUnits) wr[i] = load16<kSystem>(sr, u * 16u);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + (uint32_t)i * T;
        if (u < nUnitsQ) store16<kPlain>(dq, u * 16u, wq[i]);
        if (hasRes && u < nUnits) store16<kPlain>(dr, u * 16u, wr[i]);
      }
    }
  }
  trace_stamp(a.trace, 3);
  block_handshake(v, n, rank, b, a.budget);  // every reader is done with this rank's buffers
  trace_stamp(a.trace, 4);
}

// The checks of a call's arguments, host only: 0, 4 (invalid) or 5, as allReduceRmsNormPullCheck -- which
// judges x, the residual, res_out, gamma, the shape, the lanes and the grid (asked with y == x, the one form in
// which it counts no y of 2-byte elements) -- and then what is new: cols % 32, the format, and on every view a q
// of rows * cols (MXFP8) or rows * cols / 2 (MXFP4) bytes (view.output, 16-byte aligned) and a scale of rows *
// cols / 32 bytes (any alignment) that overlap no buffer of any view.  The descriptor limit is applied to a
// workgroup's range of x, the largest.
int allReduceRmsNormMxPullCheck(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                                void* const* resOut, const void* const* gamma, void* const* scale, size_t rows,
                                size_t cols, int dtype, int format, int& nblocks, int& nthreads, int* upl,
                                ArNormPullGeom* g) {
  if (!views || !scale || nviews < 1 || nviews > kMaxRanks || cols % 32 || (format != kMxFp8 && format != kMxFp4))
    return 4;
  mscclppAmdRankView inPlace[kMaxRanks];
  for (int i = 0; i < nviews; ++i) {
    inPlace[i] = views[i];
    inPlace[i].output = const_cast<void*>(views[i].input);
  }
  if (const int rc = allReduceRmsNormPullCheck(inPlace, nviews, nranks, residual, resOut, gamma, rows, cols, dtype,
                                               nblocks, nthreads, upl, g))
    return rc;
  struct Buf { const void* p; size_t n; };
  Buf all[kMaxRanks * 6];
  int nb = 0, nOut = 0;  // the first nOut are the q and the scales
  for (int i = 0; i < nviews; ++i) {
    if (!views[i].output || !scale[i] || (uintptr_t)views[i].output % 16) return 4;
    all[nb++] = Buf{views[i].output, format == kMxFp8 ? rows * cols : rows * cols / 2};
    all[nb++] = Buf{scale[i], rows * cols / 32};
  }
  nOut = nb;
  for (int i = 0; i < nviews; ++i) {
    all[nb++] = Buf{views[i].input, rows * cols * 2};
    all[nb++] = Buf{gamma[i], cols * 2};
    if (residual && residual[i]) {
      all[nb++] = Buf{residual[i], rows * cols * 2};
      all[nb++] = Buf{resOut[i], rows * cols * 2};
    }
  }
  for (int o = 0; o < nOut; ++o)
    for (int c = o + 1; c < nb; ++c)
      if (arNormOverlap(all[o].p, all[o].n, all[c].p, all[c].n)) return 4;
  return 0;
}

template <int DT, int UPL, int FMT>
static int launchArNormMxPullT(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                               void* const* resOut, void* const* peerResOut, const void* const* gamma,
                               void* const* scale, void* const* peerScale, const ArNormPullGeom& g, float eps,
                               float invCols, int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  auto fill = [&](auto& args) {
    for (int i = 0; i < nviews; ++i) {
      args.residual[i] = residual ? residual[i] : nullptr;
      args.resOut[i] = resOut ? resOut[i] : nullptr;
      args.gamma[i] = gamma[i];
      args.scale[i] = (uint8_t*)scale[i];
      for (int q = 0; q < kMaxRanks; ++q) {
        args.peerResOut[i][q] = args.residual[i] && q < nranks ? peerResOut[i * kMaxRanks + q] : nullptr;
        args.peerScale[i][q] = q < nranks ? peerScale[i * kMaxRanks + q] : nullptr;
      }
    }
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.eps = eps;
    args.invCols = invCols;
    args.nranks = nranks;
    return 0;
  };
  return launchViews(allreduceRmsNormMxPullKernel<DT, UPL, 1, FMT>, allreduceRmsNormMxPullKernel<DT, UPL, kMaxRanks, FMT>,
                     views, nviews, nblocks, nthreads, s, fill);
}

template <int DT, int FMT>
static int launchArNormMxPullDT(int upl, const mscclppAmdRankView* views, int nviews, int nranks,
                                const void* const* residual, void* const* resOut, void* const* peerResOut,
                                const void* const* gamma, void* const* scale, void* const* peerScale,
                                const ArNormPullGeom& g, float eps, float invCols, int nblocks, int nthreads,
                                uint64_t budget, hipStream_t s) {
#define MSCCLPP_AMD_ARNORM_MX_PULL_ARGS \
  views, nviews, nranks, residual, resOut, peerResOut, gamma, scale, peerScale, g, eps, invCols, nblocks, nthreads, budget, s
  switch (upl) {
    case 1: return launchArNormMxPullT<DT, 1, FMT>(MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
    case 2: return launchArNormMxPullT<DT, 2, FMT>(MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
    default: return launchArNormMxPullT<DT, 4, FMT>(MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
  }
}

// 4: invalid, nothing launched and no device touched; 5: a workgroup's range exceeds one descriptor, or the
// grid cannot be resident.  residual / resOut / peerResOut: as launchAllReduceRmsNormPull.  scale: one entry per
// view; peerScale: nviews x kMaxRanks entries, [i * kMaxRanks + q] = rank q's scale as view i has it mapped.
// The views' other fields (tokens, peerInput, peerOutput, ...) are the caller's to check.
int launchAllReduceRmsNormMxPull(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                                 void* const* resOut, void* const* peerResOut, const void* const* gamma,
                                 void* const* scale, void* const* peerScale, size_t rows, size_t cols, int dtype,
                                 int format, float eps, int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  int upl = 0;
  ArNormPullGeom g;
  if (const int rc = allReduceRmsNormMxPullCheck(views, nviews, nranks, residual, resOut, gamma, scale, rows, cols,
                                                 dtype, format, nblocks, nthreads, &upl, &g))
    return rc;
  if (!peerScale || (residual && residual[0] && !peerResOut)) return 4;
  for (int i = 0; i < nviews; ++i)
    for (int q = 0; q < nranks; ++q)
      if (!peerScale[i * kMaxRanks + q] || (residual && residual[0] && !peerResOut[i * kMaxRanks + q])) return 4;
  const float invCols = 1.0f / (float)cols;
  if (format == kMxFp8) {
    if (dtype == kF16) return launchArNormMxPullDT<kF16, kMxFp8>(upl, MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
    return launchArNormMxPullDT<kBF16, kMxFp8>(upl, MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
  }
  if (dtype == kF16) return launchArNormMxPullDT<kF16, kMxFp4>(upl, MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
  return launchArNormMxPullDT<kBF16, kMxFp4>(upl, MSCCLPP_AMD_ARNORM_MX_PULL_ARGS);
}

}  // namespace mscclpp_amd
