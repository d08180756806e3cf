// Fused AllReduce + residual add + RMSNorm whose normalised rows leave as OCP FP8 e4m3 with one fp32 scale per
// row: allreduce_rmsnorm_pull.hip's two-shot zero-copy pull with a dynamic per-row quantisation behind it
// (DESIGN.md §17k).  Steps 1-4 are §17i's, in §17j's order (so res_out, and y before it is quantised, are that
// kernel's bits at the same (cols, nthreads)); then
//
//   amax  = max_j |y_j|                  of the ROUNDED y (DT)
//   scale = max(amax / 448, 2^-126)      fp32, correctly rounded; stored to scale[row]
//   inv   = 1 / scale                    fp32, correctly rounded
//   q_j   = e4m3(clamp(y_j * inv, +-448)) one fp32 product, clamped, rounded once (RNE); one byte at q[row][j]
//
//  * The geometry, the three handshakes, the visibility discipline and the descriptors are §17j's: rank q owns
//    rows [q R, (q + 1) R), workgroup b of every rank the same row range of every slice.  A row is cols / 8 lane
//    units: 16 bytes of x and res_out, 8 bytes of q; cols % 16 == 0 keeps every row of q, and so every
//    workgroup's range of it, whole 16-byte units.
//  * Phase 1, per row: the loads, the rank-order sum, the residual, the rounding, the res_out store, the sum of
//    squares and rstd exactly as §17j, the prefetch of row i + 1's first batch ahead of the first barrier
//    included.  Pass 2 writes y, packed in DT, over the registers that held zq and takes the lane's amax as an
//    unsigned 16-bit maximum of the sign-cleared patterns (v_pk_max_u16; exact for every finite value, and a
//    maximum has no order).  Wave butterfly, one LDS word per wave in a second array (double buffered by the
//    row's parity like the first), a second barrier.  Pass 3 decodes y, multiplies by inv, clamps, converts two
//    pairs per word (v_cvt_pk_fp8_f32) and stores the unit's 8 bytes -- contiguous across the lanes.  Lane 0
//    stores the row's scale.
//  * Phase 2: workgroup b's range of every other slice of q (16-byte units), its rows' scales (dwords, out of
//    peerScale[q]) and, with a residual, its range of res_out are copied from their owners: system-scope loads,
//    plain stores.  q holds half of y's bytes, so every second batch of the loop carries res_out alone.
//  * q and scale overlap nothing; res_out == residual is carried as in §17j.  A row whose y holds a NaN or an
//    infinity has an unspecified q and scale; its res_out and its neighbours are as defined.
//    Trace stamps: 0 start, 1 entry handshake done, 2 own rows quantised, 3 peers' rows gathered, 4 end.
#include "allreduce_rmsnorm.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

template <int NV>
struct ArNormQuantPullArgs {
  Views<NV> views;           // output: q
  const void* residual[NV];  // null on every view, or on none
  void* resOut[NV];
  const void* gamma[NV];
  float* scale[NV];
  const void* peerResOut[NV][kMaxRanks];  // rank q's res_out as this view has it mapped
  const void* peerScale[NV][kMaxRanks];   // ... and its scale
  ArNormPullGeom g;
  uint64_t budget;
  uint64_t* trace;
  float eps;
  float invCols;  // 1.0f / (float)cols, computed once by the host
  int nranks;
  int pad;
};
static_assert(sizeof(ArNormQuantPullArgs<kMaxRanks>) <= 4096,
              "in-process AllReduce+RMSNorm quantising pull arguments exceed the kernel-argument limit");

// Four waves per SIMD (at most 128 VGPRs), as allreduceRmsNormPullKernel.
template <int DT, int UPL, int NV>
__global__ void __launch_bounds__(512, 4) allreduceRmsNormQuantPullKernel(ArNormQuantPullArgs<NV> a) {
  // units whose loads are in flight together: (ranks + residual) x 4 VGPRs each
  constexpr int PB = UPL == 2 ? 2 : 1;
  __shared__ uint32_t waveWords[2][2][8];  // [the row's parity][sum of squares, amax][wave]: 128 bytes
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const ArNormPullGeom& g = a.g;
  const uint32_t T = blockDim.x, t = threadIdx.x, b = blockIdx.x;
  const uint32_t rowBytes = g.upr * 16u, qRowBytes = g.upr * 8u;
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
    const auto rsc = arnorm_rsrc(a.scale[vi] + row0, nrows * 4u);
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
      // the next row's first batch goes out ahead of this row's barriers (all of it at UPL <= 2)
      if (row + 1 < nrows) issue(rowOff + rowBytes, 0);

      // row sum: wave butterfly, one LDS word per wave (double buffered), wave order
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1)
        ss = ss + __builtin_bit_cast(float, arnorm_xor_lane(__builtin_bit_cast(uint32_t, ss), m, t));
      uint32_t* ws = waveWords[row & 1u][0];
      if ((t & 63u) == 0) ws[t >> 6] = __builtin_bit_cast(uint32_t, ss);
      __syncthreads();
      float total = __builtin_bit_cast(float, ws[0]);
      for (uint32_t wv = 1; wv < T / 64; ++wv) total = total + __builtin_bit_cast(float, ws[wv]);
      const float ms = fp32_product(total, a.invCols);
      const float rstd = __builtin_amdgcn_rsqf(fp32_value(ms + a.eps));

      // pass 2: y over zq's registers, and the lane's amax of the sign-cleared patterns
      arnorm_u16x2 am2 = {0, 0};
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        if (!ok[k]) continue;
        uint32_t y[4];
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
        zq[k] = u32x4{y[0], y[1], y[2], y[3]};
      }
      // row amax: wave butterfly, one LDS word per wave (double buffered), a second barrier
      uint32_t am = am2.x > am2.y ? am2.x : am2.y;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = arnorm_xor_lane(am, m, t);
        am = am > o ? am : o;
      }
      uint32_t* wm = ws + 8;
      if ((t & 63u) == 0) wm[t >> 6] = am;
      __syncthreads();
      am = wm[0];
      for (uint32_t wv = 1; wv < T / 64; ++wv) am = am > wm[wv] ? am : wm[wv];
      // both divisions are plain fp32 divisions, correctly rounded (the full expansion, no bare v_rcp_f32)
      const float amax = arnorm_lo<DT>(am);
      const float scale = fmaxf(amax / 448.0f, 0x1p-126f);
      const float inv = 1.0f / scale;
      if (t == 0) store4<kPlain>(rsc, row * 4u, __builtin_bit_cast(uint32_t, scale));

      // pass 3: the unit's 8 bytes of q
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        if (!ok[k]) continue;
        uint32_t q0 = arnorm_quant2<DT, false>(zq[k][0], inv, sat, 0u);
        uint32_t q1 = arnorm_quant2<DT, false>(zq[k][2], inv, sat, 0u);
        q0 = arnorm_quant2<DT, true>(zq[k][1], inv, sat, q0);
        q1 = arnorm_quant2<DT, true>(zq[k][3], inv, sat, q1);
        store8<kPlain>(rq, (rowOff + uoff[k]) >> 1, u32x2{q0, q1});  // 8 bytes of q per 16 of x
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
    {  // the rows' scales: one dword per lane and round
      const auto ssc = arnorm_rsrc((const float*)a.peerScale[vi][q] + qrow0, qrows * 4u);
      const auto dsc = arnorm_rsrc(a.scale[vi] + qrow0, qrows * 4u);
      for (uint32_t i = t; i < qrows; i += T) store4<kPlain>(dsc, i * 4u, load4<kSystem>(ssc, i * 4u));
    }
    const uint64_t at = (uint64_t)qrow0 * rowBytes, qat = (uint64_t)qrow0 * qRowBytes;
    const uint32_t len = qrows * rowBytes, qlen = qrows * qRowBytes;
    const uint32_t nUnitsQ = qlen / 16u, nUnits = hasRes ? len / 16u : nUnitsQ;  // (upr is even: len / 16 = 2 nUnitsQ)
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
// which it counts no y of 2-byte elements) -- and then what is new: cols % 16, and on every view a q of rows *
// cols bytes (view.output, 16-byte aligned) and a scale of rows * 4 bytes (4-byte aligned) that overlap no
// buffer of any view.  The descriptor limit is applied to a workgroup's range of x, the largest.
int allReduceRmsNormQuantPullCheck(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                                   void* const* resOut, const void* const* gamma, void* const* scale, size_t rows,
                                   size_t cols, int dtype, int& nblocks, int& nthreads, int* upl, ArNormPullGeom* g) {
  if (!views || !scale || nviews < 1 || nviews > kMaxRanks || cols % 16) return 4;
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
    if (!views[i].output || !scale[i] || (uintptr_t)views[i].output % 16 || (uintptr_t)scale[i] % 4) return 4;
    all[nb++] = Buf{views[i].output, rows * cols};
    all[nb++] = Buf{scale[i], rows * 4};
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

template <int DT, int UPL>
static int launchArNormQuantPullT(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                                  void* const* resOut, void* const* peerResOut, const void* const* gamma,
                                  void* const* scale, void* const* peerScale, const ArNormPullGeom& g, float eps,
                                  float invCols, int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  auto fill = [&](auto& args) {
    for (int i = 0; i < nviews; ++i) {
      args.residual[i] = residual ? residual[i] : nullptr;
      args.resOut[i] = resOut ? resOut[i] : nullptr;
      args.gamma[i] = gamma[i];
      args.scale[i] = (float*)scale[i];
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
  return launchViews(allreduceRmsNormQuantPullKernel<DT, UPL, 1>, allreduceRmsNormQuantPullKernel<DT, UPL, kMaxRanks>,
                     views, nviews, nblocks, nthreads, s, fill);
}

template <int DT>
static int launchArNormQuantPullDT(int upl, const mscclppAmdRankView* views, int nviews, int nranks,
                                   const void* const* residual, void* const* resOut, void* const* peerResOut,
                                   const void* const* gamma, void* const* scale, void* const* peerScale,
                                   const ArNormPullGeom& g, float eps, float invCols, int nblocks, int nthreads,
                                   uint64_t budget, hipStream_t s) {
#define MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS \
  views, nviews, nranks, residual, resOut, peerResOut, gamma, scale, peerScale, g, eps, invCols, nblocks, nthreads, budget, s
  switch (upl) {
    case 1: return launchArNormQuantPullT<DT, 1>(MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS);
    case 2: return launchArNormQuantPullT<DT, 2>(MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS);
    default: return launchArNormQuantPullT<DT, 4>(MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS);
  }
}

// 4: invalid, nothing launched and no device touched; 5: a workgroup's range exceeds one descriptor, or the
// grid cannot be resident.  residual / resOut / peerResOut: as launchAllReduceRmsNormPull.  scale: one entry per
// view; peerScale: nviews x kMaxRanks entries, [i * kMaxRanks + q] = rank q's scale as view i has it mapped.
// The views' other fields (tokens, peerInput, peerOutput, ...) are the caller's to check.
int launchAllReduceRmsNormQuantPull(const mscclppAmdRankView* views, int nviews, int nranks,
                                    const void* const* residual, void* const* resOut, void* const* peerResOut,
                                    const void* const* gamma, void* const* scale, void* const* peerScale, size_t rows,
                                    size_t cols, int dtype, float eps, int nblocks, int nthreads, uint64_t budget,
                                    hipStream_t s) {
  int upl = 0;
  ArNormPullGeom g;
  if (const int rc = allReduceRmsNormQuantPullCheck(views, nviews, nranks, residual, resOut, gamma, scale, rows, cols,
                                                    dtype, nblocks, nthreads, &upl, &g))
    return rc;
  if (!peerScale || (residual && residual[0] && !peerResOut)) return 4;
  for (int i = 0; i < nviews; ++i)
    for (int q = 0; q < nranks; ++q)
      if (!peerScale[i * kMaxRanks + q] || (residual && residual[0] && !peerResOut[i * kMaxRanks + q])) return 4;
  const float invCols = 1.0f / (float)cols;
  if (dtype == kF16) return launchArNormQuantPullDT<kF16>(upl, MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS);
  return launchArNormQuantPullDT<kBF16>(upl, MSCCLPP_AMD_ARNORM_QUANT_PULL_ARGS);
}

}  // namespace mscclpp_amd
