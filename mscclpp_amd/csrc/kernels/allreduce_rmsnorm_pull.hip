// Fused AllReduce + residual add + RMSNorm of fp16 / bf16 rows for prefill sizes: a two-shot zero-copy pull
// (DESIGN.md §17j).  The operation is allreduce_rmsnorm_ll.hip's, steps 1-4 of §17i, unchanged:
//
//   s   = x_0 + x_1 + ... + x_{n-1}     fp32, operands in RANK order, one RNE add each
//   zq  = (DT)(s + residual)            one fp32 add, rounded once (RNE); stored as res_out.  No residual: (DT)s
//   ms  = (sum_j zq_j^2) * invCols      fp32, of the ROUNDED zq; invCols = 1.0f / cols from the host
//   y_j = (DT)((zq_j * rstd) * gamma_j) fp32, rounded once; rstd = v_rsq_f32(ms + eps)
//
// but every row is reduced, added to and normalised ONCE, by the rank that owns it, and then copied:
//
//  * Rows over ranks: R = ceil(rows / n); rank q owns rows [q R, min((q + 1) R, rows)) -- the last owner's
//    slice may be short, and with rows < n some ranks own nothing.
//  * Rows over workgroups: workgroup b of EVERY rank owns rows [b rpb, (b + 1) rpb) of each slice, rpb =
//    ceil(R / gridDim.x): one contiguous byte range of y and res_out per slice, and the peers' workgroup b
//    is the only one it ever waits for (channel b, as pullReduceKernel).  Every workgroup takes all three
//    handshakes, also one without a row.
//  * Entry handshake (every x is final), then phase 1 over the own slice, row by row.  A row is cols / 8
//    units of 16 bytes; lane t owns units t, t + T, ..., at most UPL of them (1, 2 or 4, from cols and T).
//    PB units at a time, the own x and the residual by plain local loads and every peer's x by
//    load16<kSystem> out of peerInput[k], all issued before any arithmetic; then per unit the fp32 sum in
//    rank order, the residual, one rounding -- the row stays packed in DT, 4 VGPRs per unit -- the plain
//    store of res_out and the lane's fma chain over zq^2 (units and elements ascending).  The first batch of
//    row i + 1 is issued ahead of row i's barrier.  Row sum: wave butterfly (__shfl_xor 32, ..., 1), one LDS
//    word per wave, double buffered by the row's parity, ONE barrier, the wave words added in wave order:
//    the order is a function of (cols, T) alone.  Second pass over the packed registers with the lane's
//    gamma words (loaded once, before the entry handshake), plain stores of y.
//  * Middle handshake (every peer's rows of workgroup b are stored and released), then phase 2: for q =
//    rank + 1, ... (mod n) workgroup b's byte range of q's slice is copied out of peerOutput[q] into y, and
//    with a residual out of q's res_out (peerResOut[q]) into res_out -- load16<kSystem>, plain stores,
//    kCopyUnits units per lane and buffer in flight.  Nothing is ever written to a peer.
//  * Exit handshake: every reader is done with this rank's x, y and res_out.
//  * Visibility is pullReduceKernel's discipline (pull_reduce.hip): plain stores, the drain and barrier inside
//    block_handshake, a system-scope release before the token add, sc0 sc1 loads after the acquire.
//  * In place: before the middle handshake a rank writes only its own slice of y and res_out, which no peer
//    reads as x (a peer reads ITS slice of this rank's x) and whose residual rows only this rank reads; after
//    it, workgroup b writes range b of the other slices, which the owners' workgroup b -- the one it has just
//    met -- has finished reading.  So y == x and res_out == residual are carried; the host refuses any other
//    overlap.
//  * Every buffer is addressed through a descriptor rebased to the workgroup's range (64-bit) and of exactly
//    its length, with 32-bit offsets inside it; a unit slot past the row's end loads the row's last unit
//    (unused) and stores nothing.
//    Trace stamps: 0 start, 1 entry handshake done, 2 own rows normalised, 3 peers' rows gathered, 4 end.
#include "allreduce_rmsnorm.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

template <int NV>
struct ArNormPullArgs {
  Views<NV> views;
  const void* residual[NV];  // null on every view, or on none
  void* resOut[NV];
  const void* gamma[NV];
  const void* peerResOut[NV][kMaxRanks];  // rank q's res_out as this view has it mapped
  ArNormPullGeom g;
  uint64_t budget;
  uint64_t* trace;
  float eps;
  float invCols;  // 1.0f / (float)cols, computed once by the host
  int nranks;
  int pad;
};
static_assert(sizeof(ArNormPullArgs<kMaxRanks>) <= 4096, "in-process AllReduce+RMSNorm pull arguments exceed the kernel-argument limit");

// Four waves per SIMD (at most 128 VGPRs): 8 in-process ranks x 64 workgroups of 512 lanes stay co-resident.
template <int DT, int UPL, int NV>
__global__ void __launch_bounds__(512, 4) allreduceRmsNormPullKernel(ArNormPullArgs<NV> a) {
  // units whose loads are in flight together: (ranks + residual) x 4 VGPRs each
  constexpr int PB = UPL == 2 ? 2 : 1;
  __shared__ float waveSum[2][8];
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const ArNormPullGeom& g = a.g;
  const uint32_t T = blockDim.x, t = threadIdx.x, b = blockIdx.x;
  const uint32_t rowBytes = g.upr * 16u;
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
    const uint32_t len = nrows * rowBytes;  // <= kBlkOffsetLimit (the host)
    const auto rx = arnorm_rsrc((const uint8_t*)v.input + at, len);
    const auto ry = arnorm_rsrc((uint8_t*)v.output + at, len);
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
    for (uint32_t row = 0; row < nrows; ++row) {
      const uint32_t rowOff = row * rowBytes;
      u32x4 zq[UPL];
      float ss = 0.0f;
#pragma unroll
      for (int k0 = 0; k0 < UPL; k0 += PB) {
        if (k0 > 0) issue(rowOff, k0);
#pragma unroll
        for (int i = 0; i < PB; ++i) {
          const int k = k0 + i;
          // zq of the unit: the fp32 sum over the ranks in rank order, plus the residual where there is
          // one, rounded once.  (The words are copied out of the vectors first: see bench_add2 in
          // allreduce_ll.hip.)
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

      // row sum: wave butterfly, one LDS word per wave (double buffered: one barrier per row), wave order
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
      float* ws = waveSum[row & 1u];
      if ((t & 63u) == 0) ws[t >> 6] = ss;
      __syncthreads();
      float total = ws[0];
      for (uint32_t wv = 1; wv < T / 64; ++wv) total = total + ws[wv];
      const float ms = fp32_product(total, a.invCols);
      const float rstd = __builtin_amdgcn_rsqf(fp32_value(ms + a.eps));

      // second pass over the packed registers
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        if (!ok[k]) continue;
        uint32_t y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t z = zq[k][j], gw = gam[k][j];
          const float lo = fp32_product(fp32_product(arnorm_lo<DT>(z), rstd), arnorm_lo<DT>(gw));
          const float hi = fp32_product(fp32_product(arnorm_hi<DT>(z), rstd), arnorm_hi<DT>(gw));
          y[j] = arnorm_pack<DT>(lo, hi);
        }
        store16<kPlain>(ry, rowOff + uoff[k], u32x4{y[0], y[1], y[2], y[3]});
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
    const uint64_t at = (uint64_t)qrow0 * rowBytes;
    const uint32_t len = qrows * rowBytes, nUnits = len / 16u;
    const auto sy = arnorm_rsrc((const uint8_t*)v.peerOutput[q] + at, len);
    const auto dy = arnorm_rsrc((uint8_t*)v.output + at, len);
    const auto sr = arnorm_rsrc(hasRes ? (const uint8_t*)a.peerResOut[vi][q] + at : nullptr, hasRes ? len : 0u);
    const auto dr = arnorm_rsrc(hasRes ? (uint8_t*)a.resOut[vi] + at : nullptr, hasRes ? len : 0u);
    for (uint32_t u0 = t; u0 < nUnits; u0 += T * U) {
      u32x4 wy[U], wr[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + (uint32_t)i * T;
        if (u >= nUnits) continue;
        wy[i] = load16<kSystem>(sy, u * 16u);
        if (hasRes) wr[i] = load16<kSystem>(sr, u * 16u);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + (uint32_t)i * T;
        if (u >= nUnits) continue;
        store16<kPlain>(dy, u * 16u, wy[i]);
        if (hasRes) store16<kPlain>(dr, u * 16u, wr[i]);
      }
    }
  }
  trace_stamp(a.trace, 3);
  block_handshake(v, n, rank, b, a.budget);  // every reader is done with this rank's buffers
  trace_stamp(a.trace, 4);
}

// The default grid: a function of (nranks, rows, cols) alone, so every rank derives the same one: 32 KiB of a
// rank's slice per workgroup, 8 .. 32, and at most R.  Read off the in-process measurement of DESIGN.md §17j (8
// ranks on one GPU): 8 workgroups at 1 MiB, 16 at 4 MiB and 32 at 8 and 32 MiB were the fastest grids tried,
// and 64 -- where 8 ranks x 64 workgroups are two per CU of the one GPU measured -- lost at every size (a rank
// alone on its GPU may want more, which nobody has measured).
int allReduceRmsNormPullDefaultBlocks(int nranks, uint64_t rows, uint64_t cols) {
  const uint64_t slice = (rows + (uint64_t)nranks - 1) / (uint64_t)nranks;
  uint64_t want = (slice * cols * 2 + (32u << 10) - 1) / (32u << 10);
  want = want < 8 ? 8 : want > 32 ? 32 : want;
  return (int)(want < slice ? want : slice ? slice : 1);
}

// The checks of a call's arguments, host only: 0, 4 (invalid) or 5 (a workgroup's range exceeds one
// descriptor); the views' input / output are the only fields read.  nthreads and nblocks come back as the
// launch takes them, *upl as its units per lane, *g as its geometry.  There is no byte cap and no scratch.
int allReduceRmsNormPullCheck(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                              void* const* resOut, const void* const* gamma, size_t rows, size_t cols, int dtype,
                              int& nblocks, int& nthreads, int* upl, ArNormPullGeom* g) {
  if (!views || !gamma || nviews < 1 || nviews > kMaxRanks || nranks < 2 || nranks > kMaxRanks) return 4;
  if (rows == 0 || cols == 0 || cols % 8 || (dtype != kF16 && dtype != kBF16)) return 4;
  // the lane limit: at most 4 units per lane, at the lanes asked for (default: 256, or 512 above 8192 columns)
  if (nthreads <= 0) nthreads = cols > 8192 ? 512 : 256;
  if (!launchShapeOk(nblocks, kMaxChannels, nthreads)) return 4;
  const uint64_t upr = cols / 8, perLane = (upr + nthreads - 1) / nthreads;
  if (perLane > (uint64_t)kArNormPullMaxUPL) return 4;
  if (upl) *upl = perLane <= 1 ? 1 : perLane <= 2 ? 2 : 4;
  const uint64_t counted = rows > (1ull << 32) ? (1ull << 32) : (uint64_t)rows;  // (no overflow: cols is bounded)
  if (!arNormBuffersOk(views, nviews, residual, resOut, gamma, counted * cols * 2, cols, 16)) return 4;
  if (rows > 0x7fffffffull) return 5;
  if (nblocks <= 0) nblocks = allReduceRmsNormPullDefaultBlocks(nranks, rows, cols);
  ArNormPullGeom geom;
  geom.rows = (uint32_t)rows;
  geom.upr = (uint32_t)upr;
  geom.slice = (uint32_t)((rows + (uint64_t)nranks - 1) / (uint64_t)nranks);
  geom.rpb = (geom.slice + (uint32_t)nblocks - 1) / (uint32_t)nblocks;
  if ((uint64_t)geom.rpb * cols * 2 > kBlkOffsetLimit) return 5;  // more workgroups carry it
  if (g) *g = geom;
  return 0;
}

template <int DT, int UPL>
static int launchArNormPullT(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                             void* const* resOut, void* const* peerResOut, const void* const* gamma,
                             const ArNormPullGeom& g, float eps, float invCols, int nblocks, int nthreads, uint64_t budget,
                             hipStream_t s) {
  auto fill = [&](auto& args) {
    for (int i = 0; i < nviews; ++i) {
      args.residual[i] = residual ? residual[i] : nullptr;
      args.resOut[i] = resOut ? resOut[i] : nullptr;
      args.gamma[i] = gamma[i];
      for (int q = 0; q < kMaxRanks; ++q)
        args.peerResOut[i][q] = args.residual[i] && q < nranks ? peerResOut[i * kMaxRanks + q] : nullptr;
    }
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.eps = eps;
    args.invCols = invCols;
    args.nranks = nranks;
    return 0;
  };
  return launchViews(allreduceRmsNormPullKernel<DT, UPL, 1>, allreduceRmsNormPullKernel<DT, UPL, kMaxRanks>, views,
                     nviews, nblocks, nthreads, s, fill);
}

template <int DT>
static int launchArNormPullDT(int upl, const mscclppAmdRankView* views, int nviews, int nranks,
                              const void* const* residual, void* const* resOut, void* const* peerResOut,
                              const void* const* gamma, const ArNormPullGeom& g, float eps, float invCols, int nblocks,
                              int nthreads, uint64_t budget, hipStream_t s) {
#define MSCCLPP_AMD_ARNORM_PULL_ARGS \
  views, nviews, nranks, residual, resOut, peerResOut, gamma, g, eps, invCols, nblocks, nthreads, budget, s
  switch (upl) {
    case 1: return launchArNormPullT<DT, 1>(MSCCLPP_AMD_ARNORM_PULL_ARGS);
    case 2: return launchArNormPullT<DT, 2>(MSCCLPP_AMD_ARNORM_PULL_ARGS);
    default: return launchArNormPullT<DT, 4>(MSCCLPP_AMD_ARNORM_PULL_ARGS);
  }
}

// 4: invalid, nothing launched and no device touched; 5: a workgroup's range exceeds one descriptor, or the
// grid cannot be resident.  residual / resOut: null, or host arrays with one entry per view, all null or
// none; peerResOut: with a residual, nviews x kMaxRanks entries, [i * kMaxRanks + q] = rank q's res_out as
// view i has it mapped.  The views' other fields (tokens, peerInput, peerOutput, ...) are the caller's to check.
int launchAllReduceRmsNormPull(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                               void* const* resOut, void* const* peerResOut, const void* const* gamma, size_t rows,
                               size_t cols, int dtype, float eps, int nblocks, int nthreads, uint64_t budget,
                               hipStream_t s) {
  int upl = 0;
  ArNormPullGeom g;
  if (const int rc = allReduceRmsNormPullCheck(views, nviews, nranks, residual, resOut, gamma, rows, cols, dtype, nblocks,
                                               nthreads, &upl, &g))
    return rc;
  if (residual && residual[0]) {
    if (!peerResOut) return 4;
    for (int i = 0; i < nviews; ++i)
      for (int q = 0; q < nranks; ++q)
        if (!peerResOut[i * kMaxRanks + q]) return 4;
  }
  const float invCols = 1.0f / (float)cols;
  if (dtype == kF16) return launchArNormPullDT<kF16>(upl, MSCCLPP_AMD_ARNORM_PULL_ARGS);
  return launchArNormPullDT<kBF16>(upl, MSCCLPP_AMD_ARNORM_PULL_ARGS);
}

}  // namespace mscclpp_amd
