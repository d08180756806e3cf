// Fused small AllReduce + residual add + RMSNorm of fp16 / bf16 rows: one hop of LL8 packets, the
// protocol of pullReduceLLKernel (pull_reduce_ll.hip), with the row normalised in the registers of the
// lanes that reduced it.  Every rank k holds x_k[rows][cols], a replicated
// residual[rows][cols] (or none), a replicated gamma[cols] and eps; every rank ends with
//
//   s   = x_0 + x_1 + ... + x_{n-1}     fp32, operands in RANK order (pull_reduce_device.hpp), one RNE add each
//   zq  = (DT)(s + residual)            one fp32 add, rounded once (RNE); stored as res_out.  No residual: (DT)s
//   ms  = (sum_j zq_j^2) * invCols      fp32, of the ROUNDED zq; invCols = 1.0f / cols from the host
//   y_j = (DT)((zq_j * rstd) * gamma_j) fp32, rounded once; rstd = v_rsq_f32(ms + eps)
//
//  * Workgroups own ROWS: workgroup b takes rows b, b + gridDim.x, ...  A row is cols / 4 packet units
//    (8 payload bytes = 4 elements <-> one 16-byte unit {w0, flag, w1, flag}, ll_units.hpp); lane t owns
//    units t, t + T, ... of the row, at most UPL of them (UPL in {1, 2, 4, 8}, from cols and T).
//  * Per row: the lane's own payload loads are issued and put into region `rank` of every peer's half;
//    then, PB units at a time, the residual loads and the first poll of all peer regions are issued before
//    any compare (poll_issue / poll_eval), units that missed take the bounded unit_wait, and the unit is
//    reduced in rank order, the residual added, rounded and kept packed (2 VGPRs per unit) while zq^2 is
//    accumulated per lane (fma, units in ascending order).  res_out is stored as soon as zq exists.
//  * Row sum: lane partial -> wave butterfly (__shfl_xor 32, 16, ..., 1) -> one LDS word per wave, double
//    buffered by the row's parity -> one barrier -> every lane adds the wave words in wave order.  The
//    order depends on (cols, T) alone, never on rank, grid or timing, so every rank gets the same bits.
//  * Second pass over the packed registers: decode, scale by rstd and the lane's gamma words (loaded once
//    per workgroup, before the first poll; per row at UPL = 8, see kGammaOnce), round, store y.
//  * A lane stores only units it has loaded itself and no peer reads user memory, so y == x and
//    res_out == residual are carried.  Every user buffer, every peer's region (the puts) and the own half
//    on the waiting path are addressed through a buffer resource of exactly their length, so the hardware
//    clips any offset outside them; the first poll (poll_issue: the whole 32-bit range over the half) is
//    held inside the n regions by its offsets alone (p < n, the unit at or below the message's last).
//  * Every workgroup, also one without a row, ends in bump_flags.  The two scratch halves are safe to
//    reuse by the argument of pull_reduce_ll.hip: rows >= 1, so every rank polls a packet of every other
//    rank in every call.  The scratch and the flags are the communicator's, shared with the other LL kernels.
//    Trace stamps (of the workgroup's last row): 0 start, 1 puts issued, 2 reduced, 3 normalised.
#include "allreduce_rmsnorm.hpp"
#include "launch.hpp"
#include "ll_units.hpp"

#include <stdlib.h>

namespace mscclpp_amd {

// The one statement of the geometry; the launcher and the scratch requirement both use it.
struct ArNormGeom {
  uint32_t rows;
  uint32_t upr;     // packet units per row = cols / 4
  uint32_t region;  // bytes one source rank occupies in a scratch half = rows * upr * 16
  uint32_t bytes;   // of one [rows][cols] buffer
  uint64_t half;    // the n regions, rounded up to 256 bytes; the scratch is two of them
};

constexpr uint64_t kArNormMaxBytes = 1ull << 20;  // the reference's LL bound (kLLOffsetLimit's comment)
constexpr int kArNormMaxUPL = 8;

static bool arNormGeometry(int nranks, uint64_t rows, uint64_t cols, int dtype, ArNormGeom* out) {
  if (nranks < 2 || nranks > kMaxRanks || rows == 0 || cols == 0 || cols % 4) return false;
  if (dtype != kF16 && dtype != kBF16) return false;
  if (cols > 512ull * 4 * kArNormMaxUPL || rows > kArNormMaxBytes || rows * cols * 2 > kArNormMaxBytes) return false;
  ArNormGeom g{};
  g.rows = (uint32_t)rows;
  g.upr = (uint32_t)(cols / 4);
  g.region = g.rows * g.upr * 16u;
  g.bytes = g.rows * g.upr * 8u;
  g.half = ((uint64_t)nranks * g.region + 255) & ~255ull;
  *out = g;
  return true;
}

size_t allReduceRmsNormScratchRequired(int nranks, size_t rows, size_t cols, int dtype) {
  ArNormGeom g;
  return arNormGeometry(nranks, rows, cols, dtype, &g) ? (size_t)(2 * g.half) : 0;
}

// MSCCLPP_AMD_ARNORM_MAX_BYTES: the largest rows * cols * 2 the call carries; 0 refuses every call; read
// once; values above 1 MiB count as 1 MiB, which is also the default.
static uint64_t arNormMaxBytes() {
  static const uint64_t v = [] {
    const char* e = getenv("MSCCLPP_AMD_ARNORM_MAX_BYTES");
    if (!e || !*e || *e == '-') return kArNormMaxBytes;
    char* end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e) return kArNormMaxBytes;
    return (uint64_t)(x > kArNormMaxBytes ? kArNormMaxBytes : x);
  }();
  return v;
}

template <int NV>
struct ArNormArgs {
  Views<NV> views;
  const void* residual[NV];  // null on every view, or on none
  void* resOut[NV];
  const void* gamma[NV];
  ArNormGeom g;
  uint64_t budget;
  uint64_t* trace;
  float eps;
  float invCols;  // 1.0f / (float)cols, computed once by the host
  int nranks;
  int pad;
};
static_assert(sizeof(ArNormArgs<kMaxRanks>) <= 4096, "in-process AllReduce+RMSNorm arguments exceed the kernel-argument limit");

// zq of one word: the fp32 sum over the ranks in rank order (x[p] is rank p's word, `own` at position
// rank), plus the residual word where there is one, rounded once.
template <int DT>
__device__ __forceinline__ uint32_t arnorm_word(const uint32_t* x, int n, bool hasRes, uint32_t res) {
  float lo = arnorm_lo<DT>(x[0]), hi = arnorm_hi<DT>(x[0]);
#pragma unroll
  for (int p = 1; p < kMaxRanks; ++p)
    if (p < n) {
      lo = lo + arnorm_lo<DT>(x[p]);
      hi = hi + arnorm_hi<DT>(x[p]);
    }
  if (hasRes) {
    lo = fp32_value(lo) + arnorm_lo<DT>(res);
    hi = fp32_value(hi) + arnorm_hi<DT>(res);
  }
  return arnorm_pack<DT>(fp32_value(lo), fp32_value(hi));
}

// Four waves per SIMD (at most 128 VGPRs): 8 in-process ranks x the default grid stay co-resident.
template <int DT, int UPL, int NV>
__global__ void __launch_bounds__(512, 4) allreduceRmsNormLLKernel(ArNormArgs<NV> a) {
  // units whose first polls are in flight together: 32 VGPRs of raw packets each
  constexpr int PB = UPL == 2 ? 2 : 1;
  __shared__ float waveSum[2][8];
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const ArNormGeom& g = a.g;
  const uint32_t T = blockDim.x, G = gridDim.x, t = threadIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const bool hasRes = a.residual[vi] != nullptr;
  const auto rx = arnorm_rsrc(v.input, g.bytes);
  const auto ry = arnorm_rsrc(v.output, g.bytes);
  const auto rres = arnorm_rsrc(a.residual[vi], hasRes ? g.bytes : 0u);
  const auto rro = arnorm_rsrc(a.resOut[vi], hasRes ? g.bytes : 0u);
  const auto rgam = arnorm_rsrc(a.gamma[vi], g.upr * 8u);
  trace_stamp(a.trace, 0);
  const uint32_t flagv = __hip_atomic_load(v.flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // The lane's units of a row: t, t + T, ...; the same slots are live in every row.  A slot past the row's
  // end does not store and is not waited for; its loads go where its index points, held inside the buffer
  // (unitAt), and their values are not used.
  const uint32_t lastUnit = g.rows * g.upr - 1;
  // The lane's gamma words are the same for every row: loaded once, before the first poll -- but at
  // UPL = 8, where 16 more registers held across the polls would spill: there they are loaded per row,
  // behind the row's last poll and ahead of the row sum's barrier (one row per workgroup up to 64 rows).
  constexpr bool kGammaOnce = UPL < 8;
  bool ok[UPL];
  u32x2 gam[UPL];
  auto loadGamma = [&] {
#pragma unroll
    for (int k = 0; k < UPL; ++k) gam[k] = load8<kPlain>(rgam, (ok[k] ? t + (uint32_t)k * T : g.upr - 1) * 8u);
  };
#pragma unroll
  for (int k = 0; k < UPL; ++k) ok[k] = t + (uint32_t)k * T < g.upr;
  if constexpr (kGammaOnce) loadGamma();
  const uint32_t flag = wave_uniform(flagv);
  const uint64_t base = (flag & 1u) ? v.scratchBytes / 2 : 0;
  const uint64_t myRegion = base + (uint64_t)rank * g.region;  // my region in any peer's scratch
  const uint8_t* scr = (const uint8_t*)v.scratch + base;
  const auto rscr = arnorm_rsrc(scr, (uint32_t)n * g.region);

  for (uint32_t row = blockIdx.x; row < g.rows; row += G) {
    const uint32_t unit0 = row * g.upr;
    auto unitAt = [&](int k) {  // slot k's unit in the message
      const uint32_t j = unit0 + (uint32_t)k * T + t;
      return j < lastUnit ? j : lastUnit;
    };
    u32x2 own[UPL];
#pragma unroll
    for (int k = 0; k < UPL; ++k) own[k] = load8<kPlain>(rx, unitAt(k) * 8u);
    // put: my payload of the row into my region of every peer's half (no load inside the loop: see
    // pull_reduce_ll.hip)
#pragma unroll 1
    for (int q = 0; q < n; ++q) {
      if (q == rank) continue;
      const auto rq = arnorm_rsrc((uint8_t*)v.peerScratch[q] + myRegion, g.region);
#pragma unroll
      for (int k = 0; k < UPL; ++k)
        if (ok[k]) unit_put<kSystem>(rq, unitAt(k) * 16u, own[k], flag, false);
    }
    trace_stamp(a.trace, 1);

    u32x2 zq[UPL];
    float ss = 0.0f;
#pragma unroll
    for (int k0 = 0; k0 < UPL; k0 += PB) {
      u32x2 res[PB];
      u32x4 raw[PB][kMaxRanks];
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        res[i] = load8<kPlain>(rres, unitAt(k0 + i) * 8u);  // (zeros without a residual: a zero-length resource)
        poll_issue(scr, g.region, unitAt(k0 + i) * 16u, peers, raw[i]);
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int k = k0 + i;
        const uint32_t pk = unitAt(k) * 16u;
        u32x2 w[kMaxRanks];
        uint32_t missing = poll_eval(raw[i], flag, peers, w);
        if (!ok[k]) missing = 0;  // (another lane's unit, or another row's: not this lane's to wait for)
        if (missing) {
#pragma unroll
          for (int p = 0; p < kMaxRanks; ++p)
            if ((missing >> p) & 1u) w[p] = unit_wait(rscr, (uint32_t)p * g.region + pk, flag, false, a.budget, v.err);
        }
        // (the words are copied out of the vectors first: see bench_add2 in allreduce_ll.hip)
        uint32_t lo[kMaxRanks], hi[kMaxRanks];
#pragma unroll
        for (int p = 0; p < kMaxRanks; ++p) {
          const u32x2 x = p == rank ? own[k] : w[p];
          lo[p] = x.x;
          hi[p] = x.y;
        }
        zq[k] = u32x2{arnorm_word<DT>(lo, n, hasRes, res[i].x), arnorm_word<DT>(hi, n, hasRes, res[i].y)};
        if (hasRes && ok[k]) store8<kPlain>(rro, unitAt(k) * 8u, zq[k]);
        if (ok[k]) {
          const float e0 = arnorm_lo<DT>(zq[k].x), e1 = arnorm_hi<DT>(zq[k].x);
          const float e2 = arnorm_lo<DT>(zq[k].y), e3 = arnorm_hi<DT>(zq[k].y);
          ss = __builtin_fmaf(e0, e0, ss);
          ss = __builtin_fmaf(e1, e1, ss);
          ss = __builtin_fmaf(e2, e2, ss);
          ss = __builtin_fmaf(e3, e3, ss);
        }
      }
    }
    trace_stamp(a.trace, 2);
    if constexpr (!kGammaOnce) loadGamma();

    // row sum: wave butterfly, one LDS word per wave (double buffered: one barrier per row), wave order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
    float* ws = waveSum[(row / G) & 1u];
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
      const float y0 = fp32_product(fp32_product(arnorm_lo<DT>(zq[k].x), rstd), arnorm_lo<DT>(gam[k].x));
      const float y1 = fp32_product(fp32_product(arnorm_hi<DT>(zq[k].x), rstd), arnorm_hi<DT>(gam[k].x));
      const float y2 = fp32_product(fp32_product(arnorm_lo<DT>(zq[k].y), rstd), arnorm_lo<DT>(gam[k].y));
      const float y3 = fp32_product(fp32_product(arnorm_hi<DT>(zq[k].y), rstd), arnorm_hi<DT>(gam[k].y));
      store8<kPlain>(ry, unitAt(k) * 8u, u32x2{arnorm_pack<DT>(y0, y1), arnorm_pack<DT>(y2, y3)});
    }
    trace_stamp(a.trace, 3);
  }
  bump_flags(v.flags, flag);
}

template <int DT, int UPL>
static int launchArNormT(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                         void* const* resOut, const void* const* gamma, const ArNormGeom& g, float eps, float invCols,
                         int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  auto fill = [&](auto& args) {
    for (int i = 0; i < nviews; ++i) {
      args.residual[i] = residual ? residual[i] : nullptr;
      args.resOut[i] = resOut ? resOut[i] : nullptr;
      args.gamma[i] = gamma[i];
    }
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.eps = eps;
    args.invCols = invCols;
    args.nranks = nranks;
    return 0;
  };
  return launchViews(allreduceRmsNormLLKernel<DT, UPL, 1>, allreduceRmsNormLLKernel<DT, UPL, kMaxRanks>, views, nviews,
                     nblocks, nthreads, s, fill);
}

template <int DT>
static int launchArNormDT(int upl, const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                          void* const* resOut, const void* const* gamma, const ArNormGeom& g, float eps, float invCols,
                          int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
#define MSCCLPP_AMD_ARNORM_ARGS views, nviews, nranks, residual, resOut, gamma, g, eps, invCols, nblocks, nthreads, budget, s
  switch (upl) {
    case 1: return launchArNormT<DT, 1>(MSCCLPP_AMD_ARNORM_ARGS);
    case 2: return launchArNormT<DT, 2>(MSCCLPP_AMD_ARNORM_ARGS);
    case 4: return launchArNormT<DT, 4>(MSCCLPP_AMD_ARNORM_ARGS);
    default: return launchArNormT<DT, 8>(MSCCLPP_AMD_ARNORM_ARGS);
  }
}

// The checks of a call's arguments, host only: 0, 4 (invalid) or 5 (a size the path does not carry); the
// views' input / output are the only fields read.  nthreads comes back as the lanes the launch takes, *upl
// as its units per lane.  The communicator asks this before it touches its own bookkeeping.
int allReduceRmsNormCheck(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                          void* const* resOut, const void* const* gamma, size_t rows, size_t cols, int dtype,
                          int nblocks, int& nthreads, int* upl) {
  if (!views || !gamma || nviews < 1 || nviews > kMaxRanks || nranks < 2 || nranks > kMaxRanks) return 4;
  if (rows == 0 || cols == 0 || cols % 4 || (dtype != kF16 && dtype != kBF16)) return 4;
  if (nblocks > kFlagSlots) return 4;
  // the lane limit: at most 8 units per lane, at the lanes asked for (default: 256, or 512 above 8192 columns)
  if (nthreads <= 0) nthreads = cols > 8192 ? 512 : 256;
  if (!launchShapeOk(nblocks, kFlagSlots, nthreads)) return 4;
  const uint64_t upr = cols / 4, perLane = (upr + nthreads - 1) / nthreads;
  if (perLane > (uint64_t)kArNormMaxUPL) return 4;
  if (upl) *upl = perLane <= 1 ? 1 : perLane <= 2 ? 2 : perLane <= 4 ? 4 : 8;
  const uint64_t bytes = (rows > (1ull << 32) ? (1ull << 32) : (uint64_t)rows) * cols * 2;  // (no overflow: cols is bounded)
  // pointers: present, 8-byte aligned, a residual with its output on every view or on none, and no overlap
  // but y == x and resOut == residual
  if (!arNormBuffersOk(views, nviews, residual, resOut, gamma, bytes, cols, 8)) return 4;
  ArNormGeom g;
  return bytes > arNormMaxBytes() || !arNormGeometry(nranks, rows, cols, dtype, &g) ? 5 : 0;
}

// 4: invalid, nothing launched and no device touched; 5: not carried with this scratch, size or grid.
// residual / resOut: null, or host arrays with one entry per view, all null or none.  The views' other
// fields (scratch, flags, err, rank, peerScratch) are the caller's to check.
int launchAllReduceRmsNorm(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                           void* const* resOut, const void* const* gamma, size_t rows, size_t cols, int dtype, float eps,
                           int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  int upl = 0;
  if (const int rc = allReduceRmsNormCheck(views, nviews, nranks, residual, resOut, gamma, rows, cols, dtype, nblocks,
                                           nthreads, &upl))
    return rc;
  ArNormGeom g;
  arNormGeometry(nranks, rows, cols, dtype, &g);
  if (nblocks <= 0) nblocks = (int)(rows < 64 ? rows : 64);
  for (int i = 0; i < nviews; ++i)
    if (views[i].scratchBytes != views[0].scratchBytes || views[i].scratchBytes < 2 * g.half) return 5;
  const float invCols = 1.0f / (float)cols;
  if (dtype == kF16) return launchArNormDT<kF16>(upl, MSCCLPP_AMD_ARNORM_ARGS);
  return launchArNormDT<kBF16>(upl, MSCCLPP_AMD_ARNORM_ARGS);
}

}  // namespace mscclpp_amd
