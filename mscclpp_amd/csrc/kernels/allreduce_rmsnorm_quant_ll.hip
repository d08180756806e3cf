// Fused small AllReduce + residual add + RMSNorm whose normalised rows leave QUANTISED: allreduce_rmsnorm_ll.hip's
// one hop of LL8 packets with the quantisation done in the registers that reduced the row.
// Steps 1-4 are §17i's in that kernel's own order -- protocol, geometry, scratch halves, flags, rank-order sum,
// residual, one rounding, the fma chain, the butterfly and the wave words -- so res_out, and y before it is
// quantised, are all_reduce_rms_norm's bits at the same (cols, nthreads); y is not stored.  Then one of
//
//   FP8_ROW (§17k steps 5-7)   amax = max_j |y_j| of the ROUNDED row; scale = max(amax / 448, 2^-126) -> scale[row]
//                              (fp32); inv = 1 / scale; q_j = e4m3(clamp(y_j * inv, +-448)): one byte at q[row][j]
//   MXFP8 / MXFP4 (§17l 5-7)   per block B of 32 columns: E = max(e32(amax_B) - emax, 0), one byte at scale[row][B];
//                              q_j = fmt(y_j * 2^(127 - E)), saturating; MXFP8 one byte per column, MXFP4 column 2i
//                              in the low and 2i + 1 in the high nibble of q[row][i]
//
//  * Every rank holds every whole row in registers, so q and the scales are local stores: nothing is gathered,
//    nothing is registered, there is no peer-scale table and no handshake.
//  * A unit is 4 elements here (8 bytes of x), so an MX block is EIGHT adjacent units: lanes 8m .. 8m + 7 of one
//    slot.  The block's maximum is the 16-bit integer maximum of the sign-cleared patterns (§17k) carried over
//    the eight lanes by three DPP moves -- quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror -- with no
//    LDS and no second barrier; lane 0 of the group stores E.  y is converted out of the registers it was made in.
//  * FP8_ROW needs the row's maximum: §17k's wave butterfly (partner lane from threadIdx.x), one LDS word per wave
//    beside the sum's, double buffered by the row's parity like it, and a second barrier per row.  y is written
//    packed over zq between the barriers and converted after the second; lane 0 stores the row's scale.
//  * q of a unit is 4 bytes (FP8_ROW, MXFP8) or 2 bytes (MXFP4) at half or a quarter of the unit's offset in x,
//    contiguous across the lanes (MXFP4: one buffer_store_short per lane; pairing lanes for dword stores costs a
//    DPP move and an OR per unit and saves no store instruction).  q and scale are addressed through descriptors
//    of exactly their bytes.
//  * Nothing of the quantisation is live across the poll batch, the register peak of §17i: the +-448 bound sits
//    in one scalar register, inv and E are made after the row sum, gamma is taken as §17i does (once at UPL < 8,
//    per row at UPL = 8) and decoded per row behind an empty asm volatile, and what derives from threadIdx.x
//    for the row's tail (the per-row gamma offsets, the butterflies' partner addresses) is made per row.
//  * q and scale overlap nothing; res_out == residual is carried.  A row (FP8_ROW) or block (MX) whose y holds a
//    NaN or an infinity has an unspecified q and scale; its res_out and its neighbours are as defined.
//    Trace stamps (of the workgroup's last row): 0 start, 1 puts issued, 2 reduced, 3 normalised and quantised.
#include "allreduce_rmsnorm.hpp"
#include "launch.hpp"
#include "ll_units.hpp"

namespace mscclpp_amd {

constexpr int kQuantFp8Row = MSCCLPP_AMD_QUANT_FP8_ROW;

// allreduce_rmsnorm_ll.hip's ArNormGeom as this kernel reads it, from a shape its check has accepted.
struct ArNormQuantGeom {
  uint32_t rows;
  uint32_t upr;     // packet units per row = cols / 4
  uint32_t region;  // bytes one source rank occupies in a scratch half = rows * upr * 16
  uint32_t bytes;   // of one [rows][cols] buffer of x
};

template <int NV>
struct ArNormQuantArgs {
  Views<NV> views;           // output: q
  const void* residual[NV];  // null on every view, or on none
  void* resOut[NV];
  const void* gamma[NV];
  void* scale[NV];
  ArNormQuantGeom g;
  uint64_t budget;
  uint64_t* trace;
  float eps;
  float invCols;  // 1.0f / (float)cols, computed once by the host
  int nranks;
  int pad;
};
static_assert(sizeof(ArNormQuantArgs<kMaxRanks>) <= 4096,
              "in-process AllReduce+RMSNorm quantising LL arguments exceed the kernel-argument limit");

// zq of one word, as allreduce_rmsnorm_ll.hip's arnorm_word: the fp32 sum over the ranks in rank order, plus the
// residual word where there is one, rounded once.
template <int DT>
__device__ __forceinline__ uint32_t arnorm_quant_word(const uint32_t* x, int n, bool hasRes, uint32_t res) {
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

// The maximum of v over the eight lanes 8m .. 8m + 7: the quad's, then the other quad's by row_half_mirror
// (lane i of a half row reads lane 7 - i, which holds the other quad's maximum).
__device__ __forceinline__ uint32_t arnorm_octet_max(uint32_t v) {
  v = arnorm_quad_max(v);
  const uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);
  return v > o ? v : o;
}

// Four waves per SIMD (at most 128 VGPRs), as allreduceRmsNormLLKernel.
template <int DT, int UPL, int FMT, int NV>
__global__ void __launch_bounds__(512, 4) allreduceRmsNormQuantLLKernel(ArNormQuantArgs<NV> a) {
  // units whose first polls are in flight together: 32 VGPRs of raw packets each
  constexpr int PB = UPL == 2 ? 2 : 1;
  constexpr bool kRow = FMT == kQuantFp8Row;
  constexpr uint32_t kEmax = FMT == kMxFp8 ? 8u : 2u;
  constexpr uint32_t kQShift = FMT == kMxFp4 ? 2u : 1u;  // a unit's bytes of q: 8 >> kQShift
  __shared__ uint32_t waveWords[2][kRow ? 2 : 1][8];     // [the row's parity][sum of squares, amax][wave]
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const ArNormQuantGeom& g = a.g;
  const uint32_t T = blockDim.x, G = gridDim.x, t = threadIdx.x;
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  const bool hasRes = a.residual[vi] != nullptr;
  const auto rx = arnorm_rsrc(v.input, g.bytes);
  const auto rq = arnorm_rsrc(v.output, g.bytes >> kQShift);
  const auto rsc = arnorm_rsrc(a.scale[vi], kRow ? g.rows * 4u : g.rows * (g.upr >> 3));
  const auto rres = arnorm_rsrc(a.residual[vi], hasRes ? g.bytes : 0u);
  const auto rro = arnorm_rsrc(a.resOut[vi], hasRes ? g.bytes : 0u);
  const auto rgam = arnorm_rsrc(a.gamma[vi], g.upr * 8u);
  trace_stamp(a.trace, 0);
  const uint32_t flagv = __hip_atomic_load(v.flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // The lane's units of a row: t, t + T, ...; the same slots are live in every row.  A slot past the row's end
  // does not store and is not waited for; its loads go where its index points, held inside the buffer (unitAt),
  // and their values are not used.
  const uint32_t lastUnit = g.rows * g.upr - 1;
  constexpr bool kGammaOnce = UPL < 8;  // (allreduceRmsNormLLKernel: 16 more registers across the polls would spill)
  bool ok[UPL];
  u32x2 gam[UPL];
  auto loadGamma = [&](uint32_t lane) {  // lane: threadIdx.x
#pragma unroll
    for (int k = 0; k < UPL; ++k) gam[k] = load8<kPlain>(rgam, (ok[k] ? lane + (uint32_t)k * T : g.upr - 1) * 8u);
  };
#pragma unroll
  for (int k = 0; k < UPL; ++k) ok[k] = t + (uint32_t)k * T < g.upr;
  if constexpr (kGammaOnce) loadGamma(t);
  const uint32_t flag = wave_uniform(flagv);
  const uint64_t base = (flag & 1u) ? v.scratchBytes / 2 : 0;
  const uint64_t myRegion = base + (uint64_t)rank * g.region;  // my region in any peer's scratch
  const uint8_t* scr = (const uint8_t*)v.scratch + base;
  const auto rscr = arnorm_rsrc(scr, (uint32_t)n * g.region);
  float sat = 448.0f;
  asm("" : "+s"(sat));  // no instruction: the bound as a register value (arnorm_sat448)

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
      const auto rp = arnorm_rsrc((uint8_t*)v.peerScratch[q] + myRegion, g.region);
#pragma unroll
      for (int k = 0; k < UPL; ++k)
        if (ok[k]) unit_put<kSystem>(rp, unitAt(k) * 16u, own[k], flag, false);
    }
    trace_stamp(a.trace, 1);

    u32x2 zq[UPL];  // the row packed in DT: zq up to rstd, y after it
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
        zq[k] = u32x2{arnorm_quant_word<DT>(lo, n, hasRes, res[i].x), arnorm_quant_word<DT>(hi, n, hasRes, res[i].y)};
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
    // threadIdx.x again, behind an empty asm: what follows derives from it -- the per-row gamma offsets and the
    // butterflies' partner addresses -- is made here, per row, and not held in 8 + 6 registers across the polls
    uint32_t tl = t;
    asm volatile("" : "+v"(tl));
    if constexpr (!kGammaOnce) loadGamma(tl);

    // row sum: wave butterfly (the lanes of __shfl_xor 32, 16, ..., 1, the partner from threadIdx.x), one LDS
    // word per wave (double buffered by the row's parity), wave order: allreduceRmsNormLLKernel's sum, bit for bit
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
      ss = ss + __builtin_bit_cast(float, arnorm_xor_lane(__builtin_bit_cast(uint32_t, ss), m, tl));
    uint32_t* ws = waveWords[(row / G) & 1u][0];
    if ((t & 63u) == 0) ws[t >> 6] = __builtin_bit_cast(uint32_t, ss);
    __syncthreads();
    float total = __builtin_bit_cast(float, ws[0]);
    for (uint32_t wv = 1; wv < T / 64; ++wv) total = total + __builtin_bit_cast(float, ws[wv]);
    const float ms = fp32_product(total, a.invCols);
    const float rstd = __builtin_amdgcn_rsqf(fp32_value(ms + a.eps));

    // y of slot k, packed in DT, and the maximum of its four sign-cleared patterns
    auto normalise = [&](int k, arnorm_u16x2& am2) {
      uint32_t y[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t z = zq[k][j];
        uint32_t gw = gam[k][j];
        asm volatile("" : "+v"(gw));  // no instruction: gamma is decoded here, per row, and stays packed across rows
        const float lo = fp32_product(fp32_product(arnorm_lo<DT>(z), rstd), arnorm_lo<DT>(gw));
        const float hi = fp32_product(fp32_product(arnorm_hi<DT>(z), rstd), arnorm_hi<DT>(gw));
        y[j] = arnorm_pack<DT>(lo, hi);
        am2 = __builtin_elementwise_max(am2, __builtin_bit_cast(arnorm_u16x2, y[j] & 0x7fff7fffu));
      }
      return u32x2{y[0], y[1]};
    };

    if constexpr (kRow) {
      // pass 2: y over zq's registers, and the lane's amax
      arnorm_u16x2 am2 = {0, 0};
#pragma unroll
      for (int k = 0; k < UPL; ++k)
        if (ok[k]) zq[k] = normalise(k, am2);
      // row amax: wave butterfly, one LDS word per wave beside the sum's, a second barrier
      uint32_t am = am2.x > am2.y ? am2.x : am2.y;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = arnorm_xor_lane(am, m, tl);
        am = am > o ? am : o;
      }
      uint32_t* wm = ws + 8;
      if ((t & 63u) == 0) wm[t >> 6] = am;
      __syncthreads();
      am = wm[0];
      for (uint32_t wv = 1; wv < T / 64; ++wv) am = am > wm[wv] ? am : wm[wv];
      // both divisions are plain fp32 divisions, correctly rounded (the full expansion, no bare v_rcp_f32)
      const float amax = arnorm_lo<DT>(am);
      const float scale = fmaxf(amax / sat, 0x1p-126f);  // sat: 448.0f, in the scalar register it already has
      const float inv = 1.0f / scale;
      if (t == 0) store4<kPlain>(rsc, row * 4u, __builtin_bit_cast(uint32_t, scale));
      // pass 3: the unit's 4 bytes of q
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        if (!ok[k]) continue;
        uint32_t q0 = arnorm_quant2<DT, false>(zq[k].x, inv, sat, 0u);
        q0 = arnorm_quant2<DT, true>(zq[k].y, inv, sat, q0);
        store4<kPlain>(rq, unitAt(k) * 4u, q0);
      }
    } else {
      // pass 2, per unit: y, the block's amax and E, the conversion, the stores
#pragma unroll
      for (int k = 0; k < UPL; ++k) {
        // T is a multiple of 64 and cols % 32 == 0 is upr % 8 == 0 (the host's check): the eight lanes 8m ..
        // 8m + 7 of a slot hold units 8m' .. 8m' + 7 of the row -- one block -- and are all live or all dead, so
        // every lane the three DPP moves read from is active here.
        if (!ok[k]) continue;
        arnorm_u16x2 am2 = {0, 0};
        const u32x2 y = normalise(k, am2);
        const uint32_t am = arnorm_octet_max(am2.x > am2.y ? am2.x : am2.y);
        // E: the exponent field of amax as fp32 (an exact conversion), less emax, not below 0
        const uint32_t e32 = __builtin_bit_cast(uint32_t, arnorm_lo<DT>(am)) >> 23;
        const uint32_t E = e32 > kEmax ? e32 - kEmax : 0u;
        const uint32_t u = unitAt(k);  // (a live slot: the unit itself)
        if constexpr (FMT == kMxFp8) {
          const float f = __builtin_bit_cast(float, (254u - E) << 23);  // 2^(127 - E): E <= 247, a normal number
          uint32_t q0 = arnorm_quant2<DT, false>(y.x, f, sat, 0u);
          q0 = arnorm_quant2<DT, true>(y.y, f, sat, q0);
          store4<kPlain>(rq, u * 4u, q0);
        } else {
          const float x = __builtin_bit_cast(float, E << 23);  // the instruction divides by 2^(its exponent field - 127)
          uint32_t q0 = 0u;
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y.x), arnorm_hi<DT>(y.x), x, 0);
          q0 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q0, arnorm_lo<DT>(y.y), arnorm_hi<DT>(y.y), x, 1);
          __builtin_amdgcn_raw_buffer_store_b16((uint16_t)q0, rq, u * 2u, 0, kPlain);
        }
        if ((t & 7u) == 0)  // unit u is the first of block u / 8; upr % 8 == 0, so row * (upr / 8) + ... = u / 8
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)E, rsc, u >> 3, 0, kPlain);
      }
    }
    trace_stamp(a.trace, 3);
  }
  bump_flags(v.flags, flag);
}

// The checks of a call's arguments, host only: 0, 4 (invalid) or 5 (a size the path does not carry), as
// allReduceRmsNormCheck -- which judges x, the residual, res_out, gamma, the shape, the lanes, the grid and the
// size cap in bytes of x (asked with y == x, the one form in which it counts no y of 2-byte elements) -- and then
// what is new: the format, cols % 32 for the MX formats, and on every view a q (view.output, 4-byte aligned) of
// rows * cols bytes (rows * cols / 2: MXFP4) and a scale of rows * 4 bytes (FP8_ROW, 4-byte aligned) or rows *
// cols / 32 bytes (MX, any alignment) that overlap no buffer of any view.
int allReduceRmsNormQuantCheck(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                               void* const* resOut, const void* const* gamma, void* const* scale, size_t rows,
                               size_t cols, int dtype, int format, int nblocks, int& nthreads, int* upl) {
  const bool row = format == kQuantFp8Row;
  if (!views || !scale || nviews < 1 || nviews > kMaxRanks) return 4;
  if (!row && ((format != kMxFp8 && format != kMxFp4) || cols % 32)) return 4;
  mscclppAmdRankView inPlace[kMaxRanks];
  for (int i = 0; i < nviews; ++i) {
    inPlace[i] = views[i];
    inPlace[i].output = const_cast<void*>(views[i].input);
  }
  if (const int rc = allReduceRmsNormCheck(inPlace, nviews, nranks, residual, resOut, gamma, rows, cols, dtype, nblocks,
                                           nthreads, upl))
    return rc;
  struct Buf { const void* p; size_t n; };
  Buf all[kMaxRanks * 6];
  int nb = 0, nOut = 0;  // the first nOut are the q and the scales
  for (int i = 0; i < nviews; ++i) {
    if (!views[i].output || !scale[i] || (uintptr_t)views[i].output % 4 || (row && (uintptr_t)scale[i] % 4)) return 4;
    all[nb++] = Buf{views[i].output, format == kMxFp4 ? rows * cols / 2 : rows * cols};
    all[nb++] = Buf{scale[i], row ? rows * 4 : rows * cols / 32};
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
static int launchArNormQuantT(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                              void* const* resOut, const void* const* gamma, void* const* scale,
                              const ArNormQuantGeom& g, float eps, float invCols, int nblocks, int nthreads,
                              uint64_t budget, hipStream_t s) {
  auto fill = [&](auto& args) {
    for (int i = 0; i < nviews; ++i) {
      args.residual[i] = residual ? residual[i] : nullptr;
      args.resOut[i] = resOut ? resOut[i] : nullptr;
      args.gamma[i] = gamma[i];
      args.scale[i] = scale[i];
    }
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.eps = eps;
    args.invCols = invCols;
    args.nranks = nranks;
    return 0;
  };
  return launchViews(allreduceRmsNormQuantLLKernel<DT, UPL, FMT, 1>, allreduceRmsNormQuantLLKernel<DT, UPL, FMT, kMaxRanks>,
                     views, nviews, nblocks, nthreads, s, fill);
}

template <int DT, int FMT>
static int launchArNormQuantDT(int upl, const mscclppAmdRankView* views, int nviews, int nranks,
                               const void* const* residual, void* const* resOut, const void* const* gamma,
                               void* const* scale, const ArNormQuantGeom& g, float eps, float invCols, int nblocks,
                               int nthreads, uint64_t budget, hipStream_t s) {
#define MSCCLPP_AMD_ARNORM_QUANT_ARGS \
  views, nviews, nranks, residual, resOut, gamma, scale, g, eps, invCols, nblocks, nthreads, budget, s
  switch (upl) {
    case 1: return launchArNormQuantT<DT, 1, FMT>(MSCCLPP_AMD_ARNORM_QUANT_ARGS);
    case 2: return launchArNormQuantT<DT, 2, FMT>(MSCCLPP_AMD_ARNORM_QUANT_ARGS);
    case 4: return launchArNormQuantT<DT, 4, FMT>(MSCCLPP_AMD_ARNORM_QUANT_ARGS);
    default: return launchArNormQuantT<DT, 8, FMT>(MSCCLPP_AMD_ARNORM_QUANT_ARGS);
  }
}

template <int FMT>
static int launchArNormQuantF(int dtype, int upl, const mscclppAmdRankView* views, int nviews, int nranks,
                              const void* const* residual, void* const* resOut, const void* const* gamma,
                              void* const* scale, const ArNormQuantGeom& g, float eps, float invCols, int nblocks,
                              int nthreads, uint64_t budget, hipStream_t s) {
  if (dtype == kF16) return launchArNormQuantDT<kF16, FMT>(upl, MSCCLPP_AMD_ARNORM_QUANT_ARGS);
  return launchArNormQuantDT<kBF16, FMT>(upl, MSCCLPP_AMD_ARNORM_QUANT_ARGS);
}

// 4: invalid, nothing launched and no device touched; 5: not carried with this scratch, size or grid.
// residual / resOut: as launchAllReduceRmsNorm; scale: one entry per view.  The scratch needed is
// allReduceRmsNormScratchRequired's.  The views' other fields (scratch, flags, err, rank, peerScratch) are the
// caller's to check.
int launchAllReduceRmsNormQuant(const mscclppAmdRankView* views, int nviews, int nranks, const void* const* residual,
                                void* const* resOut, const void* const* gamma, void* const* scale, size_t rows,
                                size_t cols, int dtype, int format, float eps, int nblocks, int nthreads,
                                uint64_t budget, hipStream_t s) {
  int upl = 0;
  if (const int rc = allReduceRmsNormQuantCheck(views, nviews, nranks, residual, resOut, gamma, scale, rows, cols, dtype,
                                                format, nblocks, nthreads, &upl))
    return rc;
  ArNormQuantGeom g{};
  g.rows = (uint32_t)rows;
  g.upr = (uint32_t)(cols / 4);
  g.region = g.rows * g.upr * 16u;
  g.bytes = g.rows * g.upr * 8u;
  const size_t need = allReduceRmsNormScratchRequired(nranks, rows, cols, dtype);
  if (nblocks <= 0) nblocks = (int)(rows < 64 ? rows : 64);
  for (int i = 0; i < nviews; ++i)
    if (!need || views[i].scratchBytes != views[0].scratchBytes || views[i].scratchBytes < need) return 5;
  const float invCols = 1.0f / (float)cols;
  if (format == kMxFp8) return launchArNormQuantF<kMxFp8>(dtype, upl, MSCCLPP_AMD_ARNORM_QUANT_ARGS);
  if (format == kMxFp4) return launchArNormQuantF<kMxFp4>(dtype, upl, MSCCLPP_AMD_ARNORM_QUANT_ARGS);
  return launchArNormQuantF<kQuantFp8Row>(dtype, upl, MSCCLPP_AMD_ARNORM_QUANT_ARGS);
}

}  // namespace mscclpp_amd
