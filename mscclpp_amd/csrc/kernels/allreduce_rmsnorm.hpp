// What the fused AllReduce + residual add + RMSNorm kernels share (allreduce_rmsnorm_ll.hip,
// allreduce_rmsnorm_pull.hip, allreduce_rmsnorm_quant_pull.hip, allreduce_rmsnorm_mx_pull.hip,
// allreduce_rmsnorm_quant_ll.hip): the element decode / encode of the definition, the e4m3
// conversion and the block maximum of the quantising kernels, the geometry of the pull kernels and the host's
// check of a call's buffers.
#pragma once

#include "common.hpp"
#include "mscclpp_amd/pull_reduce_device.hpp"

namespace mscclpp_amd {

// A buffer resource over exactly `bytes` bytes at p: an offset outside it loads zeros and stores nothing.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t arnorm_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

template <int DT>
__device__ __forceinline__ float arnorm_lo(uint32_t w) {
  if constexpr (DT == kF16) return f16_to_f32(w & 0xffffu);
  else return bf16_lo(w);
}
template <int DT>
__device__ __forceinline__ float arnorm_hi(uint32_t w) {
  if constexpr (DT == kF16) return f16_to_f32(w >> 16);
  else return bf16_hi(w);
}
// Two fp32 values, each rounded once (RNE) to DT and packed {lo, hi}.  The arguments are values of their
// own (fp32_value / fp32_product), so no conversion is selected together with the operation before it.
template <int DT>
__device__ __forceinline__ uint32_t arnorm_pack(float lo, float hi) {
  if constexpr (DT == kF16) {
    const _Float16 l = (_Float16)lo, h = (_Float16)hi;
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  } else {
    const __bf16 l = (__bf16)lo, h = (__bf16)hi;
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  }
}

typedef uint16_t arnorm_u16x2 __attribute__((ext_vector_type(2)));

// fp8_sat<false> (reduce_device.hpp) with its bound in ONE scalar register: v_med3_f32 takes sat and -sat off the
// same operand, where the two literals 448 and -448 cost a VGPR held across the row loop.
__device__ __forceinline__ float arnorm_sat448(float v, float sat) {
  if ((__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u) v = __builtin_amdgcn_fmed3f(v, sat, -sat);
  return v;
}

// Two DT elements of y times inv, clamped to +-448 and rounded (RNE) into byte pair `Hi` of `old`.
template <int DT, bool Hi>
__device__ __forceinline__ uint32_t arnorm_quant2(uint32_t yw, float inv, float sat, uint32_t old) {
  const float lo = arnorm_sat448(fp32_product(arnorm_lo<DT>(yw), inv), sat);
  const float hi = arnorm_sat448(fp32_product(arnorm_hi<DT>(yw), inv), sat);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(lo, hi, (int)old, Hi);
}

// __shfl_xor(v, m, 64) with the partner lane taken from threadIdx.x, which is live anyway, instead of a lane
// index held across the row loop: the same lanes, so the same sums in the same order.
__device__ __forceinline__ uint32_t arnorm_xor_lane(uint32_t v, int m, uint32_t t) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((t ^ (uint32_t)m) & 63u) << 2), (int)v);
}

// The microscaling formats of the block-scaling kernels (allreduce_rmsnorm_mx_pull.hip,
// allreduce_rmsnorm_quant_ll.hip).
constexpr int kMxFp8 = MSCCLPP_AMD_MX_FP8_E4M3, kMxFp4 = MSCCLPP_AMD_MX_FP4_E2M1;

// The maximum of v over the quad of lanes t ^ 1, t ^ 2 (DPP quad_perm [1,0,3,2], then [2,3,0,1]).
__device__ __forceinline__ uint32_t arnorm_quad_max(uint32_t v) {
  uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xb1, 0xf, 0xf, true);
  v = v > o ? v : o;
  o = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4e, 0xf, 0xf, true);
  return v > o ? v : o;
}

// The two-shot pull kernels' (allreduce_rmsnorm_pull.hip and its two quantising forms) one statement of
// the geometry; the host's checks, the launchers and the kernels use it.
struct ArNormPullGeom {
  uint32_t rows;
  uint32_t upr;    // 16-byte units per row = cols / 8
  uint32_t slice;  // R: rows per rank
  uint32_t rpb;    // rows per workgroup inside a slice
};

// Workgroup b's rows of rank q's slice: [*row0, *row0 + the result).
__host__ __device__ inline uint32_t arNormPullRows(const ArNormPullGeom& g, uint32_t q, uint32_t b, uint32_t* row0) {
  const uint64_t lo = (uint64_t)b * g.rpb;
  uint64_t hi = lo + g.rpb < g.slice ? lo + g.rpb : g.slice;
  const uint64_t first = (uint64_t)q * g.slice + lo;
  hi += (uint64_t)q * g.slice;
  if (hi > g.rows) hi = g.rows;
  *row0 = (uint32_t)first;
  return lo < g.slice && first < hi ? (uint32_t)(hi - first) : 0u;
}

constexpr int kArNormPullMaxUPL = 4;
constexpr int kArNormPullCopyUnits = 4;  // phase 2: 16-byte loads per lane and buffer in flight

inline bool arNormOverlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}

// The buffers of a call, host only: x, y and gamma present on every view, a residual with its output on every
// view or on none, every pointer aligned to `align` bytes, and no overlap but y == x and resOut == residual --
// inside a view between any two buffers, between views wherever one of the two is written (replicated
// read-only buffers may be shared).  bytes: of one [rows][cols] buffer.
inline bool arNormBuffersOk(const mscclppAmdRankView* views, int nviews, const void* const* residual,
                            void* const* resOut, const void* const* gamma, uint64_t bytes, size_t cols, unsigned align) {
  struct Buf { const void* p; size_t n; bool written; int view; };
  Buf all[kMaxRanks * 5];
  int nb = 0;
  const bool withRes = residual && residual[0];
  for (int i = 0; i < nviews; ++i) {
    const void* x = views[i].input;
    const void* y = views[i].output;
    const void* r = residual ? residual[i] : nullptr;
    const void* ro = resOut ? resOut[i] : nullptr;
    if (!x || !y || !gamma[i] || (r != nullptr) != withRes || (ro != nullptr) != withRes) return false;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)r | (uintptr_t)ro | (uintptr_t)gamma[i]) % align) return false;
    all[nb++] = Buf{x, bytes, y == x, i};
    if (y != x) all[nb++] = Buf{y, bytes, true, i};
    all[nb++] = Buf{gamma[i], cols * 2, false, i};
    if (withRes) {
      all[nb++] = Buf{r, bytes, ro == r, i};
      if (ro != r) all[nb++] = Buf{ro, bytes, true, i};
    }
  }
  for (int b = 0; b < nb; ++b)
    for (int c = 0; c < b; ++c)
      if ((all[b].view == all[c].view || all[b].written || all[c].written) &&
          arNormOverlap(all[b].p, all[b].n, all[c].p, all[c].n))
        return false;
  return true;
}

}  // namespace mscclpp_amd
