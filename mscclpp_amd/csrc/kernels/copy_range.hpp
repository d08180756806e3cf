// The alignment-aware pull copy of the zero-copy byte movers (alltoall.hip, sendrecv.hip): loads with
// the caller's cache policy (system scope for a peer's buffer), plain local stores.
//
// A range whose source and destination both start 16-byte aligned moves in 16-byte units, U loads
// in flight per lane before their stores; any other one moves at the widest power of two (1, 2, 4,
// 8 bytes) dividing both addresses -- correct, not fast.  Tails move byte by byte: no byte outside
// [dst, dst + len) is written and none outside [src, src + len) is read.
#pragma once

#include "common.hpp"

namespace mscclpp_amd {

template <int Policy, int W>
__device__ __forceinline__ void copy_narrow(const uint8_t* src, uint8_t* dst, uint64_t nUnits, uint32_t tid, uint32_t T) {
  const auto rs = make_rsrc(src);
  const auto rd = make_rsrc(dst);
  for (uint64_t u = tid; u < nUnits; u += T) {  // (64-bit: nUnits may sit within T of 2^32)
    const uint32_t off = (uint32_t)(u * W);
    if constexpr (W == 8)
      store8<kPlain>(rd, off, load8<Policy>(rs, off));
    else if constexpr (W == 4)
      store4<kPlain>(rd, off, load4<Policy>(rs, off));
    else if constexpr (W == 2)
      __builtin_amdgcn_raw_buffer_store_b16(__builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, Policy), rd, off, 0, kPlain);
    else
      __builtin_amdgcn_raw_buffer_store_b8(__builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, Policy), rd, off, 0, kPlain);
  }
}

// dst[0, len) = src[0, len); len <= kBlkOffsetLimit (one buffer resource each, rebased here).
template <int Policy, int U>
__device__ __forceinline__ void copy_range(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t tid, uint32_t T) {
  const uint32_t mis = ((uint32_t)(uintptr_t)src | (uint32_t)(uintptr_t)dst) & 15u;
  uint64_t done;
  if (mis == 0) {
    const auto rs = make_rsrc(src);
    const auto rd = make_rsrc(dst);
    const uint32_t nUnits = (uint32_t)(len / 16);
    for (uint32_t u0 = tid; u0 < nUnits; u0 += T * U) {
      u32x4 w[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * T;
        if (u < nUnits) w[k] = load16<Policy>(rs, u * 16u);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const uint32_t u = u0 + k * T;
        if (u < nUnits) store16<kPlain>(rd, u * 16u, w[k]);
      }
    }
    done = (uint64_t)nUnits * 16;
  } else if (mis & 1u) {
    done = 0;
  } else if (mis & 2u) {
    copy_narrow<Policy, 2>(src, dst, len / 2, tid, T);
    done = len & ~1ull;
  } else if (mis & 4u) {
    copy_narrow<Policy, 4>(src, dst, len / 4, tid, T);
    done = len & ~3ull;
  } else {
    copy_narrow<Policy, 8>(src, dst, len / 8, tid, T);
    done = len & ~7ull;
  }
  if (done < len) copy_narrow<Policy, 1>(src + done, dst + done, len - done, tid, T);
}

}  // namespace mscclpp_amd
