// The per-workgroup token handshake of the bulk collectives (allreduce_bulk.hip, alltoall.hip, reduce.hip).
#pragma once

#include "common.hpp"

namespace mscclpp_amd {

__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// All lanes of the block: publish every prior store, then lane p < nranks signals peer p on
// channel `ch`; then lanes wait for the peers' matching signals.
__device__ __forceinline__ void block_handshake(const mscclppAmdRankView& v, int nranks, int rank, uint32_t ch,
                                                uint64_t budget) {
  drain_stores();
  __syncthreads();
  const int p = (int)threadIdx.x;
  if (p < nranks && p != rank) {
    // my token slot inside peer p's token array: [rank][ch]
    uint64_t* remote = v.peerTokens[p] + (uint64_t)rank * kMaxChannels + ch;
    add_release_sys(remote, 1);
    uint64_t* mine = v.tokens + (uint64_t)p * kMaxChannels + ch;
    uint64_t* exp = v.expected + (uint64_t)p * kMaxChannels + ch;
    // the counter lives in ordinary device memory and is touched once per handshake: agent-scope
    // atomics keep it out of any XCD's stale L2 line whichever XCD this block lands on next launch
    const uint64_t want = __hip_atomic_fetch_add(exp, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    SpinGuard g(budget);
    while (ld_relaxed_sys(mine) < want) {
      __builtin_amdgcn_s_sleep(2);
      if (g.expired()) {
        // detail: channel | peer << 16, rank, tokens seen (low 16 bits) | wanted (low 16 bits) << 16
        report_error_detail(v.err, kErrSemaphoreTimeout, ch | ((uint32_t)p << 16), (uint32_t)rank,
                            ((uint32_t)ld_relaxed_sys(mine) & 0xffffu) | ((uint32_t)want << 16));
        break;
      }
    }
    acquire_sys();  // the invalidate completes before the barrier
  }
  __syncthreads();
}

}  // namespace mscclpp_amd
