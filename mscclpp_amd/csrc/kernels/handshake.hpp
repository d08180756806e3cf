// The per-workgroup token handshake of the bulk collectives (allreduce_bulk.hip, alltoall.hip, reduce.hip)
// and its one-way halves for point-to-point transfers (sendrecv.hip).
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

// The two halves of a handshake on their own, for a point-to-point transfer (sendrecv.hip), whose
// synchronisation is one-way: the sender posts "ready" and later waits for "done", the receiver
// waits for "ready" and later posts "done".  Per (pair, channel) a transfer costs each side one
// token_post and one token_wait -- one add into the peer's slot, one increment of the own expected
// slot -- which is what one block_handshake costs, so the counters stay in step with the
// collectives that share them.  One lane calls each; the caller orders the workgroup around it
// (drain_stores + barrier before a post that publishes stores, a barrier after a wait).
__device__ __forceinline__ void token_post(uint64_t* peerTokens, int rank, uint32_t ch) {
  // my token slot inside the peer's token array: [rank][ch]
  add_release_sys(peerTokens + (uint64_t)rank * kMaxChannels + ch, 1);
}

__device__ __forceinline__ void token_wait(uint64_t* tokens, uint64_t* expected, uint32_t* err, int peer, int rank,
                                           uint32_t ch, uint64_t budget) {
  uint64_t* mine = tokens + (uint64_t)peer * kMaxChannels + ch;
  uint64_t* exp = expected + (uint64_t)peer * kMaxChannels + ch;
  // (agent scope: as block_handshake)
  const uint64_t want = __hip_atomic_fetch_add(exp, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  SpinGuard g(budget);
  while (ld_relaxed_sys(mine) < want) {
    __builtin_amdgcn_s_sleep(2);
    if (g.expired()) {
      // detail: channel | peer << 16, rank, tokens seen (low 16 bits) | wanted (low 16 bits) << 16
      report_error_detail(err, kErrSemaphoreTimeout, ch | ((uint32_t)peer << 16), (uint32_t)rank,
                          ((uint32_t)ld_relaxed_sys(mine) & 0xffffu) | ((uint32_t)want << 16));
      break;
    }
  }
  acquire_sys();  // the invalidate completes before the caller's barrier
}

}  // namespace mscclpp_amd
