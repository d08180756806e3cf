// The LL-packet unit helpers shared by the LL kernels (allreduce_ll.hip, pull_reduce_ll.hip): a lane's
// 16-byte packet unit (put, poll, bounded wait, timeout detail), the 8-byte payload load / store with
// a tail, and the word count a message covers.
#pragma once

#include "common.hpp"

namespace mscclpp_amd {

// ---- packet-major units ------------------------------------------------------------------------
// One lane owns one "unit": 8 payload bytes <-> 16 packet bytes, i.e. one LL16 packet
// {P[2i], f, P[2i+1], f} or the two LL8 packets {P[2i], f}, {P[2i+1], f} -- the same 16-byte image.
// Consecutive lanes own consecutive units, so every packet store / poll of a wave is one contiguous
// 1 KiB access made of whole 64-byte lines (partial-line packet stores cost a full line each on
// gfx950: WRITE_SIZE 5*S instead of 3*S in the self-reduce microbench), and the payload side is a
// contiguous 512 B dwordx2 access.
template <int Policy>
__device__ __forceinline__ void unit_put(__amdgpu_buffer_rsrc_t pk, uint32_t pbyte, u32x2 w, uint32_t flag,
                                         bool single) {
  if (!single)
    store16<Policy>(pk, pbyte, u32x4{w.x, flag, w.y, flag});
  else
    store8<Policy>(pk, pbyte, u32x2{w.x, flag});  // lone trailing LL8 packet
}
__device__ __forceinline__ bool unit_try(__amdgpu_buffer_rsrc_t pk, uint32_t pbyte, uint32_t flag, u32x2& w,
                                         bool single) {
  if (!single) {
    u32x4 a = load16<kSystem>(pk, pbyte);
    w = u32x2{a.x, a.z};
    return a.y == flag && a.w == flag;
  }
  u32x2 a = load8<kSystem>(pk, pbyte);
  w = u32x2{a.x, 0};
  return a.y == flag;
}
// Timeout detail of one packet unit: the first of its flag words that differs from `flag`, re-read.
__device__ __forceinline__ uint32_t unit_flag_seen(__amdgpu_buffer_rsrc_t pk, uint32_t pbyte, uint32_t flag,
                                                   bool single) {
  if (single) return load8<kSystem>(pk, pbyte).y;
  const u32x4 a = load16<kSystem>(pk, pbyte);
  return a.y != flag ? a.y : a.w;
}
__device__ __forceinline__ u32x2 unit_get(__amdgpu_buffer_rsrc_t pk, uint32_t pbyte, uint32_t flag, bool single,
                                          uint64_t budget, uint32_t* err) {
  u32x2 w;
  if (unit_try(pk, pbyte, flag, w, single)) return w;
  SpinGuard g(budget);
  while (!unit_try(pk, pbyte, flag, w, single)) {
    __builtin_amdgcn_s_sleep(1);
    if (g.expired()) {
      report_packet_timeout(err, flag, pbyte, unit_flag_seen(pk, pbyte, flag, single));
      return u32x2{0, 0};
    }
  }
  return w;
}

// First poll of unit `pbyte` in every peer's region (peer p's at p * stride of `base`): all loads
// are issued, unconditionally and in one basic block, before any value is compared, so they are in
// flight together (a compare right after each load, or a load under a branch, made the compiler wait
// for it before issuing the next: one memory round trip per peer).  A slot that is not a peer (own
// rank, p >= nranks) is loaded through a zero-length buffer resource: out of range, it returns zeros
// without touching memory.  Returns the mask of peers whose packet had not landed; w[p] holds the
// payload of the others.
__device__ __forceinline__ void poll_issue(const uint8_t* base, uint32_t stride, uint32_t pbyte, uint32_t peers,
                                           u32x4* raw) {
#pragma unroll
  for (int p = 0; p < kMaxRanks; ++p) {
    const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0,
                                                     ((peers >> p) & 1u) ? 0xFFFFFFFFu : 0u, 0x00020000);
    raw[p] = load16<kSystem>(r, (uint32_t)p * stride + pbyte);
  }
}
__device__ __forceinline__ uint32_t poll_eval(const u32x4* raw, uint32_t flag, uint32_t peers, u32x2* w) {
  uint32_t missing = 0;
#pragma unroll
  for (int p = 0; p < kMaxRanks; ++p) {
    w[p] = u32x2{raw[p].x, raw[p].z};
    if (raw[p].y != flag || raw[p].w != flag) missing |= 1u << p;
  }
  return missing & peers;
}
__device__ __forceinline__ uint32_t poll_units(const uint8_t* base, uint32_t stride, uint32_t pbyte, uint32_t flag,
                                               uint32_t peers, u32x2* w) {
  u32x4 raw[kMaxRanks];
  poll_issue(base, stride, pbyte, peers, raw);
  return poll_eval(raw, flag, peers, w);
}
// A unit whose first poll missed: spin until it lands (the caller keeps the values of the units
// that were ready, so only the missing ones are read again).
__device__ __forceinline__ u32x2 unit_wait(__amdgpu_buffer_rsrc_t pk, uint32_t pbyte, uint32_t flag, bool single,
                                           uint64_t budget, uint32_t* err) {
  u32x2 w;
  SpinGuard g(budget);
  do {
    __builtin_amdgcn_s_sleep(1);
    if (unit_try(pk, pbyte, flag, w, single)) return w;
  } while (!g.expired());
  report_packet_timeout(err, flag, pbyte, unit_flag_seen(pk, pbyte, flag, single));
  return u32x2{0, 0};
}
// 8-byte payload at byte `off` of `base`, of which `valid` bytes are inside the buffer
__device__ __forceinline__ u32x2 payload_ld(__amdgpu_buffer_rsrc_t r, const uint8_t* base, uint64_t off, uint32_t valid) {
  if (valid >= 8) return load8<kPlain>(r, (uint32_t)off);
  uint32_t w0 = 0, w1 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if ((uint32_t)i < valid) {
      const uint32_t v = (uint32_t)base[off + i] << ((i % 4) * 8);
      if (i < 4) w0 |= v; else w1 |= v;
    }
  }
  return u32x2{w0, w1};
}
__device__ __forceinline__ void payload_st(__amdgpu_buffer_rsrc_t r, uint8_t* base, uint64_t off, u32x2 v, uint32_t valid) {
  if (valid >= 8) {
    store8<kPlain>(r, (uint32_t)off, v);
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if ((uint32_t)i < valid) base[off + i] = (uint8_t)((i < 4 ? v.x : v.y) >> ((i % 4) * 8));
}

// ---- host-side geometry --------------------------------------------------------------------------
// 32-bit words the LL kernels cover: (count*sizeof(T)+sizeof(T))/sizeof(int) for 1- and 2-byte T
// (allreduce_packet.cu:51-52, allreduce_allpair_packet.cu:20).  Deviation: for 1-byte T with
// count % 4 in {1, 2} that stops short of the buffer (its last bytes would never be reduced), so
// the words are rounded up there; every other size keeps the reference's count.
static inline uint64_t llWords(size_t bytes, int dtype) {
  const int es = elem_bytes(dtype);
  if (es == 4) return bytes / 4;
  uint64_t W = (bytes + es) / 4;
  if (W * 4 < bytes) W = (bytes + 3) / 4;
  return W;
}

// The LL kernels address a buffer, and all source regions of a scratch half, from one buffer
// resource each (32-bit offsets: the whole packet exchange of a bucket stays in one descriptor, no
// per-unit rebasing on the latency path).  So an LL bucket is bounded: its bytes, and the n regions
// of a scratch half, must lie within 4 GiB of their base -- LL16 to just under 2 GiB per rank,
// LL8 to 2 GiB / n; beyond, the call is refused (ncclInvalidUsage) rather than wrapped.  The
// reference runs these protocols below 1 MiB (algorithm_selector.cc:107-117); larger buckets take the
// bulk paths, which rebase per workgroup and per pass.
constexpr uint64_t kLLOffsetLimit = 0xFFFFFFFFull - 64;

}  // namespace mscclpp_amd
