// ncclAllToAll / ncclAllToAllv: a zero-copy pull over xGMI.
//
// The reference leaves both to the vendor library (nccl.cc:794-821 is a TODO; the alltoall kernels
// of test/mscclpp-test/alltoall_test.cu are compiled for CUDA only), so this is no restatement.
//
// Rank r's receive segment from peer p is read straight out of p's send buffer (system-scope
// 16-byte buffer loads, as broadcastKernel reads the root) and stored into r's own receive buffer
// with plain stores: every store is local, nothing is written into a peer's user buffer (DESIGN.md
// §5: remote plain / nt stores into user buffers went stale).  A table of n segments {srcOff into
// peer p's send buffer, dstOff into the own receive buffer, len}, in bytes, drives the kernel;
// equal-split AllToAll is the table srcOff = rank * B, dstOff = p * B, len = B.
//
//  * Entry handshake per workgroup (channel = blockIdx.x): the peers' send buffers are final (their
//    producers ran earlier on the peers' streams) and this rank's earlier stream work on its receive
//    buffer is over.
//  * Workgroup b owns the sub-range [b * blk_p, (b + 1) * blk_p) of every segment p, blk_p =
//    ceil(len_p / nblocks) rounded up to 16, and visits the n segments starting at a peer rotated
//    by rank and workgroup index, so one rank's workgroups are spread over all links at any moment
//    and the ranks do not all read the same source at once.
//  * Exit handshake: no peer still reads this rank's send buffer when its kernel ends.  Every
//    workgroup takes both handshakes, also one whose sub-ranges are all empty.
//  * A sub-range whose source and destination both start 16-byte aligned moves in 16-byte units, U
//    loads in flight per lane before their stores; any other one moves at the widest power of two
//    (1, 2, 4, 8 bytes) dividing both addresses -- correct, not fast.  Tails move byte by byte: no
//    byte outside [dstOff, dstOff + len) is written and none outside the source segment is read.
#include <mutex>
#include <type_traits>

#include "copy_range.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

typedef mscclppAmdAllToAllSeg A2ASeg;

// The segment table of a launch: by value for the one-view (one rank per process) launch -- nothing
// to copy, and a captured graph keeps it in the kernel node -- and through a device buffer
// ([view][kMaxRanks]) for the in-process launch, whose 8 views leave no room for 64 entries in the
// 4 KiB of kernel arguments.
template <int NV>
struct A2ASegs {
  const A2ASeg* tab;
  __device__ __forceinline__ A2ASeg at(int view, int p) const { return tab[view * kMaxRanks + p]; }
};
template <>
struct A2ASegs<1> {
  A2ASeg s[kMaxRanks];
  __device__ __forceinline__ A2ASeg at(int, int p) const { return s[p]; }
};

template <int NV>
struct A2AArgs {
  Views<NV> views;
  A2ASegs<NV> segs;
  uint64_t budget;
  uint64_t* trace;  // phase stamps: 0 start, 1 entry handshake done, 2 segments stored, 3 end
  int nranks;
  int pad;
};
struct A2ATableArg {
  A2ASeg s[kMaxRanks * kMaxRanks];
};
constexpr size_t kKernargLimit = 4096;
static_assert(sizeof(mscclppAmdRankView) == 336, "Views<kMaxRanks> is sized against the kernel-argument limit");
static_assert(sizeof(A2AArgs<1>) <= kKernargLimit, "one-view AllToAll arguments exceed the kernel-argument limit");
static_assert(sizeof(A2AArgs<kMaxRanks>) <= kKernargLimit, "in-process AllToAll arguments exceed the kernel-argument limit");
static_assert(sizeof(A2ATableArg) + 16 <= kKernargLimit, "the staged segment table exceeds the kernel-argument limit");

template <int NV, int U>
__global__ void __launch_bounds__(512) alltoallKernel(A2AArgs<NV> a) {
  const int vi = NV == 1 ? 0 : (int)blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const uint32_t T = blockDim.x, tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
  trace_stamp(a.trace, 0);
  block_handshake(v, n, rank, b, a.budget);
  trace_stamp(a.trace, 1);
#pragma unroll 1
  for (int s = 0; s < n; ++s) {
    const int p = (int)(((uint32_t)(rank + 1 + s) + b) % (uint32_t)n);
    const A2ASeg seg = a.segs.at(vi, p);
    const uint64_t blk = blockBytes(seg.len, nb);
    const uint64_t bOff = (uint64_t)b * blk;
    if (bOff >= seg.len) continue;
    const uint64_t len = seg.len - bOff < blk ? seg.len - bOff : blk;
    uint8_t* dst = (uint8_t*)v.output + seg.dstOff + bOff;
    if (p == rank)
      copy_range<kPlain, U>((const uint8_t*)v.input + seg.srcOff + bOff, dst, len, tid, T);
    else
      copy_range<kSystem, U>((const uint8_t*)v.peerInput[p] + seg.srcOff + bOff, dst, len, tid, T);
  }
  trace_stamp(a.trace, 2);
  block_handshake(v, n, rank, b, a.budget);
  trace_stamp(a.trace, 3);
}

__global__ void alltoallTableKernel(A2ATableArg t, A2ASeg* dst) {
  if (threadIdx.x < kMaxRanks * kMaxRanks) dst[threadIdx.x] = t.s[threadIdx.x];
}

// 256 KiB of the busiest rank's receive bytes per workgroup, 8..128 workgroups.  Every rank of a
// collective must launch the same grid (workgroup b hand-shakes with the peers' workgroup b), so a
// caller with one view passes the shape it derived from what every rank knows.
int alltoallDefaultBlocks(uint64_t maxRecvBytes) {
  const uint64_t want = (maxRecvBytes + (256u << 10) - 1) / (256u << 10);
  return (int)(want < 8 ? 8 : want > 128 ? 128 : want);
}

// Device copies of the in-process launches' tables: a ring of slots per device, each filled on the
// launch's stream right before its kernel (so a captured graph refills its slot at every replay).
// A slot comes round again after kTableSlots launches; the in-process harness (tests, tools) keeps
// far fewer in flight.  The ring is allocated at a device's first launch, which therefore must not
// happen under stream capture.
constexpr int kTableSlots = 64, kTableDevices = 64;
static A2ASeg* nextTableSlot() {
  static std::mutex mu;
  static A2ASeg* ring[kTableDevices] = {};
  static unsigned next[kTableDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kTableDevices) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!ring[dev] && hipMalloc((void**)&ring[dev], (size_t)kTableSlots * sizeof(A2ATableArg)) != hipSuccess) {
    ring[dev] = nullptr;
    return nullptr;
  }
  return ring[dev] + (size_t)(next[dev]++ % kTableSlots) * kMaxRanks * kMaxRanks;
}

// segs: host, [nviews][nranks].
int launchAllToAll(const mscclppAmdRankView* views, int nviews, int nranks, const A2ASeg* segs, int nblocks,
                   int nthreads, uint64_t budget, hipStream_t s) {
  if (nblocks <= 0) {
    uint64_t most = 0;
    for (int i = 0; i < nviews; ++i) {
      uint64_t sum = 0;
      for (int p = 0; p < nranks; ++p) sum += segs[i * nranks + p].len;
      most = sum > most ? sum : most;
    }
    nblocks = alltoallDefaultBlocks(most);
  }
  if (!launchShapeOk(nblocks, kMaxChannels, nthreads)) return 4;
  for (int i = 0; i < nviews * nranks; ++i)
    if (blockBytes(segs[i].len, (uint32_t)nblocks) > kBlkOffsetLimit) return 5;
  return launchViews(alltoallKernel<1, 4>, alltoallKernel<kMaxRanks, 4>, views, nviews, nblocks, nthreads, s, [&](auto& a) {
    a.budget = budget;
    a.trace = g_mscclppAmdTrace;
    a.nranks = nranks;
    if constexpr (std::is_same_v<decltype(a.segs), A2ASegs<1>>) {
      for (int p = 0; p < nranks; ++p) a.segs.s[p] = segs[p];
    } else {  // the table of every view goes through a device slot, filled on the stream right before the kernel
      A2ATableArg t{};
      for (int i = 0; i < nviews; ++i)
        for (int p = 0; p < nranks; ++p) t.s[i * kMaxRanks + p] = segs[i * nranks + p];
      A2ASeg* slot = nextTableSlot();
      if (!slot) return 1;
      hipLaunchKernelGGL(alltoallTableKernel, dim3(1), dim3(64), 0, s, t, slot);
      a.segs.tab = slot;
    }
    return 0;
  });
}

}  // namespace mscclpp_amd
