// ncclReduce: a one-shot zero-copy pull-reduce at the root.
//
// The reference leaves ncclReduce to the vendor library (nccl.cc:521-542 returns ncclInternalError
// without one), so this is no restatement.  Only the root moves data: it reads every peer's send
// buffer in place over xGMI (system-scope 16-byte buffer loads, as allreduceZeroCopyKernel reads its
// slice), reduces in ring order starting at itself -- root, root+1, ..., root+n-1 (mod n) -- and
// stores the result into its own receive buffer with plain local stores.  Nothing is written to any
// peer (remote plain / nt stores into user buffers went stale).
//
//  * Every rank launches the same grid; workgroup b hand-shakes with the peers' workgroup b on
//    channel b at entry and at exit, also a workgroup whose sub-range is empty.  Entry: all send
//    buffers are final (their producers ran earlier on the ranks' streams) and the root's earlier
//    stream work on its receive buffer is over.  Exit: the root has finished reading, so a non-root
//    rank may overwrite its send buffer in its next stream operation.  Non-root workgroups do nothing
//    between the two handshakes: they read and write no user memory.
//  * On the root workgroup b owns [b * blk, (b + 1) * blk) of the message (blockBytes).  Per
//    16-byte unit: the own unit by a local load, the same unit of every peer by system-scope loads,
//    all issued before any arithmetic; U units per lane are in flight (the loads of all U units come
//    first, then the reduces and stores).  A lane stores only units it has itself loaded, so the
//    root may reduce in place (send == recv).
//  * The arithmetic is the other bulk kernels': Accum<DT, OP, 4> where the accumulation type is
//    wider than the element (fp8 in half / float), reduce4<DT, OP> otherwise.
//  * The last unit of a message that is no multiple of 16 bytes moves byte by byte (load_tail /
//    store_tail): no byte outside [recv, recv + bytes) is written and none outside a send buffer's
//    `bytes` is read.  Pointers need their element's alignment only, and the misalignment may differ
//    between ranks and between a rank's send and receive buffers: each buffer is addressed through a
//    descriptor of its own, rebased to the workgroup's range (64-bit), with 32-bit offsets inside it.
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

// Units per lane in flight, from the resource report of the 60 instantiations (hipcc
// -Rpass-analysis=kernel-resource-usage; none uses scratch at any U):
//   U = 1: 53..82 VGPRs, 5..7 waves per SIMD (most are held at 7 by their SGPRs: 8 descriptors);
//   U = 2: 88..116 VGPRs, 4..5 waves per SIMD;   U = 4: 158..186 VGPRs, 2..3 waves per SIMD.
// One rank per process launches at most 128 workgroups of 8 waves on 256 CUs, 2 waves per SIMD, so
// there occupancy buys nothing and the loads in flight per lane (U * n * 16 bytes) hide the xGMI
// latency.  U = 2 doubles them (256 bytes per lane at 8 ranks) and still leaves two 512-lane
// workgroups per CU, which the in-process launch of 8 ranks x 64 workgroups needs to be resident at
// once; U = 4 would leave one (8 x 32).
constexpr int kReduceUnits = 2;

template <int NV>
struct ReduceArgs {
  Views<NV> views;
  uint64_t bytes;
  uint64_t blk;     // blockBytes(bytes, gridDim.x)
  uint64_t budget;
  uint64_t* trace;  // phase stamps: 0 start, 1 entry handshake done, 2 result stored, 3 end
  int nranks;
  int root;
};
static_assert(sizeof(ReduceArgs<kMaxRanks>) <= 4096, "in-process Reduce arguments exceed the kernel-argument limit");

template <int DT, int OP, int NV, int U>
__global__ void __launch_bounds__(512) reduceKernel(ReduceArgs<NV> a) {
  const mscclppAmdRankView& v = a.views.v[NV == 1 ? 0 : blockIdx.y];
  const int rank = v.rank, n = a.nranks, root = a.root;
  const uint32_t T = blockDim.x, tid = threadIdx.x, b = blockIdx.x;
  trace_stamp(a.trace, 0);
  block_handshake(v, n, rank, b, a.budget);
  trace_stamp(a.trace, 1);
  const uint64_t bOff = (uint64_t)b * a.blk;
  if (rank == root && bOff < a.bytes) {
    const uint64_t len = a.bytes - bOff < a.blk ? a.bytes - bOff : a.blk;  // <= kBlkOffsetLimit
    const uint32_t nUnits = (uint32_t)((len + 15) / 16);
    const uint8_t* own = (const uint8_t*)v.input + bOff;
    uint8_t* dst = (uint8_t*)v.output + bOff;
    const auto rin = make_rsrc(own);
    const auto rout = make_rsrc(dst);
    const uint8_t* pin[kMaxRanks];  // pin[k]: the send buffer of the k-th rank after the root, this range
#pragma unroll
    for (int k = 1; k < kMaxRanks; ++k) pin[k] = k < n ? (const uint8_t*)v.peerInput[(root + k) % n] + bOff : nullptr;
    for (uint32_t u0 = tid; u0 < nUnits; u0 += T * U) {
      u32x4 w[U][kMaxRanks];
      uint32_t vb[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + i * T;
        vb[i] = u < nUnits ? clamp_valid(len, (uint64_t)u * 16, 16) : 0;
        if (vb[i] == 0) continue;
        w[i][0] = load_payload<kNonTemporal>(rin, own, (uint64_t)u * 16, vb[i]);
#pragma unroll
        for (int k = 1; k < kMaxRanks; ++k)
          if (k < n)
            w[i][k] = vb[i] >= 16 ? load16<kSystem>(make_rsrc(pin[k]), u * 16u) : load_tail(pin[k] + (uint64_t)u * 16, vb[i]);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (vb[i] == 0) continue;
        const uint32_t u = u0 + i * T;
        u32x4 acc;
        if constexpr (AccWord<DT, OP>::kWide) {
          Accum<DT, OP, 4> sum(w[i][0]);
#pragma unroll
          for (int k = 1; k < kMaxRanks; ++k)
            if (k < n) sum.add(w[i][k]);
          acc = sum.template get<u32x4>();
        } else {
          acc = w[i][0];
#pragma unroll
          for (int k = 1; k < kMaxRanks; ++k)
            if (k < n) acc = reduce4<DT, OP>(acc, w[i][k]);
        }
        store_payload<kPlain>(rout, dst, (uint64_t)u * 16, acc, vb[i]);
      }
    }
  }
  trace_stamp(a.trace, 2);
  block_handshake(v, n, rank, b, a.budget);
  trace_stamp(a.trace, 3);
}

// 32 KiB of the message per workgroup, 8..64 workgroups.  Broadcast and AllToAll take 256 KiB per
// workgroup, 8..128, but there every rank's workgroups move data; here only the root's do, and the
// in-process sweep (8, 32 and 64 workgroups are the fastest 512-lane grids at 64 KiB,
// 1 MiB and 48 MiB) wants them earlier.  The upper end is 64 so that the default grid of 8
// in-process ranks (8 x 64 workgroups of 512 lanes, two per CU) is resident at once at this kernel's
// register count.  Every rank of a collective must launch the same grid (workgroup b hand-shakes
// with the peers' workgroup b): the rule takes the byte count alone.
int reduceDefaultBlocks(uint64_t bytes) {
  const uint64_t want = (bytes + (32u << 10) - 1) / (32u << 10);
  return (int)(want < 8 ? 8 : want > 64 ? 64 : want);
}

template <int DT, int OP>
static int launchReduceT(const mscclppAmdRankView* views, int nviews, int nranks, uint64_t bytes, uint64_t blk, int root,
                         int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  return launchViews(reduceKernel<DT, OP, 1, kReduceUnits>, reduceKernel<DT, OP, kMaxRanks, kReduceUnits>, views, nviews,
                     nblocks, nthreads, s, [&](auto& args) {
                       args.bytes = bytes;
                       args.blk = blk;
                       args.budget = budget;
                       args.trace = g_mscclppAmdTrace;
                       args.nranks = nranks;
                       args.root = root;
                       return 0;
                     });
}

int launchReduce(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype, int op, int root,
                 int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  if (nblocks <= 0) nblocks = reduceDefaultBlocks(bytes);
  if (!launchShapeOk(nblocks, kMaxChannels, nthreads)) return 4;
  if (root < 0 || root >= nranks || bytes == 0) return 4;
  if (dtype < 0 || dtype >= MSCCLPP_AMD_NUM_DTYPES || (op != kSum && op != kMin) || bytes % (size_t)elem_bytes(dtype))
    return 4;
  const uint64_t blk = blockBytes(bytes, (uint32_t)nblocks);
  if (blk > kBlkOffsetLimit) return 5;  // more workgroups needed: one workgroup's range is one descriptor
  MSCCLPP_AMD_DISPATCH_ALL(dtype, op, launchReduceT, views, nviews, nranks, (uint64_t)bytes, blk, root, nblocks, nthreads,
                           budget, s);
}

}  // namespace mscclpp_amd
