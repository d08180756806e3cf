// ncclSend / ncclRecv (and their groups): a zero-copy pull over xGMI, one launch per rank running a
// small table of point-to-point operations.
//
// The reference leaves both calls to the vendor library (nccl.cc:774-792 returns ncclInternalError
// without one), so this is no restatement.  Data moves as in alltoall.hip: the RECEIVER reads the
// bytes straight out of the sender's buffer (system-scope loads through the IPC mapping) and stores
// them into its own buffer with plain stores; nothing is ever stored into a peer's user buffer
// (DESIGN.md §5), and the sender's part of the kernel moves no data at all.
//
// An operation {src, dst, send, recv, bytes} is run by the views that are its src or its dst.
// Synchronisation is pairwise and one-way, so the operations fused into one launch cannot form a
// wait cycle (a ring where every rank sends to r + 1 and receives from r - 1 would, with a symmetric
// handshake per operation: each rank would sit in a handshake whose partner sits in another one):
//
//  1. entry: every send operation posts "ready" to its receiver and waits for nothing.  Ready says:
//     the kernel has started, so the send buffer's producers, earlier on the sender's stream, are over.
//  2. the receive operations run in table order: wait for the sender's "ready", pull the
//     workgroup's sub-range, drain the stores, post "done" to the sender.
//  3. exit: every send operation waits for its "done", so the sender's kernel does not end while its
//     buffer is still being read, and its next stream operation may overwrite the buffer.
//
// A wait of step 2 depends only on the sender's kernel having started, a wait of step 3 only on the
// receiver having reached that operation: both follow table order on every rank, and a launch whose
// peers were all launched completes.  (What still deadlocks is the NCCL classic: two ranks that each
// issue an UNGROUPED send to the other before their receive, i.e. two kernels per stream.)
//
// Channels.  nb(op) workgroups carry an operation, a pure function of its byte count
// (sendrecvBlocks), so both sides derive it alone; workgroup b < nb(op) owns channel base + b and the
// sub-range [b * blk, (b + 1) * blk), blk = ceil(bytes / nb) rounded up to 16.  base = 0 when the
// sender has the lower rank, kSRDirChannels otherwise: the two directions of a pair never share a
// token slot, or B's "done" for A -> B could be taken by A for B's "ready" of B -> A when B issues
// the two in separate kernels.  Per (pair, channel) an operation costs each side one token_post and
// one token_wait, exactly one block_handshake's worth, so the counters stay in step with the
// collectives that share them.  Several operations of one pair and direction count up on the
// channels they share: the k-th send meets the k-th receive.  The grid is the largest nb of the
// table; a workgroup skips the operations with nb(op) <= b.
#include "copy_range.hpp"
#include "handshake.hpp"
#include "launch.hpp"

namespace mscclpp_amd {

typedef mscclppAmdSendRecvOp SROp;

constexpr int kSRMaxOps = MSCCLPP_AMD_SENDRECV_MAX_OPS;
constexpr int kSRDirChannels = kMaxChannels / 2;  // channels (and most workgroups) per direction of a pair
static_assert(2 * kSRDirChannels <= kMaxChannels, "both directions of a pair need their own channels");
static_assert(kSRMaxOps <= 64, "one lane of the first wave per operation posts and awaits its tokens");

// Loads in flight per lane (U x 16 bytes), from the resource report of the two instantiations
// (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no scratch at any U):
//   U = 1, 2, 4, 8 -> 22, 27, 37, 59 VGPRs in both; SGPRs 74, 75, 78, 87 with one view and 70, 71,
//   74, 81 with eight; the report says 8 waves per SIMD for all of them.
// VGPRs never limit occupancy, so U is not bought with waves.  SGPRs do at U = 8: above 80 a CU admits
// one wave per SIMD fewer than the report and the occupancy query say, and the largest in-process
// launch the launcher admits (8 views x 128 workgroups x 8 waves: every wave slot of 256 CUs) would
// strand workgroups that the resident ones wait for.  U = 4 stays at or below 78 and is AllToAll's
// value, 64 bytes of loads per lane in flight; the in-process sweep has no fabric
// latency to hide, so it cannot rank the smaller values, and the choice stays AllToAll's until a
// sweep over real xGMI says otherwise.
constexpr int kSendRecvUnits = 4;

// Workgroups of an operation: kSRBytesPerBlock of the message each, 1..kSRDefaultMaxBlocks.  The rule
// takes the byte count alone (sender and receiver derive the same value with no exchange); `force`
// > 0 is the explicit grid of the tests and the sweep (up to kSRDirChannels).  128 KiB comes from the
// in-process sweep (512 lanes, us for one transfer / a ring of eight): a workgroup
// alone moves about 50 GB/s, so 1 MiB wants 8 workgroups (6.2 / 8.8; 4: 7.8 / 9.8; 16: 5.5 / 10.4)
// and 64 KiB one (4.8 / 5.4; 4: 4.0 / 5.2; 16: 4.6 / 7.6).  AllToAll's 256 KiB gives 1 MiB four.  The
// default stops at 64, as Reduce's: 8 in-process views x 64 workgroups of 512 lanes fill half the wave
// slots of 256 CUs, a margin that a launch at 128 (all of them) does not have; 48 MiB at 64 runs at
// 24.7 / 191 us (32: 37.8 / 182).
constexpr uint64_t kSRBytesPerBlock = 128u << 10;
constexpr uint64_t kSRDefaultMaxBlocks = 64;
__host__ __device__ inline uint32_t sendrecvBlocks(uint64_t bytes, int force) {
  if (force > 0) return (uint32_t)force;
  const uint64_t want = (bytes + kSRBytesPerBlock - 1) / kSRBytesPerBlock;
  return (uint32_t)(want < 1 ? 1 : want > kSRDefaultMaxBlocks ? kSRDefaultMaxBlocks : want);
}
__host__ __device__ inline uint32_t sendrecvChannelBase(int src, int dst) { return src < dst ? 0u : (uint32_t)kSRDirChannels; }

// What the kernel needs of a rank view: the token plumbing (a quarter of mscclppAmdRankView, so that
// eight views and the table travel by value in one launch's arguments).
struct SRView {
  uint64_t* tokens;
  uint64_t* expected;
  uint32_t* err;
  uint64_t* peerTokens[kMaxRanks];
  int32_t rank;
  int32_t pad;
};

template <int NV>
struct SRArgs {
  SRView views[NV];
  SROp ops[kSRMaxOps];
  uint64_t budget;
  uint64_t* trace;  // phase stamps: 0 start, 1 readies posted, 2 receives stored, 3 dones seen
  int nops;
  int force;        // > 0: nb of every operation
};
static_assert(sizeof(SROp) == 32, "mscclppAmdSendRecvOp is part of the C ABI");
static_assert(sizeof(SRArgs<1>) <= 4096, "one-view Send/Recv arguments exceed the kernel-argument limit");
static_assert(sizeof(SRArgs<kMaxRanks>) <= 4096, "in-process Send/Recv arguments exceed the kernel-argument limit");

template <int NV, int U>
__global__ void __launch_bounds__(512) sendrecvKernel(SRArgs<NV> a) {
  const SRView& v = a.views[NV == 1 ? 0 : blockIdx.y];
  const int rank = v.rank, nops = a.nops;
  const uint32_t T = blockDim.x, tid = threadIdx.x, b = blockIdx.x;
  trace_stamp(a.trace, 0);
  // lane i of the first wave owns the tokens of send operation i (nops <= 64 <= T)
  bool sends = false;
  int to = 0;
  uint32_t ch = 0;
  if (tid < (uint32_t)nops) {
    const SROp op = a.ops[tid];
    sends = op.src == rank && b < sendrecvBlocks(op.bytes, a.force);
    to = op.dst;
    ch = sendrecvChannelBase(op.src, op.dst) + b;
  }
  if (sends) token_post(v.peerTokens[to], rank, ch);
  trace_stamp(a.trace, 1);
#pragma unroll 1
  for (int i = 0; i < nops; ++i) {
    const SROp op = a.ops[i];
    if (op.dst != rank) continue;
    const uint32_t nb = sendrecvBlocks(op.bytes, a.force);
    if (b >= nb) continue;  // (uniform over the workgroup: the barriers below are safe)
    const uint32_t rch = sendrecvChannelBase(op.src, op.dst) + b;
    if (tid == 0) token_wait(v.tokens, v.expected, v.err, op.src, rank, rch, a.budget);
    __syncthreads();
    const uint64_t blk = blockBytes(op.bytes, nb), bOff = (uint64_t)b * blk;
    if (bOff < op.bytes) {
      const uint64_t len = op.bytes - bOff < blk ? op.bytes - bOff : blk;  // <= kBlkOffsetLimit
      copy_range<kSystem, U>((const uint8_t*)op.send + bOff, (uint8_t*)op.recv + bOff, len, tid, T);
    }
    drain_stores();
    __syncthreads();
    if (tid == 0) token_post(v.peerTokens[op.src], rank, rch);
  }
  trace_stamp(a.trace, 2);
  if (sends) token_wait(v.tokens, v.expected, v.err, to, rank, ch, a.budget);
  trace_stamp(a.trace, 3);
}

int sendrecvDefaultBlocks(uint64_t bytes) { return (int)sendrecvBlocks(bytes, 0); }

// Every argument was checked by the caller (mscclppAmdSendRecvLaunch) except the launch shape and
// the sizes; nothing here touches the device before those checks have passed.
int launchSendRecv(const mscclppAmdRankView* views, int nviews, int nranks, const SROp* ops, int nops, int nblocks,
                   int nthreads, uint64_t budget, hipStream_t s) {
  if (!launchShapeOk(nblocks, kSRDirChannels, nthreads)) return 4;
  if (nops < 1 || nops > kSRMaxOps) return 4;
  uint32_t grid = 0;
  for (int i = 0; i < nops; ++i) {
    const uint32_t nb = sendrecvBlocks(ops[i].bytes, nblocks);
    if (blockBytes(ops[i].bytes, nb) > kBlkOffsetLimit) return 5;  // more workgroups carry it
    grid = nb > grid ? nb : grid;
  }
  auto go = [&](auto kern, auto args) {
    for (int i = 0; i < nviews; ++i) {
      SRView& v = args.views[i];
      v.tokens = views[i].tokens;
      v.expected = views[i].expected;
      v.err = views[i].err;
      for (int q = 0; q < nranks; ++q) v.peerTokens[q] = views[i].peerTokens[q];
      v.rank = views[i].rank;
    }
    for (int i = 0; i < nops; ++i) args.ops[i] = ops[i];
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.nops = nops;
    args.force = nblocks > 0 ? nblocks : 0;
    return launchResident(kern, kern, (int)grid, nviews, nthreads, s, args);
  };
  if (nviews == 1) return go(sendrecvKernel<1, kSendRecvUnits>, SRArgs<1>{});
  return go(sendrecvKernel<kMaxRanks, kSendRecvUnits>, SRArgs<kMaxRanks>{});
}

}  // namespace mscclpp_amd
