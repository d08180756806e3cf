// ncclMax / ncclAvg for Reduce, ReduceScatter and AllReduce, SUM / MIN / MAX / AVG of int64, uint64
// and int8, and PreMulSum (ncclRedOpCreatePreMulSum) of fp16 / bf16 / fp32: one zero-copy pull-reduce
// kernel.
//
// The reference carries SUM and MIN of fp16, bf16, fp32, int32, uint32, uint8 and fp8 (and leaves the
// other operations and types to the vendor library), so
// this is no restatement; the arithmetic is defined in mscclpp_amd/pull_reduce_device.hpp.  As in
// reduce.hip every load of a peer's memory is a system-scope 16-byte buffer load of its user
// buffer in place, the reduction happens in registers, and every store is a plain store into the
// rank's own receive buffer: nothing is written to any peer.
//
//  * Geometry: a host-computed table.  Rank q reduces [srcOff[q], srcOff[q] + len[q]) of EVERY
//    rank's send buffer, in rank order 0 .. n - 1, and stores the result at dstOff[q] of its own
//    receive buffer.  Reduce: only the root's len is non-zero; ReduceScatter: srcOff[q] = q * bytes;
//    AllReduce: q's slice of the message, and `gather` is set.  One `blk` (bytes per workgroup, a
//    multiple of 16) comes from the largest len, so workgroup b owns the same sub-range b of every
//    rank's range, and hand-shakes with the peers' workgroup b on channel b only.
//  * Entry handshake (every workgroup, also one whose share is empty): all send buffers are final
//    and every rank's earlier stream work on its receive buffer is over.
//  * Phase 1: per 16-byte unit the own unit by a local load and the same unit of every peer's send
//    buffer by load16<kSystem>, each at its position in rank order; the loads of all U units of a
//    lane are issued before any arithmetic.  A lane stores only units it has itself loaded, and a
//    rank's peers read from its send buffer only THEIR ranges, so the in-place forms hold: Reduce
//    with send == recv on the root, ReduceScatter with recv == send + rank * bytes, AllReduce with
//    send == recv.
//  * AllReduce only: a middle handshake, then for every q != rank sub-range b of q's slice is
//    copied out of peerOutput[q] (load16<kSystem>) into the own receive buffer.  Visibility is
//    allreduceTestK5Kernel's discipline (allreduce_bulk.hip): phase 1 stores plainly, every wave
//    drains its stores (s_waitcnt vmcnt(0)) and meets the workgroup barrier inside block_handshake,
//    whose signalling lanes then run a system-scope release fence (the XCD's L2 written back, and
//    waited for) before the token add; the peer reads with system-scope loads after its acquire.
//    Write-through (sc0 sc1) stores would drop the lines from the L2 that the same rank's next
//    kernel reads the result from, for no gain: the release is paid by the handshake anyway.
//  * 64-bit elements span two words of a unit: their accumulators take and return a word pair
//    (pull_acc_words).  A range that ends on an odd 64-bit element has an 8-byte tail, moved byte by
//    byte like any other; the zero-filled rest of that unit is reduced and not stored.
//  * Exit handshake: every reader is done with this rank's send and receive buffers.
//  * PreMulSum only: every rank has a scalar of its own, and the rank that reduces a range needs
//    every rank's.  They are exchanged inside the kernel, per workgroup, through the DIAGONAL of the
//    token arrays: slot [rank][b] of a rank's own array, which no handshake touches (a rank never
//    signals itself), which every peer has mapped already (peerTokens[rank]), and which is uncached
//    memory.  Lane 0 of workgroup b (also one whose share is empty) stores its view's scalar there --
//    the fp32 bits in the 64-bit word, a system-scope store -- before the entry handshake, whose drain,
//    barrier and release publish it with the token add; after the handshake's acquire lane k < n of
//    every wave reads rank k's slot with a system-scope load (one round trip for all n) and the wave
//    reads the values out lane by lane (v_readlane): they are uniform and cost SGPRs, not VGPRs.
//    Every peer reads them before it enters any later handshake, so after the exit handshake no
//    reader is left and lane 0 stores 0 back: a token array equals its expected counters after every
//    launch, as before.  The next launch of the rank on the stream publishes after this one's end.
//    The scalar is an immediate in the kernel arguments, or is read by lane 0 through a device
//    pointer to one element of the element type when the kernel runs (a graph replay sees the value
//    of its own time).
//  * Tails and alignment as reduce.hip: the last unit of a range that is no multiple of 16 bytes
//    moves byte by byte; no byte outside [recv + dstOff, + len) is written and none outside a send
//    buffer's extent is read.  Pointers need their element's alignment only and the misalignment
//    may differ between ranks and between send and receive: one descriptor per buffer, rebased to
//    the workgroup's range (64-bit), with 32-bit offsets inside it.
#include "handshake.hpp"
#include "launch.hpp"
#include "mscclpp_amd/pull_reduce_device.hpp"

#include <type_traits>

namespace mscclpp_amd {

// Units per lane in flight, from the resource report of the 62 instantiations (hipcc
// -Rpass-analysis=kernel-resource-usage; DESIGN.md §17d, §17e and §17f have the tables; none uses
// scratch, the 64-bit AVG stays at 96 VGPRs and PreMulSum at 92 with U = 2, so no instantiation needs
// a U of its own).  As for
// reduceKernel, U = 2 keeps 256 bytes of loads per lane in flight at 8 ranks and stays at or below
// 128 VGPRs, i.e. two 512-lane workgroups per CU, which the in-process launch of 8 ranks x 64
// workgroups needs to be resident at once.
constexpr int kPullReduceUnits = 2;

template <int NV>
struct PullReduceArgs {
  Views<NV> views;
  uint64_t srcOff[kMaxRanks];  // rank q reduces [srcOff[q], + len[q]) of every send buffer
  uint64_t dstOff[kMaxRanks];  // into its receive buffer at dstOff[q]
  uint64_t len[kMaxRanks];
  uint64_t blk;     // blockBytes(max len, gridDim.x): of the largest range of the collective
  uint64_t budget;
  uint64_t* trace;  // phase stamps: 0 start, 1 entry handshake done, 2 reduced, 3 gathered, 4 end
  float invN;       // 1.0f / (float)nranks, computed once by the host (AVG of the float types)
  int nranks;
  int gather;       // AllReduce: phase 2 copies the peers' reduced slices
};
// PreMulSum's arguments: the same and a scalar per view.  A type of its own, because a longer
// argument block moves the implicit arguments behind it (the block size is read from there) and so
// changes the code of every kernel that takes it: the other operations keep theirs to the byte.
template <int NV>
struct PullPreMulArgs : PullReduceArgs<NV> {
  float scale[NV];            // the rank's scalar, unless ...
  const void* scalePtr[NV];   // ... non-null: one element of the element type in device memory, read by the kernel
};
static_assert(sizeof(PullPreMulArgs<kMaxRanks>) <= 4096, "in-process pull-reduce arguments exceed the kernel-argument limit");

template <int OP, int NV>
using PullArgsFor = std::conditional_t<OP == kPullPreMulSum, PullPreMulArgs<NV>, PullReduceArgs<NV>>;

template <int DT, int OP, int NV, int U>
__global__ void __launch_bounds__(512) pullReduceKernel(PullArgsFor<OP, NV> a) {
  const mscclppAmdRankView& v = a.views.v[NV == 1 ? 0 : blockIdx.y];
  const int rank = v.rank, n = a.nranks;
  const uint32_t T = blockDim.x, tid = threadIdx.x, b = blockIdx.x;
  trace_stamp(a.trace, 0);
  [[maybe_unused]] float sc[kMaxRanks];  // PreMulSum: rank k's scalar
  if constexpr (OP == kPullPreMulSum) {
    if (tid == 0) {
      const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
      const float s = a.scalePtr[vi] ? premul_scalar_at<DT>(a.scalePtr[vi]) : a.scale[vi];
      st_relaxed_sys(v.tokens + (uint64_t)rank * kMaxChannels + b, (uint64_t)__builtin_bit_cast(uint32_t, s));
    }
  }
  block_handshake(v, n, rank, b, a.budget);
  if constexpr (OP == kPullPreMulSum) {
    // lane k < n of every wave loads rank k's slot (one round trip for all of them), and the values
    // are then read out of its register lane by lane: uniform, so they cost SGPRs, not VGPRs
    const int lane = (int)(tid & 63u);
    uint32_t got = 0;
    if (lane < n) {
      const uint64_t* slot = (lane == rank ? v.tokens : v.peerTokens[lane]) + (uint64_t)lane * kMaxChannels + b;
      got = (uint32_t)ld_relaxed_sys(slot);
    }
#pragma unroll
    for (int k = 0; k < kMaxRanks; ++k) sc[k] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_readlane((int)got, k));
  }
  trace_stamp(a.trace, 1);
  const uint64_t bOff = (uint64_t)b * a.blk;
  if (bOff < a.len[rank]) {
    const uint64_t left = a.len[rank] - bOff;
    const uint64_t len = left < a.blk ? left : a.blk;  // <= kBlkOffsetLimit
    const uint32_t nUnits = (uint32_t)((len + 15) / 16);
    const uint64_t sOff = a.srcOff[rank] + bOff;
    const uint8_t* own = (const uint8_t*)v.input + sOff;
    uint8_t* dst = (uint8_t*)v.output + a.dstOff[rank] + bOff;
    const auto rin = make_rsrc(own);
    const auto rout = make_rsrc(dst);
    const uint8_t* pin[kMaxRanks];  // pin[k]: rank k's send buffer, this range
#pragma unroll
    for (int k = 0; k < kMaxRanks; ++k) pin[k] = k < n && k != rank ? (const uint8_t*)v.peerInput[k] + sOff : nullptr;
    for (uint32_t u0 = tid; u0 < nUnits; u0 += T * U) {
      u32x4 w[U][kMaxRanks];
      uint32_t vb[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t u = u0 + i * T;
        vb[i] = u < nUnits ? clamp_valid(len, (uint64_t)u * 16, 16) : 0;
        if (vb[i] == 0) continue;
#pragma unroll
        for (int k = 0; k < kMaxRanks; ++k)
          if (k < n) {
            if (k == rank)
              w[i][k] = load_payload<kNonTemporal>(rin, own, (uint64_t)u * 16, vb[i]);
            else
              w[i][k] = vb[i] >= 16 ? load16<kSystem>(make_rsrc(pin[k]), u * 16u) : load_tail(pin[k] + (uint64_t)u * 16, vb[i]);
          }
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (vb[i] == 0) continue;
        const uint32_t u = u0 + i * T;
        u32x4 r;
        if constexpr (pull_acc_words(DT) == 2) {  // a 64-bit element: words j (low) and j + 1
#pragma unroll
          for (int j = 0; j < 4; j += 2) {
            PullAcc<DT, OP> acc;
            acc.first(w[i][0][j] | (uint64_t)w[i][0][j + 1] << 32);
#pragma unroll
            for (int k = 1; k < kMaxRanks; ++k)
              if (k < n) acc.next(w[i][k][j] | (uint64_t)w[i][k][j + 1] << 32);
            const uint64_t e = acc.word(n, a.invN);
            r[j] = (uint32_t)e;
            r[j + 1] = (uint32_t)(e >> 32);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            PullAcc<DT, OP> acc;
            if constexpr (OP == kPullPreMulSum) {
              acc.first(w[i][0][j], sc[0]);
#pragma unroll
              for (int k = 1; k < kMaxRanks; ++k)
                if (k < n) acc.next(w[i][k][j], sc[k]);
            } else {
              acc.first(w[i][0][j]);
#pragma unroll
              for (int k = 1; k < kMaxRanks; ++k)
                if (k < n) acc.next(w[i][k][j]);
            }
            r[j] = acc.word(n, a.invN);
          }
        }
        store_payload<kPlain>(rout, dst, (uint64_t)u * 16, r, vb[i]);
      }
    }
  }
  trace_stamp(a.trace, 2);
  if (a.gather) {
    block_handshake(v, n, rank, b, a.budget);  // every peer's sub-range b of its slice is reduced and released
#pragma unroll 1
    for (int k = 1; k < n; ++k) {
      const int q = (rank + k) % n;
      if (bOff >= a.len[q]) continue;
      const uint64_t left = a.len[q] - bOff;
      const uint64_t len = left < a.blk ? left : a.blk;
      const uint32_t nUnits = (uint32_t)((len + 15) / 16);
      const uint64_t off = a.dstOff[q] + bOff;
      const uint8_t* src = (const uint8_t*)v.peerOutput[q] + off;
      uint8_t* dst = (uint8_t*)v.output + off;
      const auto rs = make_rsrc(src);
      const auto rd = make_rsrc(dst);
      for (uint32_t u0 = tid; u0 < nUnits; u0 += T * U) {
        u32x4 w[U];
        uint32_t vb[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
          const uint32_t u = u0 + i * T;
          vb[i] = u < nUnits ? clamp_valid(len, (uint64_t)u * 16, 16) : 0;
          if (vb[i]) w[i] = load_payload<kSystem>(rs, src, (uint64_t)u * 16, vb[i]);
        }
#pragma unroll
        for (int i = 0; i < U; ++i)
          if (vb[i]) store_payload<kPlain>(rd, dst, (uint64_t)(u0 + i * T) * 16, w[i], vb[i]);
      }
    }
    trace_stamp(a.trace, 3);
  }
  block_handshake(v, n, rank, b, a.budget);
  if constexpr (OP == kPullPreMulSum) {  // every peer has read the scalar: the slot is 0 again
    if (tid == 0) st_relaxed_sys(v.tokens + (uint64_t)rank * kMaxChannels + b, 0);
  }
  trace_stamp(a.trace, 4);
}


int reduceDefaultBlocks(uint64_t bytes);  // reduce.hip

// The default grid is a function of (collective, bytes) alone, so every rank derives the same one;
// the rules are read off the in-process sweep of DESIGN.md §17d (8 ranks on one GPU, 512 lanes).
// Reduce: reduceDefaultBlocks (32 KiB of the message per workgroup, 8..64): only the root's workgroups
// move data, and 8 / 32 / 64 are the fastest grids at 64 KiB / 1 MiB / 48 MiB here as there.
// ReduceScatter (bytes = a rank's block): 32 KiB per workgroup, 8..32; AllReduce: 64 KiB of the message
// per workgroup, 8..32.  In both every rank's workgroups move data, and 32 beat 64 at 48 MiB per rank
// (8 ranks x 32 = one workgroup per CU of the one GPU measured; a rank alone on its GPU may want
// more, which nobody has measured).  No rule exceeds 64, so that 8 in-process ranks x the default
// grid of 512-lane workgroups (two per CU at this kernel's register count) are resident at once.
int pullReduceDefaultBlocks(int coll, uint64_t bytes) {
  if (coll == MSCCLPP_AMD_PULL_REDUCE) return reduceDefaultBlocks(bytes);
  const uint64_t per = coll == MSCCLPP_AMD_PULL_ALLREDUCE ? (64u << 10) : (32u << 10);
  const uint64_t want = (bytes + per - 1) / per;
  return (int)(want < 8 ? 8 : want > 32 ? 32 : want);
}

// The one statement of the geometry (bytes: the message of Reduce / AllReduce, the per-rank block
// of ReduceScatter).  Returns the largest len.
uint64_t pullReduceGeometry(int coll, int nranks, uint64_t bytes, int root, uint64_t* srcOff, uint64_t* dstOff,
                            uint64_t* len) {
  uint64_t most = 0;
  const uint64_t slice = ((bytes + (uint64_t)nranks - 1) / (uint64_t)nranks + 15) & ~15ull;
  for (int q = 0; q < kMaxRanks; ++q) {
    srcOff[q] = dstOff[q] = len[q] = 0;
    if (q >= nranks) continue;
    if (coll == MSCCLPP_AMD_PULL_REDUCE) {
      len[q] = q == root ? bytes : 0;
    } else if (coll == MSCCLPP_AMD_PULL_REDUCE_SCATTER) {
      srcOff[q] = (uint64_t)q * bytes;
      len[q] = bytes;
    } else {
      const uint64_t at = (uint64_t)q * slice;
      srcOff[q] = dstOff[q] = at < bytes ? at : 0;
      len[q] = at < bytes ? (bytes - at < slice ? bytes - at : slice) : 0;
    }
    most = len[q] > most ? len[q] : most;
  }
  return most;
}

template <int DT, int OP>
static int launchPullReduceT(const mscclppAmdRankView* views, int nviews, int nranks, int coll, uint64_t bytes, int root,
                             uint64_t blk, int nblocks, int nthreads, uint64_t budget, hipStream_t s,
                             const float* scales = nullptr, const void* const* scalePtrs = nullptr) {
  auto fill = [&](auto& args) {
    pullReduceGeometry(coll, nranks, bytes, root, args.srcOff, args.dstOff, args.len);
    args.blk = blk;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.invN = 1.0f / (float)nranks;
    args.nranks = nranks;
    args.gather = coll == MSCCLPP_AMD_PULL_ALLREDUCE;
    if constexpr (OP == kPullPreMulSum) {
      for (int i = 0; i < nviews; ++i) {
        args.scale[i] = scales[i];
        args.scalePtr[i] = scalePtrs ? scalePtrs[i] : nullptr;
      }
    }
    return 0;
  };
  return launchViews(pullReduceKernel<DT, OP, 1, kPullReduceUnits>, pullReduceKernel<DT, OP, kMaxRanks, kPullReduceUnits>,
                     views, nviews, nblocks, nthreads, s, fill);
}

#define MSCCLPP_AMD_PULL_CASE2(DT, ...)                                            \
  case DT * 4 + kPullMax: return launchPullReduceT<DT, kPullMax>(__VA_ARGS__);     \
  case DT * 4 + kPullAvg: return launchPullReduceT<DT, kPullAvg>(__VA_ARGS__);
// int64 / uint64 / int8: SUM and MIN as well (the other types take those to their own kernels)
#define MSCCLPP_AMD_PULL_CASE4(DT, ...)                                            \
  case DT * 4 + kSum: return launchPullReduceT<DT, kSum>(__VA_ARGS__);             \
  case DT * 4 + kMin: return launchPullReduceT<DT, kMin>(__VA_ARGS__);             \
  MSCCLPP_AMD_PULL_CASE2(DT, __VA_ARGS__)

// scales / scalePtrs (host arrays, one entry per view): PreMulSum only, which is refused without scales.
int launchPullReduce(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype, int op,
                     int root, int nblocks, int nthreads, uint64_t budget, hipStream_t s, const float* scales,
                     const void* const* scalePtrs) {
  if (coll < MSCCLPP_AMD_PULL_REDUCE || coll > MSCCLPP_AMD_PULL_ALLREDUCE) return 4;
  if (nblocks <= 0) nblocks = pullReduceDefaultBlocks(coll, bytes);
  if (!launchShapeOk(nblocks, kMaxChannels, nthreads)) return 4;
  if (nranks < 2 || nranks > kMaxRanks || bytes == 0) return 4;
  if (coll == MSCCLPP_AMD_PULL_REDUCE && (root < 0 || root >= nranks)) return 4;
  if (!pull_reduce_takes(dtype, op) || bytes % (size_t)elem_bytes(dtype)) return 4;
  if (op == kPullPreMulSum && !scales) return 4;
  uint64_t srcOff[kMaxRanks], dstOff[kMaxRanks], len[kMaxRanks];
  const uint64_t most = pullReduceGeometry(coll, nranks, bytes, root, srcOff, dstOff, len);
  const uint64_t blk = blockBytes(most, (uint32_t)nblocks);
  if (blk > kBlkOffsetLimit) return 5;  // more workgroups needed: one workgroup's range is one descriptor
  if (op == kPullPreMulSum) {  // outside the table below, whose index dtype * 4 + op it would alias
    switch (dtype) {
      case kF16: return launchPullReduceT<kF16, kPullPreMulSum>(views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s, scales, scalePtrs);
      case kBF16: return launchPullReduceT<kBF16, kPullPreMulSum>(views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s, scales, scalePtrs);
      case kF32: return launchPullReduceT<kF32, kPullPreMulSum>(views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s, scales, scalePtrs);
      default: return 4;
    }
  }
  switch (dtype * 4 + op) {
    MSCCLPP_AMD_PULL_CASE2(kF16, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kBF16, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kF32, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kI32, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kU32, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kE4M3, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kE5M2, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE2(kU8, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE4(kI64, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE4(kU64, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    MSCCLPP_AMD_PULL_CASE4(kI8, views, nviews, nranks, coll, (uint64_t)bytes, root, blk, nblocks, nthreads, budget, s)
    default: return 4;
  }
}

}  // namespace mscclpp_amd
