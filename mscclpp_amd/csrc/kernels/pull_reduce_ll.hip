// Small AllReduce / ReduceScatter of everything the pull-reduce path carries (ncclMax / ncclAvg, the
// four operations of int64 / uint64 / int8, PreMulSum of fp16 / bf16 / fp32): one hop of LL8 packets,
// the protocol of allreduceLL8Kernel (allreduce_ll.hip), with the arithmetic of pull_reduce.hip
// (mscclpp_amd/pull_reduce_device.hpp) -- operands in RANK order 0 .. n - 1, the own payload at position
// `rank` -- so a call gives the bits the pull path gives.  Nothing of the user's is registered and
// no token is exchanged: packets go into the peers' LL scratch, and the flag in them says they landed.
//
//  * One lane owns one 16-byte packet unit = 8 payload bytes {w0, flag, w1, flag} (ll_units.hpp).  The
//    flag is a vector load issued with the lane's first payload load; the half of the scratch comes
//    from the flag's parity; every workgroup, also one that owns no unit, ends in bump_flags.
//  * AllReduce: rank r puts unit j of its message into region r of every peer's half, polls unit j
//    of the n - 1 other regions of its own half (all loads issued before any compare), reduces, and
//    stores unit j of its output.
//  * ReduceScatter (bytes = one block): rank r puts unit j of block q of its send buffer into region
//    r of rank q's half for every q != r, polls unit j of the n - 1 other regions of its own half,
//    reduces them with unit j of its own block r, and stores into its receive buffer.
//  * A unit of a 64-bit type is one element (the byte count is a multiple of 8: the word count W is
//    even and the lone trailing packet never occurs); of every other type it is two independent
//    words, and an odd W ends in the single 8-byte packet exactly as in LL8.
//  * Tail bytes are zero-filled on load and never stored; pointers need element alignment only.  The
//    lane that loads the own term of unit j stores result j, and no peer reads user memory, so
//    send == recv (AllReduce) and recv == send + rank * bytes (ReduceScatter) hold.
//  * PreMulSum: every source region has one more unit, behind its last packet unit, that holds the
//    rank's scalar as fp32 bits; the sender's workgroup 0 puts it (read through the device pointer
//    when the kernel runs, where the handle is device-resident), and every workgroup that reduces
//    polls the n - 1 scalar units before its first next().  The token diagonal is not used.
//  * Every wait is the bounded unit_wait with the caller's budget and the packet-timeout record.
//    Trace stamps: 0 start, 1 puts issued, 2 reduced.
//  * Reduce is NOT carried.  The two halves of the scratch are safe to reuse only because in every
//    LL call every rank waits for a packet of every other rank: a rank that starts call k + 2 has
//    seen packets of call k + 1 from all peers, so all of them have finished call k, whose half it
//    now overwrites.  In a Reduce only the root waits, and a fast non-root could overwrite packets
//    the root has not read.  Reduce keeps the pull path.
#include "launch.hpp"
#include "ll_units.hpp"
#include "mscclpp_amd/pull_reduce_device.hpp"

#include <stdlib.h>

namespace mscclpp_amd {

// The one statement of the geometry (bytes: the message of AllReduce, the per-rank block of
// ReduceScatter); the launcher and the scratch requirement both use it.
struct PullLLGeom {
  uint64_t bytes;
  uint64_t W;        // 32-bit words per message / block: llWords, or bytes / 4 for the 64-bit types
  uint32_t units;    // 2-word units = ceil(W / 2)
  uint32_t scalarAt; // byte offset of the scalar unit inside a region (PreMulSum) = units * 16
  uint32_t region;   // bytes one source rank occupies in a scratch half
  uint32_t pad;
  uint64_t half;     // the n regions, rounded up to 256 bytes; the scratch is two of them
};

static bool pullReduceLLGeometry(int coll, int nranks, size_t bytes, int dtype, int op, PullLLGeom* out) {
  if (coll != MSCCLPP_AMD_PULL_REDUCE_SCATTER && coll != MSCCLPP_AMD_PULL_ALLREDUCE) return false;
  if (nranks < 2 || nranks > kMaxRanks || bytes == 0 || !pull_reduce_takes(dtype, op)) return false;
  if (bytes % (size_t)elem_bytes(dtype)) return false;
  if (bytes > kLLOffsetLimit / 4) return false;  // (far above any size the path is meant for)
  PullLLGeom g{};
  g.bytes = bytes;
  g.W = elem_bytes(dtype) == 8 ? bytes / 4 : llWords(bytes, dtype);
  g.units = (uint32_t)((g.W + 1) / 2);
  g.scalarAt = g.units * 16u;
  g.region = g.scalarAt + (op == kPullPreMulSum ? 16u : 0u);
  g.half = ((uint64_t)nranks * g.region + 255) & ~255ull;
  if ((uint64_t)nranks * g.region + 16 > kLLOffsetLimit) return false;
  *out = g;
  return true;
}

size_t pullReduceLLScratchRequired(int coll, int nranks, size_t bytes, int dtype, int op) {
  PullLLGeom g;
  return pullReduceLLGeometry(coll, nranks, bytes, dtype, op, &g) ? (size_t)(2 * g.half) : 0;
}

// ll8Defaults' rule: one lane per unit, 256 lanes, up to 128 workgroups (so more than 256 KiB takes several
// passes).  A function of the byte count alone (through the unit count), so every rank derives the same
// grid.  The lanes stay at 256 at every size: 8 in-process ranks x 128 workgroups are then four
// workgroups per CU, which the kernel's 128-VGPR bound keeps resident together.
static void pullReduceLLDefaults(const PullLLGeom& g, int& nblocks, int& nthreads) {
  if (nthreads <= 0) nthreads = 256;
  if (nblocks <= 0) {
    uint64_t want = ((uint64_t)g.units + nthreads - 1) / nthreads;
    if (want < 1) want = 1;
    if (want > 128) want = 128;
    nblocks = (int)want;
  }
}

template <int NV>
struct PullLLArgs {
  Views<NV> views;
  PullLLGeom g;
  uint64_t budget;
  uint64_t* trace;
  float invN;      // 1.0f / (float)nranks, computed once by the host (AVG of the float types)
  int nranks;
  int scatter;     // ReduceScatter: block q of the send buffer goes to rank q
  int pad;
  float scale[NV];           // PreMulSum: the view's scalar, unless ...
  const void* scalePtr[NV];  // ... non-null: one element of the element type in device memory
};
static_assert(sizeof(PullLLArgs<kMaxRanks>) <= 4096, "in-process pull-reduce LL arguments exceed the kernel-argument limit");

// The reduction of one unit: x[p] is rank p's payload for p != rank, `own` stands at position rank.
template <int DT, int OP>
__device__ __forceinline__ u32x2 pull_ll_reduce(const u32x2* x, u32x2 own, int rank, int n, float invN,
                                                [[maybe_unused]] const float* sc) {
  // (the words are copied out of the vectors first: see bench_add2 in allreduce_ll.hip)
  uint32_t lo[kMaxRanks], hi[kMaxRanks];
#pragma unroll
  for (int p = 0; p < kMaxRanks; ++p) {
    const u32x2 v = p == rank ? own : x[p];
    lo[p] = v.x;
    hi[p] = v.y;
  }
  if constexpr (pull_acc_words(DT) == 2) {
    PullAcc<DT, OP> acc;
    acc.first(lo[0] | (uint64_t)hi[0] << 32);
#pragma unroll
    for (int p = 1; p < kMaxRanks; ++p)
      if (p < n) acc.next(lo[p] | (uint64_t)hi[p] << 32);
    const uint64_t e = acc.word(n, invN);
    return u32x2{(uint32_t)e, (uint32_t)(e >> 32)};
  } else {
    PullAcc<DT, OP> a0, a1;
    if constexpr (OP == kPullPreMulSum) {
      a0.first(lo[0], sc[0]);
      a1.first(hi[0], sc[0]);
#pragma unroll
      for (int p = 1; p < kMaxRanks; ++p)
        if (p < n) {
          a0.next(lo[p], sc[p]);
          a1.next(hi[p], sc[p]);
        }
    } else {
      a0.first(lo[0]);
      a1.first(hi[0]);
#pragma unroll
      for (int p = 1; p < kMaxRanks; ++p)
        if (p < n) {
          a0.next(lo[p]);
          a1.next(hi[p]);
        }
    }
    return u32x2{a0.word(n, invN), a1.word(n, invN)};
  }
}

// Four waves per SIMD (at most 128 VGPRs): 8 in-process ranks x the default grid stay co-resident.
template <int DT, int OP, int NV>
__global__ void __launch_bounds__(512, 4) pullReduceLLKernel(PullLLArgs<NV> a) {
  const uint32_t vi = NV == 1 ? 0 : blockIdx.y;
  const mscclppAmdRankView& v = a.views.v[vi];
  const int rank = v.rank, n = a.nranks;
  const PullLLGeom& g = a.g;
  const uint32_t T = blockDim.x, G = gridDim.x;
  const uint32_t gtid = blockIdx.x * T + threadIdx.x;
  const uint8_t* in = (const uint8_t*)v.input;
  // the own term: the message itself, or block `rank` of the send buffer
  const uint8_t* own = in + (a.scatter ? (uint64_t)rank * g.bytes : 0);
  uint8_t* out = (uint8_t*)v.output;
  const auto rown = make_rsrc(own);
  const auto rout = make_rsrc(out);
  const uint32_t peers = ((1u << n) - 1u) & ~(1u << rank);
  // payload bytes of unit j inside the message / block (the lone trailing packet carries one word)
  auto validOf = [&](uint32_t j) { return clamp_valid(g.bytes, (uint64_t)j * 8, 2ull * j + 1 >= g.W ? 4 : 8); };
  trace_stamp(a.trace, 0);
  // The flag is a vector load issued right before this lane's first payload load, so the two are in
  // flight together; the payload is also the own term of that unit's reduction.
  const uint32_t flagv = __hip_atomic_load(v.flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  u32x2 w0{0, 0};
  if (gtid < g.units) w0 = payload_ld(rown, own, (uint64_t)gtid * 8, validOf(gtid));
  const uint32_t flag = wave_uniform(flagv);
  const uint64_t base = (flag & 1u) ? v.scratchBytes / 2 : 0;
  const uint64_t myRegion = base + (uint64_t)rank * g.region;  // my region in any peer's scratch

  [[maybe_unused]] float ownScale = 0.0f;
  if constexpr (OP == kPullPreMulSum) {
    ownScale = a.scalePtr[vi] ? premul_scalar_at<DT>(a.scalePtr[vi]) : a.scale[vi];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll 1
      for (int q = 0; q < n; ++q) {
        if (q == rank) continue;
        const auto rq = make_rsrc((uint8_t*)v.peerScratch[q] + myRegion);
        unit_put<kSystem>(rq, g.scalarAt, u32x2{__builtin_bit_cast(uint32_t, ownScale), 0u}, flag, false);
      }
    }
  }

  // put: my payload of unit j into my region of every peer's half.  Two loops, so that the AllReduce's
  // has no load in it: a load under a branch inside it made every store wait for the one before it
  // (one vmcnt counts both; 0.4 us per peer in the put phase of the trace).
  if (!a.scatter) {
    for (uint32_t j = gtid; j < g.units; j += G * T) {
      const bool single = 2ull * j + 1 >= g.W;
      const u32x2 w = j == gtid ? w0 : payload_ld(rown, own, (uint64_t)j * 8, validOf(j));
#pragma unroll 1
      for (int q = 0; q < n; ++q) {
        if (q == rank) continue;
        const auto rq = make_rsrc((uint8_t*)v.peerScratch[q] + myRegion);
        unit_put<kSystem>(rq, j * 16u, w, flag, single);
      }
    }
  } else {
    // ReduceScatter: block q of my send buffer goes to rank q; the loads of all blocks are issued
    // before the first store
    for (uint32_t j = gtid; j < g.units; j += G * T) {
      const bool single = 2ull * j + 1 >= g.W;
      const uint32_t valid = validOf(j);
      u32x2 wq[kMaxRanks];
#pragma unroll
      for (int q = 0; q < kMaxRanks; ++q) {
        wq[q] = u32x2{0, 0};
        if ((peers >> q) & 1u) {
          const uint8_t* blk = in + (uint64_t)q * g.bytes;
          wq[q] = payload_ld(make_rsrc(blk), blk, (uint64_t)j * 8, valid);
        }
      }
#pragma unroll
      for (int q = 0; q < kMaxRanks; ++q)
        if ((peers >> q) & 1u) {
          const auto rq = make_rsrc((uint8_t*)v.peerScratch[q] + myRegion);
          unit_put<kSystem>(rq, j * 16u, wq[q], flag, single);
        }
    }
  }
  trace_stamp(a.trace, 1);

  const uint8_t* scr = (const uint8_t*)v.scratch + base;
  const auto rscr = make_rsrc(const_cast<uint8_t*>(scr));
  [[maybe_unused]] float sc[kMaxRanks];  // PreMulSum: rank p's scalar
  if constexpr (OP == kPullPreMulSum) {
    if (blockIdx.x * T < g.units) {  // this workgroup reduces: the n - 1 scalar units first
      u32x2 s[kMaxRanks];
      const uint32_t missing = poll_units(scr, g.region, g.scalarAt, flag, peers, s);
      if (missing) {
#pragma unroll
        for (int p = 0; p < kMaxRanks; ++p)
          if ((missing >> p) & 1u) s[p] = unit_wait(rscr, (uint32_t)p * g.region + g.scalarAt, flag, false, a.budget, v.err);
      }
#pragma unroll
      for (int p = 0; p < kMaxRanks; ++p) {
        const uint32_t bits = s[p].x;
        sc[p] = p == rank ? ownScale : __builtin_bit_cast(float, wave_uniform(bits));
      }
    }
  }

  // reduce in rank order.  The same lane handled unit j above, so an in-place call reads its input
  // before overwriting it.
  for (uint32_t j = gtid; j < g.units; j += G * T) {
    const bool single = 2ull * j + 1 >= g.W;
    const uint64_t off = (uint64_t)j * 8;
    const uint32_t valid = validOf(j);
    const u32x2 mine = j == gtid ? w0 : payload_ld(rown, own, off, valid);
    u32x2 w[kMaxRanks];
    // the waves without the lone trailing packet (all but at most one) poll 16-byte units with every
    // load issued before any value is looked at; the one that has it takes the per-lane path
    const uint32_t jw = wave_uniform(j);  // the wave's first unit (lanes hold consecutive units)
    const bool waveSingle = (g.W & 1) && 2ull * (jw + 63) + 1 >= g.W;
    uint32_t missing = 0;
    if (!waveSingle) {
      missing = poll_units(scr, g.region, j * 16u, flag, peers, w);
    } else {
#pragma unroll
      for (int p = 0; p < kMaxRanks; ++p) {
        w[p] = u32x2{0, 0};
        if (((peers >> p) & 1u) && !unit_try(rscr, (uint32_t)p * g.region + j * 16u, flag, w[p], single)) missing |= 1u << p;
      }
    }
    if (missing) {
#pragma unroll
      for (int p = 0; p < kMaxRanks; ++p)
        if ((missing >> p) & 1u) w[p] = unit_wait(rscr, (uint32_t)p * g.region + j * 16u, flag, single, a.budget, v.err);
    }
    payload_st(rout, out, off, pull_ll_reduce<DT, OP>(w, mine, rank, n, a.invN, sc), valid);
  }
  trace_stamp(a.trace, 2);
  bump_flags(v.flags, flag);
}

template <int DT, int OP>
static int launchPullReduceLLT(const mscclppAmdRankView* views, int nviews, int nranks, int coll, const PullLLGeom& g,
                               int nblocks, int nthreads, uint64_t budget, hipStream_t s, const float* scales,
                               const void* const* scalePtrs) {
  auto fill = [&](auto& args) {
    args.g = g;
    args.budget = budget;
    args.trace = g_mscclppAmdTrace;
    args.invN = 1.0f / (float)nranks;
    args.nranks = nranks;
    args.scatter = coll == MSCCLPP_AMD_PULL_REDUCE_SCATTER;
    if constexpr (OP == kPullPreMulSum) {
      for (int i = 0; i < nviews; ++i) {
        args.scale[i] = scales[i];
        args.scalePtr[i] = scalePtrs ? scalePtrs[i] : nullptr;
      }
    }
    return 0;
  };
  return launchViews(pullReduceLLKernel<DT, OP, 1>, pullReduceLLKernel<DT, OP, kMaxRanks>, views, nviews, nblocks,
                     nthreads, s, fill);
}

#define MSCCLPP_AMD_PULL_LL_CASE2(DT)                                                     \
  case DT * 4 + kPullMax: return launchPullReduceLLT<DT, kPullMax>(MSCCLPP_AMD_PULL_LL_ARGS); \
  case DT * 4 + kPullAvg: return launchPullReduceLLT<DT, kPullAvg>(MSCCLPP_AMD_PULL_LL_ARGS);
#define MSCCLPP_AMD_PULL_LL_CASE4(DT)                                                     \
  case DT * 4 + kSum: return launchPullReduceLLT<DT, kSum>(MSCCLPP_AMD_PULL_LL_ARGS);     \
  case DT * 4 + kMin: return launchPullReduceLLT<DT, kMin>(MSCCLPP_AMD_PULL_LL_ARGS);     \
  MSCCLPP_AMD_PULL_LL_CASE2(DT)
#define MSCCLPP_AMD_PULL_LL_ARGS views, nviews, nranks, coll, g, nblocks, nthreads, budget, s, scales, scalePtrs

// 4: invalid, nothing launched and no device touched; 5: not carried with this scratch or shape.
// scales / scalePtrs (host arrays, one entry per view): PreMulSum only, which is refused without scales.
int launchPullReduceLL(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype, int op,
                       int nblocks, int nthreads, uint64_t budget, hipStream_t s, const float* scales,
                       const void* const* scalePtrs) {
  if (coll != MSCCLPP_AMD_PULL_REDUCE_SCATTER && coll != MSCCLPP_AMD_PULL_ALLREDUCE) return 4;
  if (nranks < 2 || nranks > kMaxRanks || bytes == 0) return 4;
  if (!pull_reduce_takes(dtype, op) || bytes % (size_t)elem_bytes(dtype)) return 4;
  if ((op == kPullPreMulSum) != (scales != nullptr) || (op != kPullPreMulSum && scalePtrs)) return 4;
  if (nblocks > kFlagSlots) return 4;
  PullLLGeom g;
  if (!pullReduceLLGeometry(coll, nranks, bytes, dtype, op, &g)) return 5;
  pullReduceLLDefaults(g, nblocks, nthreads);
  if (!launchShapeOk(nblocks, kFlagSlots, nthreads)) return 4;
  for (int i = 0; i < nviews; ++i)
    if (views[i].scratchBytes != views[0].scratchBytes || views[i].scratchBytes < 2 * g.half) return 5;
  if (op == kPullPreMulSum) {  // outside the table below, whose index dtype * 4 + op it would alias
    switch (dtype) {
      case kF16: return launchPullReduceLLT<kF16, kPullPreMulSum>(MSCCLPP_AMD_PULL_LL_ARGS);
      case kBF16: return launchPullReduceLLT<kBF16, kPullPreMulSum>(MSCCLPP_AMD_PULL_LL_ARGS);
      case kF32: return launchPullReduceLLT<kF32, kPullPreMulSum>(MSCCLPP_AMD_PULL_LL_ARGS);
      default: return 4;
    }
  }
  switch (dtype * 4 + op) {
    MSCCLPP_AMD_PULL_LL_CASE2(kF16)
    MSCCLPP_AMD_PULL_LL_CASE2(kBF16)
    MSCCLPP_AMD_PULL_LL_CASE2(kF32)
    MSCCLPP_AMD_PULL_LL_CASE2(kI32)
    MSCCLPP_AMD_PULL_LL_CASE2(kU32)
    MSCCLPP_AMD_PULL_LL_CASE2(kE4M3)
    MSCCLPP_AMD_PULL_LL_CASE2(kE5M2)
    MSCCLPP_AMD_PULL_LL_CASE2(kU8)
    MSCCLPP_AMD_PULL_LL_CASE4(kI64)
    MSCCLPP_AMD_PULL_LL_CASE4(kU64)
    MSCCLPP_AMD_PULL_LL_CASE4(kI8)
    default: return 4;
  }
}

// ---- cutover -------------------------------------------------------------------------------------
// The largest byte count (the message of AllReduce, the per-rank block of ReduceScatter) the NCCL entry
// points send to this path, per collective and rank count: read off the in-process sweep of DESIGN.md
// §17g (tools/pull_reduce_perf.py --ll, profiles/pull_reduce_ll_perf_inprocess_n{2,4,8}.json): the
// largest swept size up to which this path's median beat the pull path's for fp32 MAX, fp16 AVG and
// int64 SUM alike.  Rank counts between the measured ones take the next measured count above.
// Fabric-free numbers (ranks share one GPU); over xGMI neither path has been measured.
constexpr uint64_t kPullLLMaxBytes = 1ull << 20;  // the reference's LL bound (kLLOffsetLimit's comment)
static uint64_t pullLLBuiltinMax(int coll, int nranks) {
  const bool rs = coll == MSCCLPP_AMD_PULL_REDUCE_SCATTER;
  if (nranks <= 2) return rs ? (512ull << 10) : (1024ull << 10);
  if (nranks <= 4) return rs ? (512ull << 10) : (512ull << 10);
  return rs ? (128ull << 10) : (256ull << 10);
}
// MSCCLPP_AMD_PULL_LL_MAX_BYTES: one bound for both collectives, 0 disables the path; read once; values
// above 1 MiB are clamped to it.  -1: unset.
static int64_t pullLLEnvMax() {
  static const int64_t v = [] {
    const char* e = getenv("MSCCLPP_AMD_PULL_LL_MAX_BYTES");
    if (!e || !*e) return (int64_t)-1;
    char* end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *e == '-') return (int64_t)-1;
    return (int64_t)(x > kPullLLMaxBytes ? kPullLLMaxBytes : x);
  }();
  return v;
}
bool pullReduceTakesLL(int coll, int nranks, size_t bytes) {
  if (coll != MSCCLPP_AMD_PULL_REDUCE_SCATTER && coll != MSCCLPP_AMD_PULL_ALLREDUCE) return false;
  if (nranks < 2 || nranks > kMaxRanks || bytes == 0) return false;
  const int64_t env = pullLLEnvMax();
  const uint64_t most = env >= 0 ? (uint64_t)env : pullLLBuiltinMax(coll, nranks);
  return bytes <= most;
}

}  // namespace mscclpp_amd
