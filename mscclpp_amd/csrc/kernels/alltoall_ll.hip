// Small ncclAllToAll / ncclAllToAllv: one hop of LL8 packets, a push through the LL scratch.
//
// The pull kernel of alltoall.hip registers the send buffer with every peer and takes two handshakes;
// a small exchange is bound by both.  Here nothing of the user's is registered and no token moves:
// rank r packs what it sends to rank q into packet units, stores them into region r of q's scratch
// half, and q unpacks them into its own receive buffer once their flags say they landed -- the protocol
// of allreduceLL8Kernel (allreduce_ll.hip) and pullReduceLLKernel (pull_reduce_ll.hip), with the same
// flags and the same scratch, so calls of all three may alternate.  One kernel serves the equal split
// and AllToAllv: a table of one entry per peer q, {sendOff, sendLen, recvOff, recvLen} in bytes, drives
// it (sendLen[r -> q] == recvLen[q <- r] is the caller's contract).
//
//  * One lane owns one 16-byte packet unit = 8 payload bytes {w0, flag, w1, flag} (ll_units.hpp).
//    Every unit is a whole unit: there is no lone 8-byte trailing packet, the last unit of a segment is
//    zero-filled past the segment's end.  Unit j of segment p -> r sits at p * region + 16 * j of rank
//    r's half; region = wireUnits(maxSeg) * 16 with maxSeg the largest segment of the whole n x n matrix
//    (self segments included), which every rank derives alike; a half is n regions rounded up to 256
//    bytes, and the flag's parity chooses the half.
//  * wireUnits(len) = max(1, ceil(len / 8)): a zero-length segment still sends ONE arrival unit with
//    payload zero, which the receiver polls and stores nothing of.  That keeps the argument by which the
//    two halves are safe to reuse: in every LL call every rank waits for a packet of
//    every other rank, so a rank that starts call k + 2 has seen packets of call k + 1 from all peers,
//    all of which have therefore finished call k, whose half it now overwrites.  AllToAllv tables with
//    zero rows or columns, or a rank that moves nothing at all, need no special case.
//  * Put: for unit index j = global lane id, strided by the grid, the lane loads unit j of every
//    outgoing segment that has one -- all loads issued before the first store, as the ReduceScatter put
//    of pull_reduce_ll.hip does, and no load under a branch inside the store loop -- and stores each
//    into region `rank` of that peer's half.  Consecutive lanes hold consecutive units, so a wave's
//    packet stores are contiguous 1 KiB runs of whole 64-byte lines.  The self segment is a local plain
//    copy by the same lanes and produces no packets.
//  * Receive: poll_units over the n - 1 other regions (all loads issued before any compare, non-peers
//    through the zero-length descriptor); a lane looks only at the units its segments have.  Only what
//    missed takes the bounded unit_wait with the caller's budget and the packet-timeout record; no wait
//    is unbounded.  payload_st stores into the own receive buffer at recvOff[p] + 8 j with `valid`
//    clamped to the segment (a2a_st: a segment's one partial unit goes byte by byte): no byte outside
//    [recvOff, recvOff + recvLen) is written and none outside a send segment is read.
//  * Segment starts need byte alignment only on either side.  Each buffer descriptor is built at the
//    segment's base, so offsets beyond 4 GiB of a buffer are carried; the 32-bit offsets stay inside
//    one region.
//  * The flag is a vector load issued with the lane's first payload loads; every workgroup, also one
//    that owns no unit, ends in bump_flags.  Trace stamps: 0 start, 1 puts issued, 2 stored.
#include "launch.hpp"
#include "ll_units.hpp"

#include <stdlib.h>

namespace mscclpp_amd {

typedef mscclppAmdAllToAllLLSeg A2ALLSeg;

__host__ __device__ inline uint64_t a2aWireUnits(uint64_t len) { return len ? (len + 7) / 8 : 1; }

// The one statement of the geometry; the launcher and the scratch requirement both use it.
struct A2ALLGeom {
  uint32_t units;   // wireUnits(maxSeg): the unit indices a lane may own
  uint32_t region;  // bytes one source rank occupies in a scratch half
  uint64_t half;    // the n regions, rounded up to 256 bytes; the scratch is two of them
};

static bool alltoallLLGeometry(int nranks, uint64_t maxSeg, A2ALLGeom* out) {
  if (nranks < 2 || nranks > kMaxRanks) return false;
  if (maxSeg > kLLOffsetLimit / 4) return false;  // (far above any size the path is meant for)
  const uint64_t units = a2aWireUnits(maxSeg), region = units * 16;
  if ((uint64_t)nranks * region + 16 > kLLOffsetLimit) return false;
  out->units = (uint32_t)units;
  out->region = (uint32_t)region;
  out->half = ((uint64_t)nranks * region + 255) & ~255ull;
  return true;
}

size_t alltoallLLScratchRequired(int nranks, size_t maxSegBytes) {
  A2ALLGeom g;
  return alltoallLLGeometry(nranks, maxSegBytes, &g) ? (size_t)(2 * g.half) : 0;
}

// One lane per unit index, 256 lanes, 1 to 128 workgroups: a function of wireUnits(maxSeg) alone, so
// every rank derives the same grid.
static void alltoallLLDefaults(const A2ALLGeom& g, int& nblocks, int& nthreads) {
  if (nthreads <= 0) nthreads = 256;
  if (nblocks <= 0) {
    uint64_t want = ((uint64_t)g.units + nthreads - 1) / nthreads;
    nblocks = (int)(want < 1 ? 1 : want > 128 ? 128 : want);
  }
}

// What the kernel reads of a rank view.  The in-process launch carries its whole n x n table by value
// beside these (a captured graph keeps both in the kernel node, and no device buffer is staged): eight
// full views would leave no room for it in the 4 KiB of kernel arguments.
struct A2ALLView {
  const void* input;
  void* output;
  void* scratch;
  void* peerScratch[kMaxRanks];
  uint32_t* flags;
  uint32_t* err;
  uint64_t scratchBytes;
  int32_t rank;
  int32_t pad;
  A2ALLView& operator=(const mscclppAmdRankView& v) {
    input = v.input;
    output = v.output;
    scratch = v.scratch;
    for (int q = 0; q < kMaxRanks; ++q) peerScratch[q] = v.peerScratch[q];
    flags = v.flags;
    err = v.err;
    scratchBytes = v.scratchBytes;
    rank = v.rank;
    pad = 0;
    return *this;
  }
};
template <int NV>
struct A2ALLViews {
  A2ALLView v[NV];
};

// A table entry as the kernel reads it: the lengths are bounded by the geometry (one region stays inside
// one descriptor), and 32-bit lengths keep a segment's state in three scalar registers fewer.
struct A2ALLDevSeg {
  uint64_t sendOff, recvOff;
  uint32_t sendLen, recvLen;
};
// bytes of unit j that lie inside a segment of `len` bytes
__device__ __forceinline__ uint32_t a2a_valid(uint32_t len, uint32_t j) {
  const uint32_t at = j * 8u;
  return at >= len ? 0u : len - at < 8u ? len - at : 8u;
}
// whether a segment of `len` bytes has a unit j on the wire: its payload units, or its one arrival unit
__device__ __forceinline__ bool a2a_has_unit(uint32_t len, uint32_t j) { return j * 8u < (len ? len : 1u); }

template <int NV>
struct A2ALLArgs {
  A2ALLViews<NV> views;
  A2ALLDevSeg tab[NV][kMaxRanks];  // [view][peer]
  A2ALLGeom g;
  uint64_t budget;
  uint64_t* trace;
  int nranks;
  int pad;
};
constexpr size_t kA2ALLKernargLimit = 4096;
static_assert(sizeof(A2ALLArgs<1>) <= kA2ALLKernargLimit, "one-view AllToAll LL arguments exceed the kernel-argument limit");
static_assert(sizeof(A2ALLArgs<kMaxRanks>) <= kA2ALLKernargLimit,
              "in-process AllToAll LL arguments exceed the kernel-argument limit");

// A unit's 8 payload bytes at byte `off` of the segment behind `r` (base `base`), of which `valid` lie
// inside it: whole units go through payload_ld / payload_st; a segment's one partial unit moves byte by
// byte through the same descriptor in a loop that is NOT unrolled.  (payload_ld's tail addresses its
// bytes through a 64-bit pointer per lane and is unrolled: once per peer on either side, that cost this
// kernel 70 spilled VGPRs under its 128-VGPR bound.)
__device__ __forceinline__ u32x2 a2a_ld(__amdgpu_buffer_rsrc_t r, const uint8_t* base, uint32_t off, uint32_t valid) {
  if (valid >= 8) return payload_ld(r, base, off, 8);
  uint64_t w = 0;
#pragma unroll 1
  for (uint32_t i = 0; i < valid; ++i) w |= (uint64_t)__builtin_amdgcn_raw_buffer_load_b8(r, off + i, 0, kPlain) << (8 * i);
  return u32x2{(uint32_t)w, (uint32_t)(w >> 32)};
}
__device__ __forceinline__ void a2a_st(__amdgpu_buffer_rsrc_t r, uint8_t* base, uint32_t off, u32x2 v, uint32_t valid) {
  if (valid >= 8) {
    payload_st(r, base, off, v, 8);
    return;
  }
  uint64_t w = v.x | (uint64_t)v.y << 32;
#pragma unroll 1
  for (uint32_t i = 0; i < valid; ++i, w >>= 8) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)w, r, off + i, 0, kPlain);
}

// Four waves per SIMD (at most 128 VGPRs): 8 in-process ranks x the default grid stay co-resident.
template <int NV>
__global__ void __launch_bounds__(512, 4) alltoallLLKernel(A2ALLArgs<NV> a) {
  // (blockIdx.y also where NV == 1 and it is 0: with the constant the compiler loads the whole table into
  // scalar registers at entry and spills 31 of them into VGPR lanes; indexed, an entry is loaded where used)
  const uint32_t vi = blockIdx.y;
  const A2ALLView& v = a.views.v[vi];
  const A2ALLDevSeg* tab = a.tab[vi];
  const int rank = v.rank, n = a.nranks;
  const A2ALLGeom& g = a.g;
  const uint32_t T = blockDim.x, G = gridDim.x;
  const uint32_t gtid = blockIdx.x * T + threadIdx.x;
  const uint8_t* in = (const uint8_t*)v.input;
  uint8_t* out = (uint8_t*)v.output;
  const uint32_t all = (1u << n) - 1u, peers = all & ~(1u << rank);
  trace_stamp(a.trace, 0);

  // The flag is a vector load issued right before this lane's first payload loads, so they are in
  // flight together: it is first looked at behind them.
  const uint32_t flagv = __hip_atomic_load(v.flags + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint8_t* selfSrc = in + tab[rank].sendOff;
  uint8_t* selfDst = out + tab[rank].recvOff;
  const uint32_t selfLen = tab[rank].sendLen;

  // put: the loads of a unit index are all issued before its first store; the store loop has none
  for (uint32_t j = gtid; j < g.units; j += G * T) {
    u32x2 wq[kMaxRanks];
#pragma unroll
    for (int q = 0; q < kMaxRanks; ++q) {
      wq[q] = u32x2{0, 0};
      if ((peers >> q) & 1u) {
        const uint8_t* seg = in + tab[q].sendOff;
        wq[q] = a2a_ld(make_rsrc(seg), seg, j * 8u, a2a_valid(tab[q].sendLen, j));
      }
    }
    const u32x2 ws = a2a_ld(make_rsrc(selfSrc), selfSrc, j * 8u, a2a_valid(selfLen, j));
    const uint32_t flag = wave_uniform(flagv);
    // my region in any peer's scratch, in the half of the flag's parity
    const uint64_t myRegion = ((flag & 1u) ? v.scratchBytes / 2 : 0) + (uint64_t)rank * g.region;
#pragma unroll
    for (int q = 0; q < kMaxRanks; ++q)
      if (((peers >> q) & 1u) && a2a_has_unit(tab[q].sendLen, j)) {
        const auto rq = make_rsrc((uint8_t*)v.peerScratch[q] + myRegion);
        unit_put<kSystem>(rq, j * 16u, wq[q], flag, false);
      }
    // the self segment: a local copy, no packet
    a2a_st(make_rsrc(selfDst), selfDst, j * 8u, ws, a2a_valid(selfLen, j));
  }
  const uint32_t flag = wave_uniform(flagv);
  const uint64_t base = (flag & 1u) ? v.scratchBytes / 2 : 0;
  trace_stamp(a.trace, 1);

  const uint8_t* scr = (const uint8_t*)v.scratch + base;
  const auto rscr = make_rsrc(const_cast<uint8_t*>(scr));
  for (uint32_t j = gtid; j < g.units; j += G * T) {
    // the regions whose segment has a unit j (its arrival unit, where the segment is empty)
    uint32_t need = 0;
#pragma unroll
    for (int p = 0; p < kMaxRanks; ++p)
      if (((peers >> p) & 1u) && a2a_has_unit(tab[p].recvLen, j)) need |= 1u << p;
    u32x2 w[kMaxRanks];
    const uint32_t missing = poll_units(scr, g.region, j * 16u, flag, peers, w) & need;
    if (missing) {
      // one copy of the wait, a loop over the peers that is NOT unrolled: eight inlined copies took the
      // kernel to its 128-VGPR bound and 50 spilled registers beyond it
#pragma unroll 1
      for (int p = 0; p < n; ++p) {
        if (!((missing >> p) & 1u)) continue;
        const u32x2 got = unit_wait(rscr, (uint32_t)p * g.region + j * 16u, flag, false, a.budget, v.err);
#pragma unroll
        for (int k = 0; k < kMaxRanks; ++k)
          if (k == p) w[k] = got;
      }
    }
#pragma unroll
    for (int p = 0; p < kMaxRanks; ++p)
      if ((peers >> p) & 1u) {
        uint8_t* dst = out + tab[p].recvOff;
        a2a_st(make_rsrc(dst), dst, j * 8u, w[p], a2a_valid(tab[p].recvLen, j));
      }
  }
  trace_stamp(a.trace, 2);
  bump_flags(v.flags, flag);
}

// table: host, [nviews][nranks], entry [i][q] = what views[i].rank sends to and receives from rank q.
// maxSeg: the largest segment of the whole n x n matrix, which every rank must pass alike (it sets the
// region stride); ~0: derive it from `table`, which holds the whole matrix when nviews == nranks.
// 4: invalid, nothing launched and no device touched; 5: not carried with this scratch or shape.
int launchAllToAllLL(const mscclppAmdRankView* views, int nviews, int nranks, const A2ALLSeg* table, uint64_t maxSeg,
                     int nblocks, int nthreads, uint64_t budget, hipStream_t s) {
  if (nranks < 2 || nranks > kMaxRanks || nviews < 1 || nviews > nranks || !table) return 4;
  if (nblocks > kFlagSlots) return 4;
  uint64_t most = 0;
  for (int i = 0; i < nviews; ++i) {
    const A2ALLSeg* row = table + (size_t)i * nranks;
    const int r = views[i].rank;
    if (row[r].sendLen != row[r].recvLen) return 4;  // the self segment
    for (int k = 0; k < nviews; ++k)  // what one view sends another, the other expects
      if (row[views[k].rank].sendLen != table[(size_t)k * nranks + r].recvLen) return 4;
    for (int q = 0; q < nranks; ++q) {
      most = row[q].sendLen > most ? row[q].sendLen : most;
      most = row[q].recvLen > most ? row[q].recvLen : most;
    }
  }
  if (maxSeg == ~0ull) maxSeg = most;
  if (most > maxSeg) return 4;
  A2ALLGeom g;
  if (!alltoallLLGeometry(nranks, maxSeg, &g)) return 5;
  alltoallLLDefaults(g, nblocks, nthreads);
  if (!launchShapeOk(nblocks, kFlagSlots, nthreads)) return 4;
  for (int i = 0; i < nviews; ++i)
    if (views[i].scratchBytes != views[0].scratchBytes || views[i].scratchBytes < 2 * g.half) return 5;
  return launchViews(alltoallLLKernel<1>, alltoallLLKernel<kMaxRanks>, views, nviews, nblocks, nthreads, s, [&](auto& a) {
    for (int i = 0; i < nviews; ++i)
      for (int q = 0; q < nranks; ++q) {
        const A2ALLSeg& e = table[(size_t)i * nranks + q];
        a.tab[i][q] = {e.sendOff, e.recvOff, (uint32_t)e.sendLen, (uint32_t)e.recvLen};  // (<= maxSeg < 4 GiB)
      }
    a.g = g;
    a.budget = budget;
    a.trace = g_mscclppAmdTrace;
    a.nranks = nranks;
    return 0;
  });
}

// ---- cutover -------------------------------------------------------------------------------------
// The largest segment of the matrix up to which ncclAllToAll / ncclAllToAllv take this path, per rank
// count: read off the in-process sweep of DESIGN.md §17h (tools/alltoall_perf.py --ll, profiles/
// alltoall_ll_perf_inprocess_n{2,4,8}.json): the largest swept size up to which this kernel's median
// was at or below the pull kernel's of the same run.  Rank counts between the measured ones take the
// next measured count above.  Fabric-free numbers (ranks share one GPU); nothing over xGMI has been
// measured.
constexpr uint64_t kA2ALLMaxBytes = 1ull << 20;  // the reference's LL bound (kLLOffsetLimit's comment)
static uint64_t alltoallLLBuiltinMax(int nranks) {
  if (nranks <= 2) return 1024ull << 10;
  if (nranks <= 4) return 512ull << 10;
  return 256ull << 10;
}
// MSCCLPP_AMD_A2A_LL_MAX_BYTES: 0 disables the path; read once; values above 1 MiB are clamped to it.
// -1: unset.
static int64_t alltoallLLEnvMax() {
  static const int64_t v = [] {
    const char* e = getenv("MSCCLPP_AMD_A2A_LL_MAX_BYTES");
    if (!e || !*e) return (int64_t)-1;
    char* end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *e == '-') return (int64_t)-1;
    return (int64_t)(x > kA2ALLMaxBytes ? kA2ALLMaxBytes : x);
  }();
  return v;
}
bool alltoallTakesLL(int nranks, size_t maxSegBytes) {
  if (nranks < 2 || nranks > kMaxRanks || maxSegBytes == 0) return false;
  const int64_t env = alltoallLLEnvMax();
  const uint64_t most = env >= 0 ? (uint64_t)env : alltoallLLBuiltinMax(nranks);
  return maxSegBytes <= most;
}

}  // namespace mscclpp_amd
