// The host side of a collective launch, stated once: the launch-shape rule, the descriptor limit,
// the split of a range over workgroups, and the path from rank views to hipLaunchKernelGGL.
#pragma once

#include "common.hpp"
#include "launchers.hpp"  // what the host runtime calls: a kernel source defines what is declared there

namespace mscclpp_amd {

// Each workgroup addresses its sub-range of a buffer from one buffer resource (32-bit offsets): a
// launch whose per-workgroup range would exceed that is refused (ncclInvalidUsage) -- more
// workgroups carry it (every default shape does up to hundreds of GiB).
constexpr uint64_t kBlkOffsetLimit = 0xFFFFFFFFull - 64;

// A workgroup's sub-range of `len` bytes split over `nblocks` workgroups: ceil(len / nblocks)
// rounded up to whole 16-byte units.  Workgroup b owns [b * blk, (b + 1) * blk).
__host__ __device__ inline uint64_t blockBytes(uint64_t len, uint32_t nblocks) {
  return ((len + nblocks - 1) / nblocks + 15) & ~15ull;
}

// The launch shape every collective takes: at most `maxBlocks` workgroups of 64, 128, ..., 512
// lanes (nthreads <= 0: 512).  False: ncclInvalidArgument.
inline bool launchShapeOk(int nblocks, int maxBlocks, int& nthreads) {
  if (nthreads <= 0) nthreads = 512;
  return nblocks <= maxBlocks && nthreads >= 64 && nthreads <= 512 && nthreads % 64 == 0;
}

// `kern` on x workgroups per view: 0, or 1 for a HIP launch error.
template <typename Kernel, typename... Args>
inline int launchKernel(Kernel kern, int x, int nviews, int nthreads, hipStream_t s, const Args&... args) {
  hipLaunchKernelGGL(kern, dim3(x, nviews), dim3(nthreads), 0, s, args...);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// The launch of a collective kernel: 5 (ncclInvalidUsage) without launching when the x * nviews
// workgroups cannot be resident at once -- they wait on each other and on the peers', so a grid
// that is not would deadlock.  Co-residency is asked of `ask`: the kernel itself, but for the bulk
// kernel's modes.
template <typename Kernel, typename... Args>
inline int launchResident(Kernel ask, Kernel kern, int x, int nviews, int nthreads, hipStream_t s, const Args&... args) {
  if (!grid_coresident(ask, nthreads, (long)x * nviews)) return 5;
  return launchKernel(kern, x, nviews, nthreads, s, args...);
}

// The same from rank views, for kernels that take Views<NV> first and `args` after it: k1 is the
// NV = 1 instantiation (one rank per process), kN the one with a view per in-process rank.
template <typename... P>
inline int launchViews(void (*ask1)(Views<1>, P...), void (*askN)(Views<kMaxRanks>, P...), void (*k1)(Views<1>, P...),
                       void (*kN)(Views<kMaxRanks>, P...), const mscclppAmdRankView* views, int nviews, int x,
                       int nthreads, hipStream_t s, const P&... args) {
  if (nviews == 1) {
    Views<1> vw;
    vw.v[0] = views[0];
    return launchResident(ask1, k1, x, nviews, nthreads, s, vw, args...);
  }
  Views<kMaxRanks> vw{};
  for (int i = 0; i < nviews; ++i) vw.v[i] = views[i];
  return launchResident(askN, kN, x, nviews, nthreads, s, vw, args...);
}
template <typename... P>
inline int launchViews(void (*k1)(Views<1>, P...), void (*kN)(Views<kMaxRanks>, P...), const mscclppAmdRankView* views,
                       int nviews, int x, int nthreads, hipStream_t s, const P&... args) {
  return launchViews(k1, kN, k1, kN, views, nviews, x, nthreads, s, args...);
}

// ... and for kernels whose one argument is a struct with a `views` member (k1 takes its one-view
// form, kN the other).  `fill` sets the struct's other members once the grid is known to be
// resident, and returns 0, or the code to refuse the launch with.
template <typename A1, typename AN, typename Fill>
inline int launchViews(void (*k1)(A1), void (*kN)(AN), const mscclppAmdRankView* views, int nviews, int x, int nthreads,
                       hipStream_t s, Fill fill) {
  auto go = [&](auto kern, auto a) {
    if (!grid_coresident(kern, nthreads, (long)x * nviews)) return 5;
    for (int i = 0; i < nviews; ++i) a.views.v[i] = views[i];
    if (const int rc = fill(a)) return rc;
    return launchKernel(kern, x, nviews, nthreads, s, a);
  };
  return nviews == 1 ? go(k1, A1{}) : go(kN, AN{});
}

}  // namespace mscclpp_amd
