// The host entry points of the collective kernels, declared once: the kernel sources that define
// them see these declarations through launch.hpp, the host runtime through comm_internal.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mscclpp_amd/mscclpp_amd.h"

namespace mscclpp_amd {
int launchAllReduceLL(int algo, const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype,
                      int op, int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int launchCollectiveBulk(int mode, int algo, const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes,
                         int dtype, int op, int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int launchAllReduceBulk(int algo, const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype,
                        int op, int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int launchAllReducePipeline(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype, int op,
                            int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int launchBroadcast(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int root, int nblocks,
                    int nthreads, uint64_t budget, hipStream_t s);
int launchAllToAll(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdAllToAllSeg* segs,
                   int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int alltoallDefaultBlocks(uint64_t maxRecvBytes);
int launchAllToAllLL(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdAllToAllLLSeg* table,
                     uint64_t maxSeg, int nblocks, int nthreads, uint64_t budget, hipStream_t s);
size_t alltoallLLScratchRequired(int nranks, size_t maxSegBytes);
bool alltoallTakesLL(int nranks, size_t maxSegBytes);
int launchReduce(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype, int op, int root,
                 int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int reduceDefaultBlocks(uint64_t bytes);
int launchPullReduce(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype, int op,
                     int root, int nblocks, int nthreads, uint64_t budget, hipStream_t s, const float* scales = nullptr,
                     const void* const* scalePtrs = nullptr);
int pullReduceDefaultBlocks(int coll, uint64_t bytes);
int launchPullReduceLL(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype, int op,
                       int nblocks, int nthreads, uint64_t budget, hipStream_t s, const float* scales,
                       const void* const* scalePtrs);
size_t pullReduceLLScratchRequired(int coll, int nranks, size_t bytes, int dtype, int op);
bool pullReduceTakesLL(int coll, int nranks, size_t bytes);
int launchSendRecv(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdSendRecvOp* ops, int nops,
                   int nblocks, int nthreads, uint64_t budget, hipStream_t s);
int sendrecvDefaultBlocks(uint64_t bytes);
size_t ll16ScratchRequired(int nranks, size_t bytes, int dtype);
size_t ll8ScratchRequired(int nranks, size_t bytes, int dtype);
size_t testLLScratchRequired(int nranks, size_t bytes);
size_t testK2ScratchRequired(int nranks, size_t bytes);
struct BulkGeom;
size_t bulkScratchRequired(int nranks, size_t bytes, size_t maxScratch, BulkGeom* out, int nblocks);
}  // namespace mscclpp_amd
