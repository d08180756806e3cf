/*
 * mscclpp_amd extension C ABI (libmscclpp_amd.so).  Plain pointers and sizes only.
 *
 * The NCCL drop-in entry points live in nccl.h.  This header adds what the reference exposes
 * through its C++ API (include/mscclpp/core.hpp, algorithm.hpp, gpu_utils.hpp) and that the
 * parity tests and the benchmark need:
 *   - uncached device allocation and flag buffers (gpu_utils.cc:139-147, algorithm.cc:251-268)
 *   - the 1-GPU LL16 pack+sum+unpack microbench kernel (BASELINE config 2)
 *   - explicit-view AllReduce launchers: every rank's buffers and mapped peer pointers are passed
 *     in, so the same kernels run either one rank per process (views = 1) or several ranks of a
 *     single process on one GPU (views = n, "in-process ranks", used by the parity tests)
 *   - Algorithm::execute with an explicit algorithm (algorithm.hpp:108-113)
 *
 * Return codes are ncclResult_t values (0 = success, 1 = HIP error, 3 = internal, 4 = invalid
 * argument, 5 = invalid usage).
 */
#ifndef MSCCLPP_AMD_H_
#define MSCCLPP_AMD_H_

#include <stddef.h>
#include <stdint.h>

#include "nccl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCCLPP_AMD_MAX_RANKS 8
#define MSCCLPP_AMD_FLAG_SLOTS 4096
#define MSCCLPP_AMD_MAX_CHANNELS 256

/* dtype / op codes of the extension API (ncclDataType_t / ncclRedOp_t are mapped onto these) */
enum { MSCCLPP_AMD_F16 = 0, MSCCLPP_AMD_BF16 = 1, MSCCLPP_AMD_F32 = 2, MSCCLPP_AMD_I32 = 3, MSCCLPP_AMD_U32 = 4 };
/* OCP FP8 (gfx950 hardware formats; the reference's DataType::FLOAT8_E4M3FN / FLOAT8_E5M2,
 * gpu_data_types.hpp:170-183).  The code also names the accumulation type of
 * Algorithm::execute(..., accumDtype) (algorithm.hpp:108-113, common.hpp:89-100): the element
 * type itself (AUTO), half or float. */
enum {
  MSCCLPP_AMD_E4M3 = 5,
  MSCCLPP_AMD_E5M2 = 6,
  MSCCLPP_AMD_E4M3_ACC_F16 = 7,
  MSCCLPP_AMD_E5M2_ACC_F16 = 8,
  MSCCLPP_AMD_E4M3_ACC_F32 = 9,
  MSCCLPP_AMD_E5M2_ACC_F32 = 10,
  /* uint8 (ncclUint8; Adapter<Op, uint8_t, uint8_t>, common.hpp:132-133): wrapping add / unsigned
   * min per byte (gpu_data_types.hpp:577-640) */
  MSCCLPP_AMD_U8 = 11,
  /* the software float8 e4m3b15 (DataType::FLOAT8_E4M3B15, gpu_data_types.hpp:78-155; no NCCL
   * dtype): accumulated in itself, half or float, as the OCP codes above */
  MSCCLPP_AMD_E4M3B15 = 12,
  MSCCLPP_AMD_E4M3B15_ACC_F16 = 13,
  MSCCLPP_AMD_E4M3B15_ACC_F32 = 14,
  MSCCLPP_AMD_NUM_DTYPES = 15
};
enum { MSCCLPP_AMD_SUM = 0, MSCCLPP_AMD_MIN = 1 };
/* ncclMax / ncclAvg: accepted ONLY by mscclppAmdPullReduceLaunch (and through it by ncclAllReduce /
 * ncclReduceScatter / ncclReduce); every other entry point keeps the op range SUM .. MIN. */
enum { MSCCLPP_AMD_MAX = 2, MSCCLPP_AMD_AVG = 3 };
/* PreMulSum (ncclRedOpCreatePreMulSum): accepted ONLY by mscclppAmdPullReduceLaunchScaled (and through
 * it by ncclAllReduce / ncclReduceScatter / ncclReduce with a live handle), with F16, BF16 and F32.
 * Code 4 names nothing and stays refused everywhere. */
enum { MSCCLPP_AMD_PREMUL_SUM = 5 };
/* int64 / uint64 / int8 (ncclInt64 / ncclUint64 / ncclInt8): likewise accepted ONLY by
 * mscclppAmdPullReduceLaunch (and through it by ncclAllReduce / ncclReduceScatter / ncclReduce), there
 * with all of SUM, MIN, MAX and AVG.  They lie beyond MSCCLPP_AMD_NUM_DTYPES, which keeps bounding the
 * types of every other entry point. */
enum { MSCCLPP_AMD_I64 = 16, MSCCLPP_AMD_U64 = 17, MSCCLPP_AMD_I8 = 18 };
/* the collectives of mscclppAmdPullReduceLaunch */
enum { MSCCLPP_AMD_PULL_REDUCE = 0, MSCCLPP_AMD_PULL_REDUCE_SCATTER = 1, MSCCLPP_AMD_PULL_ALLREDUCE = 2 };

/* AllReduce algorithms (names follow the reference's AlgorithmCollection keys) */
enum {
  MSCCLPP_AMD_ALGO_AUTO = 0,
  MSCCLPP_AMD_ALGO_PACKET = 1,   /* default_allreduce_packet: LL16 two-hop (allreduce_packet.cu:15-151) */
  MSCCLPP_AMD_ALGO_ALLPAIR = 2,  /* default_allreduce_allpair_packet: LL8 one-hop (allreduce_allpair_packet.cu:15-69) */
  MSCCLPP_AMD_ALGO_FULLMESH = 3, /* default_allreduce_fullmesh: bulk all-pairs RS+AG (allreduce_fullmesh.cu:24-166) */
  MSCCLPP_AMD_ALGO_RSAG = 4,     /* default_allreduce_rsag: ring-order bulk RS+AG (allreduce_rsag.cu:33-128) */
  MSCCLPP_AMD_ALGO_RSAG_ZC = 5,  /* default_allreduce_rsag_zero_copy: reads peers' inputs, writes peers' outputs,
                                    no scratch (allreduce_rsag_zero_copy.cu:41-112) */
  MSCCLPP_AMD_ALGO_RSAG_PIPELINE = 6, /* default_allreduce_rsag_pipeline: put / reduce / recv workgroups
                                         pipelined over a circular scratch (allreduce_rsag_pipeline.cu:85-222) */
  /* the int32 kernels of the mscclpp-test harness (test/mscclpp-test/allreduce_test.cu), by number */
  MSCCLPP_AMD_ALGO_TEST_K2 = 102, /* allreduce2, one node: LL16 one-hop all-pairs, harness scratch layout (:841-943) */
  MSCCLPP_AMD_ALGO_TEST_K5 = 105, /* allreduce5 (AMD branch): in-place RS by remote reads + ring AG by gets (:959-970) */
  MSCCLPP_AMD_ALGO_TEST_K6 = 106, /* allreduce6: LL16 two-hop, harness scratch layout (:972-1034) */
  MSCCLPP_AMD_ALGO_TEST_K7 = 107  /* allreduce7: LL8 two-hop, harness scratch layout (:1036-1093) */
};

/* One rank's view of the buffers of an AllReduce.  Pointers to other ranks' memory are the
 * addresses at which this rank has them mapped (IPC), or plain device pointers for in-process
 * ranks.  Entry [rank] of every peer array is this rank's own buffer. */
typedef struct {
  const void* input;
  void* output;
  void* scratch;                                   /* own scratch (two halves) */
  void* peerScratch[MSCCLPP_AMD_MAX_RANKS];        /* rank q's scratch as mapped here */
  void* peerOutput[MSCCLPP_AMD_MAX_RANKS];         /* rank q's output (bulk direct writes) */
  uint64_t* tokens;                                /* own inbound tokens [MAX_RANKS][MAX_CHANNELS] */
  uint64_t* peerTokens[MSCCLPP_AMD_MAX_RANKS];     /* rank q's tokens as mapped here */
  uint64_t* expected;                              /* own expected counters [MAX_RANKS][MAX_CHANNELS] */
  uint32_t* flags;                                 /* MSCCLPP_AMD_FLAG_SLOTS words, initialised to 1,
                                                      16-byte aligned */
  uint32_t* err;                                   /* device error word (0 = ok) */
  uint64_t scratchBytes;
  int32_t rank;
  int32_t pad;
  const void* peerInput[MSCCLPP_AMD_MAX_RANKS];    /* rank q's input as mapped here (zero-copy reads) */
  uint64_t* pipeSems;                              /* rsag_pipeline: 3 x 256 + 64 intra-launch counters,
                                                      zero before the first launch; every launch leaves
                                                      them zero (graph replays need no memset) */
} mscclppAmdRankView;

/* ---- memory ------------------------------------------------------------------------------- */
/* Uncached memory (hipDeviceMallocUncached, zeroed; the reference's GpuBuffer on AMD,
 * gpu_utils.cc:139-147) comes from a process-lifetime pool: mscclppAmdFree hands a pooled block back
 * to the pool, never to HIP, so no later allocation is placed where uncached memory was (DESIGN.md
 * §21).  The free does not synchronize: the block is reused only after a device synchronize, paid by
 * the allocation that reuses it.  mscclppAmdFree hipFree's anything else.
 * mscclppAmdUncachedPoolStats: bytes allocated from HIP, in use, and free in the pool. */
int mscclppAmdMallocUncached(void** ptr, size_t bytes);
int mscclppAmdMalloc(void** ptr, size_t bytes);
int mscclppAmdFree(void* ptr);
int mscclppAmdUncachedPoolStats(size_t* held, size_t* inUse, size_t* freeBytes);
/* Imports of peers' memory in this process: IPC mappings open now, and how many of them are kept
 * imports of peers' pooled uncached blocks (scratch, tokens, GpuBuffer), which stay mapped until
 * the process exits -- the import-side twin of the pool.  mscclppAmdIpcKeptRanges
 * writes up to `cap` (mapped address, bytes) pairs of the kept imports and their count to *n.  Any
 * pointer may be NULL. */
int mscclppAmdIpcStats(size_t* openMappings, size_t* keptImports);
int mscclppAmdIpcKeptRanges(uint64_t* addrs, uint64_t* bytes, size_t cap, size_t* n);
/* Forget the kept imports (after a device synchronize): each closes unless a live communicator still
 * holds it.  For a long-lived process whose peers come and go (an elastic job re-creating its peer
 * processes): a kept import keeps the exited peer's memory alive.  Call it only with no communicator
 * of the departed peers left, and expect this process's next allocations to be placed where the
 * closed mappings were -- the hazard DESIGN.md §21 describes, which the kept imports otherwise rule
 * out. */
int mscclppAmdIpcReleaseKept(size_t* released);
int mscclppAmdFlagsInit(uint32_t* flags, void* stream);

/* ---- 1-GPU microbench (BASELINE config 2) ------------------------------------------------- */
/* out = x (op) unpack(pack(y, flag)); pkts: 2*bytes of (uncached) device memory; bytes % 16 == 0.
 * 256-lane workgroups with 4 KiB per round; nblocks <= 0 selects the default grid (one workgroup per
 * 4 KiB up to 1024 of them), nblocks > 0 that grid (<= 1024).  budgetTicks: spin budget in 10 ns
 * ticks.  flags: MSCCLPP_AMD_FLAG_SLOTS words, 16-byte aligned.  The packet hand-off runs between the
 * waves of each workgroup. */
int mscclppAmdSelfReduceLL16(const void* x, const void* y, void* pkts, void* out, size_t bytes, int dtype, int op,
                             uint32_t* flags, int nblocks, uint64_t budgetTicks, uint32_t* err, void* stream);
/* The default shape for `bytes`: waves per workgroup, KiB per wave and round, workgroups, skewed. */
int mscclppAmdSelfReduceLL16DefaultShape(size_t bytes, int* waves, int* units, int* nblocks, int* skew);
/* The shape mscclppAmdSelfReduceLL16 launches for `bytes` on a caller's grid (nblocks > 0; <= 0: the
 * default): waves per workgroup, KiB per wave and round, the grid (an odd nblocks rounded up to even)
 * and the rounds between packing a tile and consuming it.  nblocks > 1024: ncclInvalidArgument. */
int mscclppAmdSelfReduceLL16GridShape(size_t bytes, int nblocks, int* waves, int* units, int* grid, int* skew);

/* Ceiling helpers used by the benchmark.  mscclppAmdCopy is a plain streaming copy (HBM ceiling);
 * mscclppAmdCopyJobs runs njobs copies in ONE launch, blocksPerJob workgroups each (the xGMI probe:
 * all peers' links driven from one kernel on one stream).  (Kernel shape sweeps and first-poll miss
 * counts of the self-reduce live in the test diagnostics library, tests/bin/libselfreduce_diag.so.) */
int mscclppAmdCopy(const void* src, void* dst, size_t bytes, int nblocks, void* stream);
int mscclppAmdCopyJobs(const void* const* srcs, void* const* dsts, const size_t* bytes, int njobs, int blocksPerJob,
                       void* stream);
/* The same with the cache policy of the loads / stores: 0 = sc0 sc1 (system scope, what the
 * collectives use for remote accesses), 1 = plain, 2 = nt, 3 = sc1 (agent scope).  Combinations
 * carried: any store policy with system loads; plain or system stores with plain loads; system stores
 * with nt or agent loads.  4 = a combination not carried. */
int mscclppAmdCopyJobsPolicy(const void* const* srcs, void* const* dsts, const size_t* bytes, int njobs,
                             int blocksPerJob, int loadPolicy, int storePolicy, void* stream);
/* The self-reduce's exact memory accesses (Y read, packets stored and the partner's read two rounds
 * late, X read, O written: 7 * bytes over the same buffers, grid and rounds) with no flags, readiness
 * tests or LDS: the streaming ceiling of that access mix.  bytes: a multiple of 8 KiB; pkts: 2 * bytes.
 * The output is meaningless. */
int mscclppAmdSelfReduceStream(const void* x, const void* y, void* pkts, void* out, size_t bytes, void* stream);
/* An independent streaming ceiling of the same 4:3 read:write mix, with none of the self-reduce's
 * layout or grid: X, Y (bytes each) and pin (2 * bytes) read, pout (2 * bytes) and out written, one
 * grid-stride loop, 2048 workgroups by default, non-temporal accesses.  bytes % 4096 == 0. */
int mscclppAmdMixStream(const void* x, const void* y, const void* pin, void* pout, void* out, size_t bytes, int nblocks,
                        void* stream);

/* ---- explicit-view AllReduce ------------------------------------------------------------- */
/* Launch `algo` for `nviews` ranks of an `nranks`-rank AllReduce in ONE kernel launch (views[i]
 * is handled by blockIdx.y == i).  nviews == 1 is the one-rank-per-process form; nviews ==
 * nranks runs every rank of the collective inside this process.  Every workgroup waits on other
 * ranks' workgroups, so nblocks * nviews workgroups must be resident at once; a grid that is not
 * returns ncclInvalidUsage (5) without launching. */
int mscclppAmdAllReduceLaunch(int algo, const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes,
                              int dtype, int op, int nblocks, int nthreads, uint64_t budgetTicks, void* stream);
/* coll 0 AllReduce (bytes = buffer), 1 ReduceScatter / 2 AllGather (bytes = nranks * block, block %
 * 16 == 0) through the bulk all-pairs kernel (reduce-scatter / all-gather halves of fullmesh). */
int mscclppAmdCollectiveLaunch(int coll, int algo, const mscclppAmdRankView* views, int nviews, int nranks,
                               size_t bytes, int dtype, int op, int nblocks, int nthreads, uint64_t budgetTicks,
                               void* stream);
/* AllToAll / AllToAllv by a zero-copy pull (kernels/alltoall.hip).  One segment per peer p, in bytes:
 * the rank receives `len` bytes at `dstOff` of its output from `srcOff` of peer p's input
 * (views[i].peerInput[p]; p == rank: its own input, a local copy).  Equal-split AllToAll of blocks
 * of B bytes is srcOff = rank * B, dstOff = p * B, len = B.  Zero-length segments are skipped;
 * segments may start at any byte (16-byte aligned starts on both sides take the fast path). */
typedef struct {
  uint64_t srcOff;
  uint64_t dstOff;
  uint64_t len;
} mscclppAmdAllToAllSeg;
/* Views as for mscclppAmdAllReduceLaunch (input = send buffer, output = receive buffer, peerInput[q]
 * = rank q's send buffer; no scratch).  segs: host memory, [nviews][nranks], copied before the call
 * returns.  nblocks <= 0: 256 KiB of the busiest view's receive bytes per workgroup, 8..128; every
 * rank of one collective must launch the same nblocks.  With nviews > 1 the table travels through
 * a device buffer the library allocates at the device's first such launch (not under capture).
 * 4: a null or out-of-range argument or launch shape; 5: a workgroup's range of a segment exceeds
 * 4 GiB (more workgroups carry it), or the grid cannot be resident at once. */
int mscclppAmdAllToAllLaunch(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdAllToAllSeg* segs,
                             int nblocks, int nthreads, uint64_t budgetTicks, void* stream);
/* Small AllToAll / AllToAllv by one hop of LL8 packets through the ranks' LL scratch (kernels/
 * alltoall_ll.hip): a push, nothing of the user's is registered and no token is
 * exchanged.  One entry per peer q, in bytes: the rank sends `sendLen` bytes at `sendOff` of its input to
 * rank q, and receives `recvLen` bytes from q at `recvOff` of its output (q == rank: a local copy).  What
 * r sends q must be what q expects from r.  Segments may start at any byte and may be empty. */
typedef struct {
  uint64_t sendOff;
  uint64_t sendLen;
  uint64_t recvOff;
  uint64_t recvLen;
} mscclppAmdAllToAllLLSeg;
/* Views as for mscclppAmdPullReduceLLLaunch (input = send buffer, output = receive buffer, scratch /
 * peerScratch / flags shared with the other LL kernels, so calls may alternate).  table: host memory,
 * [nviews][nranks], copied before the call returns.  The region stride comes from the largest length in
 * `table`: with nviews == nranks that is the whole matrix; with fewer views every process must pass
 * tables with the same largest length (the equal split does).  nblocks / nthreads <= 0: one lane per 8
 * bytes of the largest segment, 256 lanes, 1 to 128 workgroups.
 * 4 (nothing is launched, no device is touched): null fields, nranks outside 2..8, a rank twice, flags
 * not 16-byte aligned, a length one view sends that the receiving view does not expect, a bad launch
 * shape; 5: views whose scratchBytes differ or are below mscclppAmdAllToAllLLScratchRequired, a segment
 * size the path does not carry, or a grid that cannot be resident at once. */
int mscclppAmdAllToAllLLLaunch(const mscclppAmdRankView* views, int nviews, int nranks,
                               const mscclppAmdAllToAllLLSeg* table, int nblocks, int nthreads, uint64_t budgetTicks,
                               void* stream);
/* Scratch bytes per rank that call needs when its largest segment has maxSegBytes: two halves of nranks
 * regions of max(1, ceil(maxSegBytes / 8)) 16-byte units, each half rounded up to 256; 0: not carried. */
size_t mscclppAmdAllToAllLLScratchRequired(int nranks, size_t maxSegBytes);
/* 1 when ncclAllToAll / ncclAllToAllv send a call whose largest segment has maxSegBytes to the LL path,
 * else 0: 0 < maxSegBytes <= the built-in bound of nranks, or <=
 * MSCCLPP_AMD_A2A_LL_MAX_BYTES where that is set (0 disables the path, values above 1 MiB count as
 * 1 MiB; read once; it must be equal on all ranks). */
int mscclppAmdAllToAllTakesLL(int nranks, size_t maxSegBytes);
/* Reduce to `root` by a zero-copy pull-reduce at the root (kernels/reduce.hip): the root reads
 * `bytes` of every rank's input (views[root].peerInput[q] = rank q's send buffer), reduces in ring
 * order root, root + 1, ..., root + n - 1 (mod n) with the arithmetic of the AllReduce kernels, and
 * stores the result into its own output; the other ranks only hand-shake (their output is not
 * touched and may be NULL).  In place on the root (input == output) is carried.  dtype: any reduce
 * type code above; bytes: a multiple of its element size; pointers need the element's alignment only.
 * nblocks <= 0: 32 KiB per workgroup, 8..64; every rank of one collective must launch the same
 * nblocks.  4: a null or out-of-range argument or launch shape (nothing is launched); 5: a
 * workgroup's range exceeds 4 GiB (more workgroups carry it), or the grid cannot be resident at once. */
int mscclppAmdReduceLaunch(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype, int op,
                           int root, int nblocks, int nthreads, uint64_t budgetTicks, void* stream);
/* ncclMax / ncclAvg of Reduce, ReduceScatter and AllReduce, and all four operations of int64 /
 * uint64 / int8, by one zero-copy pull-reduce kernel
 * (kernels/pull_reduce.hip; arithmetic: pull_reduce_device.hpp).  Operands are taken in rank order
 * 0 .. n - 1 whichever rank reduces an element, so the three collectives give the same bits for
 * the same inputs.  coll MSCCLPP_AMD_PULL_REDUCE: `bytes` of every input reduced into the root's
 * output (other outputs untouched, may be NULL); _REDUCE_SCATTER: inputs hold nranks * bytes, rank
 * q's output receives block q (bytes); _ALLREDUCE: every output receives the `bytes` reduced -- rank
 * q reduces slice q (ceil(bytes / nranks) rounded up to 16) and the ranks then copy one another's
 * slices out of peerOutput[q].  Views as for mscclppAmdReduceLaunch, plus peerOutput[q] for
 * AllReduce.  In place is carried as input == output (Reduce on the root, AllReduce) and output ==
 * input + rank * bytes (ReduceScatter); the caller rules out any other overlap.  op: MSCCLPP_AMD_MAX
 * or MSCCLPP_AMD_AVG with dtype F16, BF16, F32, I32, U32, U8, E4M3, E5M2; MSCCLPP_AMD_SUM, _MIN, _MAX
 * or _AVG with dtype I64, U64, I8 (wrapping sums, signed / unsigned compares, the exact sum divided
 * by nranks toward zero); pointers need the element's alignment only (8 bytes for I64 / U64).  root
 * is read for Reduce only.  nblocks <= 0: mscclppAmdPullReduceDefaultBlocks, a function of (coll,
 * bytes) alone; every rank of one collective must launch the same nblocks.  4 (nothing is launched,
 * no device is touched): SUM / MIN of the eight types that have their own kernels for them, any
 * other op or dtype code, a byte count of 0 or one that splits an element, a bad root, coll or
 * launch shape, null fields; 5: a workgroup's range exceeds 4 GiB (more workgroups carry it), or the grid
 * cannot be resident at once. */
int mscclppAmdPullReduceLaunch(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype,
                               int op, int root, int nblocks, int nthreads, uint64_t budgetTicks, void* stream);
/* PreMulSum by the same kernel: op MSCCLPP_AMD_PREMUL_SUM with dtype F16, BF16 or F32 only.  The view
 * of rank k multiplies rank k's operand by rank k's scalar (one fp32 multiply, rounded before the fp32
 * sum in rank order; the sum is rounded once to the element type: pull_reduce_device.hpp), so the
 * scalars may differ between ranks; the kernel exchanges them itself.  scales: host array, one fp32
 * per view (the scalar of views[i].rank; a caller holding it in the element type decodes it, which
 * is exact).  scalePtrs: NULL, or a host array of one pointer per view; a non-null entry overrides
 * that view's immediate and points to ONE element of the element type in device memory, read when
 * the kernel runs (so a graph replay reads the value of its own time).  Everything else, and every
 * refusal, is as for mscclppAmdPullReduceLaunch; NULL scales, and any other op or dtype, answer 4. */
int mscclppAmdPullReduceLaunchScaled(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes,
                                     int dtype, int op, int root, int nblocks, int nthreads, uint64_t budgetTicks,
                                     void* stream, const float* scales, const void* const* scalePtrs);
int mscclppAmdPullReduceDefaultBlocks(int coll, uint64_t bytes);
/* The same reductions for SMALL messages by one hop of LL8 packets (kernels/pull_reduce_ll.hip; DESIGN.md
 * §17g): coll MSCCLPP_AMD_PULL_REDUCE_SCATTER or _ALLREDUCE only (a Reduce keeps the pull kernel: only
 * its root would wait for packets, which the reuse of the two scratch halves forbids), every (dtype,
 * op) mscclppAmdPullReduceLaunch / ...LaunchScaled take, operands in the same rank order, so the bits
 * are those of the pull path.  Views as for mscclppAmdAllReduceLaunch with MSCCLPP_AMD_ALGO_ALLPAIR
 * (input, output, scratch, peerScratch[q], flags, err; no tokens, no peerInput: no user buffer is read by
 * a peer and no handshake runs); the flags and the scratch are shared with the LL AllReduce kernels.
 * In place is carried as input == output (AllReduce) and output == input + rank * bytes
 * (ReduceScatter).  scales / scalePtrs: as for mscclppAmdPullReduceLaunchScaled with op
 * MSCCLPP_AMD_PREMUL_SUM, NULL for every other op.  nblocks / nthreads <= 0: one lane per 8 payload
 * bytes, 256 lanes, up to 128 workgroups -- a function of `bytes` alone.
 * 4 (nothing is launched, no device is touched): coll MSCCLPP_AMD_PULL_REDUCE or any other code, a
 * (dtype, op) the pull path refuses, a byte count of 0 or one that splits an element, nranks outside
 * 2..8, scales without PREMUL_SUM or PREMUL_SUM without scales, a bad launch shape, null fields;
 * 5: views whose scratchBytes differ or are below mscclppAmdPullReduceLLScratchRequired, a size the
 * path does not carry, or a grid that cannot be resident at once. */
int mscclppAmdPullReduceLLLaunch(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes,
                                 int dtype, int op, int nblocks, int nthreads, uint64_t budgetTicks, void* stream,
                                 const float* scales, const void* const* scalePtrs);
/* Scratch bytes per rank that call needs (two halves of nranks regions of ceil(words / 2) 16-byte
 * units, plus one unit per region for PREMUL_SUM's scalar); 0: the call is not carried. */
size_t mscclppAmdPullReduceLLScratchRequired(int coll, int nranks, size_t bytes, int dtype, int op);
/* 1 when ncclAllReduce / ncclReduceScatter send a call of `bytes` (the message / the per-rank block) of
 * these operations to the LL path, else 0: bytes <= the built-in bound of (coll, nranks) (DESIGN.md
 * §17g), or <= MSCCLPP_AMD_PULL_LL_MAX_BYTES where that is set (one bound for both collectives, 0
 * disables the path, values above 1 MiB count as 1 MiB; read once; it must be equal on all ranks). */
int mscclppAmdPullReduceTakesLL(int coll, int nranks, size_t bytes);
/* Send / Recv by a zero-copy pull (kernels/sendrecv.hip): one launch runs a table of point-to-point
 * operations, in table order.  An operation moves `bytes` from `send` on rank `src` to `recv` on
 * rank `dst`: the receiver reads `send` -- the address at which the view of rank `dst` has the
 * sender's buffer mapped; a plain device pointer for in-process ranks -- and stores into `recv`;
 * the sender's view only signals and waits, and reads neither pointer.  A view runs the operations
 * in which it is src or dst (only tokens, peerTokens, expected, err and rank of a view are used).
 * Buffers may start at any byte (16-byte aligned starts on both sides take the fast path).
 * nblocks <= 0: each operation's workgroups from its byte count (mscclppAmdSendRecvDefaultBlocks:
 * 128 KiB each, 1..64); nblocks > 0: that many for every operation (<= 128) -- the same on both
 * sides of every operation.  Sender and receiver of a pair must list the operations between them in
 * the same order.
 * 4: a null pointer, nviews not 1 or nranks, src == dst, a rank out of range, nops of 0 or above
 * MSCCLPP_AMD_SENDRECV_MAX_OPS, bytes of 0, nblocks > 128, or nthreads not a multiple of 64 in
 * 64..512 (all checked before any device call; nothing is launched); 5: a workgroup's sub-range
 * exceeds 4 GiB (more workgroups carry it), or the grid cannot be resident at once. */
#define MSCCLPP_AMD_SENDRECV_MAX_OPS 64
typedef struct {
  int32_t src, dst;
  const void* send;
  void* recv;
  uint64_t bytes;
} mscclppAmdSendRecvOp;
int mscclppAmdSendRecvLaunch(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdSendRecvOp* ops,
                             int nops, int nblocks, int nthreads, uint64_t budgetTicks, void* stream);
int mscclppAmdSendRecvDefaultBlocks(uint64_t bytes);
/* Scratch bytes per rank (both halves) that `algo` needs for `bytes` (0 if unsupported).  For the
 * pipelined RS+AG this is one stage at the default shape (32 x 512); a larger shape needs
 * mscclppAmdScratchRequiredShape. */
size_t mscclppAmdScratchRequired(int algo, int nranks, size_t bytes, int dtype);
size_t mscclppAmdScratchRequiredShape(int algo, int nranks, size_t bytes, int dtype, int nblocks, int nthreads);
/* Algorithm the selector picks: the tuned-config store's entry for this SKU, rank count and size
 * (built-in table = algorithm_selector.cc:91-139, AMD branch), MSCCLPP_AMD_ALGO_*. */
int mscclppAmdSelectAlgo(int nranks, size_t bytes, int dtype);
/* Tuned-config store (the JSON format of python/mscclpp_benchmark/tuning_config.py): load a file
 * whose profiles take precedence over the built-in table (as MSCCLPP_AMD_TUNED_CONFIG=<path> does at
 * start-up), and query the entry for a collective ("allreduce", "allgather", "reducescatter") of
 * `bytes` on `nranks` ranks: algorithm name and launch shape (0 = default).  Query returns 5 when no
 * entry applies. */
int mscclppAmdTunedConfigLoad(const char* path);
int mscclppAmdTunedConfig(const char* collective, int nranks, size_t bytes, char* algorithm, size_t algorithmLen,
                          int* nblocks, int* nthreads);
/* Where the entry that applies came from: "reference" (the reference's selector restated),
 * "fabric-free" (measured with every rank on one GPU: no link bytes priced), "reference; grid
 * fabric-free", "tuned" (a loaded file's entry without its own "source" tag) or that tag. */
int mscclppAmdTunedConfigSource(const char* collective, int nranks, size_t bytes, char* source, size_t sourceLen);

/* ---- communicator extensions -------------------------------------------------------------- */
// Phase trace of the collective kernels (the reference's NPKit events, npkit.hpp): while a buffer of
// at least MSCCLPP_AMD_TRACE_BYTES device bytes is set, every AllReduce / ReduceScatter / AllGather
// launch of this process has lane 0 of each workgroup write the wall clock (s_memrealtime ticks,
// 100 MHz) at its phase boundaries to buf[(rankView * 256 + workgroup) * 8 + event] (u64).  Events:
// bulk (fullmesh / rsag): 0 start, 1 reduce-scatter puts issued, 2 reduce-scatter handshake done,
// 3 reduce + all-gather stores issued, 4 end; zero-copy: 0 start, 1 entry handshake done, 2 reduce +
// all-gather stores issued, 3 end; LL16: 0 start, 1 step 1 (puts), 2 step 2 (reduce + broadcast),
// 3 step 3 (unpack) done; LL8: 0 start, 1 puts issued, 2 end; AllToAll: 0 start, 1 entry handshake
// done, 2 segments stored, 3 end; AllToAll LL: 0 start, 1 puts issued, 2 stored; Reduce: 0 start, 1 entry handshake done, 2 result stored (root),
// 3 end; Send/Recv: 0 start, 1 readies posted, 2 receives stored, 3 dones seen; pull-reduce (MAX /
// AVG): 0 start, 1 entry handshake done, 2 own range reduced, 3 peers' slices gathered (AllReduce
// only), 4 end.  buf = NULL turns it off.  Returns 0,
// or 4 when the buffer is too small.
#define MSCCLPP_AMD_TRACE_BYTES ((size_t)MSCCLPP_AMD_MAX_RANKS * 256 * 8 * 8)
int mscclppAmdTraceSet(void* buf, size_t bytes);

int mscclppAmdCommAllReduce(ncclComm_t comm, const void* sendbuff, void* recvbuff, size_t count, int ncclDtype,
                            int ncclOp, int algo, int nblocks, int nthreads, void* stream);
/* As above with the accumulation type of Algorithm::execute (accumNcclDtype: -1 = AUTO, i.e. the
 * element type; ncclFloat16 / ncclFloat32 for FP8 buffers). */
int mscclppAmdCommAllReduceAccum(ncclComm_t comm, const void* sendbuff, void* recvbuff, size_t count, int ncclDtype,
                                 int ncclOp, int accumNcclDtype, int algo, int nblocks, int nthreads, void* stream);
/* Reduce-type code (MSCCLPP_AMD_*) for an ncclDataType_t and accumulation type (-1 = AUTO), or -1. */
int mscclppAmdReduceType(int ncclDtype, int accumNcclDtype);
int mscclppAmdCommBarrier(ncclComm_t comm);
/* The vendor (RCCL) communicator created beside this one when MSCCLPP_AMD_NCCL_LIB_PATH is set, or
 * NULL (no vendor library, or it refused the communicator). */
int mscclppAmdCommVendorComm(ncclComm_t comm, void** vendorComm);
/* Collective: every rank passes its matching device buffer; peers[r] receives rank r's buffer as
 * mapped in this process (peers[rank] = ptr), MSCCLPP_AMD_MAX_RANKS entries (Communicator::
 * registerMemory of algorithm.hpp; registerMemory + sendMemory/recvMemory in the reference). */
int mscclppAmdCommRegisterBuffer(ncclComm_t comm, void* ptr, void** peers);
/* Collective: close every cached mapping of peers' user buffers (scratch / semaphores stay); call it
 * when buffers that were used with the communicator are freed. */
int mscclppAmdCommDeregisterAll(ncclComm_t comm);
int mscclppAmdCommGetDeviceError(ncclComm_t comm, uint32_t* code, int clear);
/* The communicator's whole error record: words4[0] = the code (as above), words4[1..3] = the detail
 * its first reporter wrote.  kErrPacketTimeout (1): the flag waited for, the byte offset of the
 * packet (or 32-byte unit) in the polled region, the flag word last read there; semaphore timeouts
 * of the bulk and executor kernels: channel / block / expected value.  clear != 0
 * zeroes all four words. */
int mscclppAmdCommGetDeviceErrorDetail(ncclComm_t comm, uint32_t* words4, int clear);
/* Registration cache state: user buffers registered (at most 64, least recently used retired
 * beyond), IPC mappings open in this process (all communicators), mappings waiting for a device
 * synchronize before they close.  Any pointer may be NULL. */
int mscclppAmdCommRegistrationStats(ncclComm_t comm, size_t* userRegistrations, size_t* liveMappings,
                                    size_t* retiredMappings);
/* Host all-gathers made by user-buffer registration so far: one per newly registered allocation,
 * one per new buffer offset inside a registered allocation (none when the communicator runs with
 * MSCCLPP_NCCL_SYMMETRIC_MEMORY, env.hpp:101-107, which *symmetricMemory reports). */
int mscclppAmdCommRegistrationExchanges(ncclComm_t comm, uint64_t* allocationExchanges, uint64_t* offsetExchanges,
                                        int* symmetricMemory);
/* Collective calls of this communicator that took the LL path of mscclppAmdPullReduceLLLaunch. */
int mscclppAmdCommPullLLCount(ncclComm_t comm, uint64_t* count);
/* ncclAllToAll / ncclAllToAllv calls of this communicator that took the LL path of
 * mscclppAmdAllToAllLLLaunch (counted apart from the above). */
int mscclppAmdCommAllToAllLLCount(ncclComm_t comm, uint64_t* count);
int mscclppAmdCommScratch(ncclComm_t comm, void** scratch, size_t* bytes);
int mscclppAmdCommFlags(ncclComm_t comm, uint32_t** flags);
/* Bootstrap all-gather of `bytes` per rank (host memory), for harnesses. */
int mscclppAmdCommAllGatherHost(ncclComm_t comm, const void* sendbuf, void* recvbuf, size_t bytes);

/* ---- host-proxy path (PortChannel / FIFO / proxy thread) ------------------------------------
 * Config-1 harness: test/allgather_test_host_offloading.cu on this library.  out[0] = us per
 * kernel (no graph), out[1] = us per kernel (graph of graphIters x 2 kernels), out[2] = 1 if the
 * gathered data is correct, out[3] = NUMA node the proxy thread was bound to (-1 if none). */
int mscclppAmdHostOffloadAllGather(ncclComm_t comm, size_t dataSize, int iters, int graphIters, double* out);
/* PortChannel all-to-all through the proxy (mode 0: put+signal, 1: putWithSignal,
 * 2: putWithSignalAndFlush).  out[0] = us per iteration (wall clock over `iters` back-to-back
 * launches after one untimed launch), out[1] = 1 if correct, out[2] = NUMA node. */
int mscclppAmdPortChannelAllToAll(ncclComm_t comm, size_t chunk, int mode, int iters, double* out);
/* The same with each iteration's own duration (a HIP event before every launch): with outLen >= 7,
 * out[3] = median, out[4] = min, out[5] = max us per iteration, out[6] = index of the slowest one;
 * with outLen >= 8, out[7] = the proxy thread's longest gap between FIFO polls in us over the timed
 * iterations (measured with MSCCLPP_AMD_PROXY_GAP_STATS=1, else 0).  With outLen >= 16 the proxy
 * stamps every timed trigger (ProxyService::enableStamps) and out[8..15] = medians over iterations,
 * us: launch -> this rank's last data copy complete, launch -> its last token update complete, that
 * token update -> kernel end (the wait for the peers' tokens), host submit time of a data copy, of a
 * token update, of a whole trigger; the slowest iteration's launch -> token complete; stamps taken. */
int mscclppAmdPortChannelAllToAllStats(ncclComm_t comm, size_t chunk, int mode, int iters, double* out, int outLen);
/* mscclpp-test allreduce1 (test/mscclpp-test/allreduce_test.cu:730-839): int32 ring RS + AG whose data
 * moves through PortChannels and the host proxy (hipMemcpyAsync).  out[0] = us per AllReduce (graph of
 * `iters` kernels replayed `graphLaunches` times), out[1] = 1 if every element is n(n-1)/2, out[2] =
 * NUMA node of the proxy thread.  nblocks <= 0: the harness's 24 (x 1024 threads). */
int mscclppAmdProxyRingAllReduce(ncclComm_t comm, size_t nelems, int iters, int graphLaunches, int nblocks,
                                 double* out);
int mscclppAmdLaunchRingProxyAllReduce(int* buff, const int* scratch, int rank, int nranks, size_t nelems,
                                       const void* channels4, void* gridBarrier, int nblocks, int nthreads,
                                       uint64_t budget, uint32_t* err, void* stream);
int mscclppAmdLaunchHostOffloadKernel(int rank, int nranks, const void* fifoHandle, void* semHandles, int handleIndex,
                                      uint64_t budget, uint32_t* err, void* stream);
int mscclppAmdLaunchPortChannelPut(void* chans, int nchans, const uint64_t* dstOffs, const uint64_t* srcOffs,
                                   uint64_t chunk, int mode, void* stream);

/* MemoryChannel device-surface self-test on one GPU (two in-process ranks): mode 0 LL16 packet
 * ping-pong, 1 LL8 ping-pong, 2 put + signal/wait round trip.  *failures = mismatching words.
 * Modes 3 / 4: rank 0 unpacks LL16 / LL8 packets of flag 7 that rank 1 never puts; the wait ends at
 * a 20 ms budget and devErr[0..3] (4 words) receives the error record (code, flag, packet byte,
 * flag seen). */
int mscclppAmdMemChannelSelfTest(int mode, int nElem, int nTries, int* failures, uint32_t* devErr);
/* put, get and putPackets + unpackPackets (LL16, LL8) of `bytes` (multiple of 16, meant to exceed
 * 4 GiB) on one GPU, nblocks x 256 lanes as one thread group; bad[0..3] = words that differ from the
 * source pattern after each of the four (memory_channel_device.hpp:101-215 take 64-bit offsets). */
int mscclppAmdMemChannelBigTest(uint64_t bytes, int nblocks, unsigned long long* bad, uint32_t* devErr);
/* The reference's MemoryChannel packet ping-pong latency (test/mp_unit/memory_channel_tests.cu:
 * 98-107), collective over a 2-rank communicator: a MemoryChannel into the peer's packet buffer built
 * with the host API, 1000 checked tries, then `iters` timed one-way hand-offs of nElem ints as LL8
 * (ll8 != 0) or LL16 packets.  out[0] = us per iteration (host clock between the barriers around the
 * launch), out[1] = 1 if every receive matched and no device error was recorded, out[2..5] (when
 * outLen allows) = the error record: code, flag, packet byte, flag seen. */
int mscclppAmdMemChannelPingPong(ncclComm_t comm, int nElem, int iters, int ll8, double* out, int outLen);
/* One rank's ping-pong kernel: `handle` = a host MemoryChannelDeviceHandle (dst_ = the peer's packet
 * buffer, packetBuffer_ = this rank's), rank 0 or 1, flags flagBase + 1 ... flagBase + nTries,
 * *ret = 1 on a mismatch. */
int mscclppAmdLaunchMemChannelPingPong(const void* handle, int* buff, int rank, int nElem, int nTries,
                                       uint32_t flagBase, int ll8, int* ret, void* stream);

/* ---- bootstrap (TcpBootstrap, src/core/bootstrap/bootstrap.cc:169-611) -------------------------
 * Host-only setup plane; uniqueId is the 128-byte ncclUniqueId from ncclGetUniqueId. */
int mscclppAmdBootstrapCreate(int rank, int nranks, const void* uniqueId, void** handle);
int mscclppAmdBootstrapAllGather(void* handle, const void* sendbuf, void* recvbuf, size_t bytes);
int mscclppAmdBootstrapBarrier(void* handle);
int mscclppAmdBootstrapDestroy(void* handle);

#ifdef __cplusplus
}
#endif

#endif /* MSCCLPP_AMD_H_ */
