// Internal host-runtime declarations shared by the host translation units (not installed): errors and
// logging, environment readers, device memory and IPC helpers, the communicator, the vendor fallback.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "bootstrap.hpp"
#include "mscclpp_amd/algorithm.hpp"
#include "mscclpp_amd/mscclpp_amd.h"
#include "mscclpp_amd/nccl.h"
#include "launchers.hpp"  // kernels/: the collective kernels' host entry points
#include "nccl_types.hpp"
#include "peer_mappings.hpp"

namespace mscclpp_amd {
namespace host {

struct HipError : std::runtime_error {
  hipError_t code;
  HipError(hipError_t c, const char* what) : std::runtime_error(what), code(c) {}
};

#define HIPCHECK(cmd)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (cmd);                                                                          \
    if (e_ != hipSuccess) {                                                                         \
      char buf_[256];                                                                               \
      snprintf(buf_, sizeof(buf_), "%s:%d %s -> %s", __FILE__, __LINE__, #cmd, hipGetErrorString(e_)); \
      throw HipError(e_, buf_);                                                                     \
    }                                                                                               \
  } while (0)

inline thread_local std::string gLastError;

inline int logLevel() {
  static int lvl = [] {
    const char* e = std::getenv("MSCCLPP_LOG_LEVEL");
    if (!e) return 1;
    std::string s(e);
    if (s == "DEBUG" || s == "TRACE") return 3;
    if (s == "INFO") return 2;
    if (s == "WARN") return 1;
    return 0;
  }();
  return lvl;
}

inline void warn(const std::string& m) {
  gLastError = m;
  if (logLevel() >= 1) fprintf(stderr, "[mscclpp_amd WARN] %s\n", m.c_str());
}
inline void info(const std::string& m) {
  if (logLevel() >= 2) fprintf(stderr, "[mscclpp_amd INFO] %s\n", m.c_str());
}

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const HipError& e) {
    warn(e.what());
    return ncclUnhandledCudaError;
  } catch (const mscclpp_amd::CudaError& e) {  // a failed HIP runtime call (MSCCLPP_CUDATHROW, gpu_utils.hpp)
    warn(e.what());
    return ncclUnhandledCudaError;
  } catch (const mscclpp_amd::Error& e) {  // the host channel API's errors (core.hpp)
    warn(e.what());
    switch (e.getErrorCode()) {
      case mscclpp_amd::ErrorCode::InvalidUsage: return ncclInvalidUsage;
      case mscclpp_amd::ErrorCode::RemoteError:
      case mscclpp_amd::ErrorCode::Timeout: return ncclRemoteError;
      case mscclpp_amd::ErrorCode::SystemError: return ncclSystemError;
      default: return ncclInternalError;
    }
  } catch (const std::invalid_argument& e) {
    warn(e.what());
    return ncclInvalidArgument;
  } catch (const std::logic_error& e) {  // InvalidUsage (e.g. no selector, null executor)
    warn(e.what());
    return ncclInvalidUsage;
  } catch (const std::exception& e) {
    warn(e.what());
    return ncclInternalError;
  } catch (...) {
    warn("unknown exception");
    return ncclInternalError;
  }
}

inline uint64_t spinBudgetTicks() {
  static uint64_t t = [] {
    const char* e = std::getenv("MSCCLPP_AMD_SPIN_TIMEOUT_MS");
    uint64_t ms = e ? std::strtoull(e, nullptr, 10) : 20000;
    if (ms == 0) ms = 20000;
    return ms * 100000ull;  // s_memrealtime ticks at 100 MHz
  }();
  return t;
}

// MSCCLPP_AMD_BULK_SCRATCH_MB (default 128, the reference's scratch, nccl.cc:180): the bulk scratch
// allocated once at communicator init and never re-allocated; a bucket whose n regions do not fit
// runs in several passes (bulkScratchRequired).
inline size_t bulkScratchInitBytes() {
  const char* e = std::getenv("MSCCLPP_AMD_BULK_SCRATCH_MB");
  size_t mb = e ? std::strtoull(e, nullptr, 10) : 128;
  if (mb < 64) mb = 64;
  return mb << 20;
}

// Uncached device memory (hipDeviceMallocUncached, zeroed) from the process-lifetime pool
// (uncached_pool.cpp: never returned to HIP while the process runs).  freeDevice
// returns a pooled block to the pool and hipFree's anything else, and never throws (destructors
// call it); releaseUncached is false for a pointer the pool does not own.  A release never
// synchronizes (*syncError stays hipSuccess): the block is reused only after the device has drained,
// at the allocation that reuses it (uncached_pool.cpp).
void* allocUncached(size_t bytes);
bool releaseUncached(void* p, hipError_t* syncError) noexcept;
// Fill `bytes` of device memory with `value` and return once the fill has completed on the device
// (own non-blocking stream + synchronize, as the reference's gpuMemset, gpu_utils.cc:274-283).  Every
// set-up fill of memory that a peer, a proxy or a kernel on another stream may touch next goes
// through it: a plain hipMemset is asynchronous to the host, so a host barrier or exchange after it
// orders nothing on the device.
void memsetSync(void* p, int value, size_t bytes);
void freeDevice(void* p) noexcept;
void uncachedPoolStats(size_t* held, size_t* inUse, size_t* freeBytes);
bool isPooledUncached(const void* base);  // `base` is a live block of the pool (an allocation base)

// MSCCLPP_NCCL_SYMMETRIC_MEMORY (env.hpp:101-107, env.cpp:67; any value but "0" is true): every rank
// allocates its communication buffers symmetrically, so a buffer sits at the same offset inside its
// allocation on every rank.  Registration then needs no host exchange for a new buffer inside an
// allocation that is already registered (the reference caches one context per allocation in that
// mode and passes the offset to the kernel, allreduce_fullmesh.cu:206-208, :248-257).
inline bool envSymmetricMemory() {
  const char* e = std::getenv("MSCCLPP_AMD_NCCL_SYMMETRIC_MEMORY");
  if (!e) e = std::getenv("MSCCLPP_NCCL_SYMMETRIC_MEMORY");
  return e && std::string(e) != "0";
}

inline size_t envMaxUserRegs() {
  const char* e = std::getenv("MSCCLPP_AMD_MAX_USER_REGS");
  const long v = e ? std::atol(e) : 0;
  return v > 0 ? (size_t)v : 1024;
}

inline int envAlgo() {  // MSCCLPP_AMD_ALGO, read once
  static const int algo = [] {
    const char* e = std::getenv("MSCCLPP_AMD_ALGO");
    if (!e) return (int)MSCCLPP_AMD_ALGO_AUTO;
    const std::string s(e);
    if (s == "packet") return (int)MSCCLPP_AMD_ALGO_PACKET;
    if (s == "allpair" || s == "allpair_packet") return (int)MSCCLPP_AMD_ALGO_ALLPAIR;
    if (s == "fullmesh") return (int)MSCCLPP_AMD_ALGO_FULLMESH;
    if (s == "rsag") return (int)MSCCLPP_AMD_ALGO_RSAG;
    if (s == "rsag_zc" || s == "rsag_zero_copy") return (int)MSCCLPP_AMD_ALGO_RSAG_ZC;
    if (s == "rsag_pipeline") return (int)MSCCLPP_AMD_ALGO_RSAG_PIPELINE;
    return (int)MSCCLPP_AMD_ALGO_AUTO;
  }();
  return algo;
}

}  // namespace host
}  // namespace mscclpp_amd

using namespace mscclpp_amd;
using namespace mscclpp_amd::host;

namespace mscclpp_amd {
namespace host {
// Process-wide cache of opened IPC handles (gpu_ipc_mem.cc:193-223 keeps one for HIP too): a handle
// is opened once per process however many owners hold it, and closed when the last owner drops
// its reference.  Implemented in core.cpp.
std::shared_ptr<void> openIpcHandle(const hipIpcMemHandle_t& handle);
// An import of a peer's allocation (base, bytes) exported by process `owner` (its processNonce).
// pooled: the owner's uncached pool holds the block for its whole life, so the mapping is kept open
// for the life of this process and reused by later exports of the same block (core.cpp); otherwise
// openIpcHandle.
std::shared_ptr<void> openIpcImport(const hipIpcMemHandle_t& handle, uint64_t owner, uint64_t base, uint64_t bytes,
                                    bool pooled);
uint64_t processNonce();  // random, fixed per process: tells exporters' pools apart
void keptIpcImports(std::vector<std::pair<uint64_t, uint64_t>>* ranges);  // (mapped address, bytes)
size_t releaseKeptIpcImports();  // forget every kept import (mscclppAmdIpcReleaseKept)
size_t liveIpcMappings();
// Drop a reference to a mapping on the closer thread (core.cpp): a close waits for the device to go
// idle, which must not happen on a caller's thread.  pendingMappingReleases = queued or running.
void releaseMappingLater(int device, std::shared_ptr<void> map);
size_t pendingMappingReleases();
uint64_t allocationId(const void* ptr);  // HIP_POINTER_ATTRIBUTE_BUFFER_ID (0 if unknown)
// Tuned configuration (tuning.cpp) for a collective of `bytes` on `nranks` ranks of this device's
// SKU: the algorithm name and launch shape (0 = the algorithm's default); false if none.
// nBlocks value a built-in algorithm's caller passes when it has looked the tuned launch shape up
// itself and found none: use the defaults without looking again.
constexpr int kTunedShapeResolved = -2147483647;
// Generation of the tuned-config store (changes whenever a file is loaded into it).
uint64_t tunedGeneration();
bool tunedConfig(const std::string& collective, int nranks, uint64_t bytes, std::string& algorithm, int& nblocks,
                 int& nthreads, std::string* source = nullptr);
int algoCodeOf(const std::string& name);  // MSCCLPP_AMD_ALGO_* of a default_allreduce_* name, or -1
}  // namespace host
}  // namespace mscclpp_amd

// Every rank's buffer as mapped in this process, plus the references that keep the peers' mappings
// open (entry [rank] is the local pointer and holds no reference).
struct PeerBufs {
  std::array<void*, MSCCLPP_AMD_MAX_RANKS> ptr{};
  std::array<std::shared_ptr<void>, MSCCLPP_AMD_MAX_RANKS> maps{};
  void*& operator[](int r) { return ptr[(size_t)r]; }
  void* operator[](int r) const { return ptr[(size_t)r]; }
};

struct IpcBlob {
  hipIpcMemHandle_t handle;
  uint64_t base;    // allocation base in the owner's address space (cache key)
  uint64_t offset;  // pointer - base
  uint64_t bytes;
  uint64_t owner;   // the exporting process's processNonce()
  uint32_t pooled;  // the allocation is a block of the owner's uncached pool (kept-open import)
  uint32_t pad;
};

// This process's export record of the allocation holding `ptr`.
inline IpcBlob exportBlob(const void* ptr) {
  IpcBlob b{};
  void* base = nullptr;
  size_t sz = 0;
  HIPCHECK(hipMemGetAddressRange((hipDeviceptr_t*)&base, &sz, (hipDeviceptr_t)ptr));
  HIPCHECK(hipIpcGetMemHandle(&b.handle, base));
  b.base = (uint64_t)base;
  b.offset = (uint64_t)((const char*)ptr - (char*)base);
  b.bytes = sz;
  b.owner = processNonce();
  b.pooled = isPooledUncached(base) ? 1u : 0u;
  return b;
}

inline std::shared_ptr<void> importBlob(const IpcBlob& b) {
  return openIpcImport(b.handle, b.owner, b.base, b.bytes, b.pooled != 0);
}

// The communicator.  Data first; the methods are defined in comm_registration.cpp (exchange, scratch,
// user-buffer registration, teardown), comm_collectives.cpp and comm_p2p.cpp.  How long a mapping of
// a peer's memory stays open is stated once, in peer_mappings.hpp.
struct ncclComm {
  // ---- types ------------------------------------------------------------------------------------
  // Selection memo of the NCCL entry points (comm.cpp selectAndExecute): the built-in selector's
  // choice and the tuned launch shape per (collective, message size, dtype), valid for one
  // tuned-store generation.  Used only while no user selector is set: a user's selector is asked on
  // every call, as the reference does.
  struct SelMemo {
    const char* coll = nullptr;
    size_t size = 0;
    int dtype = -1;
    uint64_t gen = 0;
    std::shared_ptr<mscclpp_amd::Algorithm> algo;
    int nb = 0, nt = 0;
  };
  // The registration of one local allocation (userRegs, pairedRegs).
  struct UserReg {
    uint64_t bufferId = 0;
    PeerBufs bases;  // symmetric memory and AllToAllv: every rank's allocation, exchanged once
    // lease.maps: every peer mapping a pointer of this allocation was resolved through
    // (registerOutput, one per peer allocation), open for as long as the registration lives;
    // lease.pinned: used under stream capture, or registered for the caller
    Lease lease;
    std::map<uint64_t, std::array<void*, MSCCLPP_AMD_MAX_RANKS>> byOffset;
    // (allocation base, HIP buffer id) of every rank's buffer this one was exchanged with (pairedRegs)
    std::array<std::pair<uint64_t, uint64_t>, MSCCLPP_AMD_MAX_RANKS> peerIdent{};
  };
  typedef std::map<std::pair<uint64_t, uint64_t>, UserReg> RegMap;  // by (allocation base, size)
  // What an AllToAllv rank tells the others about its send buffer (sendIdent, registerPaired).
  struct SendIdent {
    uint64_t base, id, off;
    uint64_t pairedBase[MSCCLPP_AMD_MAX_RANKS], pairedId[MSCCLPP_AMD_MAX_RANKS];
  };
  // A PreMulSum handle (ncclRedOpCreatePreMulSum / ncclRedOpDestroy).
  struct PreMulOp {
    bool live = false;
    ncclDataType_t datatype = ncclFloat32;
    float scalar = 0.0f;          // ncclScalarHostImmediate: decoded when the handle was created
    const void* device = nullptr;  // ncclScalarDevice: read by the kernel of every collective that uses the handle
  };
  // A send's message to its receiver (p2pPost, p2pMatch).
  struct P2pMsg {
    IpcBlob blob;    // the allocation holding the send buffer; blob.offset = the buffer inside it
    uint64_t bytes;
    uint32_t ok;     // 0: the sender could not export its buffer; both sides refuse the transfer
    uint32_t pad;
  };

  // ---- data -------------------------------------------------------------------------------------
  std::unique_ptr<StarBootstrap> boot;
  // the C++ plugin layer (algorithm.cpp): handle passed to Algorithm::execute, the collection the
  // NCCL entry points select from (nccl.cc:176, :308-314) and the executor for DSL algorithms,
  // created on the first DSL selection (collective: every rank selects the same algorithm)
  std::shared_ptr<mscclpp_amd::Communicator> cxx;
  std::unique_ptr<mscclpp_amd::AlgorithmCollection> algos;
  std::shared_ptr<mscclpp_amd::Executor> executor;
  // the vendor library's communicator for operations this path does not carry (nccl.cc:331-346),
  // present when MSCCLPP_AMD_NCCL_LIB_PATH names librccl (nccl_compat.cpp)
  void* fallback = nullptr;
  hipStream_t errStream = nullptr;  // ncclCommGetAsyncError's reads
  // the copy stream every host-channel Connection of this communicator shares (core.cpp connect);
  // owned by the connections, created by the first one
  std::weak_ptr<void> ipcStream;
  std::mutex ipcStreamMu;
  std::array<SelMemo, 16> selMemo{};
  std::mutex selMu;
  int rank = 0, nranks = 1, device = 0;
  // LL scratch (two halves, packets), bulk scratch, semaphores, flags, error word
  void* llScratch = nullptr;
  size_t llBytes = 0;
  void* bulkScratch = nullptr;
  size_t bulkBytes = 0;
  uint64_t* tokens = nullptr;
  uint64_t* expected = nullptr;
  uint32_t* flags = nullptr;
  uint32_t* err = nullptr;
  PeerBufs peerLL, peerBulk, peerTok;
  std::array<uint64_t*, MSCCLPP_AMD_MAX_RANKS> peerTokens{};
  static constexpr size_t kPipeSemsWords = 3 * 256 + 64;
  uint64_t* pipeSems = nullptr;  // rsag_pipeline's intra-launch counters (3 x 256 + done count)
  std::vector<void*> outgrown;   // scratch buffers that grew: kept allocated until destroy (ensure)

  std::mutex mu;  // held by every launch: guards the scratch above once set up, and everything below
  // the leases let go and the ones the current call hands to its kernel (peer_mappings.hpp)
  RetireQueue mappings;
  // kMaxUserRegs: 1024 by default, MSCCLPP_AMD_MAX_USER_REGS sets it.  The reference's context cache
  // has no bound (algorithm.cc:52-60); a small one made a caller cycling through more buckets
  // re-register on every call -- a host exchange, and, with the device busy, a wait for the close of
  // the same handle still in flight (openIpcHandle; 2.8 s behind a 2.8 s kernel in
  // tests/test_no_device_sync_gpu.py).  A bound is still kept: each registration keeps the peers'
  // allocations mapped, so a peer's freed buffer stays held until its registration is retired.
  const size_t kMaxUserRegs = envMaxUserRegs();
  RegMap userRegs;  // the matching-buffer collectives' registrations (registerOutput)
  // AllToAllv's send buffers.  Its ranks pass buffers of different sizes, which each rank's
  // allocator places on its own, so "my buffer X goes with your buffer Y" -- what userRegs caches,
  // keyed by the local buffer alone -- does not hold from one call to the next.  The call's own
  // all-gather therefore carries each rank's allocation identity (base, HIP buffer id), its offset
  // and the identities its cached registration was made with (sendIdent); from the gathered rows
  // every rank derives the same answer to "does any rank hold a pairing that is not the current
  // one", and if so all exchange their allocations again (registerPaired).  Offsets come from the
  // gather on every call.  These registrations live in a map of their own: re-pairing one must not
  // touch what the matching-buffer collectives cached for the same allocation.
  RegMap pairedRegs;
  uint64_t useClock = 0;  // lastUse of every lease of this communicator
  bool symmetricMemory = envSymmetricMemory();
  // host all-gathers the registration path made: allocations exchanged, offsets exchanged
  uint64_t allocExchanges = 0, offsetExchanges = 0;
  // Broadcast: the import of root's buffer, per root, and the launches that read through it; a
  // replaced slot that a graph captured waits in bcastPinned (a graph may read through it)
  std::array<Lease, MSCCLPP_AMD_MAX_RANKS> bcast;
  std::vector<Lease> bcastPinned;
  // Send / Recv: imports of the peers' send allocations, kept open per peer so that a second
  // transfer from the same allocation opens nothing: at most kP2pKept per peer, the least recently
  // used one retired beyond that, behind the events of the launches that read through it.  A launch
  // holds at most MSCCLPP_AMD_SENDRECV_MAX_OPS <= kP2pKept mappings, so the one retired is never one
  // the pending launch uses.  (Each lease holds one mapping.)
  static constexpr size_t kP2pKept = 64;
  std::array<std::vector<Lease>, MSCCLPP_AMD_MAX_RANKS> p2pImports;
  static constexpr int kP2pTag = 3;  // outside the 4k+0..2 tag spaces of core.cpp (memTag, connTag, semTag)
  uint64_t pullLLCount = 0;  // collective calls that took pullReduce's LL path
  uint64_t a2aLLCount = 0;   // ncclAllToAll / ncclAllToAllv calls that took allToAll's LL path
  // PreMulSum handles: a handle's value is ncclNumOps + its slot; a destroyed slot is taken again by
  // the next create.  With a vendor communicator the handles are the vendor library's and this
  // table stays empty.
  std::vector<PreMulOp> preMulOps;

  // ---- set-up, scratch and teardown (comm.cpp, comm_registration.cpp) ---------------------------
  void buildAlgorithms();
  // Exchange an IPC handle of the allocation holding `ptr` and return every rank's pointer as mapped
  // here (collective).  Mappings come from the process-wide cache (openIpcHandle), so a peer buffer
  // mapped by several owners is opened once; a peer that freed an allocation and got a new one at
  // the same address sends a new handle, which maps afresh.
  PeerBufs exchange(void* ptr);
  // Grow a scratch region collectively (every rank calls with the same size at the same call).
  // The outgrown buffer is kept allocated until the communicator is destroyed: freeing it let the
  // allocator hand its address range to the new buffer, and peers that imported the new buffer's
  // IPC handle then wrote through a mapping of the OLD memory (8 processes, one GPU: after the
  // bulk scratch grew 64 -> 128 MiB, two ranks' peers wrote the pipeline's stages into the old
  // buffer, tools/multi_rank_check.py).  Growth is geometric, so what is kept is at most the final size.
  //
  // Growth synchronizes the device and allocates, so it cannot happen inside a HIP graph capture:
  // a call that would grow while `stream` captures fails with ncclInvalidUsage instead (run the
  // same call once eagerly before capturing, and the scratch is already large enough).
  void ensure(void*& buf, size_t& have, PeerBufs& peers, size_t need, hipStream_t stream = nullptr);
  // Drop every cached mapping of peers' user buffers (collective).  Scratch, token and flag
  // mappings stay.  After this, the next use of any buffer registers it afresh.
  void dropUserRegistrations();
  // Every lease of this communicator, pinned ones and what is still queued included: only after a
  // device synchronize and with no graph left to replay (dropUserRegistrations, destroy).
  void dropLeases();
  void destroy();

  // ---- registration of user buffers (comm_registration.cpp) -------------------------------------
  // Peer pointers of a user buffer (the bulk kernels write results straight into every peer's
  // output, allreduce_fullmesh.cu:110-113; zero-copy reads the peers' inputs).  Cached per local
  // pointer, inside a record per local allocation, like the reference's per-buffer context cache
  // (algorithm.cc:52-60): a repeated call on the same buffer costs no host round trip.  As in the
  // reference, every rank must pass its matching buffer when a buffer is first used; which of a
  // rank's buffers share an allocation is free to differ between ranks (each new pointer brings
  // every rank's own allocation and offset).  Eviction is by local allocation, so beyond
  // kMaxUserRegs allocations the ranks must still group alike to evict alike.
  //  * The allocation is identified by (base, size, HIP buffer id): a buffer freed and re-allocated
  //    at the same address is a new allocation, registered afresh, and its old registration retired.
  //  * At most kMaxUserRegs allocations stay registered; the least recently used one is retired
  //    beyond that (every rank sees the same sequence of buffers, so every rank evicts the same).
  //  * Retired mappings close once the kernels that used them have completed (the events recorded
  //    after those launches, RetireQueue::flush), never under a running kernel and with no synchronize.
  //  * A registration used while its stream is capturing a HIP graph is pinned: the graph keeps
  //    the peer pointers in its kernel arguments, so evicting it (and closing the mappings) would
  //    leave every later replay writing through closed mappings.  Pinned entries are never evicted
  //    (the cap then only bounds the unpinned ones); capture happens in the same calls on every
  //    rank, so every rank pins the same.
  //  * A registration made for the caller (Communicator::registerMemory, mscclppAmdCommRegisterBuffer)
  //    is pinned too: the caller keeps the raw peer pointers (an algorithm plugin's context holds
  //    them for good), so no later eviction may close them.
  //  * Pinned entries are released only by dropUserRegistrations (mscclppAmdCommDeregisterAll), which
  //    must not run while a graph that captured them is still replayed, or when the address is
  //    re-used by a new allocation (the old one was freed, so its pointers were dead already).
  std::array<void*, MSCCLPP_AMD_MAX_RANKS> registerOutput(void* out, hipStream_t stream = nullptr, bool pin = false);
  size_t registrations() const { return userRegs.size() + pairedRegs.size(); }
  // `it` of `regs` is let go: its mappings close once the launches through them have completed.
  void retireReg(RegMap& regs, RegMap::iterator it);
  // The least recently used unpinned registration of `regs` goes when kMaxUserRegs unpinned ones are held.
  void evictFor(RegMap& regs);
  SendIdent sendIdent(const void* send);
  // True when rank q's cached pairing (row q of the gathered idents) is not the current buffers.
  static bool pairingStale(const SendIdent* all, int n, int q);
  // all: every rank's sendIdent of this call; collective exactly when any rank's pairing is stale.
  std::array<void*, MSCCLPP_AMD_MAX_RANKS> registerPaired(void* send, const SendIdent* all, hipStream_t stream);

  // ---- collectives (comm_collectives.cpp) -------------------------------------------------------
  mscclppAmdRankView baseView(const void* in, void* out);
  // The view of a zero-copy pull collective, for a launch that starts here: peerInput[q] is rank q's
  // send buffer, registered through `send` (registerOutput, or registerPaired where the caller
  // gathered every rank's sendIdent).  mappings.recordUses follows the launch.
  mscclppAmdRankView pullView(const void* send, void* recv, hipStream_t stream, const SendIdent* idents = nullptr);
  // The tuned launch shape of `algo` for this message, when the caller left the shape open and the
  // tuned entry names the same algorithm.
  void applyTunedShape(const char* coll, int algo, size_t bytes, int& nblocks, int& nthreads);
  int allReduce(const void* in, void* out, size_t bytes, int dtype, int op, int algo, int nblocks, int nthreads,
                hipStream_t stream);
  int allReduceLaunch(const void* in, void* out, size_t bytes, int dtype, int op, int algo, int nblocks, int nthreads,
                      hipStream_t stream);
  // ReduceScatter (mode 1) / AllGather (mode 2) through the bulk all-pairs kernel; `bytes` is the
  // per-rank block (recvcount / sendcount bytes).
  int bulkCollective(int mode, const void* in, void* out, size_t blockBytes, int dtype, int op, int algo, int nblocks,
                     int nthreads, hipStream_t stream);
  int bulkCollectiveLaunch(int mode, const void* in, void* out, size_t blockBytes, int dtype, int op, int algo,
                           int nblocks, int nthreads, hipStream_t stream);
  // Broadcast: every rank all-gathers an IPC handle (root: its send buffer; others: their receive
  // buffer, only so the call stays collective) and opens only the root's.  Done on every call: the
  // root's buffer is not known to the other ranks in advance, so a per-buffer cache could not stay
  // consistent across ranks.
  int broadcast(const void* send, void* recv, size_t bytes, int root, int nblocks, int nthreads, hipStream_t stream);
  // AllToAll(v) by a zero-copy pull (kernels/alltoall.hip): segs[p] = what this rank receives from
  // rank p, in bytes.  The send buffer is what the peers read, so it is the one registered
  // (collective on first use, cached per allocation, pinned under capture); every store goes to this
  // rank's own receive buffer, which needs no registration.  nblocks: the same on every rank.
  // idents: every rank's sendIdent of this call where the caller gathered them (AllToAllv,
  // registerPaired); null: registerOutput, the other collectives' contract of matching buffers.
  // ll / maxSeg: the same call as the table of kernels/alltoall_ll.hip (ll[q] = what this rank sends to and
  // receives from rank q) and the largest segment of the whole matrix, which every rank knows alike.  A
  // call the rule sends there (alltoallTakesLL) registers nothing and builds no pullView.
  int allToAll(const void* send, void* recv, const mscclppAmdAllToAllSeg* segs, int nblocks, hipStream_t stream,
               const SendIdent* idents = nullptr, const mscclppAmdAllToAllLLSeg* ll = nullptr, uint64_t maxSeg = 0);
  // Reduce to `root` by a zero-copy pull-reduce at the root (kernels/reduce.hip).  The send buffer is
  // what the root reads, so it is the one registered, on every rank (collective on first use, cached
  // per allocation, pinned under capture: the matching-buffer contract of AllToAll); the result is
  // stored by the root into its own receive buffer, which is never registered.  recv is used on the
  // root only.  Every rank derives the same grid from the byte count.
  int reduce(const void* send, void* recv, size_t bytes, int dtype, int op, int root, hipStream_t stream);
  // ncclMax / ncclAvg of Reduce, ReduceScatter and AllReduce, and every operation of int64 / uint64 /
  // int8 (kernels/pull_reduce.hip), the pattern of reduce(): the send buffer is
  // what the peers read, so it is registered on every rank; an AllReduce's peers also read this rank's
  // reduced slice out of its receive buffer, which is registered too (the same registration when in
  // place).  bytes: the message of Reduce / AllReduce, the per-rank block of ReduceScatter.  Every
  // rank derives the same grid from (coll, bytes).
  // op MSCCLPP_AMD_PREMUL_SUM: this rank's scalar is `scale`, or, where scalePtr is
  // non-null, the element of the element type it points to in device memory when the kernel runs.
  int pullReduce(int coll, const void* send, void* recv, size_t bytes, int dtype, int op, int root, hipStream_t stream,
                 float scale = 0.0f, const void* scalePtr = nullptr);
  ncclRedOp_t preMulCreate(const PreMulOp& e);
  // The live entry of `op` (a copy: the caller launches after the lock is dropped, and the handle may
  // be destroyed as soon as the collective call has returned), or false.
  bool preMulFind(ncclRedOp_t op, PreMulOp* out, bool destroy = false);

  // ---- Send / Recv by a zero-copy pull (comm_p2p.cpp; kernels/sendrecv.hip) ------
  // Point-to-point, so nothing here is collective.  A send exports its buffer's allocation and
  // posts {blob, bytes, ok} to the peer through the bootstrap mailbox (never waiting for the peer);
  // a receive takes the oldest such message from that peer (the mailbox is FIFO per source and tag,
  // so the k-th receive matches the k-th send), imports the allocation and pulls.  One kernel per
  // (communicator, stream) then runs the operations of a call, or of a whole group, in call order.
  //
  // Post a send's message; false (with ok = 0 posted) when the buffer cannot be exported.
  // (No communicator state is touched: the bootstrap serialises its own socket.)
  bool p2pPost(const void* send, uint64_t bytes, int peer);
  // Match a receive with the peer's oldest posted send: the sender's buffer as mapped here, or null
  // when the sender refused or announced another byte count (nothing may be launched for it).
  // *mapping: the import it lies in, for p2pLaunch.
  const void* p2pMatch(uint64_t bytes, int peer, void** mapping);
  // One kernel for the operations of this rank on `stream`, in call order (`send` of a receive =
  // what p2pMatch returned; used: the (peer, mapping) pairs its receives read through).
  int p2pLaunch(const mscclppAmdSendRecvOp* ops, int nops, const std::vector<std::pair<int, void*>>& used,
                hipStream_t stream);
};

// ---- vendor NCCL fallback (nccl_compat.cpp) --------------------------------------------------
namespace mscclpp_amd {
namespace host {
struct VendorNccl {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommFinalize)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, void*) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, void*) = nullptr;
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, void*) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, void*) = nullptr;
  ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, void*) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, void*) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, void*) = nullptr;
  ncclResult_t (*AllToAll)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, void*) = nullptr;
  ncclResult_t (*AllToAllv)(const void*, const size_t[], const size_t[], void*, const size_t[], const size_t[],
                            ncclDataType_t, ncclComm_t, void*) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*GroupSimulateEnd)(ncclSimInfo_t*) = nullptr;
  ncclResult_t (*RedOpCreatePreMulSum)(ncclRedOp_t*, void*, ncclDataType_t, ncclScalarResidence_t, ncclComm_t) = nullptr;
  ncclResult_t (*RedOpDestroy)(ncclRedOp_t, ncclComm_t) = nullptr;
};
// The vendor library named by MSCCLPP_AMD_NCCL_LIB_PATH (or MSCCLPP_NCCL_LIB_PATH), or null.
const VendorNccl* vendorNccl();
// MSCCLPP_AMD_FORCE_NCCL_FALLBACK_OPERATION ("all" or a comma list of allreduce, allgather,
// reducescatter, broadcast, alltoall, alltoallv, reduce, sendrecv) names `op`: a whole list entry
// equals it, so "reducescatter" does not name "reduce".
bool forcedFallback(const char* op);
// ncclCommInitRank with the bootstrap's connect / receive timeout given (ncclCommInitRank takes it
// from MSCCLPP_AMD_BOOTSTRAP_TIMEOUT_S); commId is the 128-byte unique id.  Returns an ncclResult_t.
int commInitRank(ncclComm_t* comm, int nranks, const void* commId, int rank, int timeoutSec);
// ncclGroupStart / ncclGroupEnd: a thread-local depth; the native Send / Recv queued meanwhile run at
// the outermost end.  Both forward to the vendor library when one is loaded.  ncclResult_t values.
int groupStart();
int groupEnd();
void initFallbackComm(ncclComm* c);                 // collective over c's bootstrap
void destroyFallbackComm(ncclComm* c, bool abort);

// What a mscclppAmd*Launch entry point's kernel dereferences through a rank view.  kTokens is the
// handshake plumbing (tokens, expected, peerTokens[q]); a kPeer* bit names a per-rank array.
enum ViewField : unsigned {
  kViewInput = 1, kViewOutput = 2, kViewScratch = 4, kViewFlags = 8, kViewPipeSems = 16, kViewErr = 32, kViewTokens = 64,
  kViewPeerInput = 128, kViewPeerOutput = 256, kViewPeerScratch = 512,
  kViewHandshake = kViewErr | kViewTokens,
};
struct ViewNeeds {
  unsigned all = 0;       // of every view; per-rank arrays at every rank q < nranks
  bool rank = true;       // every view's rank lies in [0, nranks)
  int root = -1;          // the view of this rank also needs:
  unsigned atRoot = 0;    //   these, per-rank arrays at every q
  int peer = -1;          // every view also needs the per-rank arrays
  unsigned atPeer = 0;    //   named here, at entry [peer] alone
};
// The checks every launch entry point makes before anything touches a device: views present, nviews
// 1 or nranks, 2 <= nranks <= MSCCLPP_AMD_MAX_RANKS, and every pointer `needs` names non-null.
bool viewsValid(const mscclppAmdRankView* views, int nviews, int nranks, const ViewNeeds& needs);
}  // namespace host
}  // namespace mscclpp_amd

