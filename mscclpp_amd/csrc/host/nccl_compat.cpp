// The rest of the NCCL ABI surface a framework binds (the symbols libtorch_hip.so imports), so that
// libmscclpp_amd.so can stand in for librccl.so under LD_PRELOAD / LD_AUDIT:
//
//  * native here: ncclBroadcast / ncclBcast (zero-copy pull from the root), ncclAllToAll /
//    ncclAllToAllv (zero-copy pull from every peer, kernels/alltoall.hip; the reference leaves both
//    to the vendor library, nccl.cc:794-821), ncclReduce (zero-copy pull-reduce at the root,
//    kernels/reduce.hip, for the data types and operations AllReduce carries -- ncclMax / ncclAvg and
//    every operation of int64 / uint64 / int8 by kernels/pull_reduce.hip; the reference returns
//    ncclInternalError without a vendor library, nccl.cc:521-542), ncclRedOpCreatePreMulSum /
//    ncclRedOpDestroy for fp16 / bf16 / fp32 on a communicator without a vendor one (a handle table
//    per communicator; AllReduce / ReduceScatter / Reduce with a live handle take the same kernel,
//    which exchanges the ranks' scalars itself; with a vendor communicator both calls, and the
//    handles, stay the vendor library's), ncclSend / ncclRecv between two
//    different ranks, alone or inside ncclGroupStart / ncclGroupEnd (zero-copy pull by the receiver,
//    kernels/sendrecv.hip; the reference: nccl.cc:774-792), ncclCommSplit (nccl.cc:405-435),
//    ncclCommInitRankScalable with one id, ncclCommRegister / Deregister and ncclCommWindowRegister /
//    Deregister (the path registers buffers lazily on first use, so these only hand the pointer back);
//  * forwarded to the vendor library when MSCCLPP_AMD_NCCL_LIB_PATH (or the reference's
//    MSCCLPP_NCCL_LIB_PATH) names it -- the reference's dlopen fallback, nccl.cc:72-160, :323-346:
//    ncclSend/Recv to oneself, ncclRedOpCreatePreMulSum/Destroy (of a communicator that has a vendor
//    one; natively otherwise, see above), ncclGroupSimulateEnd, group calls
//    (beside the native group queue), and AllReduce / AllGather / ReduceScatter / Broadcast /
//    AllToAll(v) / Reduce / Send / Recv for data types and operations this path does not carry or
//    that MSCCLPP_AMD_FORCE_NCCL_FALLBACK_OPERATION (reference:
//    MSCCLPP_FORCE_NCCL_FALLBACK_OPERATION, "all" or a comma list; keys alltoall, alltoallv, reduce
//    and sendrecv for the four above) forces there.  Without a vendor library the operations not
//    carried here return ncclInternalError, as the reference does for the same cases.
#include <dlfcn.h>
#include <sys/stat.h>

#include <algorithm>

#include "comm_internal.hpp"

namespace mscclpp_amd {
namespace host {

namespace {

template <typename F>
void bind(void* h, F& f, const char* name) {
  f = reinterpret_cast<F>(dlsym(h, name));
}

VendorNccl* loadVendor() {
  const char* path = std::getenv("MSCCLPP_AMD_NCCL_LIB_PATH");
  if (!path || !*path) path = std::getenv("MSCCLPP_NCCL_LIB_PATH");
  if (!path || !*path) return nullptr;
  struct stat st{};
  if (stat(path, &st) == 0 && S_ISDIR(st.st_mode)) {
    warn(std::string("MSCCLPP_AMD_NCCL_LIB_PATH points to a directory: ") + path);
    return nullptr;
  }
  // RTLD_DEEPBIND: the vendor library's own calls bind to itself, not to the symbols this library
  // interposes (nccl.cc:91)
  void* h = dlopen(path, RTLD_LAZY | RTLD_LOCAL | RTLD_NODELETE | RTLD_DEEPBIND);
  if (!h) {
    warn(std::string("cannot open the vendor NCCL library: ") + dlerror());
    return nullptr;
  }
  auto* v = new VendorNccl();
  bind(h, v->GetUniqueId, "ncclGetUniqueId");
  bind(h, v->CommInitRank, "ncclCommInitRank");
  bind(h, v->CommDestroy, "ncclCommDestroy");
  bind(h, v->CommFinalize, "ncclCommFinalize");
  bind(h, v->CommAbort, "ncclCommAbort");
  bind(h, v->AllReduce, "ncclAllReduce");
  bind(h, v->AllGather, "ncclAllGather");
  bind(h, v->ReduceScatter, "ncclReduceScatter");
  bind(h, v->Broadcast, "ncclBroadcast");
  bind(h, v->Reduce, "ncclReduce");
  bind(h, v->Send, "ncclSend");
  bind(h, v->Recv, "ncclRecv");
  bind(h, v->AllToAll, "ncclAllToAll");
  bind(h, v->AllToAllv, "ncclAllToAllv");
  bind(h, v->GroupStart, "ncclGroupStart");
  bind(h, v->GroupEnd, "ncclGroupEnd");
  bind(h, v->GroupSimulateEnd, "ncclGroupSimulateEnd");
  bind(h, v->RedOpCreatePreMulSum, "ncclRedOpCreatePreMulSum");
  bind(h, v->RedOpDestroy, "ncclRedOpDestroy");
  if (!v->GetUniqueId || !v->CommInitRank || !v->CommDestroy || !v->GroupStart || !v->GroupEnd) {
    warn(std::string("the vendor NCCL library lacks core entry points: ") + path);
    delete v;
    return nullptr;
  }
  return v;
}

}  // namespace

const VendorNccl* vendorNccl() {
  static VendorNccl* v = loadVendor();
  return v;
}

bool forcedFallback(const char* op) {
  const char* e = std::getenv("MSCCLPP_AMD_FORCE_NCCL_FALLBACK_OPERATION");
  if (!e || !*e) e = std::getenv("MSCCLPP_FORCE_NCCL_FALLBACK_OPERATION");
  if (!e || !*e) return false;
  const std::string list(e);
  if (list == "all") return true;
  size_t pos = 0;
  while (pos <= list.size()) {
    const size_t next = std::min(list.find(',', pos), list.size());
    if (list.compare(pos, next - pos, op) == 0 && next - pos == std::strlen(op)) return true;
    pos = next + 1;
  }
  return false;
}

void initFallbackComm(ncclComm* c) {
  const VendorNccl* v = vendorNccl();
  if (!v) return;
  ncclUniqueId id{};
  if (c->rank == 0 && v->GetUniqueId(&id) != ncclSuccess) std::memset(&id, 0, sizeof(id));
  std::vector<ncclUniqueId> ids((size_t)c->nranks);
  c->boot->allGather(&id, ids.data(), sizeof(ncclUniqueId));  // rank 0's id to everyone (nccl.cc:332-337)
  ncclComm_t fb = nullptr;
  const ncclResult_t r = v->CommInitRank(&fb, c->nranks, ids[0], c->rank);
  if (r != ncclSuccess) {
    // e.g. several ranks on one device, which the vendor library refuses: run without fallback
    warn("vendor NCCL communicator unavailable (code " + std::to_string((int)r) +
         "); operations outside this path will return ncclInternalError");
    return;
  }
  c->fallback = fb;
}

void destroyFallbackComm(ncclComm* c, bool abort) {
  const VendorNccl* v = vendorNccl();
  if (!v || !c->fallback) return;
  ncclComm_t fb = (ncclComm_t)c->fallback;
  if (abort && v->CommAbort)
    (void)v->CommAbort(fb);
  else
    (void)v->CommDestroy(fb);
  c->fallback = nullptr;
}

// `v` has every pointer `f` names; its per-rank arrays at ranks [q0, q1).
static bool viewHas(const mscclppAmdRankView& v, unsigned f, int q0, int q1) {
  if ((f & kViewInput && !v.input) || (f & kViewOutput && !v.output) || (f & kViewScratch && !v.scratch) ||
      (f & kViewFlags && !v.flags) || (f & kViewPipeSems && !v.pipeSems) || (f & kViewErr && !v.err) ||
      (f & kViewTokens && (!v.tokens || !v.expected)))
    return false;
  for (int q = q0; q < q1; ++q)
    if ((f & kViewTokens && !v.peerTokens[q]) || (f & kViewPeerInput && !v.peerInput[q]) ||
        (f & kViewPeerOutput && !v.peerOutput[q]) || (f & kViewPeerScratch && !v.peerScratch[q]))
      return false;
  return true;
}

bool viewsValid(const mscclppAmdRankView* views, int nviews, int nranks, const ViewNeeds& needs) {
  if (!views || nranks < 2 || nranks > MSCCLPP_AMD_MAX_RANKS || (nviews != 1 && nviews != nranks)) return false;
  for (int i = 0; i < nviews; ++i) {
    const mscclppAmdRankView& v = views[i];
    if (needs.rank && (v.rank < 0 || v.rank >= nranks)) return false;
    if (!viewHas(v, needs.all, 0, nranks) || !viewHas(v, needs.atPeer, needs.peer, needs.peer + 1)) return false;
    if (v.rank == needs.root && !viewHas(v, needs.atRoot, 0, nranks)) return false;
  }
  return true;
}

}  // namespace host
}  // namespace mscclpp_amd

using mscclpp_amd::host::forcedFallback;
using mscclpp_amd::host::vendorNccl;

// The vendor communicator of `comm`, or null (no vendor library, or it refused this communicator).
static inline ncclComm_t vendorComm(ncclComm_t comm) { return comm ? (ncclComm_t)comm->fallback : nullptr; }

// The reference's answer for an operation it does not carry and cannot forward: ncclInternalError
// with a warning (nccl.cc:521-542, :774-821, :840-844).
static ncclResult_t unavailable(const char* what) {
  warn(std::string(what) + " is not carried by this path and no vendor NCCL library is configured "
                           "(set MSCCLPP_AMD_NCCL_LIB_PATH)");
  return ncclInternalError;
}

// ---- Send / Recv and group calls -----------------------------------------------------------------
// A byte move by the zero-copy pull kernel (kernels/sendrecv.hip, ncclComm::p2pPost / p2pMatch /
// p2pLaunch).  A call outside a group is a group of one.  At the outermost ncclGroupEnd all sends
// are posted first (a post never waits for the peer), then all receives are matched (each waits for
// the peer's post only), then one kernel per (communicator, stream) runs that pair's operations in
// call order.  A transfer that one side refuses (a send buffer that cannot be exported, which the
// receiver learns from the message; a byte count that differs, which only the receiver sees) is
// left out of the table and the call returns ncclInvalidArgument; the rest of the group still runs.
namespace {
struct QueuedP2p {
  ncclComm_t comm;
  void* stream;
  bool send;
  const void* sbuf;  // a send's buffer; a receive's: the sender's buffer as mapped here, once matched
  void* rbuf;
  uint64_t bytes;
  int peer;
  void* mapping = nullptr;
  bool dropped = false;
};
thread_local int gGroupDepth = 0;
thread_local std::vector<QueuedP2p> gGroupQueue;

int flushP2p() {
  std::vector<QueuedP2p> q;
  q.swap(gGroupQueue);
  // more operations than one kernel's table holds: refused before anything is posted (splitting a
  // group over several kernels can deadlock: the peers' tables would not line up)
  for (size_t i = 0; i < q.size(); ++i) {
    size_t same = 0;
    for (const auto& o : q) same += o.comm == q[i].comm && o.stream == q[i].stream;
    if (same > MSCCLPP_AMD_SENDRECV_MAX_OPS) {
      warn("a group holds " + std::to_string(same) + " Send / Recv operations on one communicator and stream; at most " +
           std::to_string(MSCCLPP_AMD_SENDRECV_MAX_OPS) + " are carried");
      return (int)ncclInvalidUsage;
    }
  }
  int result = ncclSuccess;
  for (auto& o : q)
    if (o.send && !o.comm->p2pPost(o.sbuf, o.bytes, o.peer)) {
      o.dropped = true;
      result = ncclInvalidArgument;
    }
  for (auto& o : q)
    if (!o.send) {
      o.sbuf = o.comm->p2pMatch(o.bytes, o.peer, &o.mapping);
      if (!o.sbuf) {
        o.dropped = true;
        result = ncclInvalidArgument;
      }
    }
  std::vector<bool> launched(q.size(), false);
  for (size_t i = 0; i < q.size(); ++i) {
    if (launched[i]) continue;
    std::vector<mscclppAmdSendRecvOp> ops;
    std::vector<std::pair<int, void*>> used;
    for (size_t j = i; j < q.size(); ++j) {
      const QueuedP2p& o = q[j];
      if (o.comm != q[i].comm || o.stream != q[i].stream) continue;
      launched[j] = true;
      if (o.dropped) continue;
      const int me = o.comm->rank;
      ops.push_back({o.send ? me : o.peer, o.send ? o.peer : me, o.sbuf, o.rbuf, o.bytes});
      if (!o.send) used.emplace_back(o.peer, o.mapping);
    }
    if (ops.empty()) continue;
    const int rc = q[i].comm->p2pLaunch(ops.data(), (int)ops.size(), used, (hipStream_t)q[i].stream);
    if (rc != 0 && result == ncclSuccess) result = rc;
  }
  return result;
}

int p2pCall(bool send, const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int peer,
            ncclComm_t comm, void* stream) {
  if (!comm) return (int)ncclInvalidArgument;
  if (count == 0) return (int)ncclSuccess;  // no exchange, no launch (on both sides: the counts match)
  if (peer < 0 || peer >= comm->nranks) return (int)ncclInvalidArgument;
  const size_t tb = ncclTypeBytes(datatype);
  const char* what = send ? "ncclSend" : "ncclRecv";
  // to oneself (every call on a one-rank communicator included) is not carried
  if (peer == comm->rank || forcedFallback("sendrecv")) {
    if (vendorComm(comm) && vendorNccl()->Send && vendorNccl()->Recv)
      return send ? (int)vendorNccl()->Send(sendbuff, count, datatype, peer, vendorComm(comm), stream)
                  : (int)vendorNccl()->Recv(recvbuff, count, datatype, peer, vendorComm(comm), stream);
    if (peer == comm->rank) return (int)unavailable(what);
  }
  if (tb == 0 || (send ? !sendbuff : !recvbuff)) return (int)ncclInvalidArgument;
  if (streamCapturing((hipStream_t)stream)) {
    warn(std::string(what) + " exchanges a message between the hosts on every call, which a captured graph cannot replay");
    return (int)ncclInvalidUsage;
  }
  QueuedP2p o{comm, stream, send, sendbuff, recvbuff, (uint64_t)count * tb, peer};
  gGroupQueue.push_back(o);
  return gGroupDepth > 0 ? (int)ncclSuccess : flushP2p();
}
}  // namespace

namespace mscclpp_amd {
namespace host {
int groupStart() {
  ++gGroupDepth;
  return vendorNccl() ? (int)vendorNccl()->GroupStart() : (int)ncclSuccess;
}

int groupEnd() {
  int result = ncclSuccess;
  if (gGroupDepth > 0 && --gGroupDepth == 0 && !gGroupQueue.empty()) result = guarded([&] { return flushP2p(); });
  const int vr = vendorNccl() ? (int)vendorNccl()->GroupEnd() : (int)ncclSuccess;
  return result != ncclSuccess ? result : vr;
}
}  // namespace host
}  // namespace mscclpp_amd

extern "C" {

ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, void* stream) {
  return (ncclResult_t)guarded([&] {
    if (!comm) return (int)ncclInvalidArgument;
    const size_t bytes = count * ncclTypeBytes(datatype);
    if (comm->nranks == 1) {  // nccl.cc:552-557
      if (sendbuff != recvbuff && bytes)
        HIPCHECK(hipMemcpyAsync(recvbuff, sendbuff, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
      return (int)ncclSuccess;
    }
    if (root < 0 || root >= comm->nranks) return (int)ncclInvalidArgument;
    if ((sendbuff == nullptr && root == comm->rank) || recvbuff == nullptr || bytes == 0)  // nccl.cc:559-564
      return (int)ncclInvalidArgument;
    if (vendorComm(comm) && forcedFallback("broadcast"))
      return (int)vendorNccl()->Broadcast(sendbuff, recvbuff, count, datatype, root, vendorComm(comm), stream);
    return comm->broadcast(sendbuff, recvbuff, bytes, root, 0, 0, (hipStream_t)stream);
  });
}

ncclResult_t ncclBcast(void* buff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm, void* stream) {
  return ncclBroadcast(buff, buff, count, datatype, root, comm, stream);  // nccl.cc:544-547
}

ncclResult_t ncclCommSplit(ncclComm_t comm, int color, int key, ncclComm_t* newcomm, ncclConfig_t* config) {
  return (ncclResult_t)guarded([&] {
    if (!comm || !newcomm) return (int)ncclInvalidArgument;
    *newcomm = NCCL_COMM_NULL;
    struct Info {
      int color, key, rank;
    };
    std::vector<Info> infos((size_t)comm->nranks);
    Info mine{color, key, comm->rank};
    comm->boot->allGather(&mine, infos.data(), sizeof(Info));
    std::vector<Info> group;
    for (const Info& i : infos)
      if (i.color == color) group.push_back(i);
    std::stable_sort(group.begin(), group.end(), [](const Info& a, const Info& b) {
      return a.key != b.key ? a.key < b.key : a.rank < b.rank;
    });
    int newRank = 0;
    for (size_t i = 0; i < group.size(); ++i)
      if (group[i].rank == comm->rank) newRank = (int)i;
    // the new group's rank 0 creates the id; every rank learns every group's id (nccl.cc:422-430)
    ncclUniqueId id{};
    if (color != NCCL_SPLIT_NOCOLOR && newRank == 0) {
      const ncclResult_t r = ncclGetUniqueId(&id);
      if (r != ncclSuccess) return (int)r;
    }
    std::vector<ncclUniqueId> ids((size_t)comm->nranks);
    comm->boot->allGather(&id, ids.data(), sizeof(ncclUniqueId));
    if (color == NCCL_SPLIT_NOCOLOR) return (int)ncclSuccess;
    return (int)ncclCommInitRankConfig(newcomm, (int)group.size(), ids[(size_t)group.front().rank], newRank, config);
  });
}

ncclResult_t ncclCommInitRankScalable(ncclComm_t* newcomm, int nranks, int myrank, int nId, ncclUniqueId* commIds,
                                      ncclConfig_t* config) {
  if (!newcomm || !commIds || nId < 1) return ncclInvalidArgument;
  if (nId != 1) {
    warn("ncclCommInitRankScalable: one MI355X node needs a single unique id");
    return ncclInvalidUsage;
  }
  return ncclCommInitRankConfig(newcomm, nranks, commIds[0], myrank, config);
}

ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op,
                        int root, ncclComm_t comm, void* stream) {
  return (ncclResult_t)guarded([&] {
    if (!comm) return (int)ncclInvalidArgument;
    if (comm->nranks == 1) {
      const size_t bytes = count * ncclTypeBytes(datatype);
      if (sendbuff != recvbuff && bytes)
        HIPCHECK(hipMemcpyAsync(recvbuff, sendbuff, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
      return (int)ncclSuccess;
    }
    const bool isRoot = root == comm->rank;
    if (root < 0 || root >= comm->nranks) return (int)ncclInvalidArgument;
    if (!sendbuff || count == 0 || (isRoot && !recvbuff)) return (int)ncclInvalidArgument;
    const size_t bytes = count * ncclTypeBytes(datatype);
    // in place on the root is send == recv; any other overlap would have the root store into
    // bytes of its send buffer that another lane still reads
    if (isRoot && bytes && sendbuff != recvbuff && bufferRangesOverlap(sendbuff, bytes, recvbuff, bytes)) {
      warn("ncclReduce: the root's send and receive ranges overlap without being identical");
      return (int)ncclInvalidArgument;
    }
    const int dt = dtypeFromNccl(datatype), o = opFromNccl(op), po = pullOpFromNccl(op);
    const int pdt = pullOnlyDtypeFromNccl(datatype), pdo = pdt >= 0 ? pullOnlyOpFromNccl(op) : -1;  // as ncclAllReduce
    ncclComm::PreMulOp pm;
    const bool premul = comm->preMulFind(op, &pm);  // as ncclAllReduce
    const bool carried = premul || (pdt >= 0 ? pdo >= 0 : dt >= 0 && (o >= 0 || po >= 0));
    if (vendorComm(comm) && vendorNccl()->Reduce && (!carried || forcedFallback("reduce")))
      return (int)vendorNccl()->Reduce(sendbuff, recvbuff, count, datatype, op, root, vendorComm(comm), stream);
    if (premul) {
      if (pm.datatype != datatype) {
        warn("ncclReduce: the PreMulSum handle was created for another data type");
        return (int)ncclInvalidArgument;
      }
      return comm->pullReduce(MSCCLPP_AMD_PULL_REDUCE, sendbuff, isRoot ? recvbuff : nullptr, bytes, dt,
                              MSCCLPP_AMD_PREMUL_SUM, root, (hipStream_t)stream, pm.scalar, pm.device);
    }
    if (pdt >= 0 && pdo >= 0)  // int64 / uint64 / int8, any of the four ops: the pull-reduce kernel
      return comm->pullReduce(MSCCLPP_AMD_PULL_REDUCE, sendbuff, isRoot ? recvbuff : nullptr, bytes, pdt, pdo, root,
                              (hipStream_t)stream);
    if (dt >= 0 && po >= 0)  // ncclMax / ncclAvg: the pull-reduce kernel, rank order (kernels/pull_reduce.hip)
      return comm->pullReduce(MSCCLPP_AMD_PULL_REDUCE, sendbuff, isRoot ? recvbuff : nullptr, bytes, dt, po, root,
                              (hipStream_t)stream);
    if (dt < 0 || o < 0) return (int)unavailable("ncclReduce of this data type or operation");
    // a non-root rank's recvbuff is ignored (and may be null)
    return comm->reduce(sendbuff, isRoot ? recvbuff : nullptr, bytes, dt, o, root, (hipStream_t)stream);
  });
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      void* stream) {
  return (ncclResult_t)guarded([&] { return p2pCall(true, sendbuff, nullptr, count, datatype, peer, comm, stream); });
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, void* stream) {
  return (ncclResult_t)guarded([&] { return p2pCall(false, nullptr, recvbuff, count, datatype, peer, comm, stream); });
}

ncclResult_t ncclAllToAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclComm_t comm,
                          void* stream) {
  return (ncclResult_t)guarded([&] {
    if (!comm) return (int)ncclInvalidArgument;
    if (comm->nranks == 1) {  // nccl.cc:796-802
      const size_t bytes = count * ncclTypeBytes(datatype);
      if (sendbuff != recvbuff && bytes)
        HIPCHECK(hipMemcpyAsync(recvbuff, sendbuff, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
      return (int)ncclSuccess;
    }
    // a byte move: any data type with a size is carried.  In place is not defined for AllToAll,
    // and a pull would race with the peers' reads
    const size_t n = (size_t)comm->nranks, bytes = count * ncclTypeBytes(datatype);
    if (!sendbuff || !recvbuff || bytes == 0) return (int)ncclInvalidArgument;
    if (bufferRangesOverlap(sendbuff, n * bytes, recvbuff, n * bytes)) {
      warn("ncclAllToAll: the send and receive buffers overlap");
      return (int)ncclInvalidArgument;
    }
    if (vendorComm(comm) && vendorNccl()->AllToAll && forcedFallback("alltoall"))
      return (int)vendorNccl()->AllToAll(sendbuff, recvbuff, count, datatype, vendorComm(comm), stream);
    mscclppAmdAllToAllSeg segs[MSCCLPP_AMD_MAX_RANKS];
    mscclppAmdAllToAllLLSeg ll[MSCCLPP_AMD_MAX_RANKS];
    for (size_t p = 0; p < n; ++p) {
      segs[p] = {(uint64_t)comm->rank * bytes, p * bytes, bytes};
      ll[p] = {p * bytes, bytes, p * bytes, bytes};
    }
    return comm->allToAll(sendbuff, recvbuff, segs, mscclpp_amd::alltoallDefaultBlocks(n * bytes),
                          (hipStream_t)stream, nullptr, ll, bytes);
  });
}

ncclResult_t ncclAllToAllv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[], void* recvbuff,
                           const size_t recvcounts[], const size_t rdispls[], ncclDataType_t datatype, ncclComm_t comm,
                           void* stream) {
  if (!comm) return ncclInvalidArgument;
  return (ncclResult_t)guarded([&] {
    const size_t tb = ncclTypeBytes(datatype);
    if (comm->nranks == 1) {  // nccl.cc:812-818: block 0 to block 0
      if (!recvcounts || !sdispls || !rdispls) return (int)ncclInvalidArgument;
      const size_t bytes = recvcounts[0] * tb;
      if (bytes)
        HIPCHECK(hipMemcpyAsync((char*)recvbuff + rdispls[0] * tb, (const char*)sendbuff + sdispls[0] * tb, bytes,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream));
      return (int)ncclSuccess;
    }
    if (vendorComm(comm) && vendorNccl()->AllToAllv && forcedFallback("alltoallv"))
      return (int)vendorNccl()->AllToAllv(sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls, datatype,
                                          vendorComm(comm), stream);
    // A pull reads peer p's segment at p's sdispls[rank], which lives on p's host: every rank
    // all-gathers its counts and send displacements (elements) on each call, as broadcast() gathers
    // its handles.  Every rank then checks the WHOLE matrix and its peers' own argument checks, so
    // all ranks return the same answer and none launches a kernel that would wait for one that
    // refused.
    const int n = comm->nranks, me = comm->rank;
    // The row also carries the identity of this rank's send buffer and of the buffers its cached
    // registration was made with (ncclComm::sendIdent): AllToAllv's buffers differ in size between
    // ranks, so which buffer goes with which is settled per call, by every rank from the same rows.
    struct Row {
      uint64_t ok;
      ncclComm::SendIdent ident;
      uint64_t send[MSCCLPP_AMD_MAX_RANKS], sdis[MSCCLPP_AMD_MAX_RANKS], recv[MSCCLPP_AMD_MAX_RANKS];
    };
    Row mine{};
    mine.ok = sendbuff && recvbuff && sendcounts && sdispls && recvcounts && rdispls && tb;
    if (mine.ok) {
      try {
        std::lock_guard<std::mutex> lk(comm->mu);
        mine.ident = comm->sendIdent(sendbuff);
      } catch (const std::exception& e) {  // not device memory: still take part in the gather below
        warn(std::string("ncclAllToAllv: ") + e.what());
        (void)hipGetLastError();
        mine.ok = 0;
      }
    }
    if (mine.ok) {
      uint64_t sLo = ~0ull, sHi = 0, rLo = ~0ull, rHi = 0;
      for (int p = 0; p < n; ++p) {
        mine.send[p] = sendcounts[p];
        mine.sdis[p] = sdispls[p];
        mine.recv[p] = recvcounts[p];
        if (sendcounts[p]) {
          sLo = std::min<uint64_t>(sLo, sdispls[p] * tb);
          sHi = std::max<uint64_t>(sHi, (sdispls[p] + sendcounts[p]) * tb);
        }
        if (recvcounts[p]) {
          rLo = std::min<uint64_t>(rLo, rdispls[p] * tb);
          rHi = std::max<uint64_t>(rHi, (rdispls[p] + recvcounts[p]) * tb);
        }
      }
      if (sLo < sHi && rLo < rHi &&
          bufferRangesOverlap((const char*)sendbuff + sLo, sHi - sLo, (const char*)recvbuff + rLo, rHi - rLo)) {
        warn("ncclAllToAllv: the send and receive ranges overlap");
        mine.ok = 0;
      }
    }
    std::vector<Row> all((size_t)n);
    {
      std::lock_guard<std::mutex> lk(comm->mu);
      comm->boot->allGather(&mine, all.data(), sizeof(Row));
    }
    uint64_t mostRecv = 0, maxSeg = 0;  // maxSeg: the largest segment of the matrix, for the LL path
    for (int r = 0; r < n; ++r) {
      if (!all[(size_t)r].ok) {
        warn("ncclAllToAllv: rank " + std::to_string(r) + " passed invalid arguments");
        return (int)ncclInvalidArgument;
      }
      uint64_t sum = 0;
      for (int p = 0; p < n; ++p) {
        if (all[(size_t)r].recv[p] != all[(size_t)p].send[r]) {
          warn("ncclAllToAllv: rank " + std::to_string(r) + " expects " + std::to_string(all[(size_t)r].recv[p]) +
               " elements from rank " + std::to_string(p) + ", which sends " + std::to_string(all[(size_t)p].send[r]));
          return (int)ncclInvalidArgument;
        }
        sum += all[(size_t)r].recv[p] * tb;
        maxSeg = std::max<uint64_t>(maxSeg, all[(size_t)r].recv[p] * tb);
      }
      mostRecv = std::max(mostRecv, sum);
    }
    mscclppAmdAllToAllSeg segs[MSCCLPP_AMD_MAX_RANKS];
    mscclppAmdAllToAllLLSeg ll[MSCCLPP_AMD_MAX_RANKS];
    for (int p = 0; p < n; ++p) {
      segs[p] = {all[(size_t)p].sdis[me] * tb, (uint64_t)rdispls[p] * tb, (uint64_t)recvcounts[p] * tb};
      ll[p] = {(uint64_t)sdispls[p] * tb, (uint64_t)sendcounts[p] * tb, (uint64_t)rdispls[p] * tb,
               (uint64_t)recvcounts[p] * tb};
    }
    ncclComm::SendIdent idents[MSCCLPP_AMD_MAX_RANKS];
    for (int r = 0; r < n; ++r) idents[r] = all[(size_t)r].ident;
    return comm->allToAll(sendbuff, recvbuff, segs, mscclpp_amd::alltoallDefaultBlocks(mostRecv), (hipStream_t)stream,
                          idents, ll, maxSeg);
  });
}

ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                      ncclScalarResidence_t residence, ncclComm_t comm) {
  if (vendorComm(comm) && vendorNccl()->RedOpCreatePreMulSum)
    return vendorNccl()->RedOpCreatePreMulSum(op, scalar, datatype, residence, vendorComm(comm));
  // native (kernels/pull_reduce.hip): a handle of this communicator's own table
  return (ncclResult_t)guarded([&] {
    if (!op || !scalar || !comm) return (int)ncclInvalidArgument;
    if (residence != ncclScalarDevice && residence != ncclScalarHostImmediate) return (int)ncclInvalidArgument;
    if (datatype != ncclFloat16 && datatype != ncclBfloat16 && datatype != ncclFloat32)
      return (int)unavailable("ncclRedOpCreatePreMulSum of this data type");
    if (comm->nranks == 1)  // x * s alone, which no kernel here computes
      return (int)unavailable("ncclRedOpCreatePreMulSum on a one-rank communicator");
    ncclComm::PreMulOp e;
    e.datatype = datatype;
    if (residence == ncclScalarDevice) {
      e.device = scalar;
    } else if (datatype == ncclFloat32) {
      std::memcpy(&e.scalar, scalar, sizeof(float));
    } else {  // the element's bits, decoded exactly
      uint16_t h = 0;
      std::memcpy(&h, scalar, sizeof(h));
      e.scalar = datatype == ncclBfloat16 ? bf16BitsToFloat(h) : f16BitsToFloat(h);
    }
    *op = comm->preMulCreate(e);
    return (int)ncclSuccess;
  });
}

ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm) {
  if (vendorComm(comm) && vendorNccl()->RedOpDestroy) return vendorNccl()->RedOpDestroy(op, vendorComm(comm));
  // (the launches that used the handle carry its scalar, or its pointer, in their arguments)
  return (ncclResult_t)guarded([&] {
    if (!comm || !comm->preMulFind(op, nullptr, /*destroy=*/true)) return (int)ncclInvalidArgument;
    return (int)ncclSuccess;
  });
}

ncclResult_t ncclGroupSimulateEnd(ncclSimInfo_t* simInfo) {
  if (vendorNccl() && vendorNccl()->GroupSimulateEnd) return vendorNccl()->GroupSimulateEnd(simInfo);
  return unavailable("ncclGroupSimulateEnd");
}

ncclResult_t ncclCommRegister(const ncclComm_t comm, void* buff, size_t size, void** handle) {
  if (!comm || !buff || !size || !handle) return ncclInvalidArgument;
  *handle = buff;  // buffers are registered (IPC-mapped) lazily by the algorithm that first uses them
  return ncclSuccess;
}

ncclResult_t ncclCommDeregister(const ncclComm_t comm, void* handle) {
  if (!comm || !handle) return ncclInvalidArgument;
  return ncclSuccess;
}

ncclResult_t ncclCommWindowRegister(ncclComm_t comm, void* buff, size_t size, ncclWindow_t* win, int) {
  if (!comm || !buff || !size || !win) return ncclInvalidArgument;
  *win = reinterpret_cast<ncclWindow_t>(buff);  // mapped lazily by the algorithm that first uses it
  return ncclSuccess;
}

ncclResult_t ncclCommWindowDeregister(ncclComm_t comm, ncclWindow_t win) {
  if (!comm || !win) return ncclInvalidArgument;
  return ncclSuccess;
}

int mscclppAmdCommVendorComm(ncclComm_t comm, void** vendorComm) {
  if (!comm || !vendorComm) return ncclInvalidArgument;
  *vendorComm = comm->fallback;
  return ncclSuccess;
}

int mscclppAmdCommRegisterBuffer(ncclComm_t comm, void* ptr, void** peers) {
  return guarded([&] {
    if (!comm || !ptr || !peers) return (int)ncclInvalidArgument;
    auto v = comm->cxx->registerMemory(ptr);
    for (int r = 0; r < MSCCLPP_AMD_MAX_RANKS; ++r) peers[r] = r < (int)v.size() ? v[(size_t)r] : nullptr;
    return (int)ncclSuccess;
  });
}

int mscclppAmdCommDeregisterAll(ncclComm_t comm) {
  return guarded([&] {
    if (!comm) return (int)ncclInvalidArgument;
    std::lock_guard<std::mutex> lk(comm->mu);
    comm->dropUserRegistrations();
    return (int)ncclSuccess;
  });
}

// Broadcast for in-process ranks (parity tests): views as for mscclppAmdAllReduceLaunch; input =
// the rank's send buffer (read on the root only), output = its receive buffer, peerInput[root] =
// the root's send buffer.
int mscclppAmdBroadcastLaunch(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int root,
                              int nblocks, int nthreads, uint64_t budgetTicks, void* stream) {
  return guarded([&] {
    if (bytes == 0 || root < 0 || root >= nranks) return (int)ncclInvalidArgument;
    ViewNeeds needs;
    needs.all = kViewOutput | kViewHandshake;
    needs.rank = false;  // (a view's rank is only compared with the root)
    needs.root = needs.peer = root;
    needs.atRoot = kViewInput;
    needs.atPeer = kViewPeerInput;
    if (!viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    return mscclpp_amd::launchBroadcast(views, nviews, nranks, bytes, root, nblocks, nthreads,
                                        budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream);
  });
}

// AllToAll(v) for in-process ranks: views as above, peerInput[q] = rank q's send buffer.
int mscclppAmdAllToAllLaunch(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdAllToAllSeg* segs,
                             int nblocks, int nthreads, uint64_t budgetTicks, void* stream) {
  return guarded([&] {
    ViewNeeds needs;
    needs.all = kViewInput | kViewOutput | kViewHandshake | kViewPeerInput;
    if (!segs || !viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    return mscclpp_amd::launchAllToAll(views, nviews, nranks, segs, nblocks, nthreads,
                                       budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream);
  });
}

// Reduce for in-process ranks: views as above, peerInput[q] = rank q's send buffer (read by the root
// only), output = the receive buffer (used on the root only).  Everything is checked before a
// device is touched; a refusal launches nothing.
int mscclppAmdReduceLaunch(const mscclppAmdRankView* views, int nviews, int nranks, size_t bytes, int dtype, int op,
                           int root, int nblocks, int nthreads, uint64_t budgetTicks, void* stream) {
  return guarded([&] {
    if (root < 0 || root >= nranks) return (int)ncclInvalidArgument;
    if (dtype < 0 || dtype >= MSCCLPP_AMD_NUM_DTYPES || (op != MSCCLPP_AMD_SUM && op != MSCCLPP_AMD_MIN))
      return (int)ncclInvalidArgument;
    if (bytes == 0) return (int)ncclInvalidArgument;  // (a byte count that splits an element: launchReduce)
    ViewNeeds needs;
    needs.all = kViewInput | kViewHandshake;
    needs.root = root;  // the only view that reads and writes user memory
    needs.atRoot = kViewOutput | kViewPeerInput;
    if (!viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    return mscclpp_amd::launchReduce(views, nviews, nranks, bytes, dtype, op, root, nblocks, nthreads,
                                     budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream);
  });
}

// Send / Recv for in-process ranks (and the one-view form ncclSend / ncclRecv launch): everything is
// checked before a device is touched; a refusal launches nothing.
int mscclppAmdSendRecvLaunch(const mscclppAmdRankView* views, int nviews, int nranks, const mscclppAmdSendRecvOp* ops,
                             int nops, int nblocks, int nthreads, uint64_t budgetTicks, void* stream) {
  return guarded([&] {
    ViewNeeds needs;
    needs.all = kViewHandshake;
    if (!ops || !viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    if (nops < 1 || nops > MSCCLPP_AMD_SENDRECV_MAX_OPS) return (int)ncclInvalidArgument;
    for (int i = 0; i < nops; ++i) {
      const mscclppAmdSendRecvOp& o = ops[i];
      if (o.src < 0 || o.src >= nranks || o.dst < 0 || o.dst >= nranks || o.src == o.dst || o.bytes == 0)
        return (int)ncclInvalidArgument;
      // the receiving view dereferences both pointers, a sending view neither
      bool received = false;
      for (int k = 0; k < nviews; ++k) received = received || views[k].rank == o.dst;
      if (received && (!o.send || !o.recv)) return (int)ncclInvalidArgument;
    }
    return mscclpp_amd::launchSendRecv(views, nviews, nranks, ops, nops, nblocks, nthreads,
                                       budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream);
  });
}

int mscclppAmdSendRecvDefaultBlocks(uint64_t bytes) { return mscclpp_amd::sendrecvDefaultBlocks(bytes); }

// ncclMax / ncclAvg of Reduce / ReduceScatter / AllReduce, and the four operations of int64 / uint64 /
// int8, for in-process ranks (and the one-view form the NCCL entry points launch): everything is
// checked before a device is touched; a refusal launches nothing.
// `scaled`: mscclppAmdPullReduceLaunchScaled, which takes PreMulSum (with its scalars) and nothing else.
static int pullReduceLaunch(bool scaled, const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes,
                            int dtype, int op, int root, int nblocks, int nthreads, uint64_t budgetTicks, void* stream,
                            const float* scales, const void* const* scalePtrs) {
  return guarded([&] {
    if (coll < MSCCLPP_AMD_PULL_REDUCE || coll > MSCCLPP_AMD_PULL_ALLREDUCE) return (int)ncclInvalidArgument;
    const bool reduce = coll == MSCCLPP_AMD_PULL_REDUCE, all = coll == MSCCLPP_AMD_PULL_ALLREDUCE;
    if (reduce && (root < 0 || root >= nranks)) return (int)ncclInvalidArgument;
    // SUM / MIN of the eight types that have their own kernels for them are refused; of int64 / uint64 /
    // int8, which have no other kernel, they are taken
    const bool pullOnly = dtype == MSCCLPP_AMD_I64 || dtype == MSCCLPP_AMD_U64 || dtype == MSCCLPP_AMD_I8;
    if (scaled) {
      const bool floats = dtype == MSCCLPP_AMD_F16 || dtype == MSCCLPP_AMD_BF16 || dtype == MSCCLPP_AMD_F32;
      if (op != MSCCLPP_AMD_PREMUL_SUM || !floats || !scales) return (int)ncclInvalidArgument;
    } else if (op != MSCCLPP_AMD_MAX && op != MSCCLPP_AMD_AVG &&
               !(pullOnly && (op == MSCCLPP_AMD_SUM || op == MSCCLPP_AMD_MIN)))
      return (int)ncclInvalidArgument;
    if (bytes == 0) return (int)ncclInvalidArgument;  // (the dtype codes and a split element: launchPullReduce)
    // what moves data: every view, but for Reduce the root's alone (the others read and write no user memory)
    const unsigned moves = kViewOutput | kViewPeerInput | (all ? kViewPeerOutput : 0u);
    ViewNeeds needs;
    needs.all = kViewInput | kViewHandshake | (reduce ? 0u : moves);
    if (reduce) needs.root = root, needs.atRoot = moves;
    if (!viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    unsigned seen = 0;
    for (int i = 0; i < nviews; ++i) {  // no rank twice
      if ((seen >> views[i].rank) & 1u) return (int)ncclInvalidArgument;
      seen |= 1u << views[i].rank;
    }
    return mscclpp_amd::launchPullReduce(views, nviews, nranks, coll, bytes, dtype, op, root, nblocks, nthreads,
                                         budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream,
                                         scaled ? scales : nullptr, scaled ? scalePtrs : nullptr);
  });
}

int mscclppAmdPullReduceLaunch(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes, int dtype,
                               int op, int root, int nblocks, int nthreads, uint64_t budgetTicks, void* stream) {
  return pullReduceLaunch(false, views, nviews, nranks, coll, bytes, dtype, op, root, nblocks, nthreads, budgetTicks,
                          stream, nullptr, nullptr);
}

// PreMulSum for in-process ranks (and the one-view form): scales[i] / scalePtrs[i] belong to views[i].
int mscclppAmdPullReduceLaunchScaled(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes,
                                     int dtype, int op, int root, int nblocks, int nthreads, uint64_t budgetTicks,
                                     void* stream, const float* scales, const void* const* scalePtrs) {
  return pullReduceLaunch(true, views, nviews, nranks, coll, bytes, dtype, op, root, nblocks, nthreads, budgetTicks,
                          stream, scales, scalePtrs);
}

int mscclppAmdPullReduceDefaultBlocks(int coll, uint64_t bytes) { return mscclpp_amd::pullReduceDefaultBlocks(coll, bytes); }

// The same reductions of a small AllReduce / ReduceScatter by one hop of LL8 packets, for in-process
// ranks (and the one-view form the NCCL entry points launch): everything is checked before a device is
// touched; a refusal launches nothing.  (The collective, the (dtype, op) pairs, the byte count and the
// scalars: launchPullReduceLL, which answers 4 before it looks at a view.)
int mscclppAmdPullReduceLLLaunch(const mscclppAmdRankView* views, int nviews, int nranks, int coll, size_t bytes,
                                 int dtype, int op, int nblocks, int nthreads, uint64_t budgetTicks, void* stream,
                                 const float* scales, const void* const* scalePtrs) {
  return guarded([&] {
    if (coll != MSCCLPP_AMD_PULL_REDUCE_SCATTER && coll != MSCCLPP_AMD_PULL_ALLREDUCE) return (int)ncclInvalidArgument;
    ViewNeeds needs;
    needs.all = kViewInput | kViewOutput | kViewScratch | kViewFlags | kViewErr | kViewPeerScratch;
    if (!viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    unsigned seen = 0;
    for (int i = 0; i < nviews; ++i) {
      const mscclppAmdRankView& v = views[i];
      if ((seen >> v.rank) & 1u) return (int)ncclInvalidArgument;  // no rank twice
      seen |= 1u << v.rank;
      if ((uintptr_t)v.flags % 16) return (int)ncclInvalidArgument;  // 16-byte flag refresh
    }
    return mscclpp_amd::launchPullReduceLL(views, nviews, nranks, coll, bytes, dtype, op, nblocks, nthreads,
                                           budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream, scales,
                                           scalePtrs);
  });
}

size_t mscclppAmdPullReduceLLScratchRequired(int coll, int nranks, size_t bytes, int dtype, int op) {
  return mscclpp_amd::pullReduceLLScratchRequired(coll, nranks, bytes, dtype, op);
}

int mscclppAmdPullReduceTakesLL(int coll, int nranks, size_t bytes) {
  return mscclpp_amd::pullReduceTakesLL(coll, nranks, bytes) ? 1 : 0;
}

// Small AllToAll(v) by one hop of LL8 packets, for in-process ranks (and the one-view form the NCCL entry
// points launch): everything is checked before a device is touched; a refusal launches nothing.  (The
// table, the rank count and the lengths between views: launchAllToAllLL.)
int mscclppAmdAllToAllLLLaunch(const mscclppAmdRankView* views, int nviews, int nranks,
                               const mscclppAmdAllToAllLLSeg* table, int nblocks, int nthreads, uint64_t budgetTicks,
                               void* stream) {
  return guarded([&] {
    ViewNeeds needs;
    needs.all = kViewInput | kViewOutput | kViewScratch | kViewFlags | kViewErr | kViewPeerScratch;
    if (!table || !viewsValid(views, nviews, nranks, needs)) return (int)ncclInvalidArgument;
    unsigned seen = 0;
    for (int i = 0; i < nviews; ++i) {
      const mscclppAmdRankView& v = views[i];
      if ((seen >> v.rank) & 1u) return (int)ncclInvalidArgument;  // no rank twice
      seen |= 1u << v.rank;
      if ((uintptr_t)v.flags % 16) return (int)ncclInvalidArgument;  // 16-byte flag refresh
    }
    return mscclpp_amd::launchAllToAllLL(views, nviews, nranks, table, ~0ull, nblocks, nthreads,
                                         budgetTicks ? budgetTicks : spinBudgetTicks(), (hipStream_t)stream);
  });
}

size_t mscclppAmdAllToAllLLScratchRequired(int nranks, size_t maxSegBytes) {
  return mscclpp_amd::alltoallLLScratchRequired(nranks, maxSegBytes);
}

int mscclppAmdAllToAllTakesLL(int nranks, size_t maxSegBytes) {
  return mscclpp_amd::alltoallTakesLL(nranks, maxSegBytes) ? 1 : 0;
}

int mscclppAmdCommAllToAllLLCount(ncclComm_t comm, uint64_t* count) {
  if (!comm || !count) return ncclInvalidArgument;
  std::lock_guard<std::mutex> lk(comm->mu);
  *count = comm->a2aLLCount;
  return ncclSuccess;
}

int mscclppAmdCommPullLLCount(ncclComm_t comm, uint64_t* count) {
  if (!comm || !count) return ncclInvalidArgument;
  std::lock_guard<std::mutex> lk(comm->mu);
  *count = comm->pullLLCount;
  return ncclSuccess;
}

}  // extern "C"
