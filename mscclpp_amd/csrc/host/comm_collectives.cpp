// ncclComm: the collectives' host side -- rank views, scratch, registration and the kernel launch.
#include "comm_internal.hpp"

mscclppAmdRankView ncclComm::baseView(const void* in, void* out) {
  mscclppAmdRankView v{};
  v.input = in;
  v.output = out;
  v.tokens = tokens;
  v.expected = expected;
  v.flags = flags;
  v.err = err;
  v.rank = rank;
  for (int r = 0; r < nranks; ++r) v.peerTokens[r] = peerTokens[r];
  return v;
}

mscclppAmdRankView ncclComm::pullView(const void* send, void* recv, hipStream_t stream, const SendIdent* idents) {
  mappings.beginLaunch();
  mscclppAmdRankView v = baseView(send, recv);
  const auto ins = idents ? registerPaired(const_cast<void*>(send), idents, stream)
                          : registerOutput(const_cast<void*>(send), stream);
  for (int r = 0; r < nranks; ++r) v.peerInput[r] = ins[r];
  return v;
}

void ncclComm::applyTunedShape(const char* coll, int algo, size_t bytes, int& nblocks, int& nthreads) {
  if (nblocks > 0 || nthreads > 0) return;
  std::string name;
  int nb = 0, nt = 0;
  if (tunedConfig(coll, nranks, bytes, name, nb, nt) && algoCodeOf(name) == algo) {
    nblocks = nb;
    nthreads = nt;
  }
}

int ncclComm::allReduce(const void* in, void* out, size_t bytes, int dtype, int op, int algo, int nblocks, int nthreads,
                        hipStream_t stream) {
  std::lock_guard<std::mutex> lk(mu);
  mappings.beginLaunch();
  const int rc = allReduceLaunch(in, out, bytes, dtype, op, algo, nblocks, nthreads, stream);
  mappings.recordUses(stream, device);
  return rc;
}

int ncclComm::allReduceLaunch(const void* in, void* out, size_t bytes, int dtype, int op, int algo, int nblocks,
                              int nthreads, hipStream_t stream) {
  if (algo == MSCCLPP_AMD_ALGO_AUTO) algo = envAlgo();
  if (algo == MSCCLPP_AMD_ALGO_AUTO) {
    algo = mscclppAmdSelectAlgo(nranks, bytes, dtype);
    applyTunedShape("allreduce", algo, bytes, nblocks, nthreads);
  }
  // the pipelined RS+AG carries 2- and 4-byte types only; others take fullmesh, which carries all
  if (algo == MSCCLPP_AMD_ALGO_RSAG_PIPELINE && dtype != MSCCLPP_AMD_F16 && dtype != MSCCLPP_AMD_BF16 &&
      dtype != MSCCLPP_AMD_F32 && dtype != MSCCLPP_AMD_I32 && dtype != MSCCLPP_AMD_U32)
    algo = MSCCLPP_AMD_ALGO_FULLMESH;
  mscclppAmdRankView v = baseView(in, out);
  if (algo == MSCCLPP_AMD_ALGO_PACKET || algo == MSCCLPP_AMD_ALGO_ALLPAIR || algo == MSCCLPP_AMD_ALGO_TEST_K6 ||
      algo == MSCCLPP_AMD_ALGO_TEST_K7 || algo == MSCCLPP_AMD_ALGO_TEST_K2) {
    const size_t need = algo == MSCCLPP_AMD_ALGO_PACKET    ? ll16ScratchRequired(nranks, bytes, dtype)
                        : algo == MSCCLPP_AMD_ALGO_ALLPAIR ? ll8ScratchRequired(nranks, bytes, dtype)
                        : algo == MSCCLPP_AMD_ALGO_TEST_K2 ? testK2ScratchRequired(nranks, bytes)
                                                           : testLLScratchRequired(nranks, bytes);
    if (need == 0) return ncclInvalidUsage;
    ensure(llScratch, llBytes, peerLL, need, stream);
    v.scratch = llScratch;
    v.scratchBytes = llBytes;
    for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerLL[r];
    return launchAllReduceLL(algo, &v, 1, nranks, bytes, dtype, op, nblocks, nthreads, spinBudgetTicks(), stream);
  }
  if (algo == MSCCLPP_AMD_ALGO_FULLMESH || algo == MSCCLPP_AMD_ALGO_RSAG) {
    // the scratch allocated at init bounds a pass; larger buckets take several passes
    size_t need = bytes + 16 * (size_t)nranks * 64;
    const size_t cap = bulkBytes;
    if (need > cap) need = cap;
    ensure(bulkScratch, bulkBytes, peerBulk, need, stream);
    v.scratch = bulkScratch;
    v.scratchBytes = bulkBytes;
    for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerBulk[r];
    auto outs = registerOutput(out, stream);
    for (int r = 0; r < nranks; ++r) v.peerOutput[r] = outs[r];
    return launchAllReduceBulk(algo, &v, 1, nranks, bytes, dtype, op, nblocks, nthreads, spinBudgetTicks(), stream);
  }
  if (algo == MSCCLPP_AMD_ALGO_TEST_K5) {
    if (in != out) {
      warn("mscclpp-test kernel 5 runs in place (sendbuff == recvbuff)");
      return ncclInvalidUsage;
    }
    auto bufs = registerOutput(out, stream);
    for (int r = 0; r < nranks; ++r) v.peerOutput[r] = bufs[r];
    return launchAllReduceBulk(algo, &v, 1, nranks, bytes, dtype, op, nblocks, nthreads, spinBudgetTicks(), stream);
  }
  if (algo == MSCCLPP_AMD_ALGO_RSAG_PIPELINE) {
    // every remote store lands in the bulk scratch: no user-buffer registration at all
    size_t need = 2 * bytes + 16 * (size_t)nranks * 64;
    if (need > bulkBytes) need = bulkBytes;  // fewer stages, never a re-allocation
    ensure(bulkScratch, bulkBytes, peerBulk, need, stream);
    v.scratch = bulkScratch;
    v.scratchBytes = bulkBytes;
    for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerBulk[r];
    if (!pipeSems) {  // counters must start at zero; each launch leaves them at zero (allreduce_bulk.hip)
      HIPCHECK(hipMalloc((void**)&pipeSems, kPipeSemsWords * sizeof(uint64_t)));
      HIPCHECK(hipMemset(pipeSems, 0, kPipeSemsWords * sizeof(uint64_t)));
    }
    v.pipeSems = pipeSems;
    return launchAllReducePipeline(&v, 1, nranks, bytes, dtype, op, nblocks, nthreads, spinBudgetTicks(), stream);
  }
  if (algo == MSCCLPP_AMD_ALGO_RSAG_ZC) {
    // zero-copy: peers' inputs and outputs are mapped once per buffer (the reference registers
    // both as remote memories, allreduce_rsag_zero_copy.cu:25-27); no scratch
    auto outs = registerOutput(out, stream);
    auto ins = registerOutput(const_cast<void*>(in), stream);
    for (int r = 0; r < nranks; ++r) {
      v.peerOutput[r] = outs[r];
      v.peerInput[r] = ins[r];
    }
    return launchAllReduceBulk(algo, &v, 1, nranks, bytes, dtype, op, nblocks, nthreads, spinBudgetTicks(), stream);
  }
  return ncclInvalidArgument;
}

int ncclComm::bulkCollective(int mode, const void* in, void* out, size_t blockBytes, int dtype, int op, int algo,
                             int nblocks, int nthreads, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(mu);
  mappings.beginLaunch();
  const int rc = bulkCollectiveLaunch(mode, in, out, blockBytes, dtype, op, algo, nblocks, nthreads, stream);
  mappings.recordUses(stream, device);
  return rc;
}

int ncclComm::bulkCollectiveLaunch(int mode, const void* in, void* out, size_t blockBytes, int dtype, int op, int algo,
                                   int nblocks, int nthreads, hipStream_t stream) {
  if (blockBytes % 16) {
    warn("ReduceScatter/AllGather blocks must be a multiple of 16 bytes on this path");
    return ncclInvalidUsage;
  }
  const size_t total = blockBytes * nranks;
  mscclppAmdRankView v = baseView(in, out);
  size_t need = total + 16 * (size_t)nranks * 64;
  const size_t cap = bulkBytes;
  if (need > cap) need = cap;
  ensure(bulkScratch, bulkBytes, peerBulk, need, stream);
  v.scratch = bulkScratch;
  v.scratchBytes = bulkBytes;
  for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerBulk[r];
  if (mode == 2) {
    auto outs = registerOutput(out, stream);
    for (int r = 0; r < nranks; ++r) v.peerOutput[r] = outs[r];
  } else {
    for (int r = 0; r < nranks; ++r) v.peerOutput[r] = out;  // unused by ReduceScatter
  }
  if (algo != MSCCLPP_AMD_ALGO_RSAG) algo = MSCCLPP_AMD_ALGO_FULLMESH;
  return launchCollectiveBulk(mode, algo, &v, 1, nranks, total, dtype, op, nblocks, nthreads, spinBudgetTicks(),
                              stream);
}

int ncclComm::broadcast(const void* send, void* recv, size_t bytes, int root, int nblocks, int nthreads,
                        hipStream_t stream) {
  std::lock_guard<std::mutex> lk(mu);
  const void* mine = rank == root ? send : recv;
  const IpcBlob blob = exportBlob(mine);
  std::vector<IpcBlob> all(nranks);
  boot->allGather(&blob, all.data(), sizeof(IpcBlob));
  mscclppAmdRankView v = baseView(rank == root ? send : recv, recv);
  const bool captured = streamCapturing(stream);
  if (rank != root) {
    // the mapping stays referenced until a later broadcast from the same root replaces it (and
    // is then retired: the kernel below may still be queued).  A mapping used under stream
    // capture is kept until dropUserRegistrations instead: the graph's replays read through it
    // (pinned: sticky while the same mapping stays in the slot).
    auto m = importBlob(all[root]);
    Lease& slot = bcast[(size_t)root];
    if (!slot.maps.empty() && slot.maps[0] != m) {
      if (slot.pinned) bcastPinned.push_back(std::move(slot));
      else mappings.retire(std::move(slot));
      slot = Lease();
    }
    if (slot.maps.empty()) slot.maps.push_back(m);
    if (captured) slot.pinned = true;
    v.peerInput[root] = (char*)m.get() + all[root].offset;
  }
  const int rc = launchBroadcast(&v, 1, nranks, bytes, root, nblocks, nthreads, spinBudgetTicks(), stream);
  if (rank != root && rc == 0 && !captured) bcast[(size_t)root].uses.record(stream, device);
  mappings.flush(device);
  return rc;
}

int ncclComm::allToAll(const void* send, void* recv, const mscclppAmdAllToAllSeg* segs, int nblocks, hipStream_t stream,
                       const SendIdent* idents, const mscclppAmdAllToAllLLSeg* ll, uint64_t maxSeg) {
  std::lock_guard<std::mutex> lk(mu);
  // Small exchanges: one hop of LL8 packets through the LL scratch (kernels/alltoall_ll.hip; DESIGN.md
  // §17h) -- nothing is registered and no token is exchanged.  The rule is a function of (nranks,
  // maxSeg) and the environment, so every rank decides alike.  Under capture a scratch that would have
  // to grow cannot (ensure); such a call takes the pull path instead -- the capture state and llBytes
  // are the same on every rank.
  if (ll && alltoallTakesLL(nranks, maxSeg)) {
    const size_t need = alltoallLLScratchRequired(nranks, maxSeg);
    if (need && (need <= llBytes || !streamCapturing(stream))) {
      mappings.beginLaunch();
      mscclppAmdRankView v = baseView(send, recv);
      ensure(llScratch, llBytes, peerLL, need, stream);
      v.scratch = llScratch;
      v.scratchBytes = llBytes;
      for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerLL[r];
      const int rc = launchAllToAllLL(&v, 1, nranks, ll, maxSeg, 0, 0, spinBudgetTicks(), stream);
      mappings.recordUses(stream, device);
      if (rc == 0) ++a2aLLCount;
      return rc;
    }
  }
  mscclppAmdRankView v = pullView(send, recv, stream, idents);
  const int rc = launchAllToAll(&v, 1, nranks, segs, nblocks, 0, spinBudgetTicks(), stream);
  mappings.recordUses(stream, device);
  return rc;
}

int ncclComm::reduce(const void* send, void* recv, size_t bytes, int dtype, int op, int root, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(mu);
  mscclppAmdRankView v = pullView(send, rank == root ? recv : nullptr, stream);
  const int rc = launchReduce(&v, 1, nranks, bytes, dtype, op, root, 0, 0, spinBudgetTicks(), stream);
  mappings.recordUses(stream, device);
  return rc;
}

int ncclComm::pullReduce(int coll, const void* send, void* recv, size_t bytes, int dtype, int op, int root,
                         hipStream_t stream, float scale, const void* scalePtr) {
  std::lock_guard<std::mutex> lk(mu);
  // Small AllReduce / ReduceScatter: one hop of LL8 packets through the LL scratch (kernels/
  // pull_reduce_ll.hip) -- nothing is registered and no token is exchanged.  The
  // rule is a function of (coll, nranks, bytes) and the environment, so every rank decides alike.
  // Under capture a scratch that would have to grow cannot (ensure); such a call takes the pull
  // path instead -- the capture state and llBytes are the same on every rank.
  if (coll != MSCCLPP_AMD_PULL_REDUCE && pullReduceTakesLL(coll, nranks, bytes)) {
    const size_t need = pullReduceLLScratchRequired(coll, nranks, bytes, dtype, op);
    if (need && (need <= llBytes || !streamCapturing(stream))) {
      mappings.beginLaunch();
      mscclppAmdRankView v = baseView(send, recv);
      ensure(llScratch, llBytes, peerLL, need, stream);
      v.scratch = llScratch;
      v.scratchBytes = llBytes;
      for (int r = 0; r < nranks; ++r) v.peerScratch[r] = peerLL[r];
      const bool scaled = op == MSCCLPP_AMD_PREMUL_SUM;
      const int rc = launchPullReduceLL(&v, 1, nranks, coll, bytes, dtype, op, 0, 0, spinBudgetTicks(), stream,
                                        scaled ? &scale : nullptr, scaled ? &scalePtr : nullptr);
      mappings.recordUses(stream, device);
      if (rc == 0) ++pullLLCount;
      return rc;
    }
  }
  mscclppAmdRankView v = pullView(send, recv, stream);
  if (coll == MSCCLPP_AMD_PULL_ALLREDUCE) {
    if (recv == send) {  // in place: the same registration
      for (int r = 0; r < nranks; ++r) v.peerOutput[r] = const_cast<void*>(v.peerInput[r]);
    } else {
      const auto outs = registerOutput(recv, stream);
      for (int r = 0; r < nranks; ++r) v.peerOutput[r] = outs[r];
    }
  }
  const int rc = launchPullReduce(&v, 1, nranks, coll, bytes, dtype, op, root, 0, 0, spinBudgetTicks(), stream, &scale,
                                  &scalePtr);
  mappings.recordUses(stream, device);
  return rc;
}

ncclRedOp_t ncclComm::preMulCreate(const PreMulOp& e) {
  std::lock_guard<std::mutex> lk(mu);
  size_t slot = 0;
  while (slot < preMulOps.size() && preMulOps[slot].live) ++slot;
  if (slot == preMulOps.size()) preMulOps.emplace_back();
  preMulOps[slot] = e;
  preMulOps[slot].live = true;
  return (ncclRedOp_t)((int)ncclNumOps + (int)slot);
}

bool ncclComm::preMulFind(ncclRedOp_t op, PreMulOp* out, bool destroy) {
  const long slot = (long)(int)op - (long)ncclNumOps;
  if (slot < 0) return false;  // a built-in operation: no lock on the path of every collective call
  std::lock_guard<std::mutex> lk(mu);
  if (slot >= (long)preMulOps.size() || !preMulOps[(size_t)slot].live) return false;
  if (out) *out = preMulOps[(size_t)slot];
  if (destroy) preMulOps[(size_t)slot].live = false;
  return true;
}
