// ncclComm: exchange of IPC handles, scratch growth, registration of user buffers and teardown.
#include "comm_internal.hpp"

// MSCCLPP_AMD_DEBUG_IPC: one line for the allocation `b` as `rank` exported it (peer < 0), or as
// imported from `peer` and mapped at `mapped`.
static void debugIpc(int rank, int peer, const IpcBlob& b, const void* ptr, const void* mapped) {
  if (!std::getenv("MSCCLPP_AMD_DEBUG_IPC")) return;
  if (peer < 0) {
    std::fprintf(stderr, "ipc rank %d export ptr %p base %llx bytes %llu id %llu pooled %u\n", rank, ptr,
                 (unsigned long long)b.base, (unsigned long long)b.bytes,
                 (unsigned long long)allocationId((void*)b.base), b.pooled);
    return;
  }
  std::string hex;
  const unsigned char* h = reinterpret_cast<const unsigned char*>(&b.handle);
  for (size_t i = 0; i < sizeof(b.handle); ++i) {
    char c[3];
    std::snprintf(c, sizeof c, "%02x", h[i]);
    hex += c;
  }
  std::fprintf(stderr, "ipc rank %d peer %d base %llx bytes %llu handle %s mapped %p\n", rank, peer,
               (unsigned long long)b.base, (unsigned long long)b.bytes, hex.c_str(), mapped);
}

PeerBufs ncclComm::exchange(void* ptr) {
  const IpcBlob mine = exportBlob(ptr);
  debugIpc(rank, -1, mine, ptr, nullptr);
  info("rank " + std::to_string(rank) + ": got ipc handle, all-gather");
  std::vector<IpcBlob> all(nranks);
  boot->allGather(&mine, all.data(), sizeof(IpcBlob));
  PeerBufs res;
  for (int r = 0; r < nranks; ++r) {
    if (r == rank) {
      res[r] = ptr;
      continue;
    }
    res.maps[(size_t)r] = importBlob(all[r]);
    res[r] = (char*)res.maps[(size_t)r].get() + all[r].offset;
    debugIpc(rank, r, all[r], nullptr, res.maps[(size_t)r].get());
  }
  return res;
}

void ncclComm::ensure(void*& buf, size_t& have, PeerBufs& peers, size_t need, hipStream_t stream) {
  if (need <= have) return;
  if (streamCapturing(stream))
    throw std::logic_error("scratch must grow to " + std::to_string(need) +
                           " bytes, which cannot happen while the stream is capturing a graph: run this call "
                           "once before capture");
  size_t want = have ? have : (size_t)64 << 20;
  while (want < need) want *= 2;
  HIPCHECK(hipDeviceSynchronize());
  boot->barrier();  // every rank has drained its previous use of the old buffers
  peers = PeerBufs();  // our mappings of the peers' old buffers close here
  if (buf) outgrown.push_back(buf);
  buf = allocUncached(want);
  have = want;
  peers = exchange(buf);
  boot->barrier();
  info("rank " + std::to_string(rank) + " scratch grown to " + std::to_string(want));
}

void ncclComm::retireReg(RegMap& regs, RegMap::iterator it) {
  UserReg& reg = it->second;
  if (reg.lease.pinned)
    info("rank " + std::to_string(rank) + ": pinned registration of allocation " + std::to_string(it->first.first) +
         " retired (its address now belongs to a new allocation)");
  for (auto& m : reg.bases.maps)
    if (m) reg.lease.maps.push_back(std::move(m));
  mappings.retire(std::move(reg.lease));
  regs.erase(it);
}

void ncclComm::evictFor(RegMap& regs) {
  size_t unpinned = 0;
  for (const auto& e : regs) unpinned += e.second.lease.pinned ? 0 : 1;
  if (unpinned < kMaxUserRegs) return;
  auto lru = regs.end();
  for (auto j = regs.begin(); j != regs.end(); ++j)
    if (!j->second.lease.pinned && (lru == regs.end() || j->second.lease.lastUse < lru->second.lease.lastUse)) lru = j;
  retireReg(regs, lru);
}

std::array<void*, MSCCLPP_AMD_MAX_RANKS> ncclComm::registerOutput(void* out, hipStream_t stream, bool pin) {
  void* base = nullptr;
  size_t sz = 0;
  HIPCHECK(hipMemGetAddressRange((hipDeviceptr_t*)&base, &sz, (hipDeviceptr_t)out));
  const uint64_t bid = allocationId(base);
  const auto key = std::make_pair((uint64_t)base, (uint64_t)sz);
  auto it = userRegs.find(key);
  if (it != userRegs.end() && it->second.bufferId != bid) {
    retireReg(userRegs, it);  // the address now belongs to another allocation
    it = userRegs.end();
  }
  if (it == userRegs.end()) {
    evictFor(userRegs);
    UserReg reg;
    reg.bufferId = bid;
    // symmetric memory: every rank's matching allocation, exchanged now (collective); otherwise the
    // peers' allocations come with each new pointer below
    if (symmetricMemory) reg.bases = exchange(base);
    ++allocExchanges;
    it = userRegs.emplace(key, std::move(reg)).first;
  }
  UserReg& reg = it->second;
  reg.lease.lastUse = ++useClock;
  if (pin || streamCapturing(stream)) reg.lease.pinned = true;
  const uint64_t off = (uint64_t)((char*)out - (char*)base);
  auto pit = reg.byOffset.find(off);
  if (pit == reg.byOffset.end()) {
    std::array<void*, MSCCLPP_AMD_MAX_RANKS> res{};
    if (symmetricMemory) {
      // the application declared symmetric allocation: the offset is the same on every rank and
      // this call stays local
      for (int r = 0; r < nranks; ++r) res[r] = (r == rank) ? out : (char*)reg.bases[r] + off;
    } else {
      // A pointer this rank has not passed before: one host all-gather carries every rank's
      // allocation (handle, base, bytes) and the offset of ITS buffer inside it, and each peer
      // pointer is built from that rank's own pair.  Which of a rank's buffers share an allocation
      // is its allocator's business -- a caching allocator fed rank-dependent sizes groups them
      // differently per rank -- so no peer base cached for the local allocation may be combined with
      // an offset the peer took in another one (that read foreign memory, with no error).  The call
      // is collective exactly when the buffer is new, which every rank sees alike (every rank passes
      // its matching buffer); a peer allocation already mapped is found open (openIpcHandle).
      PeerBufs now = exchange(out);
      ++offsetExchanges;
      auto& held = reg.lease.maps;
      for (int r = 0; r < nranks; ++r) {
        res[r] = now[r];
        auto& m = now.maps[(size_t)r];
        if (m && std::find(held.begin(), held.end(), m) == held.end()) held.push_back(std::move(m));
      }
    }
    pit = reg.byOffset.emplace(off, res).first;
  }
  const auto res = pit->second;
  mappings.touch(reg.lease);
  mappings.flush(device);
  return res;
}

ncclComm::SendIdent ncclComm::sendIdent(const void* send) {
  void* base = nullptr;
  size_t sz = 0;
  HIPCHECK(hipMemGetAddressRange((hipDeviceptr_t*)&base, &sz, (hipDeviceptr_t)send));
  SendIdent s{};
  s.base = (uint64_t)base;
  s.id = allocationId(base);
  s.off = (uint64_t)((const char*)send - (char*)base);
  auto it = pairedRegs.find(std::make_pair((uint64_t)base, (uint64_t)sz));
  if (it != pairedRegs.end() && it->second.bufferId == s.id)
    for (int r = 0; r < nranks; ++r) {
      s.pairedBase[r] = it->second.peerIdent[(size_t)r].first;
      s.pairedId[r] = it->second.peerIdent[(size_t)r].second;
    }
  return s;
}

bool ncclComm::pairingStale(const SendIdent* all, int n, int q) {
  for (int r = 0; r < n; ++r)
    if (r != q && (all[q].pairedBase[r] != all[r].base || all[q].pairedId[r] != all[r].id || !all[r].id)) return true;
  return false;
}

std::array<void*, MSCCLPP_AMD_MAX_RANKS> ncclComm::registerPaired(void* send, const SendIdent* all, hipStream_t stream) {
  bool reexchange = false;
  for (int q = 0; q < nranks; ++q) reexchange = reexchange || pairingStale(all, nranks, q);
  const SendIdent& me = all[rank];
  size_t sz = 0;
  void* base = nullptr;
  HIPCHECK(hipMemGetAddressRange((hipDeviceptr_t*)&base, &sz, (hipDeviceptr_t)send));
  const auto key = std::make_pair(me.base, (uint64_t)sz);
  auto it = pairedRegs.find(key);
  if (it != pairedRegs.end() && (reexchange || it->second.bufferId != me.id)) {
    retireReg(pairedRegs, it);  // (an unchanged peer's mapping is found open again at its address)
    it = pairedRegs.end();
  }
  if (it == pairedRegs.end()) {
    if (!reexchange) throw std::logic_error("AllToAllv registration out of step");
    evictFor(pairedRegs);
    UserReg reg;
    reg.bufferId = me.id;
    reg.bases = exchange(base);
    ++allocExchanges;
    for (int r = 0; r < nranks; ++r) reg.peerIdent[(size_t)r] = std::make_pair(all[r].base, all[r].id);
    it = pairedRegs.emplace(key, std::move(reg)).first;
  }
  UserReg& reg = it->second;
  reg.lease.lastUse = ++useClock;
  if (streamCapturing(stream)) reg.lease.pinned = true;
  std::array<void*, MSCCLPP_AMD_MAX_RANKS> res{};
  for (int r = 0; r < nranks; ++r) res[r] = r == rank ? send : (char*)reg.bases[r] + all[r].off;
  mappings.touch(reg.lease);
  mappings.flush(device);
  return res;
}

void ncclComm::dropLeases() {
  userRegs.clear();
  pairedRegs.clear();
  for (auto& slot : bcast) slot = Lease();
  bcastPinned.clear();
  for (auto& kept : p2pImports) kept.clear();
  mappings.clear();
}

void ncclComm::dropUserRegistrations() {
  HIPCHECK(hipDeviceSynchronize());
  boot->barrier();  // no rank still runs a kernel that uses a mapping being closed
  dropLeases();
  boot->barrier();
}

void ncclComm::destroy() {
  (void)hipDeviceSynchronize();
  for (auto& m : selMemo) m = SelMemo();
  algos.reset();
  executor.reset();
  if (boot) {
    try {
      boot->barrier();
    } catch (...) {
    }
  }
  dropLeases();
  peerLL = peerBulk = peerTok = PeerBufs();
  freeDevice(llScratch);
  freeDevice(bulkScratch);
  for (void* p : outgrown) freeDevice(p);
  outgrown.clear();
  freeDevice(tokens);
  if (expected) (void)hipFree(expected);
  if (flags) (void)hipFree(flags);
  if (err) (void)hipFree(err);
  if (errStream) (void)hipStreamDestroy(errStream);
  if (pipeSems) (void)hipFree(pipeSems);
  pipeSems = nullptr;
  errStream = nullptr;
  llScratch = bulkScratch = nullptr;
  tokens = expected = nullptr;
  flags = err = nullptr;
}
