// ncclComm: Send / Recv by a zero-copy pull (kernels/sendrecv.hip).
#include "comm_internal.hpp"

bool ncclComm::p2pPost(const void* send, uint64_t bytes, int peer) {
  P2pMsg msg{};
  msg.bytes = bytes;
  try {
    msg.blob = exportBlob(send);
    msg.ok = 1;
  } catch (const std::exception& e) {  // e.g. host memory: the peer still gets its message
    warn(std::string("ncclSend: the buffer cannot be exported: ") + e.what());
    (void)hipGetLastError();
    msg.blob = IpcBlob{};
  }
  boot->send(&msg, sizeof(msg), peer, kP2pTag);
  return msg.ok != 0;
}

const void* ncclComm::p2pMatch(uint64_t bytes, int peer, void** mapping) {
  P2pMsg msg{};
  boot->recv(&msg, sizeof(msg), peer, kP2pTag);  // (outside mu: this waits for the peer's call)
  std::lock_guard<std::mutex> lk(mu);
  if (!msg.ok) {
    warn("ncclRecv: rank " + std::to_string(peer) + " could not export its send buffer");
    return nullptr;
  }
  if (msg.bytes != bytes) {
    warn("ncclRecv: rank " + std::to_string(peer) + " sends " + std::to_string(msg.bytes) + " bytes, " +
         std::to_string(bytes) + " expected (its kernel ends at the spin budget)");
    return nullptr;
  }
  auto m = importBlob(msg.blob);
  auto& kept = p2pImports[(size_t)peer];
  auto it = std::find_if(kept.begin(), kept.end(), [&](const Lease& i) { return i.maps[0] == m; });
  if (it == kept.end()) {
    if (kept.size() >= kP2pKept) {
      auto lru = std::min_element(kept.begin(), kept.end(),
                                  [](const Lease& x, const Lease& y) { return x.lastUse < y.lastUse; });
      mappings.retire(std::move(*lru));
      kept.erase(lru);
    }
    kept.emplace_back();
    it = kept.end() - 1;
    it->maps.push_back(m);
  }
  it->lastUse = ++useClock;
  *mapping = m.get();
  return (const char*)m.get() + msg.blob.offset;
}

int ncclComm::p2pLaunch(const mscclppAmdSendRecvOp* ops, int nops, const std::vector<std::pair<int, void*>>& used,
                        hipStream_t stream) {
  std::lock_guard<std::mutex> lk(mu);
  mscclppAmdRankView v = baseView(nullptr, nullptr);
  const int rc = launchSendRecv(&v, 1, nranks, ops, nops, 0, 0, spinBudgetTicks(), stream);
  if (rc == 0)
    for (const auto& t : used)
      for (auto& i : p2pImports[(size_t)t.first])
        if (i.maps[0].get() == t.second) i.uses.record(stream, device);
  mappings.flush(device);
  return rc;
}
