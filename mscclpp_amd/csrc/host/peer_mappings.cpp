// Lifetime of mappings of peers' memory: use events, leases and their retirement (peer_mappings.hpp).
#include "peer_mappings.hpp"

#include "comm_internal.hpp"

namespace mscclpp_amd {
namespace host {

bool streamCapturing(hipStream_t stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return stream && hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

UseEvents::~UseEvents() {
  for (auto& e : ev) (void)hipEventDestroy(e.second);
}

void UseEvents::record(hipStream_t s, int device) {
  for (auto& e : ev)
    if (e.first == s) {
      HIPCHECK(hipEventRecord(e.second, s));
      return;
    }
  if (ev.size() >= 8) {  // a caller cycling through many streams: forget the uses that completed
    size_t k = 0;
    for (auto& e : ev) {
      if (hipEventQuery(e.second) == hipSuccess) (void)hipEventDestroy(e.second);
      else ev[k++] = e;
    }
    (void)hipGetLastError();
    ev.resize(k);
  }
  int cur = device;
  HIPCHECK(hipGetDevice(&cur));
  if (cur != device) HIPCHECK(hipSetDevice(device));
  hipEvent_t x = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&x, hipEventDisableTiming);
  if (cur != device) (void)hipSetDevice(cur);
  HIPCHECK(e);
  ev.push_back({s, x});
  HIPCHECK(hipEventRecord(x, s));
}

bool UseEvents::allComplete() {
  for (auto& e : ev) {
    const hipError_t q = hipEventQuery(e.second);
    if (q == hipErrorNotReady) return false;
    if (q != hipSuccess) (void)hipGetLastError();  // a failed event cannot hold a mapping open
  }
  return true;
}

void RetireQueue::retire(Lease&& l) {
  for (auto t = touched_.begin(); t != touched_.end();)  // not recorded for a launch any more
    t = *t == &l.uses ? touched_.erase(t) : t + 1;
  if (!l.maps.empty() || !l.uses.ev.empty()) retired_.push_back(std::move(l));
}

void RetireQueue::flush(int device) {
  size_t keep = 0;
  for (size_t i = 0; i < retired_.size(); ++i) {
    if (retired_[i].uses.allComplete()) {
      for (auto& m : retired_[i].maps) releaseMappingLater(device, std::move(m));
    } else {
      if (keep != i) retired_[keep] = std::move(retired_[i]);
      ++keep;
    }
  }
  retired_.resize(keep);
}

void RetireQueue::clear() {
  retired_.clear();
  touched_.clear();
}

size_t RetireQueue::pendingMaps() const {
  size_t k = 0;
  for (const auto& r : retired_) k += r.maps.size();
  return k;
}

void RetireQueue::recordUses(hipStream_t stream, int device) {
  if (touched_.empty()) return;  // the LL paths register nothing: no extra host call per launch
  if (!streamCapturing(stream))
    for (UseEvents* u : touched_) u->record(stream, device);
  touched_.clear();
}

}  // namespace host
}  // namespace mscclpp_amd
