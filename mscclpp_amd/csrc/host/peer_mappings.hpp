// The lifetime of a mapping of a peer's memory, stated once.  A mapping stays open until every
// launch that read or wrote through it has completed, then closes on the closer thread
// (releaseMappingLater), and never closes while a captured graph may replay through it:
//  * a Lease holds the mappings, the events of their last uses, and whether a graph holds them;
//  * its keeper (a user registration, a Broadcast slot, a Send / Recv import) records a use after
//    each launch through it, unless the stream is capturing -- then the lease is pinned instead;
//  * a keeper that lets an unpinned lease go retires it to the RetireQueue, which closes it at a
//    later call, once its events have completed: no call waits for another stream's work and none
//    synchronizes the device (the reference's context cache never synchronizes either,
//    algorithm.cc:52-60);
//  * a pinned lease is let go only where the caller vouches that no graph replays through it
//    (ncclComm::dropLeases: deregistration and destruction, after a device synchronize), or when
//    its address has passed to a new allocation (its pointers were dead already).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace mscclpp_amd {
namespace host {

// `stream` is being captured into a graph.  (An invalidated capture counts: the launch that follows
// fails anyway, and pinning one registration more is the conservative side.)
bool streamCapturing(hipStream_t stream);

// Where a mapping was last used: one event per stream that launched a kernel through it, recorded
// right after that launch (re-recorded by later launches on the same stream).  Owns its events.
struct UseEvents {
  std::vector<std::pair<hipStream_t, hipEvent_t>> ev;
  UseEvents() = default;
  UseEvents(UseEvents&& o) noexcept { ev.swap(o.ev); }
  UseEvents& operator=(UseEvents&& o) noexcept {  // (what this held goes with `o`)
    ev.swap(o.ev);
    return *this;
  }
  ~UseEvents();
  // `device`: the communicator's (and the stream's); the event is created there whatever device
  // the calling thread has current
  void record(hipStream_t s, int device);
  // Every recorded use has completed (never blocks; a failed event cannot hold a mapping open).
  bool allComplete();
};

// Mappings kept open for one keeper, with the launches that last went through them.
struct Lease {
  std::vector<std::shared_ptr<void>> maps;
  UseEvents uses;
  uint64_t lastUse = 0;  // the keeper's clock, for its least-recently-used choice
  bool pinned = false;   // used under stream capture, or handed to the caller: never evicted
};

// Leases their keepers let go, which queued kernels may still use, and the leases the current call
// handed to its kernel.
class RetireQueue {
 public:
  // `l` is let go: it closes once its last uses have completed (flush).  It is no longer recorded
  // for the current launch.
  void retire(Lease&& l);
  // Close the retired leases whose last uses have completed; the others wait for a later call.
  // Never blocks.
  void flush(int device);
  // Every retired lease, whatever is still queued: only after a device synchronize (teardown).
  void clear();
  size_t pendingMaps() const;  // mappings still waiting for their last launches to complete

  // Launch scope: beginLaunch at the start of an entry point, touch for every lease whose pointers
  // the call hands to its kernel, recordUses after the launch on `stream`.  Under capture nothing
  // is recorded -- those leases are pinned (never retired while a graph may replay).
  void beginLaunch() { touched_.clear(); }
  void touch(Lease& l) { touched_.push_back(&l.uses); }
  void recordUses(hipStream_t stream, int device);

 private:
  std::vector<Lease> retired_;
  std::vector<UseEvents*> touched_;
};

}  // namespace host
}  // namespace mscclpp_amd
