// The proxy-side device surface: ProxyTrigger, FifoDeviceHandle::push / poll / sync and every overload
// of BasePortChannelDeviceHandle / PortChannelDeviceHandle, written once in the reference's spellings
// (mscclpp:: names, <mscclpp/...> headers only), plus the host half that consumes their output
// (ProxyService::handleTrigger, Connection::write).
//
//   test_proxy_primitives <case file> <output file>
//
// The case file is one text line per case, "<idx> <op> <n> <v0> ... <vn-1>"
// (tests/proxy_primitive_cases.py writes it and holds the model).  Per case the host sets up state,
// launches ONE generic kernel <<<grid, lanes>>>, synchronises, and appends to the output file the raw
// ring (all `size` slots, both words), head / tail / tailCache, the semaphore words, the per-call
// array of returned positions, the arenas and the 4-word error record.  It compares nothing: the
// Python side judges, bit for bit.
//
// THE RULE, for both builds: nothing waits for something that is not already there.
//   Groups T (trigger images) and F (positions, laps, poll) have no proxy thread.  The ring
//   (zero-filled), `tail` and `flushDonePos` are pinned, device-mapped words the host sets before the
//   launch.  A case that calls a flush form is refused unless its flushDonePos lies above every
//   position it can reach, so waitFlush's first load ends it; a case that pushes past one lap is
//   refused unless its tail is at least its total push count, so sync returns on its first load; and
//   concurrent pushers are refused unless the ring holds them all (no sync is entered).  The
//   reference's waits are unbounded: here none of them ever takes a second iteration.
//   Groups P (through this library's proxy, loopback) and R (refusals that handleTrigger and
//   Connection::write define) wait only for the running proxy, every wait under the handles'
//   wall-clock budget (MSCCLPP_AMD_SPIN_TIMEOUT_MS, 3 s here), and a wait() is issued only for a
//   signal pushed earlier in the same launch.  No case makes a wait expire on purpose.
//
// With -DPRIMS_REFERENCE the same source compiles against the reference's own include tree.  Groups
// P and R need this library's host side and are compiled out there, and so are the 2^32 cases (the
// reference truncates or asserts; this library refuses with kErrBadGeometry).
#include <hip/hip_runtime.h>

#include <mscclpp/fifo_device.hpp>
#include <mscclpp/port_channel_device.hpp>
#include <mscclpp/semaphore_device.hpp>
#ifndef PRIMS_REFERENCE
#include <mscclpp/core.hpp>
#include <mscclpp/gpu_utils.hpp>
#include <mscclpp/port_channel.hpp>
#endif

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#define HIPCHECK(x)                                                                              \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) {                                                                      \
      std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));    \
      std::exit(2);                                                                              \
    }                                                                                            \
  } while (0)

namespace {

constexpr uint64_t kMagic = 0x3159584F52505644ull;
constexpr uint64_t kMaxRing = 1024;             // slots allocated for the hand-built ring
constexpr uint64_t kMaxPos = 4096;              // returned positions per case
constexpr uint64_t kNoPos = ~0ull;              // a call that returns nothing
constexpr int kMaxV = 48;
#ifndef PRIMS_REFERENCE
constexpr uint64_t kBudgetTicks = 2'000'000;    // 20 ms, groups T and F (never used up: see THE RULE)
constexpr uint64_t kArenaBytes = 96 << 10;      // group P: four registered memories
constexpr uint64_t kWitnessBytes = 3 * kArenaBytes;
constexpr int kProxyFifo = 8;
constexpr int kMaxPuts = 8;
#endif

enum Op : int {
  // members, on a hand-built handle (groups T and F); the six put forms also inside `place`
  OP_PUT, OP_PUT_SAME, OP_PWS, OP_PWS_SAME, OP_PWSF, OP_PWSF_SAME, OP_SIGNAL, OP_FLUSH, OP_PUSH, OP_POLL,
  // through the proxy (groups P and R)
  OP_PLACE, OP_ORDER, OP_ACCOUNT, OP_LAPS, OP_REFUSE, OP_COUNT
};
const char* const kOpNames[OP_COUNT] = {"put", "put_same", "putWithSignal", "putWithSignal_same",
                                        "putWithSignalAndFlush", "putWithSignalAndFlush_same", "signal", "flush",
                                        "push", "poll", "place", "order", "account", "laps", "refuse"};

// v[] of a member case
enum H : int {
  H_BOUND, H_RING, H_GRID, H_LANES, H_ACTIVE, H_COUNT, H_STEP, H_TYPE, H_DSTID, H_DSTOFF, H_SRCID, H_SRCOFF, H_SIZE,
  H_SEMID, H_TAIL, H_FLUSHDONE, H_N
};

struct Args {
  int op;
  uint64_t v[kMaxV];
  mscclpp::BasePortChannelDeviceHandle base;
  mscclpp::PortChannelDeviceHandle bound;
  uint64_t* pos;
  char* arena[4];
  char* witness;
};

// One put form on the Base handle (explicit ids) or the bound one (dst_ / src_).  The _same forms
// take the common offset from dstOff.
__device__ void putForm(mscclpp::BasePortChannelDeviceHandle& b, mscclpp::PortChannelDeviceHandle& p, bool useBound,
                        int form, mscclpp::MemoryId dstId, uint64_t dstOff, mscclpp::MemoryId srcId, uint64_t srcOff,
                        uint64_t size) {
  if (!useBound) {
    switch (form) {
      case OP_PUT: b.put(dstId, dstOff, srcId, srcOff, size); break;
      case OP_PUT_SAME: b.put(dstId, srcId, dstOff, size); break;
      case OP_PWS: b.putWithSignal(dstId, dstOff, srcId, srcOff, size); break;
      case OP_PWS_SAME: b.putWithSignal(dstId, srcId, dstOff, size); break;
      case OP_PWSF: b.putWithSignalAndFlush(dstId, dstOff, srcId, srcOff, size); break;
      case OP_PWSF_SAME: b.putWithSignalAndFlush(dstId, srcId, dstOff, size); break;
    }
  } else {
    switch (form) {
      case OP_PUT: p.put(dstOff, srcOff, size); break;
      case OP_PUT_SAME: p.put(dstOff, size); break;
      case OP_PWS: p.putWithSignal(dstOff, srcOff, size); break;
      case OP_PWS_SAME: p.putWithSignal(dstOff, size); break;
      case OP_PWSF: p.putWithSignalAndFlush(dstOff, srcOff, size); break;
      case OP_PWSF_SAME: p.putWithSignalAndFlush(dstOff, size); break;
    }
  }
}

// ---- Groups T and F: every active lane calls one member `count` times, call `ord` with
// dstOffset (or the common offset, or poll's fifoHead) = dstOff + ord * step ---------------------------
__device__ void memberGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base,
                            mscclpp::PortChannelDeviceHandle& bound, uint32_t tid) {
  const uint64_t* v = a.v;
  if (tid >= v[H_ACTIVE]) return;
  const bool useBound = v[H_BOUND] != 0;
  mscclpp::BasePortChannelDeviceHandle& h = useBound ? bound : base;
  for (uint64_t i = 0; i < v[H_COUNT]; ++i) {
    const uint64_t ord = tid * v[H_COUNT] + i;
    const uint64_t dstOff = v[H_DSTOFF] + ord * v[H_STEP];
    uint64_t ret = kNoPos;
    switch (a.op) {
      case OP_PUSH:
        ret = h.fifo_.push(mscclpp::ProxyTrigger(v[H_TYPE], (uint32_t)v[H_DSTID], dstOff, (uint32_t)v[H_SRCID],
                                                 v[H_SRCOFF], v[H_SIZE], (uint32_t)v[H_SEMID]));
        break;
      case OP_POLL:
        ret = h.fifo_.poll(dstOff);
        break;
      case OP_SIGNAL:
        h.signal();
        break;
      case OP_FLUSH:
        h.flush();
        break;
      default:
        putForm(base, bound, useBound, a.op, (uint32_t)v[H_DSTID], dstOff, (uint32_t)v[H_SRCID], v[H_SRCOFF],
                v[H_SIZE]);
    }
    a.pos[ord] = ret;
  }
}

#ifndef PRIMS_REFERENCE
// ---- Groups P and R -------------------------------------------------------------------------------------
// place: v = bound, form, nput, split[4], then nput x (dstId, dstOff, srcId, srcOff, size).  One lane
// issues the puts, flushes, and consumes the signals it asked for (they have arrived: the flush
// drained the connection).
__device__ void placeGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base,
                           mscclpp::PortChannelDeviceHandle& bound, uint32_t tid) {
  if (tid != 0) return;
  const uint64_t* v = a.v;
  const bool useBound = v[0] != 0;
  const int form = (int)v[1];
  mscclpp::BasePortChannelDeviceHandle& h = useBound ? bound : base;
  for (uint64_t p = 0; p < v[2]; ++p) {
    const uint64_t* q = v + 7 + 5 * p;
    putForm(base, bound, useBound, form, (uint32_t)q[0], q[1], (uint32_t)q[2], q[3], q[4]);
  }
  h.flush();
  if (form >= OP_PWS)
    for (uint64_t p = 0; p < v[2]; ++p) h.wait();
}

// order: v = size, rounds, srcId, srcOff, srcStep, dstId0, dstOff, witnessStride.  Workgroup 0 puts
// round r from srcOff + r * srcStep into memory dstId0 + r with a signal; workgroup 1 waits, then
// copies that destination range into the witness.
__device__ void orderGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base) {
  const uint64_t* v = a.v;
  if (blockIdx.x == 0) {
    if (threadIdx.x != 0) return;
    for (uint64_t r = 0; r < v[1]; ++r)
      base.putWithSignal((uint32_t)(v[5] + r), v[6], (uint32_t)v[2], v[3] + r * v[4], v[0]);
    base.flush();
  } else {
    for (uint64_t r = 0; r < v[1]; ++r) {
      if (threadIdx.x == 0) base.wait();
      __syncthreads();
      const volatile char* from = a.arena[v[5] + r] + v[6];
      char* to = a.witness + r * v[7];
      for (uint64_t i = threadIdx.x; i < v[0]; i += blockDim.x) to[i] = from[i];
      __syncthreads();
    }
  }
}

// account: v = k, j, dstId, srcId.  k signals (signal() and a 16-byte putWithSignal alternating), a
// flush, j waits, then poll() until it says false; pos[0] = how often it said true.
__device__ void accountGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base, uint32_t tid) {
  if (tid != 0) return;
  const uint64_t* v = a.v;
  for (uint64_t i = 0; i < v[0]; ++i) {
    if (i & 1)
      base.putWithSignal((uint32_t)v[2], 16 * i, (uint32_t)v[3], 16 * (i + 7), 16);
    else
      base.signal();
  }
  base.flush();
  for (uint64_t i = 0; i < v[1]; ++i) base.wait();
  uint64_t n = 0;
  for (uint64_t t = 0; t < v[0] + 4 && base.poll(); ++t) ++n;
  a.pos[0] = n;
}

// laps: v = lanes, per, mode, dstId, srcId.  Every lane puts `per` 16-byte cells of its own (cell c
// from source cell c + 5); mode 0: lane 0 flushes after a workgroup barrier, mode 1: every lane
// flushes after its own puts.
__device__ void lapsGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base, uint32_t tid) {
  const uint64_t* v = a.v;
  for (uint64_t i = 0; i < v[1]; ++i) {
    const uint64_t cell = tid * v[1] + i;
    base.put((uint32_t)v[3], 16 * cell, (uint32_t)v[4], 16 * (cell + 5), 16);
  }
  if (v[2] == 1) {
    base.flush();
  } else {
    __syncthreads();
    if (tid == 0) base.flush();
  }
}

// refuse: v = the refused put's (dstId, dstOff, srcId, srcOff, size), then a valid put's.
__device__ void refuseGroup(const Args& a, mscclpp::BasePortChannelDeviceHandle& base, uint32_t tid) {
  if (tid != 0) return;
  const uint64_t* v = a.v;
  base.put((uint32_t)v[0], v[1], (uint32_t)v[2], v[3], v[4]);
  base.put((uint32_t)v[5], v[6], (uint32_t)v[7], v[8], v[9]);
  base.flush();
}
#endif  // !PRIMS_REFERENCE

__global__ void __launch_bounds__(1024) proxyKernel(Args a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  mscclpp::BasePortChannelDeviceHandle base = a.base;
  mscclpp::PortChannelDeviceHandle bound = a.bound;
  if (a.op <= OP_POLL) {
    memberGroup(a, base, bound, tid);
    return;
  }
#ifndef PRIMS_REFERENCE
  switch (a.op) {
    case OP_PLACE: placeGroup(a, base, bound, tid); break;
    case OP_ORDER: orderGroup(a, base); break;
    case OP_ACCOUNT: accountGroup(a, base, tid); break;
    case OP_LAPS: lapsGroup(a, base, tid); break;
    case OP_REFUSE: refuseGroup(a, base, tid); break;
  }
#endif
}

// ---- host ---------------------------------------------------------------------------------------------
struct Case {
  uint64_t idx;
  int op;
  std::vector<uint64_t> v;
};

bool parseLine(const std::string& line, Case& c) {
  char name[64];
  unsigned long long idx, n;
  int used = 0;
  if (std::sscanf(line.c_str(), "%llu %63s %llu%n", &idx, name, &n, &used) != 3) return false;
  c.idx = idx;
  c.op = -1;
  for (int i = 0; i < OP_COUNT; ++i)
    if (!std::strcmp(name, kOpNames[i])) c.op = i;
  if (c.op < 0 || n > (unsigned long long)kMaxV) return false;
  const char* p = line.c_str() + used;
  for (unsigned long long i = 0; i < n; ++i) {
    char* end;
    const unsigned long long x = std::strtoull(p, &end, 10);
    if (end == p) return false;
    c.v.push_back(x);
    p = end;
  }
  return true;
}

#ifndef PRIMS_REFERENCE
bool inArena(uint64_t id, uint64_t off, uint64_t size) { return id < 4 && off <= kArenaBytes && size <= kArenaBytes - off; }

uint32_t pat(uint32_t idx, uint32_t arena, uint32_t j) {
  uint32_t x = (j + 1u) * 2654435761u + (idx * 4u + arena + 1u) * 0x9E3779B9u;
  x ^= x >> 15;
  return x;
}
#endif

// What the host refuses before a launch: a line that would leave the allocations, or that would make
// a wait take a second iteration where no proxy runs (THE RULE).  The table's own properties are
// asserted by the Python side.
const char* refusal(const Case& c) {
  const std::vector<uint64_t>& v = c.v;
  if (c.op <= OP_POLL) {
    if (v.size() != H_N) return "a member case has 16 values";
    const uint64_t ring = v[H_RING];
    if (ring < 1 || ring > kMaxRing || (ring & (ring - 1))) return "ring size";
    if (v[H_GRID] < 1 || v[H_GRID] > 8 || v[H_LANES] < 1 || v[H_LANES] > 1024) return "launch shape";
    if (v[H_ACTIVE] < 1 || v[H_ACTIVE] > v[H_GRID] * v[H_LANES]) return "active lanes";
    if (v[H_COUNT] < 1 || v[H_COUNT] > kMaxPos) return "call count";
    const uint64_t total = v[H_ACTIVE] * v[H_COUNT];
    if (total > kMaxPos) return "more calls than position slots";
    if (c.op != OP_POLL) {
      if (v[H_ACTIVE] > 1 && total > ring) return "concurrent pushers exceed the ring: a sync would be entered";
      if (total > ring && v[H_TAIL] < total) return "pushes past one lap need tail >= the push count";
    }
    if ((c.op == OP_FLUSH || c.op == OP_PWSF || c.op == OP_PWSF_SAME) && v[H_FLUSHDONE] <= total)
      return "a flush form needs flushDonePos above every position it can reach";
#ifdef PRIMS_REFERENCE
    const uint64_t last = v[H_DSTOFF] + (total - 1) * v[H_STEP];
    if (c.op != OP_POLL && ((last | v[H_DSTOFF] | v[H_SRCOFF] | v[H_SIZE]) >> 32 || v[H_DSTID] >= 512 ||
                            v[H_SRCID] >= 512 || v[H_SEMID] >= 1024 || v[H_TYPE] >= 8))
      return "a field that does not fit is outside the reference's contract";
#endif
    return nullptr;
  }
#ifdef PRIMS_REFERENCE
  return "groups P and R need this library's host side";
#else
  switch (c.op) {
    case OP_PLACE: {
      if (v.size() < 7 || v[2] < 1 || v[2] > (uint64_t)kMaxPuts || v.size() != 7 + 5 * v[2]) return "place: shape";
      if (v[1] > OP_PWSF_SAME) return "place: form";
      for (int i = 0; i < 4; ++i)
        if (v[3 + i] > kArenaBytes || v[3 + i] % 4) return "place: split";
      for (uint64_t p = 0; p < v[2]; ++p) {
        const uint64_t* q = v.data() + 7 + 5 * p;
        if (!inArena(q[0], q[1], q[4]) || !inArena(q[2], q[3], q[4])) return "place: a put leaves its arena";
      }
      return nullptr;
    }
    case OP_ORDER:
      if (v.size() != 8 || v[1] < 1 || v[1] > 3 || v[5] + v[1] > 4) return "order: shape";
      for (uint64_t r = 0; r < v[1]; ++r)
        if (!inArena(v[2], v[3] + r * v[4], v[0]) || !inArena(v[5] + r, v[6], v[0]) || v[2] == v[5] + r ||
            r * v[7] + v[0] > kWitnessBytes)
          return "order: a round leaves its arena";
      return nullptr;
    case OP_ACCOUNT:
      if (v.size() != 4 || v[0] < 1 || v[0] > 64 || v[1] > v[0] || v[2] > 3 || v[3] > 3) return "account: shape";
      return nullptr;
    case OP_LAPS:
      if (v.size() != 5 || v[0] < 1 || v[0] > 64 || v[1] < 1 || v[2] > 1 || v[3] > 3 || v[4] > 3 ||
          16 * (v[0] * v[1] + 5) > kArenaBytes)
        return "laps: shape";
      return nullptr;
    case OP_REFUSE:
      if (v.size() != 10) return "refuse: shape";
      // the refused put is checked by the proxy, not here; it must still fit the trigger's fields
      if ((v[1] | v[3] | v[4]) >> 32 || v[0] >= 512 || v[2] >= 512) return "refuse: the refused put must reach the proxy";
      if (!inArena(v[5], v[6], v[9]) || !inArena(v[7], v[8], v[9])) return "refuse: the valid put leaves its arena";
      return nullptr;
  }
  return "unknown op";
#endif
}

struct Record {
  uint64_t idx = 0, ringSlots = 0, npos = 0, narena = 0, arenaBytes[5] = {0, 0, 0, 0, 0};
  uint64_t handled[2] = {0, 0}, headBefore = 0, htt[3] = {0, 0, 0}, sem[8] = {0, 0, 0, 0, 0, 0, 0, 0},
           reserved = 0;
};
static_assert(sizeof(Record) == 24 * 8, "24 words");

template <typename T>
void put(std::FILE* out, const T* p, size_t n) {
  if (n && std::fwrite(p, sizeof(T), n, out) != n) {
    std::fprintf(stderr, "short write\n");
    std::exit(2);
  }
}

// Groups T and F: the hand-built handle over pinned, device-mapped words, as the product allocates them.
struct HandBuilt {
  mscclpp::ProxyTrigger *ring = nullptr, *dRing = nullptr;
  uint64_t *tail = nullptr, *dTail = nullptr, *flushDone = nullptr, *dFlushDone = nullptr;
  uint64_t *head = nullptr, *tailCache = nullptr, *tokens = nullptr;
  uint32_t* err = nullptr;

  void init() {
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    HIPCHECK(hipHostMalloc((void**)&ring, sizeof(mscclpp::ProxyTrigger) * kMaxRing, fl));
    HIPCHECK(hipHostMalloc((void**)&tail, 64, fl));
    HIPCHECK(hipHostMalloc((void**)&flushDone, 64, fl));
    HIPCHECK(hipHostGetDevicePointer((void**)&dRing, ring, 0));
    HIPCHECK(hipHostGetDevicePointer((void**)&dTail, tail, 0));
    HIPCHECK(hipHostGetDevicePointer((void**)&dFlushDone, flushDone, 0));
    HIPCHECK(hipMalloc((void**)&head, 64));
    HIPCHECK(hipMalloc((void**)&tailCache, 64));
    HIPCHECK(hipExtMallocWithFlags((void**)&tokens, 256, hipDeviceMallocUncached));
    HIPCHECK(hipExtMallocWithFlags((void**)&err, 256, hipDeviceMallocUncached));
  }
  void run(const Case& c, uint64_t* pos, std::FILE* out) {
    const std::vector<uint64_t>& v = c.v;
    const uint64_t slots = v[H_RING];
    std::memset((void*)ring, 0, sizeof(mscclpp::ProxyTrigger) * kMaxRing);
    *tail = v[H_TAIL];
    *flushDone = v[H_FLUSHDONE];
    HIPCHECK(hipMemset(head, 0, 64));
    HIPCHECK(hipMemset(tailCache, 0, 64));
    HIPCHECK(hipMemset(tokens, 0, 256));
    HIPCHECK(hipMemset(err, 0, 256));
    HIPCHECK(hipMemset(pos, 0xFF, kMaxPos * 8));
    HIPCHECK(hipDeviceSynchronize());

    // Handles, built on the host as a user of the reference builds them.
    mscclpp::FifoDeviceHandle fifo{};
    fifo.triggers = dRing;
    fifo.head = head;
    fifo.tail = dTail;
    fifo.tailCache = tailCache;
    fifo.size = (int)slots;
    fifo.sizeMask = slots - 1;
    fifo.sizeShift = 0;
    while ((1ull << fifo.sizeShift) < slots) ++fifo.sizeShift;
    mscclpp::Host2DeviceSemaphoreDeviceHandle sem{};
    sem.inboundToken = tokens;
    sem.expectedInboundToken = tokens + 1;
#ifndef PRIMS_REFERENCE
    fifo.budget = sem.budget = kBudgetTicks;
    fifo.err = sem.err = err;
#endif
    Args a{};
    a.op = c.op;
    for (size_t i = 0; i < v.size(); ++i) a.v[i] = v[i];
    a.base = mscclpp::BasePortChannelDeviceHandle((mscclpp::SemaphoreId)v[H_SEMID], sem, fifo, dFlushDone);
    a.bound = mscclpp::PortChannelDeviceHandle((mscclpp::SemaphoreId)v[H_SEMID], sem, fifo,
                                               (mscclpp::MemoryId)v[H_DSTID], (mscclpp::MemoryId)v[H_SRCID], dFlushDone);
    a.pos = pos;
    proxyKernel<<<dim3((unsigned)v[H_GRID]), dim3((unsigned)v[H_LANES])>>>(a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());

    Record rec;
    rec.idx = c.idx, rec.ringSlots = slots, rec.npos = v[H_ACTIVE] * v[H_COUNT];
    HIPCHECK(hipMemcpy(&rec.htt[0], head, 8, hipMemcpyDeviceToHost));
    rec.htt[1] = *tail;
    HIPCHECK(hipMemcpy(&rec.htt[2], tailCache, 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> hpos(rec.npos);
    HIPCHECK(hipMemcpy(hpos.data(), pos, rec.npos * 8, hipMemcpyDeviceToHost));
    uint32_t e[4];
    HIPCHECK(hipMemcpy(e, err, 16, hipMemcpyDeviceToHost));
    put(out, &rec, 1);
    put(out, (const char*)ring, sizeof(mscclpp::ProxyTrigger) * slots);
    put(out, hpos.data(), hpos.size());
    put(out, e, 4);
  }
};

#ifndef PRIMS_REFERENCE
// Groups P and R: one process, a Communicator connected to itself, ProxyService(8) so that real
// consumption crosses laps, four registered GpuBuffers and two semaphores on the one connection.
struct Loopback {
  std::shared_ptr<mscclpp::TcpBootstrap> bootstrap;
  std::shared_ptr<mscclpp::Communicator> comm;
  mscclpp::Connection conn;
  std::vector<mscclpp::GpuBuffer<char>> buffers;
  std::unique_ptr<mscclpp::GpuBuffer<char>> witness;
  std::shared_ptr<mscclpp::ProxyService> proxy;
  mscclpp::SemaphoreId sidA = 0, sidB = 0;
  uint32_t* err = nullptr;
  static constexpr mscclpp::MemoryId kBoundDst = 2, kBoundSrc = 1;

  void init() {
    bootstrap = std::make_shared<mscclpp::TcpBootstrap>(/*rank*/ 0, /*nRanks*/ 1);
    bootstrap->initialize(mscclpp::TcpBootstrap::createUniqueId());
    comm = std::make_shared<mscclpp::Communicator>(bootstrap);
    const mscclpp::Transport transport = mscclpp::Transport::CudaIpc;
    conn = comm->connect(transport, /*remoteRank*/ 0).get();
    proxy = std::make_shared<mscclpp::ProxyService>(kProxyFifo);
    for (int i = 0; i < 4; ++i) {
      buffers.emplace_back(kArenaBytes);
      const mscclpp::MemoryId id = proxy->addMemory(comm->registerMemory(buffers[i].data(), kArenaBytes, transport));
      if (id != (mscclpp::MemoryId)i) throw std::runtime_error("memory ids are not 0..3");
    }
    witness.reset(new mscclpp::GpuBuffer<char>(kWitnessBytes));
    sidA = proxy->buildAndAddSemaphore(*comm, conn);
    sidB = proxy->buildAndAddSemaphore(*comm, conn);
    err = comm->deviceErrorWord();
    proxy->startProxy(/*blocking*/ true);
  }
  void stop() {
    if (proxy) proxy->stopProxy();
  }
  static void semWords(const mscclpp::Host2DeviceSemaphoreDeviceHandle& a,
                       const mscclpp::Host2DeviceSemaphoreDeviceHandle& b, uint64_t* w) {
    HIPCHECK(hipMemcpy(w + 0, a.inboundToken, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(w + 1, a.expectedInboundToken, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(w + 2, b.inboundToken, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(w + 3, b.expectedInboundToken, 8, hipMemcpyDeviceToHost));
  }
  void run(const Case& c, uint64_t* pos, std::FILE* out) {
    const std::vector<uint64_t>& v = c.v;
    // `account` gets a fresh pair of semaphores, so its tokens are judged as absolute values
    if (c.op == OP_ACCOUNT) {
      sidA = proxy->buildAndAddSemaphore(*comm, conn);
      sidB = proxy->buildAndAddSemaphore(*comm, conn);
    }
    const mscclpp::BasePortChannelDeviceHandle hA = proxy->basePortChannel(sidA).deviceHandle();
    const mscclpp::BasePortChannelDeviceHandle hB = proxy->basePortChannel(sidB).deviceHandle();

    // arenas: bytes [0, split) seeded random, 0xA5 from there on
    uint64_t split[4];
    for (int i = 0; i < 4; ++i) split[i] = 0;
    if (c.op == OP_PLACE)
      for (int i = 0; i < 4; ++i) split[i] = v[3 + i];
    else if (c.op == OP_ORDER)
      split[v[2]] = kArenaBytes;
    else if (c.op == OP_ACCOUNT)
      split[v[3]] = kArenaBytes;
    else if (c.op == OP_LAPS)
      split[v[4]] = kArenaBytes;
    else
      split[v[7]] = kArenaBytes;
    std::vector<uint32_t> host(kWitnessBytes / 4);
    for (uint32_t i = 0; i < 4; ++i) {
      for (uint64_t j = 0; j < kArenaBytes / 4; ++j) host[j] = 4 * j < split[i] ? pat((uint32_t)c.idx, i, (uint32_t)j) : 0xA5A5A5A5u;
      HIPCHECK(hipMemcpy(buffers[i].data(), host.data(), kArenaBytes, hipMemcpyHostToDevice));
    }
    const bool hasWitness = c.op == OP_ORDER;
    if (hasWitness) HIPCHECK(hipMemset(witness->data(), 0x5A, kWitnessBytes));
    HIPCHECK(hipMemset(err, 0, 16));  // the error word is cleared between cases
    HIPCHECK(hipMemset(pos, 0xFF, kMaxPos * 8));
    HIPCHECK(hipDeviceSynchronize());

    Record rec;
    rec.idx = c.idx, rec.ringSlots = kProxyFifo, rec.npos = c.op == OP_ACCOUNT ? 1 : 0;
    rec.narena = hasWitness ? 5 : 4;
    for (int i = 0; i < 4; ++i) rec.arenaBytes[i] = kArenaBytes;
    rec.arenaBytes[4] = hasWitness ? kWitnessBytes : 0;
    semWords(hA.semaphore_, hB.semaphore_, rec.sem);
    rec.handled[0] = proxy->triggersHandled();
    HIPCHECK(hipMemcpy(&rec.headBefore, hA.fifo_.head, 8, hipMemcpyDeviceToHost));

    Args a{};
    a.op = c.op;
    for (size_t i = 0; i < v.size(); ++i) a.v[i] = v[i];
    a.base = hA;
    a.bound = proxy->portChannel(sidA, kBoundDst, kBoundSrc).deviceHandle();
    a.pos = pos;
    for (int i = 0; i < 4; ++i) a.arena[i] = buffers[i].data();
    a.witness = witness->data();
    unsigned grid = 1, lanes = 1;
    if (c.op == OP_ORDER) grid = 2, lanes = 256;
    if (c.op == OP_LAPS) lanes = (unsigned)v[0];
    proxyKernel<<<dim3(grid), dim3(lanes)>>>(a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());  // also the stream the proxy sets the error word on

    rec.handled[1] = proxy->triggersHandled();
    semWords(hA.semaphore_, hB.semaphore_, rec.sem + 4);
    HIPCHECK(hipMemcpy(&rec.htt[0], hA.fifo_.head, 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(&rec.htt[1], hA.fifo_.tail, 8, hipMemcpyDefault));
    HIPCHECK(hipMemcpy(&rec.htt[2], hA.fifo_.tailCache, 8, hipMemcpyDeviceToHost));
    mscclpp::ProxyTrigger ring[kProxyFifo];
    HIPCHECK(hipMemcpy(ring, hA.fifo_.triggers, sizeof ring, hipMemcpyDefault));
    uint64_t hpos = 0;
    HIPCHECK(hipMemcpy(&hpos, pos, 8, hipMemcpyDeviceToHost));
    uint32_t e[4];
    HIPCHECK(hipMemcpy(e, err, 16, hipMemcpyDeviceToHost));
    put(out, &rec, 1);
    put(out, (const char*)ring, sizeof ring);
    put(out, &hpos, rec.npos);
    for (int i = 0; i < 4; ++i) {
      HIPCHECK(hipMemcpy(host.data(), buffers[i].data(), kArenaBytes, hipMemcpyDeviceToHost));
      put(out, (const char*)host.data(), kArenaBytes);
    }
    if (hasWitness) {
      HIPCHECK(hipMemcpy(host.data(), witness->data(), kWitnessBytes, hipMemcpyDeviceToHost));
      put(out, (const char*)host.data(), kWitnessBytes);
    }
    put(out, e, 4);
  }
};
#endif  // !PRIMS_REFERENCE

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]);
    return 2;
  }
  // a lost signal ends in an error record, not in a long spin
  setenv("MSCCLPP_AMD_SPIN_TIMEOUT_MS", "3000", /*overwrite*/ 1);
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  std::vector<Case> cases;
  char buf[2048];
  bool needProxy = false;
  while (std::fgets(buf, sizeof buf, in)) {
    Case c;
    if (buf[0] == '\n' || buf[0] == '#') continue;
    if (!parseLine(buf, c)) {
      std::fprintf(stderr, "bad case line: %s", buf);
      return 2;
    }
    if (const char* why = refusal(c)) {
      std::fprintf(stderr, "case %llu refused (%s): %s", (unsigned long long)c.idx, why, buf);
      return 2;
    }
    needProxy = needProxy || c.op > OP_POLL;
    cases.push_back(std::move(c));
  }
  std::fclose(in);

  (void)needProxy;  // the reference build has refused such a line above
  HIPCHECK(hipSetDevice(0));
  uint64_t* pos;
  HIPCHECK(hipMalloc((void**)&pos, kMaxPos * 8));
  HandBuilt hand;
  hand.init();
  const uint64_t header[4] = {kMagic, cases.size(), kNoPos, 0};
  put(out, header, 4);
  try {
#ifndef PRIMS_REFERENCE
    Loopback loop;
    if (needProxy) loop.init();
#endif
    for (const Case& c : cases) {
      if (c.op <= OP_POLL) {
        hand.run(c, pos, out);
        continue;
      }
#ifndef PRIMS_REFERENCE
      loop.run(c, pos, out);
#endif
    }
#ifndef PRIMS_REFERENCE
    loop.stop();
#endif
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_proxy_primitives: %s\n", e.what());
    return 2;
  }
  if (std::fclose(out) != 0) {
    std::fprintf(stderr, "cannot finish %s\n", argv[2]);
    return 2;
  }
  std::printf("test_proxy_primitives: %zu cases\n", cases.size());
  return 0;
}
