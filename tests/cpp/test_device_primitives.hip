// The device primitive matrix: copy / put / get at every <Alignment, CopyRemainder>, the packet
// forms of LL16 and LL8, the packet classes, read<T> / write<T> and the semaphore handles, written
// once in the reference's spellings (mscclpp:: names, <mscclpp/...> headers only).
//
//   test_device_primitives <case file> <output file>
//
// The case file is one text line per case (tests/device_primitive_cases.py writes it and holds the
// model).  Per case the host fills three arenas -- L (the channel's src_), R (its dst_: the "peer", a
// second allocation on this device) and K (its packetBuffer_, uncached) -- launches ONE generic
// kernel <<<grid, lanes>>> that calls the named primitive with threadId = the flat id and
// numThreads = grid * lanes, and appends the three arenas and the 4-word error record to the output
// file.  It compares nothing: the Python side judges, bit for bit.
//
// Nothing here waits on something that is not already there: every packet that is read was written
// by the host before the launch, every other slot of a packet arena holds a poison packet with the
// valid flag (a mis-addressed read returns wrong data at once instead of spinning), the semaphore
// cases are loopback with the signal before the wait in the same lane, and every handle carries a
// 20 ms budget.
//
// With -DPRIMS_REFERENCE the same source compiles against the reference's own include tree.  What
// the reference cannot run is compiled out there: the semaphore group (its waits are unbounded), the
// ll16_ / ll8_ unit forms and the 3-argument readOnce (it has none), and the program refuses a copy
// with bytes below the head (the reference's copyHelper underflows there).
#include <hip/hip_runtime.h>

#include <mscclpp/copy_device.hpp>
#include <mscclpp/memory_channel_device.hpp>
#include <mscclpp/packet_device.hpp>
#include <mscclpp/semaphore_device.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

constexpr uint64_t kGuard = 256;
constexpr uint64_t kMaxArena = 160 << 10;
constexpr uint32_t kFillWord = 0xA5A5A5A5u;
constexpr uint64_t kBudgetTicks = 2'000'000;  // 20 ms
constexpr uint64_t kMagic = 0x314D495250564544ull;

enum Op : int {
  OP_COPY, OP_PUT2, OP_PUT1, OP_GET2, OP_GET1,
  OP_PUTPACKETS2, OP_PUTPACKETS1, OP_UNPACKPACKETS2, OP_UNPACKPACKETS1, OP_UNPACKPACKET, OP_COPYTOPACKETS,
  OP_COPYFROMPACKETS, OP_PUT_UNIT, OP_TRY_UNIT,
  OP_PKT_CTOR, OP_PKT_WRITE3, OP_PKT_WRITE64, OP_PKT_WRITE2, OP_PKT_CLEAR, OP_READONCE2, OP_READONCE3, OP_PKT_READ,
  OP_RW, OP_SEM_D2D, OP_SEM_BASE, OP_SEM_H2D, OP_COUNT
};
const char* const kOpNames[OP_COUNT] = {
    "copy", "put2", "put1", "get2", "get1",
    "putPackets2", "putPackets1", "unpackPackets2", "unpackPackets1", "unpackPacket", "copyToPackets",
    "copyFromPackets", "put_unit", "try_unit",
    "pkt_ctor", "pkt_write3", "pkt_write64", "pkt_write2", "pkt_clear", "readOnce2", "readOnce3", "pkt_read",
    "rw", "sem_d2d", "sem_base", "sem_h2d"};

struct Args {
  int op, p0, p1;
  uint32_t flag;
  uint64_t toff, ooff, bytes;
  mscclpp::MemoryChannelDeviceHandle ch;
  mscclpp::BaseMemoryChannelDeviceHandle base;
  mscclpp::Host2DeviceSemaphoreDeviceHandle h2d;
  char *L, *R, *K;  // the handle's src_, dst_, packetBuffer_
};

// ---- Group A ----------------------------------------------------------------------------------
template <int A, bool Rm>
__device__ void copyGroup(const Args& a, uint32_t tid, uint32_t nt) {
  mscclpp::MemoryChannelDeviceHandle ch = a.ch;
  switch (a.op) {
    case OP_COPY:
      mscclpp::copy<A, Rm>(a.R + a.toff, a.L + a.ooff, a.bytes, tid, nt);
      break;
    case OP_PUT2:
      ch.put<A, Rm>(a.toff, a.ooff, a.bytes, tid, nt);
      break;
    case OP_PUT1:
      ch.put<A, Rm>(a.toff, a.bytes, tid, nt);
      break;
    case OP_GET2:
      ch.get<A, Rm>(a.toff, a.ooff, a.bytes, tid, nt);
      break;
    case OP_GET1:
      ch.get<A, Rm>(a.toff, a.bytes, tid, nt);
      break;
  }
}

// ---- Group B and the packet classes ---------------------------------------------------------------
__device__ inline void storeFields(uint32_t* out, const mscclpp::LL16Packet& p) {
  out[0] = p.data1;
  out[1] = p.flag1;
  out[2] = p.data2;
  out[3] = p.flag2;
}
__device__ inline void storeFields(uint32_t* out, const mscclpp::LL8Packet& p) {
  out[0] = p.data;
  out[1] = p.flag;
}
__device__ inline mscclpp::LL16Packet construct(mscclpp::LL16Packet*, const uint32_t* v, uint32_t flag) {
  uint2 val;
  val.x = v[0];
  val.y = v[1];
  return mscclpp::LL16Packet(val, flag);
}
__device__ inline mscclpp::LL8Packet construct(mscclpp::LL8Packet*, const uint32_t* v, uint32_t flag) {
  return mscclpp::LL8Packet(v[0], flag);
}
__device__ inline void write3(mscclpp::LL16Packet* p, const uint32_t* v, uint32_t flag) { p->write(v[0], v[1], flag); }
__device__ inline void write3(mscclpp::LL8Packet* p, const uint32_t* v, uint32_t flag) { p->write(v[0], flag); }

// readOnce in the reference's spelling: true while the packet is NOT ready.  Record: ret, payload.
__device__ inline void readOnceRef(const mscclpp::LL16Packet* p, uint32_t flag, uint32_t* out) {
  uint2 d;
  d.x = d.y = 0;
  const bool r = p->readOnce(flag, d);
  out[0] = r;
  out[1] = d.x;
  out[2] = d.y;
}
__device__ inline void readOnceRef(const mscclpp::LL8Packet* p, uint32_t flag, uint32_t* out) {
  uint32_t d = 0;
  const bool r = p->readOnce(flag, d);
  out[0] = r;
  out[1] = d;
}

template <typename P>
__device__ void packetGroup(const Args& a, uint32_t tid, uint32_t nt) {
  using Payload = typename P::Payload;
  mscclpp::MemoryChannelDeviceHandle ch = a.ch;
  switch (a.op) {
    case OP_PUTPACKETS2:
      ch.putPackets<P>(a.toff, a.ooff, a.bytes, tid, nt, a.flag);
      break;
    case OP_PUTPACKETS1:
      ch.putPackets<P>(a.toff, a.bytes, tid, nt, a.flag);
      break;
    case OP_UNPACKPACKETS2:
      ch.unpackPackets<P>(a.toff, a.ooff, a.bytes, tid, nt, a.flag);
      break;
    case OP_UNPACKPACKETS1:
      ch.unpackPackets<P>(a.toff, a.bytes, tid, nt, a.flag);
      break;
    case OP_UNPACKPACKET:
      for (uint64_t i = tid; i < a.bytes / sizeof(Payload); i += nt)
        reinterpret_cast<Payload*>(a.L + a.ooff)[i] = ch.unpackPacket<P>(a.toff / sizeof(P) + i, a.flag);
      break;
    case OP_COPYTOPACKETS:
      mscclpp::copyToPackets<P>(a.K + a.toff, a.L + a.ooff, a.bytes, tid, nt, a.flag);
      break;
    case OP_COPYFROMPACKETS:
      mscclpp::copyFromPackets<P>(a.L + a.ooff, a.K + a.toff, a.bytes, tid, nt, a.flag);
      break;
    case OP_PKT_READ:
      for (uint64_t i = tid; i < a.bytes / sizeof(Payload); i += nt)
        reinterpret_cast<Payload*>(a.L + a.ooff)[i] = reinterpret_cast<const P*>(a.K + a.toff)[i].read(a.flag);
      break;
    // one lane per step from here on
    case OP_PKT_CTOR:
      if (tid == 0) {
        P p = construct(static_cast<P*>(nullptr), reinterpret_cast<const uint32_t*>(a.L + a.ooff), a.flag);
        storeFields(reinterpret_cast<uint32_t*>(a.K + a.toff), p);
      }
      break;
    case OP_PKT_WRITE3:
      if (tid == 0) write3(reinterpret_cast<P*>(a.K + a.toff), reinterpret_cast<const uint32_t*>(a.L + a.ooff), a.flag);
      break;
    case OP_PKT_CLEAR:
      if (tid == 0) reinterpret_cast<P*>(a.K + a.toff)->clear();
      break;
    case OP_READONCE2:
      if (tid == 0) {
        constexpr int kRec = 1 + sizeof(Payload) / 4;
        for (int k = 0; k < 4; ++k)
          readOnceRef(reinterpret_cast<const P*>(a.K + a.toff) + k, a.flag,
                      reinterpret_cast<uint32_t*>(a.L + a.ooff) + kRec * k);
      }
      break;
  }
}

// the LL16-only forms
__device__ void ll16Group(const Args& a, uint32_t tid) {
  if (tid != 0) return;
  mscclpp::LL16Packet* p = reinterpret_cast<mscclpp::LL16Packet*>(a.K + a.toff);
  const uint32_t* v = reinterpret_cast<const uint32_t*>(a.L + a.ooff);
  switch (a.op) {
    case OP_PKT_WRITE64:
      p->write((uint64_t)v[0] | ((uint64_t)v[1] << 32), a.flag);
      break;
    case OP_PKT_WRITE2: {
      uint2 val;
      val.x = v[0];
      val.y = v[1];
      p->write(val, a.flag);
      break;
    }
#ifndef PRIMS_REFERENCE
    case OP_READONCE3:
      // this library's own form: true when the packet IS ready
      for (int k = 0; k < 4; ++k) {
        uint32_t v1 = 0, v2 = 0;
        const bool r = p[k].readOnce(a.flag, v1, v2);
        uint32_t* out = reinterpret_cast<uint32_t*>(a.L + a.ooff) + 3 * k;
        out[0] = r;
        out[1] = v1;
        out[2] = v2;
      }
      break;
#endif
  }
}

#ifndef PRIMS_REFERENCE
// The hot kernels' forms: one unit = 16 payload bytes = 32 packet bytes.  try_unit stores the
// payload it saw in L and its verdict per unit in R.
__device__ void unitGroup(const Args& a, uint32_t tid, uint32_t nt) {
  const auto pk = mscclpp::make_rsrc(a.K + a.toff);
  mscclpp::u32x4* data = reinterpret_cast<mscclpp::u32x4*>(a.L + a.ooff);
  for (uint64_t i = tid; i < a.bytes / 16; i += nt) {
    const uint32_t pbyte = (uint32_t)(32 * i);
    if (a.op == OP_PUT_UNIT) {
      if (a.p0 == 16)
        mscclpp::ll16_put_unit<mscclpp::kSystem>(pk, pbyte, data[i], a.flag);
      else
        mscclpp::ll8_put_unit<mscclpp::kSystem>(pk, pbyte, data[i], a.flag);
    } else {
      mscclpp::u32x4 w;
      const bool ok = a.p0 == 16 ? mscclpp::ll16_try_unit<mscclpp::kSystem>(pk, pbyte, a.flag, w)
                                 : mscclpp::ll8_try_unit(pk, pbyte, a.flag, w);
      data[i] = w;
      reinterpret_cast<uint32_t*>(a.R)[i] = ok;
    }
  }
}

// ---- Group E: loopback, the same lane signals before it waits ----------------------------------------
template <typename H>
__device__ void d2dSteps(H& h, mscclpp::MemoryDevice2DeviceSemaphoreDeviceHandle& s, uint64_t* out) {
  out[0] = h.poll();
  out[1] = s.loadExpectedInbound();
  h.signal();
  out[2] = h.poll();
  out[3] = s.loadExpectedInbound();
  out[4] = h.poll();
  h.signal();
  h.signal();
  h.signal();
  h.wait();
  h.wait();
  h.wait();
  out[5] = s.loadInbound();
  out[6] = s.loadExpectedInbound();
  h.relaxedSignal();
  h.relaxedWait();
  out[7] = s.loadInbound();
  out[8] = s.loadExpectedInbound();
  out[9] = s.loadInboundRelaxed();
}
__device__ void semGroup(const Args& a, uint32_t tid) {
  if (tid != 0) return;
  uint64_t* out = reinterpret_cast<uint64_t*>(a.L);
  if (a.op == OP_SEM_D2D) {
    mscclpp::MemoryDevice2DeviceSemaphoreDeviceHandle s = a.ch.semaphore_;
    d2dSteps(s, s, out);
  } else if (a.op == OP_SEM_BASE) {
    mscclpp::BaseMemoryChannelDeviceHandle b = a.base;
    d2dSteps(b, b.semaphore_, out);
  } else {
    mscclpp::Host2DeviceSemaphoreDeviceHandle h = a.h2d;  // the host has set the token to 2
    h.wait();
    out[0] = h.poll();
    out[1] = h.poll();
    out[2] = h.loadExpectedInbound();
    out[3] = h.loadInbound();
  }
}
#endif  // !PRIMS_REFERENCE

// ---- Group D ----------------------------------------------------------------------------------------
template <typename T>
__device__ T rwValue(uint32_t t);
template <>
__device__ uint32_t rwValue<uint32_t>(uint32_t t) {
  return 0xC0DE0000u + t;
}
template <>
__device__ uint64_t rwValue<uint64_t>(uint32_t t) {
  return ((uint64_t)(0xFACE0000u + t) << 32) | (3 * t + 1);
}
template <>
__device__ uint2 rwValue<uint2>(uint32_t t) {
  uint2 v;
  v.x = 0xAB000000u + t;
  v.y = 0xCD000000u + t;
  return v;
}
template <typename T>
__device__ void rwGroup(const Args& a, uint32_t tid) {
  if (tid >= a.bytes) return;  // `bytes` is the element count here
  mscclpp::MemoryChannelDeviceHandle ch = a.ch;
  T* out = reinterpret_cast<T*>(a.L);
  if (a.p1) {
    ch.write<T>(a.toff + tid, rwValue<T>(tid));
    out[tid] = ch.read<T>(a.ooff + tid);
  } else {
    mscclpp::write<T>(a.R, a.toff + tid, rwValue<T>(tid));
    out[tid] = mscclpp::read<T>(a.R, a.ooff + tid);
  }
}

__global__ void __launch_bounds__(1024) primKernel(Args a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nt = gridDim.x * blockDim.x;
  if (a.op <= OP_GET1) {
    switch (a.p0 * 2 + a.p1) {
      case 4 * 2 + 1: copyGroup<4, true>(a, tid, nt); break;
      case 4 * 2 + 0: copyGroup<4, false>(a, tid, nt); break;
      case 8 * 2 + 1: copyGroup<8, true>(a, tid, nt); break;
      case 8 * 2 + 0: copyGroup<8, false>(a, tid, nt); break;
      case 16 * 2 + 1: copyGroup<16, true>(a, tid, nt); break;
      case 16 * 2 + 0: copyGroup<16, false>(a, tid, nt); break;
    }
  } else if (a.op == OP_PUT_UNIT || a.op == OP_TRY_UNIT) {
#ifndef PRIMS_REFERENCE
    unitGroup(a, tid, nt);
#endif
  } else if (a.op == OP_PKT_WRITE64 || a.op == OP_PKT_WRITE2 || a.op == OP_READONCE3) {
    ll16Group(a, tid);
  } else if (a.op < OP_RW) {
    if (a.p0 == 16)
      packetGroup<mscclpp::LL16Packet>(a, tid, nt);
    else
      packetGroup<mscclpp::LL8Packet>(a, tid, nt);
  } else if (a.op == OP_RW) {
    if (a.p0 == 4)
      rwGroup<uint32_t>(a, tid);
    else if (a.p0 == 8)
      rwGroup<uint64_t>(a, tid);
    else
      rwGroup<uint2>(a, tid);
  } else {
#ifndef PRIMS_REFERENCE
    semGroup(a, tid);
#endif
  }
}

// ---- host ---------------------------------------------------------------------------------------------
struct Case {
  long idx;
  int op;
  long long p0, p1, grid, lanes, toff, ooff, bytes, flag, size[3], init[3], imgoff, imgcount, nstale, stale[4], ref;
};

uint32_t pat(uint32_t idx, uint32_t arena, uint32_t j) {
  uint32_t x = (j + 1u) * 2654435761u + (idx * 4u + arena + 1u) * 0x9E3779B9u;
  x ^= x >> 15;
  return x;
}

bool parseLine(const std::string& line, Case& c) {
  char name[64];
  int n = 0;
  if (std::sscanf(line.c_str(), "%ld %63s%n", &c.idx, name, &n) != 2) return false;
  c.op = -1;
  for (int i = 0; i < OP_COUNT; ++i)
    if (!std::strcmp(name, kOpNames[i])) c.op = i;
  long long v[22];
  const char* p = line.c_str() + n;
  for (int i = 0; i < 22; ++i) {
    char* end;
    v[i] = std::strtoll(p, &end, 10);
    if (end == p) return false;
    p = end;
  }
  c.p0 = v[0], c.p1 = v[1], c.grid = v[2], c.lanes = v[3], c.toff = v[4], c.ooff = v[5], c.bytes = v[6], c.flag = v[7];
  for (int i = 0; i < 3; ++i) c.size[i] = v[8 + i], c.init[i] = v[11 + i];
  c.imgoff = v[14], c.imgcount = v[15], c.nstale = v[16];
  for (int i = 0; i < 4; ++i) c.stale[i] = v[17 + i];
  c.ref = v[21];
  return c.op >= 0;
}

// What the host can refuse before a launch: geometry outside the allocations.  (The table's own
// guard bands are asserted by the Python side; this only keeps a bad line inside the arenas.)
bool inBounds(const Case& c) {
  for (int i = 0; i < 3; ++i)
    if (c.size[i] < (long long)(2 * kGuard) || c.size[i] > (long long)kMaxArena || c.size[i] % 256) return false;
  if (c.grid < 1 || c.grid > 64 || c.lanes < 1 || c.lanes > 1024) return false;
  if (c.toff < 0 || c.ooff < 0 || c.bytes < 0 || c.imgoff < 0 || c.imgcount < 0 || c.nstale < 0 || c.nstale > 4)
    return false;
  // no form moves more than 2 packet bytes per payload byte, 8 bytes per element (Group D), or
  // reaches past the image
  const long long off = c.toff > c.ooff ? c.toff : c.ooff;
  const long long reach = c.op == OP_RW ? 8 * (off + c.bytes) : off + 2 * c.bytes + 64;
  if ((long long)kGuard + reach + (long long)kGuard > (long long)kMaxArena) return false;
  if ((long long)kGuard + c.imgoff + c.imgcount * 16 + (long long)kGuard > (long long)kMaxArena) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  std::vector<Case> cases;
  char buf[1024];
  while (std::fgets(buf, sizeof buf, in)) {
    Case c;
    if (buf[0] == '\n' || buf[0] == '#') continue;
    if (!parseLine(buf, c) || !inBounds(c)) {
      std::fprintf(stderr, "bad case line: %s", buf);
      return 2;
    }
    cases.push_back(c);
  }
  std::fclose(in);

  char *L, *R, *K;
  uint64_t* tokens;  // [0] d2d inbound, [1] d2d expected, [2] h2d inbound, [3] h2d expected
  uint32_t* err;
  HIPCHECK(hipMalloc(&L, kMaxArena));
  HIPCHECK(hipMalloc(&R, kMaxArena));
  HIPCHECK(hipExtMallocWithFlags((void**)&K, kMaxArena, hipDeviceMallocUncached));
  HIPCHECK(hipExtMallocWithFlags((void**)&tokens, 256, hipDeviceMallocUncached));
  HIPCHECK(hipExtMallocWithFlags((void**)&err, 256, hipDeviceMallocUncached));
  char* arena[3] = {L, R, K};
  for (int i = 0; i < 3; ++i) {
    if ((uintptr_t)arena[i] % 256) {
      std::fprintf(stderr, "arena %d is not 256-byte aligned\n", i);
      return 2;
    }
    HIPCHECK(hipMemset(arena[i], 0xA5, kMaxArena));
  }

  // Handles, built on the host as a user of the reference builds them.
  mscclpp::MemoryDevice2DeviceSemaphoreDeviceHandle sem{};
  sem.inboundToken = tokens;
  sem.remoteInboundToken = tokens;  // loopback
  sem.expectedInboundToken = tokens + 1;
  mscclpp::Host2DeviceSemaphoreDeviceHandle h2d{};
  h2d.inboundToken = tokens + 2;
  h2d.expectedInboundToken = tokens + 3;
#ifndef PRIMS_REFERENCE
  sem.budget = h2d.budget = kBudgetTicks;
  sem.err = h2d.err = err;
#endif
  const mscclpp::MemoryChannelDeviceHandle channel(sem, R + kGuard, L + kGuard, K + kGuard);
  const mscclpp::BaseMemoryChannelDeviceHandle baseChannel(sem);

  uint64_t header[8] = {kMagic, cases.size(), (uint64_t)(uintptr_t)L, (uint64_t)(uintptr_t)R, (uint64_t)(uintptr_t)K,
                        kGuard, 0, 0};
  std::fwrite(header, sizeof header, 1, out);

  std::vector<uint32_t> host(kMaxArena / 4);
  for (const Case& c : cases) {
#ifdef PRIMS_REFERENCE
    if (!c.ref) {
      std::fprintf(stderr, "case %ld (%s) is not one the reference's headers can run\n", c.idx, kOpNames[c.op]);
      return 2;
    }
    if (c.op <= OP_GET1) {
      // the reference's copyHelper computes numInt - nFirstInt unsigned: refuse bytes below the head
      const uintptr_t d = (uintptr_t)(c.op == OP_GET2 || c.op == OP_GET1 ? L : R) + kGuard + c.toff;
      const uint64_t headInts = ((d + c.p0 - 1) / c.p0 * c.p0 - d) / 4;
      if ((uint64_t)c.bytes / 4 < headInts) {
        std::fprintf(stderr, "case %ld: bytes below the head, outside the reference's contract\n", c.idx);
        return 2;
      }
    }
#endif
    for (int a = 0; a < 3; ++a) {
      const size_t words = c.size[a] / 4;
      for (size_t j = 0; j < words; ++j) {
        if (c.init[a] == 0)
          host[j] = kFillWord;
        else if (c.init[a] == 1)
          host[j] = pat((uint32_t)c.idx, a, (uint32_t)j);
        else
          host[j] = (j & 1) ? (uint32_t)c.flag : kFillWord;  // poison packets, LL16 and LL8 alike
      }
      if (c.init[a] == 2) {
        const size_t first = (kGuard + c.imgoff) / 4;
        const size_t payloadWords = c.imgcount * (c.p0 == 16 ? 2 : 1);
        for (size_t j = 0; j < payloadWords; ++j) host[first + 2 * j] = pat((uint32_t)c.idx, 3, (uint32_t)j);
        for (int s = 0; s < c.nstale; ++s) host[first + c.stale[s]] = (uint32_t)c.flag - 1u;
      }
      HIPCHECK(hipMemcpy(arena[a], host.data(), c.size[a], hipMemcpyHostToDevice));
    }
    uint64_t tok[4] = {0, 0, c.op == OP_SEM_H2D ? 2ull : 0ull, 0};
    uint32_t zero[4] = {0, 0, 0, 0};
    HIPCHECK(hipMemcpy(tokens, tok, sizeof tok, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(err, zero, sizeof zero, hipMemcpyHostToDevice));

    Args a;
    a.op = c.op, a.p0 = (int)c.p0, a.p1 = (int)c.p1, a.flag = (uint32_t)c.flag;
    a.toff = c.toff, a.ooff = c.ooff, a.bytes = c.bytes;
    a.ch = channel, a.base = baseChannel, a.h2d = h2d;
    a.L = L + kGuard, a.R = R + kGuard, a.K = K + kGuard;
    primKernel<<<dim3((unsigned)c.grid), dim3((unsigned)c.lanes)>>>(a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());

    uint32_t rec[8] = {(uint32_t)c.idx, (uint32_t)c.size[0], (uint32_t)c.size[1], (uint32_t)c.size[2], 0, 0, 0, 0};
    HIPCHECK(hipMemcpy(rec + 4, err, 16, hipMemcpyDeviceToHost));
    std::fwrite(rec, sizeof rec, 1, out);
    for (int i = 0; i < 3; ++i) {
      HIPCHECK(hipMemcpy(host.data(), arena[i], c.size[i], hipMemcpyDeviceToHost));
      std::fwrite(host.data(), 1, c.size[i], out);
    }
  }
  if (std::fclose(out) != 0) {
    std::fprintf(stderr, "cannot finish %s\n", argv[2]);
    return 2;
  }
  HIPCHECK(hipFree(L));
  HIPCHECK(hipFree(R));
  HIPCHECK(hipFree(K));
  HIPCHECK(hipFree(tokens));
  HIPCHECK(hipFree(err));
  std::printf("test_device_primitives: %zu cases\n", cases.size());
  return 0;
}
