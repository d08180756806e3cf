// NCCL data types and operations as the kernels' codes, and the exact decoding of 16-bit scalars.
#pragma once

#include <cstdint>
#include <cstring>

#include "mscclpp_amd/mscclpp_amd.h"
#include "mscclpp_amd/nccl.h"

namespace mscclpp_amd {
namespace host {

inline int dtypeFromNccl(ncclDataType_t t) {
  switch (t) {
    case ncclFloat16: return MSCCLPP_AMD_F16;
    case ncclBfloat16: return MSCCLPP_AMD_BF16;
    case ncclFloat32: return MSCCLPP_AMD_F32;
    case ncclInt32: return MSCCLPP_AMD_I32;
    case ncclUint32: return MSCCLPP_AMD_U32;
    case ncclFloat8e4m3: return MSCCLPP_AMD_E4M3;  // OCP on gfx950 (datatype_conversion.hpp:29-40)
    case ncclFloat8e5m2: return MSCCLPP_AMD_E5M2;
    case ncclUint8: return MSCCLPP_AMD_U8;  // datatype_conversion.hpp:21-22
    default: return -1;
  }
}
// (element dtype, accumulation dtype) -> reduce-type code; accum < 0 means AUTO = the element type
// (algorithm.cc:47), FP8 may accumulate in half or float (dispatchFp8Accum, common.hpp:89-100).
inline int reduceTypeFromNccl(int ncclDtype, int accum) {
  const int dt = dtypeFromNccl((ncclDataType_t)ncclDtype);
  if (dt < 0 || accum < 0 || accum == ncclDtype) return dt;
  if (dt == MSCCLPP_AMD_E4M3 || dt == MSCCLPP_AMD_E5M2) {
    const int e5 = dt == MSCCLPP_AMD_E5M2;
    if (accum == ncclFloat16) return e5 ? MSCCLPP_AMD_E5M2_ACC_F16 : MSCCLPP_AMD_E4M3_ACC_F16;
    if (accum == ncclFloat32) return e5 ? MSCCLPP_AMD_E5M2_ACC_F32 : MSCCLPP_AMD_E4M3_ACC_F32;
  }
  return -1;  // the reference returns no kernel for other (dtype, accum) pairs
}
inline size_t ncclTypeBytes(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: case ncclFloat8e4m3: case ncclFloat8e5m2: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
  }
}
inline int opFromNccl(ncclRedOp_t op) {
  if (op == ncclSum) return MSCCLPP_AMD_SUM;
  if (op == ncclMin) return MSCCLPP_AMD_MIN;
  return -1;
}
// ncclMax / ncclAvg: the operations of the pull-reduce kernel (kernels/pull_reduce.hip), which is
// no Algorithm of the collection; -1 for every other operation.
inline int pullOpFromNccl(ncclRedOp_t op) {
  if (op == ncclMax) return MSCCLPP_AMD_MAX;
  if (op == ncclAvg) return MSCCLPP_AMD_AVG;
  return -1;
}
// ncclInt64 / ncclUint64 / ncclInt8: carried by the pull-reduce kernel alone, so they have a mapper
// of their own and dtypeFromNccl keeps answering -1 for them -- its other callers (the selector, the
// forced-algorithm entry points, the accumulation-type API) must keep refusing them.
inline int pullOnlyDtypeFromNccl(ncclDataType_t t) {
  switch (t) {
    case ncclInt64: return MSCCLPP_AMD_I64;
    case ncclUint64: return MSCCLPP_AMD_U64;
    case ncclInt8: return MSCCLPP_AMD_I8;
    default: return -1;
  }
}
// ... for which that kernel also computes SUM and MIN (the other types take those to their own
// kernels); -1 for every other operation (ncclProd, PreMulSum handles).
inline int pullOnlyOpFromNccl(ncclRedOp_t op) {
  if (op == ncclSum) return MSCCLPP_AMD_SUM;
  if (op == ncclMin) return MSCCLPP_AMD_MIN;
  return pullOpFromNccl(op);
}
// The exact fp32 value of bf16 / fp16 bits (a PreMulSum scalar given as a host immediate).
inline float bf16BitsToFloat(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}
inline float f16BitsToFloat(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  uint32_t u;
  if (exp == 0x1fu) {
    u = sign | 0x7f800000u | (man << 13);  // inf / NaN
  } else if (exp != 0) {
    u = sign | ((exp + 112u) << 23) | (man << 13);
  } else if (man == 0) {
    u = sign;
  } else {  // subnormal: man * 2^-24, exact in fp32
    float f = (float)man * 5.9604644775390625e-08f;
    std::memcpy(&u, &f, sizeof(u));
    u |= sign;
  }
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}
inline bool bufferRangesOverlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace host
}  // namespace mscclpp_amd
