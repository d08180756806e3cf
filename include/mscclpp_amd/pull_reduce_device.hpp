// Arithmetic of the pull-reduce kernel (kernels/pull_reduce.hip), over packed 32-bit words: ncclMax /
// ncclAvg of the eight element types the SUM / MIN kernels carry, and all four operations of int64,
// uint64 and int8.  The reference carries SUM and MIN of its own types only (reduce_device.hpp
// restates those bit for bit), so what follows is defined here, not restated:
//
//  * operands are taken in RANK order 0, 1, ..., n - 1 on whichever rank computes the element, so
//    Reduce, ReduceScatter and AllReduce of the same inputs give the same bits;
//  * MAX, float types: every element decodes exactly to fp32; acc = x_0, then for k = 1 .. n - 1
//    `if (isnan(acc) || x_k > acc) acc = x_k`.  The result is the raw bits of the winning element --
//    a selection, never re-encoded: NaN only if every rank's element is NaN (then rank n - 1's bits),
//    and of equal values (+0 / -0) the lowest rank's bits;
//  * MAX, integers: signed compare for int32, unsigned for uint32 and uint8;
//  * AVG, float types: s = the fp32 sum of the decoded elements in rank order (one RNE add each),
//    r = s * inv_n with inv_n = 1.0f / (float)n computed by the host, and r rounded ONCE to the
//    element type: fp32 as is, (_Float16)r, (__bf16)r (RNE, none of the SUM path's clipping),
//    fp8x4_encode (saturating, RNE);
//  * AVG, integers: the exact sum (int64 / uint64 / uint32 for int32 / uint32 / uint8) divided by n,
//    truncating toward zero;
//  * int64 / uint64 / int8 (kI64, kU64, kI8; SUM and MIN too, which the other types take to their own
//    kernels).  Every one of these operations is exact, so the rank order changes no bit:
//      SUM: two's-complement wrap at the element width (the reference's rule for int32 / uint8); an
//           int8 sum is per byte, no carry crosses a byte boundary;
//      MIN / MAX: signed compare for int64 and int8, unsigned for uint64, over all 64 bits;
//      AVG: the EXACT sum divided by n, truncating toward zero -- not the wrapped sum divided by n.
//           int8: the sum of 8 values fits 16 bits.  64-bit: the sum is kept as a 96-bit two's-
//           complement value {hi, lo} (it needs 67 bits), its magnitude M = hi * 2^64 + lo has
//           hi < n, and with c1 = floor(2^64 / n), c2 = 2^64 mod n (constants per n)
//           M / n = hi * c1 + lo / n + (hi * c2 + lo % n) / n: one 64-bit divide by a constant per
//           element; the sign is put back afterwards.
//  * PreMulSum (ncclRedOpCreatePreMulSum; kPullPreMulSum), fp16 / bf16 / fp32: every rank k has a
//    scalar s_k of its own, given in the element type; rank k's operand is multiplied by rank k's
//    scalar (NCCL's rule: the input is pre-multiplied locally), so the scalars may differ between
//    ranks.  x_k and s_k decode exactly to fp32; p_k = x_k * s_k is ONE fp32 RNE multiply and a value
//    of its own (no multiply fuses with the following add: fp32_product); acc = p_0, then
//    acc = acc + p_k for k = 1 .. n - 1, one fp32 RNE add each; acc is rounded ONCE to the element
//    type exactly as AVG's result is (fp32 as is, (_Float16)acc, (__bf16)acc).  NCCL multiplies fp16
//    and bf16 operands in half precision; the fp32 product here is the more precise one.
#pragma once

#include "reduce_device.hpp"

namespace mscclpp_amd {

// Operation codes of the pull-reduce path only (MSCCLPP_AMD_MAX / MSCCLPP_AMD_AVG); the <DT, OP>
// kernels of ROp keep their range.
enum PullOp : int { kPullMax = 2, kPullAvg = 3, kPullPreMulSum = 5 };  // (4 stays refused)

// PreMulSum: the three float types a framework passes (bar double).
__host__ __device__ constexpr bool pull_premul_type(int dt) { return dt == kF16 || dt == kBF16 || dt == kF32; }

// int64 / uint64 / int8: carried by this path alone, with kSum and kMin as well.
__host__ __device__ constexpr bool pull_only_type(int dt) { return dt == kI64 || dt == kU64 || dt == kI8; }

// The reduce types the path carries: the eight element types and the three above, accumulated as
// defined above.
__host__ __device__ constexpr bool pull_reduce_carries(int dt) {
  return dt == kF16 || dt == kBF16 || dt == kF32 || dt == kI32 || dt == kU32 || dt == kE4M3 || dt == kE5M2 ||
         dt == kU8 || pull_only_type(dt);
}
// MAX / AVG for every carried type; SUM / MIN exactly for the three types that have no other kernel;
// PreMulSum for the three float types.
__host__ __device__ constexpr bool pull_reduce_takes(int dt, int op) {
  return pull_reduce_carries(dt) &&
         (op == kPullMax || op == kPullAvg || ((op == kSum || op == kMin) && pull_only_type(dt)) ||
          (op == kPullPreMulSum && pull_premul_type(dt)));
}
// 32-bit words an accumulator consumes at a time: 2 for the 64-bit types (first / next take and
// word() returns a uint64_t), 1 for every other type.
__host__ __device__ constexpr int pull_acc_words(int dt) { return dt == kI64 || dt == kU64 ? 2 : 1; }

__device__ __forceinline__ bool max_takes(float acc, float x) { return acc != acc || x > acc; }

__device__ __forceinline__ float f16_to_f32(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }

// Divide by the rank count (2 .. 8): constant divisors, so no 64-bit software divide per element.
template <typename T>
__device__ __forceinline__ T div_ranks(T s, int n) {
  switch (n) {
    case 2: return s / 2;
    case 3: return s / 3;
    case 4: return s / 4;
    case 5: return s / 5;
    case 6: return s / 6;
    case 7: return s / 7;
    default: return s / 8;
  }
}

// The fp32 product of the float AVG as a value of its own.  Without this, `(_Float16)(s * inv)` is
// selected as one v_fma_mixlo_f16 (also under `#pragma clang fp contract(off)`), which rounds the
// exact product straight to fp16 instead of to fp32 first, and adds +0, which turns -0 into +0.
// (An empty asm statement: no instruction, only the register constraint.)
__device__ __forceinline__ float fp32_product(float s, float inv) {
  float r = s * inv;
  asm("" : "+v"(r));
  return r;
}

// The fp32 sum of PreMulSum as a value of its own before it is rounded to the element type, for the
// same reason: no conversion is selected together with the add that produced it.
__device__ __forceinline__ float fp32_value(float r) {
  asm("" : "+v"(r));
  return r;
}

// Two fp32 products at once (v_pk_mul_f32), each a value of its own as in fp32_product: the halves of
// a 16-bit pair times one scalar (PreMulSum).
__device__ __forceinline__ float2_t fp32_product2(float2_t x, float s) {
  float2_t r = x * s;
  asm("" : "+v"(r));
  return r;
}

// One word's accumulator.  first(w): rank 0's word; next(w): the following rank's; word(n, inv_n):
// the result.
template <int DT, int OP>
struct PullAcc;

template <int DT>
struct PullAcc<DT, kPullMax> {
  uint32_t a;
  __device__ __forceinline__ void first(uint32_t w) { a = w; }
  __device__ __forceinline__ void next(uint32_t w) {
    if constexpr (DT == kI32) {
      a = (int32_t)w > (int32_t)a ? w : a;
    } else if constexpr (DT == kU32) {
      a = w > a ? w : a;
    } else if constexpr (DT == kU8) {
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 32; k += 8) {
        const uint32_t x = (a >> k) & 0xffu, y = (w >> k) & 0xffu;
        r |= (y > x ? y : x) << k;
      }
      a = r;
    } else if constexpr (DT == kF32) {
      a = max_takes(__builtin_bit_cast(float, a), __builtin_bit_cast(float, w)) ? w : a;
    } else if constexpr (DT == kF16) {
      const uint32_t m = (max_takes(f16_to_f32(a & 0xffffu), f16_to_f32(w & 0xffffu)) ? 0x0000ffffu : 0u) |
                         (max_takes(f16_to_f32(a >> 16), f16_to_f32(w >> 16)) ? 0xffff0000u : 0u);
      a = (w & m) | (a & ~m);
    } else if constexpr (DT == kBF16) {
      const uint32_t m = (max_takes(bf16_lo(a), bf16_lo(w)) ? 0x0000ffffu : 0u) |
                         (max_takes(bf16_hi(a), bf16_hi(w)) ? 0xffff0000u : 0u);
      a = (w & m) | (a & ~m);
    } else {
      const float4_t x = fp8x4_decode<DT == kE5M2>(a), y = fp8x4_decode<DT == kE5M2>(w);
      const uint32_t m = (max_takes(x.x, y.x) ? 0x000000ffu : 0u) | (max_takes(x.y, y.y) ? 0x0000ff00u : 0u) |
                         (max_takes(x.z, y.z) ? 0x00ff0000u : 0u) | (max_takes(x.w, y.w) ? 0xff000000u : 0u);
      a = (w & m) | (a & ~m);
    }
  }
  __device__ __forceinline__ uint32_t word(int, float) const { return a; }
};

template <>
struct PullAcc<kF32, kPullAvg> {
  float s;
  __device__ __forceinline__ void first(uint32_t w) { s = __builtin_bit_cast(float, w); }
  __device__ __forceinline__ void next(uint32_t w) {
    s = s + __builtin_bit_cast(float, w);
  }
  __device__ __forceinline__ uint32_t word(int, float inv) const {
    return __builtin_bit_cast(uint32_t, fp32_product(s, inv));
  }
};

template <>
struct PullAcc<kF16, kPullAvg> {
  float lo, hi;
  __device__ __forceinline__ void first(uint32_t w) {
    lo = f16_to_f32(w & 0xffffu);
    hi = f16_to_f32(w >> 16);
  }
  __device__ __forceinline__ void next(uint32_t w) {
    lo = lo + f16_to_f32(w & 0xffffu);
    hi = hi + f16_to_f32(w >> 16);
  }
  __device__ __forceinline__ uint32_t word(int, float inv) const {
    const _Float16 l = (_Float16)fp32_product(lo, inv), h = (_Float16)fp32_product(hi, inv);
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  }
};

template <>
struct PullAcc<kBF16, kPullAvg> {
  float lo, hi;
  __device__ __forceinline__ void first(uint32_t w) {
    lo = bf16_lo(w);
    hi = bf16_hi(w);
  }
  __device__ __forceinline__ void next(uint32_t w) {
    lo = lo + bf16_lo(w);
    hi = hi + bf16_hi(w);
  }
  __device__ __forceinline__ uint32_t word(int, float inv) const {
    const __bf16 l = (__bf16)fp32_product(lo, inv), h = (__bf16)fp32_product(hi, inv);
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  }
};

// ---- PreMulSum: first / next also take the operand's rank's scalar ---------------------------------
// Every product goes through fp32_product, so it is rounded to fp32 before the add that follows.
template <>
struct PullAcc<kF32, kPullPreMulSum> {
  float s;
  __device__ __forceinline__ void first(uint32_t w, float sc) { s = fp32_product(__builtin_bit_cast(float, w), sc); }
  __device__ __forceinline__ void next(uint32_t w, float sc) { s = s + fp32_product(__builtin_bit_cast(float, w), sc); }
  __device__ __forceinline__ uint32_t word(int, float) const { return __builtin_bit_cast(uint32_t, s); }
};

template <>
struct PullAcc<kF16, kPullPreMulSum> {
  float2_t a;  // {low half, high half}
  __device__ __forceinline__ void first(uint32_t w, float sc) {
    a = fp32_product2(float2_t{f16_to_f32(w & 0xffffu), f16_to_f32(w >> 16)}, sc);
  }
  __device__ __forceinline__ void next(uint32_t w, float sc) {
    a = a + fp32_product2(float2_t{f16_to_f32(w & 0xffffu), f16_to_f32(w >> 16)}, sc);
  }
  __device__ __forceinline__ uint32_t word(int, float) const {
    const _Float16 l = (_Float16)fp32_value(a.x), h = (_Float16)fp32_value(a.y);
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  }
};

template <>
struct PullAcc<kBF16, kPullPreMulSum> {
  float2_t a;  // {low half, high half}
  __device__ __forceinline__ void first(uint32_t w, float sc) { a = fp32_product2(float2_t{bf16_lo(w), bf16_hi(w)}, sc); }
  __device__ __forceinline__ void next(uint32_t w, float sc) {
    a = a + fp32_product2(float2_t{bf16_lo(w), bf16_hi(w)}, sc);
  }
  __device__ __forceinline__ uint32_t word(int, float) const {
    const __bf16 l = (__bf16)fp32_value(a.x), h = (__bf16)fp32_value(a.y);
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
  }
};

// A rank's scalar, given as one element of the element type, decoded exactly to fp32 (the device-
// resident form of ncclRedOpCreatePreMulSum: read when the kernel runs).
template <int DT>
__device__ __forceinline__ float premul_scalar_at(const void* p) {
  if constexpr (DT == kF32) {
    return *(const float*)p;
  } else if constexpr (DT == kF16) {
    return f16_to_f32(*(const uint16_t*)p);
  } else {
    return bf16_lo(*(const uint16_t*)p);
  }
}

template <int DT>
struct PullAccFp8Avg {
  float4_t s;
  __device__ __forceinline__ void first(uint32_t w) { s = fp8x4_decode<DT == kE5M2>(w); }
  __device__ __forceinline__ void next(uint32_t w) {
    s = s + fp8x4_decode<DT == kE5M2>(w);
  }
  __device__ __forceinline__ uint32_t word(int, float inv) const {
    return fp8x4_encode<DT == kE5M2>(
        float4_t{fp32_product(s.x, inv), fp32_product(s.y, inv), fp32_product(s.z, inv), fp32_product(s.w, inv)});
  }
};
template <>
struct PullAcc<kE4M3, kPullAvg> : PullAccFp8Avg<kE4M3> {};
template <>
struct PullAcc<kE5M2, kPullAvg> : PullAccFp8Avg<kE5M2> {};

template <>
struct PullAcc<kI32, kPullAvg> {
  int64_t s;
  __device__ __forceinline__ void first(uint32_t w) { s = (int32_t)w; }
  __device__ __forceinline__ void next(uint32_t w) { s += (int32_t)w; }
  __device__ __forceinline__ uint32_t word(int n, float) const { return (uint32_t)(int32_t)div_ranks<int64_t>(s, n); }
};

template <>
struct PullAcc<kU32, kPullAvg> {
  uint64_t s;
  __device__ __forceinline__ void first(uint32_t w) { s = w; }
  __device__ __forceinline__ void next(uint32_t w) { s += w; }
  __device__ __forceinline__ uint32_t word(int n, float) const { return (uint32_t)div_ranks<uint64_t>(s, n); }
};

template <>
struct PullAcc<kU8, kPullAvg> {
  uint32_t even, odd;  // two 16-bit sums each: bytes 0 and 2, bytes 1 and 3 (8 x 255 fits 11 bits)
  __device__ __forceinline__ void first(uint32_t w) {
    even = w & 0x00ff00ffu;
    odd = (w >> 8) & 0x00ff00ffu;
  }
  __device__ __forceinline__ void next(uint32_t w) {
    even += w & 0x00ff00ffu;
    odd += (w >> 8) & 0x00ff00ffu;
  }
  __device__ __forceinline__ uint32_t word(int n, float) const {
    return div_ranks<uint32_t>(even & 0xffffu, n) | (div_ranks<uint32_t>(odd & 0xffffu, n) << 8) |
           (div_ranks<uint32_t>(even >> 16, n) << 16) | (div_ranks<uint32_t>(odd >> 16, n) << 24);
  }
};

// ---- int8: SUM / MIN / MAX / AVG per byte ---------------------------------------------------------
template <int OP>
struct PullAccI8 {
  uint32_t a;
  __device__ __forceinline__ void first(uint32_t w) { a = w; }
  __device__ __forceinline__ void next(uint32_t w) {
    if constexpr (OP == kSum) {
      // the low seven bits of every byte add without reaching the next byte; the top bits add by xor
      a = ((a & 0x7f7f7f7fu) + (w & 0x7f7f7f7fu)) ^ ((a ^ w) & 0x80808080u);
    } else {
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 32; k += 8) {
        const int32_t x = (int8_t)(a >> k), y = (int8_t)(w >> k);
        const int32_t t = OP == kMin ? (y < x ? y : x) : (y > x ? y : x);
        r |= ((uint32_t)t & 0xffu) << k;
      }
      a = r;
    }
  }
  __device__ __forceinline__ uint32_t word(int, float) const { return a; }
};
template <>
struct PullAcc<kI8, kSum> : PullAccI8<kSum> {};
template <>
struct PullAcc<kI8, kMin> : PullAccI8<kMin> {};
template <>
struct PullAcc<kI8, kPullMax> : PullAccI8<kPullMax> {};

template <>
struct PullAcc<kI8, kPullAvg> {
  // two 16-bit sums each (bytes 0 and 2, bytes 1 and 3) of the bytes biased by 128 (x ^ 0x80 = x + 128
  // as an unsigned byte): at most 8 x 255, so no field reaches its neighbour
  uint32_t even, odd;
  __device__ __forceinline__ void first(uint32_t w) {
    w ^= 0x80808080u;
    even = w & 0x00ff00ffu;
    odd = (w >> 8) & 0x00ff00ffu;
  }
  __device__ __forceinline__ void next(uint32_t w) {
    w ^= 0x80808080u;
    even += w & 0x00ff00ffu;
    odd += (w >> 8) & 0x00ff00ffu;
  }
  static __device__ __forceinline__ uint32_t byte_of(uint32_t biased, int n) {
    return (uint32_t)div_ranks<int32_t>((int32_t)biased - 128 * n, n) & 0xffu;  // signed: toward zero
  }
  __device__ __forceinline__ uint32_t word(int n, float) const {
    return byte_of(even & 0xffffu, n) | (byte_of(odd & 0xffffu, n) << 8) | (byte_of(even >> 16, n) << 16) |
           (byte_of(odd >> 16, n) << 24);
  }
};

// ---- int64 / uint64: one element = two words ------------------------------------------------------
template <int DT, int OP>
struct PullAcc64 {
  uint64_t a;
  __device__ __forceinline__ void first(uint64_t x) { a = x; }
  __device__ __forceinline__ void next(uint64_t x) {
    if constexpr (OP == kSum) {
      a += x;
    } else if constexpr (DT == kI64) {
      const bool take = OP == kMin ? (int64_t)x < (int64_t)a : (int64_t)x > (int64_t)a;
      a = take ? x : a;
    } else {
      const bool take = OP == kMin ? x < a : x > a;
      a = take ? x : a;
    }
  }
  __device__ __forceinline__ uint64_t word(int, float) const { return a; }
};
template <>
struct PullAcc<kI64, kSum> : PullAcc64<kI64, kSum> {};
template <>
struct PullAcc<kI64, kMin> : PullAcc64<kI64, kMin> {};
template <>
struct PullAcc<kI64, kPullMax> : PullAcc64<kI64, kPullMax> {};
template <>
struct PullAcc<kU64, kSum> : PullAcc64<kU64, kSum> {};
template <>
struct PullAcc<kU64, kMin> : PullAcc64<kU64, kMin> {};
template <>
struct PullAcc<kU64, kPullMax> : PullAcc64<kU64, kPullMax> {};

// (hi * 2^64 + lo) / D for hi < D, D a rank count: see the opening comment.  The result fits 64 bits.
// (This and the two AVG accumulators below are __host__ as well, so that a host program can compare
// them with __int128 arithmetic.)
template <uint32_t D>
__host__ __device__ __forceinline__ uint64_t div96_by(uint32_t hi, uint64_t lo) {
  constexpr uint64_t kAll = ~0ull;
  constexpr uint64_t c1 = kAll / D + (kAll % D == D - 1 ? 1 : 0);  // floor(2^64 / D)
  constexpr uint32_t c2 = (uint32_t)((kAll % D + 1) % D);          // 2^64 mod D
  const uint64_t q = lo / D;
  const uint32_t r = (uint32_t)(lo - q * D);
  return (uint64_t)hi * c1 + q + (hi * c2 + r) / D;
}
__host__ __device__ __forceinline__ uint64_t div96_ranks(uint32_t hi, uint64_t lo, int n) {
  switch (n) {
    case 2: return div96_by<2>(hi, lo);
    case 3: return div96_by<3>(hi, lo);
    case 4: return div96_by<4>(hi, lo);
    case 5: return div96_by<5>(hi, lo);
    case 6: return div96_by<6>(hi, lo);
    case 7: return div96_by<7>(hi, lo);
    default: return div96_by<8>(hi, lo);
  }
}

template <>
struct PullAcc<kU64, kPullAvg> {
  uint64_t lo;
  uint32_t hi;  // carries out of lo: at most n - 1
  __host__ __device__ __forceinline__ void first(uint64_t x) {
    lo = x;
    hi = 0;
  }
  __host__ __device__ __forceinline__ void next(uint64_t x) {
    lo += x;
    hi += lo < x ? 1u : 0u;
  }
  __host__ __device__ __forceinline__ uint64_t word(int n, float) const { return div96_ranks(hi, lo, n); }
};

template <>
struct PullAcc<kI64, kPullAvg> {
  uint64_t lo;
  int32_t hi;  // {hi, lo}: the 96-bit two's-complement sum of the sign-extended operands
  __host__ __device__ __forceinline__ void first(uint64_t x) {
    lo = x;
    hi = (int64_t)x < 0 ? -1 : 0;
  }
  __host__ __device__ __forceinline__ void next(uint64_t x) {
    lo += x;
    hi += ((int64_t)x < 0 ? -1 : 0) + (lo < x ? 1 : 0);
  }
  __host__ __device__ __forceinline__ uint64_t word(int n, float) const {
    const bool neg = hi < 0;
    // the magnitude: at most n * 2^63, so its high part stays below n
    const uint64_t mlo = neg ? 0 - lo : lo;
    const uint32_t mhi = neg ? ~(uint32_t)hi + (lo == 0 ? 1u : 0u) : (uint32_t)hi;
    const uint64_t q = div96_ranks(mhi, mlo, n);
    return neg ? 0 - q : q;
  }
};

}  // namespace mscclpp_amd
