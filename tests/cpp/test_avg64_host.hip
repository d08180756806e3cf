// The 64-bit AVG accumulators of the pull-reduce kernel (include/mscclpp_amd/pull_reduce_device.hpp:
// a 96-bit sum, one divide by a constant per element), run on the HOST against __int128 arithmetic:
// the exact sum of n int64 / uint64 values divided by n, truncating toward zero, for n = 2 .. 8.
// Operands: uniform 64-bit words, boundary values (0, +-1, +-7, +-9, INT64_MIN / MAX, 2^32 +- 1),
// mixtures of both, small magnitudes of both signs, and n times the same boundary value.
// No device is touched.  Prints "avg64 OK <cases>" and exits 0, or the first mismatches and 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "mscclpp_amd/pull_reduce_device.hpp"

using namespace mscclpp_amd;

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  uint64_t seed = 12345;
  long bad = 0, cases = 0;
  const uint64_t specials[] = {0, 1, 2, 7, 8, 9, ~0ull, ~0ull - 1, ~0ull - 6, ~0ull - 8, 0x7fffffffffffffffull,
                               0x8000000000000000ull, 0x8000000000000001ull, 0x7ffffffffffffffeull, 0xffffffffull,
                               0x100000000ull, 0xfffffffffffffff9ull};
  const int ns = (int)(sizeof(specials) / sizeof(specials[0]));
  for (int n = 2; n <= 8; ++n) {
    for (long it = 0; it < 200000; ++it) {
      uint64_t x[8];
      for (int k = 0; k < n; ++k) {
        const uint64_t r = splitmix(seed);
        switch (it % 4) {
          case 0: x[k] = r; break;
          case 1: x[k] = specials[r % ns]; break;
          case 2: x[k] = (r >> 8) % 3 ? specials[r % ns] : splitmix(seed); break;
          default: x[k] = (uint64_t)((int64_t)r >> (r % 60)); break;
        }
        if (it < ns) x[k] = specials[it];  // n times the same boundary value
      }
      PullAcc<kU64, kPullAvg> u;
      PullAcc<kI64, kPullAvg> s;
      u.first(x[0]);
      s.first(x[0]);
      unsigned __int128 usum = x[0];
      __int128 ssum = (int64_t)x[0];
      for (int k = 1; k < n; ++k) {
        u.next(x[k]);
        s.next(x[k]);
        usum += x[k];
        ssum += (int64_t)x[k];
      }
      const uint64_t wantU = (uint64_t)(usum / (unsigned)n);
      const uint64_t wantS = (uint64_t)(int64_t)(ssum / n);  // C division truncates toward zero
      if (u.word(n, 0.f) != wantU || s.word(n, 0.f) != wantS) {
        if (bad < 10)
          printf("n %d case %ld: uint64 %016llx want %016llx, int64 %016llx want %016llx\n", n, it,
                 (unsigned long long)u.word(n, 0.f), (unsigned long long)wantU, (unsigned long long)s.word(n, 0.f),
                 (unsigned long long)wantS);
        ++bad;
      }
      ++cases;
    }
  }
  if (bad) {
    printf("avg64 FAILED: %ld of %ld cases\n", bad, cases);
    return 1;
  }
  printf("avg64 OK %ld\n", cases);
  return 0;
}
