// Stand-alone check of csrc/cv_divmod.h: n / d and n % d through one float multiply and ONE correction step, for 0 <= n < 2^24
// and 0 < d < 2^24.  Exhaustive in n for the divisors the UNet uses (output widths Wo and plane sizes Ho * Wo of its layers at
// 256 x 256 and 240 x 320) and for d = 1, 2, 3, 2^k +- 1, 2^24 - 1; at the multiples of d and their neighbours for a sweep of d.
// Plain C++, nothing from ROCm.  Prints "ok <divisors> <checks>", or the first failure and exits 1.
#include <cstdio>
#include <cstdint>
#include <set>

#include "cv_divmod.h"

static long long checks = 0;

static bool check(int n, int d, float rcp) {
  int q, r;
  cv_divmod(n, d, rcp, q, r);
  ++checks;
  if (q != n / d || r != n % d) {
    std::printf("FAIL n=%d d=%d: q=%d r=%d, want %d %d\n", n, d, q, r, n / d, n % d);
    return false;
  }
  return true;
}

int main() {
  const int LIM = 1 << 24;
  std::set<int> full = {1, 2, 3, LIM - 1};
  for (int k = 1; k <= 24; ++k) {
    if ((1 << k) - 1 > 0 && (1 << k) - 1 < LIM) full.insert((1 << k) - 1);
    if ((1 << k) + 1 < LIM) full.insert((1 << k) + 1);
  }
  const int sides[2][2] = {{256, 256}, {240, 320}};
  for (const auto &hw : sides)
    for (int s = 0; s <= 8; ++s) {
      const int h = hw[0] >> s, w = hw[1] >> s;
      if (h < 1 || w < 1) break;
      full.insert(w);
      full.insert(h * w);
    }
  for (int d : full) {
    const float rcp = 1.0f / (float)d;
    for (int n = 0; n < LIM; ++n)
      if (!check(n, d, rcp)) return 1;
  }
  // every d below 4096, then a stride through the rest: the multiples of d and their neighbours
  long long swept = 0;
  for (int d = 1; d < LIM; d += (d < 4096 ? 1 : 997)) {
    const float rcp = 1.0f / (float)d;
    const int step = (LIM / d > 4096) ? (LIM / d / 4096) : 1;       // at most ~4096 multiples per divisor, the last always
    for (int m = 0; (long long)m * d < LIM + d; m += step) {
      for (int e = -1; e <= 1; ++e) {
        const long long n = (long long)m * d + e;
        if (n >= 0 && n < LIM && !check((int)n, d, rcp)) return 1;
      }
    }
    const int last = (LIM - 1) / d * d;
    for (int e = -1; e <= 1; ++e)
      if (last + e >= 0 && last + e < LIM && !check(last + e, d, rcp)) return 1;
    if (!check(LIM - 1, d, rcp)) return 1;
    ++swept;
  }
  std::printf("ok %zu %lld %lld\n", full.size(), checks, swept);
  return 0;
}
