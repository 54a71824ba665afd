// Host checks of hpgq_engine_kernel.h's filter_bounds / in_filter_bounds and
// quality_q02 (tests/test_filter_bounds_cpu.py reads the lines printed here).
//
//   bounds: for every read length n in 0..252 and every segment sum S in
//   0..255 n, lo16 <= S <= hi16 of the packed word against the filter's
//   predicate in 64-bit arithmetic, over a grid of mean bounds (lo_r, hi_r),
//   length ranges and filter on / off.  One line per combination:
//     B filter min_len max_len lo_r hi_r compared mismatches
//   quality: the per-position sums of `steps` steps of 4-byte words kept as
//   a += word and q13 += b1 | b3 << 16, recovered by quality_q02, against
//   direct sums.  One line per case:
//     Q name steps mismatches
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "hpgq_engine_kernel.h"

// the filter's predicate, 64-bit; `lo` and `hi` are the products lo_r n and hi_r n
static bool direct(long long n, long long S, long long min_len, long long max_len, long long lo, long long hi,
                   bool filter) {
  return !filter | ((min_len <= n) & (n <= max_len) & (lo <= S) & (S <= hi));   // (no branches: the loop vectorises)
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng32() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// mode 0: random bytes, 1: all 0xFF, 2: all 0x00, 3: random, then the first
// half of the steps taken back out (the kernels' SubTag / UndoTag)
static int quality_case(const char *name, int steps, int mode) {
  uint32_t a = 0, q13 = 0;
  uint32_t want[4] = {0, 0, 0, 0};
  static uint32_t words[1024];
  for (int t = 0; t < steps; ++t) {
    const uint32_t w = mode == 1 ? 0xFFFFFFFFu : mode == 2 ? 0u : rng32();
    words[t] = w;
    a += w;
    q13 += ((w >> 8) & 0xFFu) | (((w >> 24) & 0xFFu) << 16);
    for (int i = 0; i < 4; ++i) want[i] += (w >> (8 * i)) & 0xFFu;
  }
  if (mode == 3) {
    for (int t = 0; t < steps / 2; ++t) {
      const uint32_t w = words[t];
      a -= w;
      q13 -= ((w >> 8) & 0xFFu) | (((w >> 24) & 0xFFu) << 16);
      for (int i = 0; i < 4; ++i) want[i] -= (w >> (8 * i)) & 0xFFu;
    }
  }
  const uint32_t q02 = hpgq::quality_q02(a, q13);
  const uint32_t got[4] = {q02 & 0xFFFFu, q13 & 0xFFFFu, q02 >> 16, q13 >> 16};
  int bad = 0;
  for (int i = 0; i < 4; ++i) bad += got[i] != want[i];
  std::printf("Q %s %d %d\n", name, steps, bad);
  return bad;
}

int main() {
  const int kNeg = -7;
  // (300: its products pass 65,535 by less than a multiple of 65,536, so a missing clamp shows)
  const int lo_rs[] = {kNeg, 0, 128 + 33 + 20, 128 + 64 + 41, 255, 256, 300, 65535, 2147483647};
  const int hi_rs[] = {0, 128 + 33 + 20, 128 + 64 + 41, 255, 256, 300, 65535, 2147483647};
  const int ranges[][2] = {{0, 0}, {50, 150}, {1, 2147483647}, {200, 100}};
  int total_bad = 0;
  // (the combinations are independent: spread over a few threads, printed in order)
  struct Combo {
    int filter, min_len, max_len, lo_r, hi_r;
    long long compared, bad;
  };
  std::vector<Combo> combos;
  for (int filter = 0; filter < 2; ++filter)
    for (const auto &rg : ranges)
      for (int lo_r : lo_rs)
        for (int hi_r : hi_rs) combos.push_back(Combo{filter, rg[0], rg[1], lo_r, hi_r, 0, 0});
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i = next++; i < combos.size(); i = next++) {
      Combo &c = combos[i];
      for (int n = 0; n <= 252; ++n) {
        const uint32_t bw = hpgq::filter_bounds(n, c.min_len, c.max_len, c.lo_r, c.hi_r, c.filter != 0);
        const long long lo = (long long)c.lo_r * n, hi = (long long)c.hi_r * n;
        for (int S = 0; S <= 255 * n; ++S) {
          const bool got = hpgq::in_filter_bounds(bw, (uint32_t)S);
          c.bad += got != direct(n, S, c.min_len, c.max_len, lo, hi, c.filter != 0);
        }
        c.compared += 255 * n + 1;
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < 8; ++t) pool.emplace_back(work);
  for (auto &t : pool) t.join();
  for (const Combo &c : combos) {
    std::printf("B %d %d %d %d %d %lld %lld\n", c.filter, c.min_len, c.max_len, c.lo_r, c.hi_r, c.compared, c.bad);
    total_bad += c.bad != 0;
  }
  // the packed words the kernels' comments name
  const bool words_ok = hpgq::filter_bounds(100, 50, 150, 181, 255, false) == 0xFFFF0000u &&
                        hpgq::filter_bounds(49, 50, 150, 181, 255, true) == 0x0000FFFFu &&
                        hpgq::filter_bounds(151, 50, 150, 181, 255, true) == 0x0000FFFFu &&
                        hpgq::filter_bounds(252, 0, 1000, 261, 300, true) == 0x0000FFFFu &&   // 65772 > 65535
                        hpgq::filter_bounds(100, 50, 150, -7, 2147483647, true) == 0xFFFF0000u &&
                        hpgq::filter_bounds(100, 50, 150, 181, 233, true) == (18100u | (23300u << 16));
  std::printf("W %d\n", words_ok ? 0 : 1);
  total_bad += !words_ok;
  total_bad += quality_case("ones", 255, 1);
  total_bad += quality_case("zeros", 255, 2);
  char name[32];
  for (int k = 0; k < 64; ++k) {
    std::snprintf(name, sizeof name, "random%d", k);
    total_bad += quality_case(name, 255, 0);
    std::snprintf(name, sizeof name, "undo%d", k);
    total_bad += quality_case(name, 255, 3);
  }
  total_bad += quality_case("one_step", 1, 1);
  return total_bad ? 1 : 0;
}
