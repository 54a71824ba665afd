// Host checks of the per-read quotients of hpgq_engine_kernel.h: div_len and
// meanq_terms_rc (the segmented kernels' unit epilogue, n <= 252, by a
// multiply-high with rtab[n] = ceil(2^32 / n)) and meanq_terms (the catch-all,
// n <= 1024, plain division), against 64-bit / __int128 arithmetic written
// from the definitions (tests/test_read_terms_cpu.py reads the lines):
//
//   key = the integer nearest to S / n, halves away from zero, S = sb - 128 n
//   bin = key & 255;   fx = floor(65536 S / n) mod 2^64;   gc bin = floor(100 gc / n)
//
//   R meanq_terms_rc pairs mismatches      every n in 1..252, sb in 0..255 n
//   G div_len_gc pairs mismatches          every n in 1..252, gc in 0..n
//   M meanq_terms pairs mismatches         every n in 1..1024, sb in 0..255 n
//   E div_len_epilogue_max pairs mismatches   per n the largest numerator of the
//                                          epilogue (and the n below it), which
//                                          must satisfy x (n - 1) < 2^32
//   X n x_max first_bad                    per n: that numerator and the first
//                                          x above it where div_len is no
//                                          longer floor(x / n) (0: none below
//                                          2^32); reported, the margin
//   C classes ties neg_mean rem_max n_one  how many of R's pairs are a tie
//                                          2 rem = n, have sb < 128 n, rem = n - 1, n = 1
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "hpgq_engine_kernel.h"

typedef __int128 i128;

static uint32_t recip(uint32_t i) { return i <= 1 ? 0u : 0xFFFFFFFFu / i + 1u; }   // the kernel's own expression (tri_body)

static i128 floor_div(i128 a, i128 b) {   // b > 0
  i128 q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the nearest integer to S / n, halves away from zero: by the floor quotient
// and the doubled remainder, no (2 S + n) / (2 n)
static long long round_away(long long S, long long n) {
  const long long q = (long long)floor_div(S, n), r = S - q * n;   // 0 <= r < n
  if (2 * r > n) return q + 1;
  if (2 * r < n) return q;
  return S > 0 ? q + 1 : q;
}

struct Want {
  uint32_t bin;
  uint64_t fx;
};
static Want want_of(uint32_t sb, uint32_t n) {
  const long long S = (long long)sb - 128ll * n;
  Want w;
  w.bin = (uint32_t)(round_away(S, n) & 255);
  w.fx = (uint64_t)(long long)floor_div((i128)S * 65536, n);
  return w;
}

struct Tally {
  long long pairs = 0, bad = 0, ties = 0, neg = 0, rem_max = 0, n_one = 0;
  void operator+=(const Tally &o) {
    pairs += o.pairs, bad += o.bad, ties += o.ties, neg += o.neg, rem_max += o.rem_max, n_one += o.n_one;
  }
};

template <class F>
static Tally over_lengths(int n_max, F per_length) {
  std::atomic<int> next{1};
  std::vector<Tally> part(8);
  std::vector<std::thread> pool;
  for (int t = 0; t < 8; ++t)
    pool.emplace_back([&, t]() {
      for (int n = next++; n <= n_max; n = next++) per_length((uint32_t)n, part[t]);
    });
  for (auto &th : pool) th.join();
  Tally all;
  for (const Tally &p : part) all += p;
  return all;
}

int main() {
  int failed = 0;
  const Tally R = over_lengths(252, [](uint32_t n, Tally &T) {
    const uint32_t rc = recip(n), one1 = n == 1u ? 1u : 0u;
    for (uint32_t sb = 0; sb <= 255u * n; ++sb) {
      uint32_t bin = ~0u;
      uint64_t fx = ~0ull;
      hpgq::meanq_terms_rc(sb, n, rc, one1, bin, fx);
      const Want w = want_of(sb, n);
      T.bad += bin != w.bin || fx != w.fx;
      const uint32_t rem = sb % n;
      T.ties += 2 * rem == n;
      T.neg += sb < 128u * n;
      T.rem_max += rem == n - 1;
      T.n_one += n == 1;
    }
    T.pairs += 255ll * n + 1;
  });
  std::printf("R meanq_terms_rc %lld %lld\n", R.pairs, R.bad);
  std::printf("C classes %lld %lld %lld %lld\n", R.ties, R.neg, R.rem_max, R.n_one);
  failed += R.bad != 0;

  const Tally Gc = over_lengths(252, [](uint32_t n, Tally &T) {
    const uint32_t rc = recip(n), one1 = n == 1u ? 1u : 0u;
    for (uint32_t gc = 0; gc <= n; ++gc) T.bad += hpgq::div_len(100u * gc, rc, one1) != (100u * gc) / n;
    T.pairs += n + 1;
  });
  std::printf("G div_len_gc %lld %lld\n", Gc.pairs, Gc.bad);
  failed += Gc.bad != 0;

  const Tally M = over_lengths(1024, [](uint32_t n, Tally &T) {
    for (uint32_t sb = 0; sb <= 255u * n; ++sb) {
      uint32_t bin = ~0u;
      uint64_t fx = ~0ull;
      hpgq::meanq_terms(sb, n, bin, fx);
      const Want w = want_of(sb, n);
      T.bad += bin != w.bin || fx != w.fx;
    }
    T.pairs += 255ll * n + 1;
  });
  std::printf("M meanq_terms %lld %lld\n", M.pairs, M.bad);
  failed += M.bad != 0;

  // div_len's stated bound.  The epilogue's numerators: sb <= 255 n, 100 gc <=
  // 100 n, rem << 16 <= (n - 1) << 16; the largest of them per n
  struct Edge {
    uint64_t x_max, first_bad;
  };
  std::vector<Edge> edges(253);
  const Tally E = over_lengths(252, [&](uint32_t n, Tally &T) {
    const uint32_t rc = recip(n), one1 = n == 1u ? 1u : 0u;
    uint64_t x_max = 255ull * n;
    if (((uint64_t)(n - 1) << 16) > x_max) x_max = (uint64_t)(n - 1) << 16;
    T.bad += !(x_max * (n - 1) < (1ull << 32));                 // inside the stated bound
    for (uint64_t x = x_max >= n ? x_max - n : 0; x <= x_max; ++x) T.bad += hpgq::div_len((uint32_t)x, rc, one1) != x / n;
    T.pairs += 1;
    // the first failure above x_max.  rc = (2^32 + e) / n, 0 <= e < n: mulhi(x,
    // rc) = floor(x / n + x e / (n 2^32)) first exceeds floor(x / n) at an x = n - 1
    // mod n with x e >= 2^32, so no x below 2^32 / e can fail: start n below it
    // (n = 1: one1 multiplies 24 bits, so x = 2^24 is the first)
    const uint64_t e = n == 1 ? 0 : (uint64_t)rc * n - (1ull << 32);
    uint64_t first = 0;
    if (n == 1) {
      first = 1ull << 24;
      T.bad += hpgq::div_len((1u << 24) - 1u, rc, one1) != (1u << 24) - 1u || hpgq::div_len(1u << 24, rc, one1) == 1u << 24;
    } else if (e != 0) {
      uint64_t x = (1ull << 32) / e;
      x = x > n ? x - n : 0;
      if (x <= x_max) x = x_max + 1;
      for (; x < (1ull << 32); ++x)
        if (hpgq::div_len((uint32_t)x, rc, one1) != x / n) {
          first = x;
          break;
        }
    }
    edges[n] = Edge{x_max, first};
  });
  std::printf("E div_len_epilogue_max %lld %lld\n", E.pairs, E.bad);
  failed += E.bad != 0;
  for (int n = 1; n <= 252; ++n)
    std::printf("X %d %llu %llu\n", n, (unsigned long long)edges[n].x_max, (unsigned long long)edges[n].first_bad);
  return failed ? 1 : 0;
}
