// hpgq_ovl_lane.h — the packed pair of `edit --clip-overlap` and what one lane
// computes on it.  Plain integer C++, compiled for the
// device by hpgq_ovl.hip and for the host by tests/sanitize/ovl_main.cpp,
// which walks every lane of every block against the host rule; §2.15's merge of
// a lane's four positions (merge4), walked by tests/sanitize/ovl_merge_main.cpp.
//
// The packed pair, in u64 words (base p of a string at bits 2p .. 2p + 1 of the
// string's words, little end first):
//
//   c1[kW1]   mate 1's codes, base k at position kLead + k: kLead / 32 zero
//             words in front and kW1 - kLead / 32 - 16 behind it
//   ok1[kW1]  01 for each base of mate 1 that is one of A C G T, 00 elsewhere
//   c2[16]    mate 2 complemented and written backwards from the top: position
//             j holds comp(s2[511 - j])
//   ok2[16]   01 where s2[511 - j] is a base
//
// A candidate insert length F makes s1[k] face s2[F - 1 - k], which is position
// j = k + 512 - F of c2: word w of c2 faces the 64 bits of c1 from position
// 32 w + F - (512 - kLead) on.  A base outside either read has ok = 00, so the
// matches of F are the popcount of eq & ok1 & ok2 over the words, whatever the
// range [lo, hi) of the rule is, and mism(F) = ov(F) - matches(F).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HPGQ_OVL_HD __host__ __device__ __forceinline__
#else
#define HPGQ_OVL_HD inline
#endif

namespace hpgq {
namespace ovl {

constexpr int kMaxLen = 512;            // HPGQ_OVL_MAX_LEN
constexpr int kWords = kMaxLen / 32;    // code words of one mate
constexpr int kLead = 128;              // positions in front of mate 1
constexpr int kW1 = 24;                 // words of c1 and of ok1
constexpr int kC1 = 0, kOk1 = kW1, kC2 = 2 * kW1, kOk2 = 2 * kW1 + kWords;
constexpr int kPairWords = 2 * kW1 + 2 * kWords;

// four validity bits -> 01 per valid base
HPGQ_OVL_HD uint32_t spread4(uint32_t ok) { return (ok & 1u) | (ok & 2u) << 1 | (ok & 4u) << 2 | (ok & 8u) << 3; }
// four 2-bit codes, last first
HPGQ_OVL_HD uint32_t rev_codes(uint32_t c) { return (c & 3u) << 6 | (c & 0xCu) << 2 | (c & 0x30u) >> 2 | (c >> 6 & 3u); }
// four validity bits, last first
HPGQ_OVL_HD uint32_t rev_bits(uint32_t ok) { return (ok & 1u) << 3 | (ok & 2u) << 1 | (ok & 4u) >> 1 | (ok >> 3 & 1u); }

// The bytes of the packed pair that hold the four bases 4 q .. 4 q + 3 of a
// mate (q = 0 .. 127), given their codes c and validity bits ok (pack4).
HPGQ_OVL_HD void put_mate1(uint8_t *pair, int q, uint32_t c, uint32_t ok) {
  pair[kC1 * 8 + kLead / 4 + q] = (uint8_t)c;
  pair[kOk1 * 8 + kLead / 4 + q] = (uint8_t)spread4(ok);
}
HPGQ_OVL_HD void put_mate2(uint8_t *pair, int q, uint32_t c, uint32_t ok) {
  pair[kC2 * 8 + 127 - q] = (uint8_t)(rev_codes(c) ^ 0xAAu);   // (comp: code ^ 2)
  pair[kOk2 * 8 + 127 - q] = (uint8_t)spread4(rev_bits(ok));
}

HPGQ_OVL_HD int ov_of(int n1, int n2, int F) { return (n1 < F ? n1 : F) - (F > n2 ? F - n2 : 0); }

// A block of 64 candidates fb, fb - 1, ..: the least of them that is a
// candidate, and the words of c2 that face a base of mate 1 for any of them.
struct Block {
  int fmin, wlo, whi;
};
HPGQ_OVL_HD Block block_of(int n1, int n2, int min_ov, int fb) {
  Block b;
  b.fmin = fb - 63 > min_ov ? fb - 63 : min_ov;
  // F's positions of c2: [max(512 - F, 512 - n2), min(n1 + 512 - F, 512))
  const int jlo = kMaxLen - (fb < n2 ? fb : n2);
  const int jhi = n1 - b.fmin < 0 ? n1 + kMaxLen - b.fmin : kMaxLen;
  b.wlo = jlo >> 5;
  b.whi = (jhi - 1) >> 5;
  return b;
}

// 64 bits of the string w[] from bit position 2 t on (t >= 0)
HPGQ_OVL_HD uint64_t window(const uint64_t *w, int t) {
  const int i = t >> 5, s = 2 * (t & 31);
  return w[i] >> s | (w[i + 1] << 1) << (63 - s);
}

HPGQ_OVL_HD int popcount64(uint64_t x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// matches(F) over the block's words (F: one of the block's candidates)
HPGQ_OVL_HD int matches_of(const uint64_t *pair, int F, int wlo, int whi) {
  int m = 0;
  for (int w = wlo; w <= whi; ++w) {
    const int t = 32 * w + F - (kMaxLen - kLead);
    const uint64_t x = window(pair + kC1, t) ^ pair[kC2 + w];
    m += popcount64(~(x | x >> 1) & window(pair + kOk1, t) & pair[kOk2 + w]);
  }
  return m;
}

// ---- §2.15's merge on the four positions of a lane ----------------------------
// Everything is arithmetic on the four bytes of a dword at once: a flag is bit 7
// of its byte, a mask the whole byte; no compare, so no lane mask and no branch.

// bit 7 of every byte -> the whole byte
HPGQ_OVL_HD uint32_t bytes_of(uint32_t flags) { return (flags >> 7) * 255u; }

// the bytes t < k of a dword (k <= 0: none, k >= 4: all)
HPGQ_OVL_HD uint32_t low_bytes(int k) { return k >= 4 ? ~0u : k <= 0 ? 0u : (1u << (8 * k)) - 1u; }

// flag where the byte of x is >= the byte of y, both unsigned
HPGQ_OVL_HD uint32_t ge4(uint32_t x, uint32_t y) {
  const uint32_t H = 0x80808080u;
  const uint32_t t = (x | H) - (y & ~H);   // (no borrow between bytes) bit 7: the low 7 bits of x >= those of y
  return ((x & ~y) | (~(x ^ y) & t)) & H;
}

// comp on the four bytes of v: byte t of the result faces byte t of v in a
// match, 0 where that is no base.  pack4's arithmetic (hpgq_reads.h): x the
// 2-bit code of each byte (A 0, C 1, T 2, G 3), the one base with that code
// compared with the byte, and the base of the complement's code x ^ 2.
HPGQ_OVL_HD uint32_t comp4(uint32_t v) {
  const uint32_t x = v >> 1 & 0x03030303u;
  const uint32_t isT = x >> 1 & ~x & 0x01010101u;
  const uint32_t d = v ^ (0x41414141u + 2u * x + 15u * isT);
  const uint32_t z = ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;   // flag: the byte is a base
  const uint32_t cx = x ^ 0x02020202u;
  const uint32_t cT = cx >> 1 & ~cx & 0x01010101u;
  return (0x41414141u + 2u * cx + 15u * cT) & bytes_of(z);
}

struct Merged4 {
  uint32_t seq, qual;     // the merged bases and quality bytes of positions p .. p + 3
  uint32_t won1, won2;    // the facing positions among them that mate 1 / mate 2 resolved
};

// Positions p .. p + 3 of a merged read: b1 / q1 mate 1's bytes there (0 from
// hi on), b2 / q2 the bytes of mate 2 that face them (anything below lo);
// k1 = hi - p positions lie below hi, k2 = lo - p below lo.  Bytes at F and
// behind are whatever comes out: the caller stores none of them.
HPGQ_OVL_HD Merged4 merge4(uint32_t b1, uint32_t q1, uint32_t b2, uint32_t q2, int k1, int k2) {
  const uint32_t H = 0x80808080u;
  const uint32_t in1 = low_bytes(k1), in2 = ~low_bytes(k2);
  const uint32_t c1 = comp4(b1), c2 = comp4(b2);
  const uint32_t a1 = (c1 + 0x7F7F7F7Fu) & H, a2 = (c2 + 0x7F7F7F7Fu) & H;   // s1[p], s2[j] is a base (comp's bytes are below 0x80)
  const uint32_t d = b2 ^ c1;
  const uint32_t match = a1 & ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d);       // s2[j] == comp(s1[p])
  const uint32_t ge = ge4(q1, q2);                                             // Q1 >= Q2: mate 2 does not win on quality
  const uint32_t two = H & in2 & (~in1 | (~match & a2 & (~a1 | ~ge)));
  const uint32_t both = H & in1 & in2 & ~match;
  const uint32_t twoB = bytes_of(two), geB = bytes_of(ge), matchB = bytes_of(H & match & in2);
  const uint32_t rc2 = c2 | (b2 & ~bytes_of(a2));
  const uint32_t top = (q1 & geB) | (q2 & ~geB);
  Merged4 m;
  m.seq = (rc2 & twoB) | (b1 & ~twoB);
  m.qual = (q2 & twoB) | (((top & matchB) | (q1 & ~matchB)) & ~twoB);
  m.won2 = (uint32_t)__builtin_popcount(both & two);
  m.won1 = (uint32_t)__builtin_popcount(both & ~two);
  return m;
}

}  // namespace ovl
}  // namespace hpgq
