"""A plain exact reference of one counter set (include/hpgq.h's layout), in
numpy int64 and Python integers.  It shares no code with the CPU oracle
(oracle/hpgq_oracle.c) and does not load it: the oracle writes the rounding
and the floor with the same integer expressions as the kernels, this module
writes them from their definitions, so a test against it pins both.

  counters(reads, lmax, mask=None, trim=None)   one mate's set
  c2_mask(reads, phred, min_len, max_len, min_q, max_q)

`reads` is anything with .seq, .qual (uint8) and .idx (int32, n + 1 offsets).

The definitions (src/stats_fastq.c:283-382):
  * a quality byte is a signed char; S is a read's sum of them, n its length;
  * hist_meanq: the key is the integer nearest to S / n, a half going away
    from zero (C's round()); the bin is key & 255.  round_half_away() takes
    the floor quotient and looks at the remainder: no (2 S + n) / (2 n);
  * ACC_MEANQ_FX16: floor(65536 S / n), summed mod 2^64;
  * hist_gc: floor(100 (G + C) / n);
  * a read of n = 0 bases has no quality and no G+C bin;
  * a read longer than lmax counts in S_LONG_READS, not in hist_len, and only
    its positions < lmax are counted;
  * pos_qsum holds signed sums in two's complement.

test_round_half_away_is_round() and test_floor_fx16() check the two integer
rules against fractions.Fraction for every (n <= 40, S).
"""
from fractions import Fraction

import numpy as np

NUM_SCALARS, MEANQ_BINS, GC_BINS = 8, 256, 101
S_NUM_INPUT, S_NUM_PASSED, S_NUM_FAILED, S_NUM_EDITED, S_NUM_STATS, S_ACC_MEANQ_FX16, S_LONG_READS = range(7)
MASK64 = (1 << 64) - 1


def offsets(lmax):
    """Where each array of a set starts (include/hpgq.h, hpgq_off_*)."""
    o = {"hist_len": NUM_SCALARS}
    o["hist_meanq"] = o["hist_len"] + lmax + 1
    o["hist_gc"] = o["hist_meanq"] + MEANQ_BINS
    o["pos_qsum"] = o["hist_gc"] + GC_BINS
    o["pos_base"] = o["pos_qsum"] + lmax          # five rows of lmax: A C G T N
    o["len"] = o["pos_base"] + 5 * lmax
    return o


def round_half_away(S, n):
    """The integer nearest to S / n (n > 0), halves away from zero; int64 arrays."""
    q = np.floor_divide(S, n)          # q <= S / n < q + 1
    r = S - q * n                      # 0 <= r < n: S / n = q + r / n
    up = (2 * r > n) | ((2 * r == n) & (S > 0))   # past the half; on it, up only when positive
    return q + up


def _windows(reads, trim):
    idx = np.asarray(reads.idx, np.int64)
    a, n = idx[:-1].copy(), np.diff(idx)
    if trim is not None:
        t = np.asarray(trim).astype(np.int64)
        ts, te = t & 0xFFFF, (t >> 16) & 0xFFFF
        a, n = a + ts, n - ts - te
        assert (n >= 0).all()
    return a, n


def _segment_sums(values, a, n):
    """sum(values[a_i : a_i + n_i]) per read (empty reads give 0)."""
    cs = np.zeros(len(values) + 1, np.int64)
    np.cumsum(values, out=cs[1:])
    return cs[a + n] - cs[a]


def quality_sums(reads, trim=None):
    """(S, n) per read: the signed-char sum over its window, the window's length."""
    a, n = _windows(reads, trim)
    return _segment_sums(np.asarray(reads.qual).view(np.int8).astype(np.int64), a, n), n


def c2_mask(reads, phred, min_len, max_len, min_q, max_q):
    """C2's filter: min_len <= n <= max_len and min_q n <= S <= max_q n, S the
    sum of (signed char - phred)."""
    sraw, n = quality_sums(reads)
    S = sraw - phred * n
    ok = (min_len <= n) & (n <= max_len) & (min_q * n <= S) & (S <= max_q * n)
    return ok.astype(np.uint8)


def counters(reads, lmax, mask=None, trim=None):
    """One mate's packed u64 set over the reads with mask != 0 (all when None),
    each cut to [ts, n - te) by its trim word ts | te << 16 (whole when None)."""
    nr = len(reads.idx) - 1
    o = offsets(lmax)
    c = [0] * o["len"]                 # Python ints: packed mod 2^64 at the end
    keep = np.ones(nr, bool) if mask is None else np.asarray(mask) != 0
    a_all, n_all = _windows(reads, trim)
    c[S_NUM_INPUT] = nr
    c[S_NUM_PASSED] = int(keep.sum())
    c[S_NUM_FAILED] = nr - c[S_NUM_PASSED]
    c[S_NUM_EDITED] = 0 if trim is None else int((np.asarray(trim) != 0).sum())
    c[S_NUM_STATS] = c[S_NUM_PASSED]
    a, n = a_all[keep], n_all[keep]
    c[S_LONG_READS] = int((n > lmax).sum())
    for L, k in zip(*np.unique(n[n <= lmax], return_counts=True)):
        c[o["hist_len"] + int(L)] = int(k)

    qual = np.asarray(reads.qual).view(np.int8).astype(np.int64)
    seq = np.asarray(reads.seq)
    S = _segment_sums(qual, a, n)
    gc = _segment_sums(((seq == ord("C")) | (seq == ord("G"))).astype(np.int64), a, n)
    has = n > 0
    Sh, nh, gh = S[has], n[has], gc[has]
    for b, k in zip(*np.unique(round_half_away(Sh, nh) & 255, return_counts=True)):
        c[o["hist_meanq"] + int(b)] = int(k)
    for b, k in zip(*np.unique(np.floor_divide(100 * gh, nh), return_counts=True)):
        c[o["hist_gc"] + int(b)] = int(k)
    assert nh.size == 0 or int(np.abs(Sh).max()) < 1 << 40   # 65536 S stays far inside int64
    c[S_ACC_MEANQ_FX16] = sum(int(v) for v in np.floor_divide(65536 * Sh, nh))

    # per position: how often each byte value sits there
    m = np.minimum(n, lmax)
    tot = int(m.sum())
    if tot:
        first = np.cumsum(m) - m
        pos = np.arange(tot, dtype=np.int64) - np.repeat(first, m)
        at = np.repeat(a, m) + pos
        signed = np.arange(256, dtype=np.int64)
        signed[128:] -= 256
        hq = np.bincount(pos * 256 + np.asarray(reads.qual)[at], minlength=lmax * 256).reshape(lmax, 256)
        hs = np.bincount(pos * 256 + seq[at], minlength=lmax * 256).reshape(lmax, 256)
        qs = hq @ signed
        for p in range(lmax):
            c[o["pos_qsum"] + p] = int(qs[p])
            for bi, ch in enumerate(b"ACGTN"):
                c[o["pos_base"] + bi * lmax + p] = int(hs[p, ch])
    return np.array([v & MASK64 for v in c], dtype=np.uint64)


# ---------------------------------------------------------------------------
# the two integer rules against exact rationals (collected by pytest; no GPU)
# ---------------------------------------------------------------------------

def _round_fraction(x):
    """C's round() of a rational, from its definition."""
    lo = x.numerator // x.denominator          # floor
    d = x - lo
    if d > Fraction(1, 2):
        return lo + 1
    if d < Fraction(1, 2):
        return lo
    return lo + 1 if x > 0 else lo             # the half: away from zero


def _all_pairs(nmax=40):
    n = np.concatenate([np.full(256 * k + 1, k, np.int64) for k in range(1, nmax + 1)])
    S = np.concatenate([np.arange(-128 * k, 128 * k + 1, dtype=np.int64) for k in range(1, nmax + 1)])
    return S, n


def test_round_half_away_is_round():
    S, n = _all_pairs()
    got = round_half_away(S, n)
    ties = 0
    for s, k, g in zip(S.tolist(), n.tolist(), got.tolist()):
        assert g == _round_fraction(Fraction(s, k)), (s, k, g)
        ties += (2 * s) % k == 0 and s % k != 0
    assert ties > 1000 and int(got.min()) == -128 and int(got.max()) == 128


def test_floor_fx16():
    S, n = _all_pairs()
    got = np.floor_divide(65536 * S, n)
    for s, k, g in zip(S.tolist(), n.tolist(), got.tolist()):
        x = Fraction(65536 * s, k)
        assert g <= x < g + 1, (s, k, g)


def test_counters_by_hand():
    """Three reads written out: lengths 3, 0 and 2, lmax 2 (so the first is long)."""
    class R:
        seq = np.frombuffer(b"GCAN.", np.uint8)
        qual = np.array([0x80, 0xFF, 0x7F, 1, 2], np.uint8)    # -128, -1, 127 | 1, 2
        idx = np.array([0, 3, 3, 5], np.int32)
    c = counters(R, 2)
    o = offsets(2)
    want = {S_NUM_INPUT: 3, S_NUM_PASSED: 3, S_NUM_STATS: 3, S_LONG_READS: 1,
            o["hist_len"] + 0: 1, o["hist_len"] + 2: 1,
            o["hist_meanq"] + 255: 1,          # -2 / 3 -> -1
            o["hist_meanq"] + 2: 1,            # 3 / 2 -> 2 (the half, away from zero)
            o["hist_gc"] + 66: 1, o["hist_gc"] + 0: 1,
            S_ACC_MEANQ_FX16: (-43691 + 98304) & MASK64,       # floor(-131072 / 3), 3 * 32768
            o["pos_qsum"] + 0: (-128 + 1) & MASK64, o["pos_qsum"] + 1: 1,
            o["pos_base"] + 2 * 2 + 0: 1,      # G at 0
            o["pos_base"] + 1 * 2 + 1: 1,      # C at 1
            o["pos_base"] + 4 * 2 + 0: 1}      # N at 0 ('.' at 1 counts nowhere)
    assert {i: int(v) for i, v in enumerate(c) if v} == want
    # the second read alone, its first base trimmed away
    c = counters(R, 2, mask=np.array([0, 0, 1]), trim=np.array([0, 0, 1], np.uint32))
    want = {S_NUM_INPUT: 3, S_NUM_PASSED: 1, S_NUM_FAILED: 2, S_NUM_EDITED: 1, S_NUM_STATS: 1,
            o["hist_len"] + 1: 1, o["hist_meanq"] + 2: 1, o["hist_gc"] + 0: 1, S_ACC_MEANQ_FX16: 2 << 16,
            o["pos_qsum"] + 0: 2}
    assert {i: int(v) for i, v in enumerate(c) if v} == want
