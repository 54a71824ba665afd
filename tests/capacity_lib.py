"""Input builders of tests/test_capacity_gpu.py (the kernels against
tests/exact_ref.py) and tests/test_exact_ref_cpu.py (the CPU oracle against
it, on the same inputs).  Everything is explicit: no random draw.

Part (a), counters at capacity: batches in which every base is one letter and
every quality one byte, so a packed on-chip counter (TriAcc's nibbles and
bytes, the catch-all's 6-bit fields) grows by one in EVERY step between two
flushes, and the per-position quality pairs by the largest or smallest byte.

Part (b), quotient edges: for a read length n one read per biased quality sum
sb (sum of byte ^ 0x80) in a set that holds every rounding edge of sb / n, and
one read per G+C count.
"""
import functools

import numpy as np

import exact_ref as X
import hpgfastq as H
import oracle_lib as O

# the segmented geometries (hpgq_engine_lds.h, Geo<G>): reads per unit, reads
# per step, the longest read
GEO = {"tri": dict(B=54, segs=3, pos=160), "hex": dict(B=48, segs=6, pos=156), "wide": dict(B=60, segs=4, pos=252)}
WAVES = 4              # waves of one workgroup (kWaves)
BYTE_EVERY = 255       # TriAcc's 8-bit counters (kByteEvery)
FLUSH_EVERY = 63       # the catch-all's 6-bit fields (kFlushEvery)
CATCH_ALL_UNIT = 64

LETTERS = {"A": ord("A"), "C": ord("C"), "G": ord("G"), "T": ord("T"), "N": ord("N"), "other": ord(".")}
QBYTES = {"7f": 0x7F, "80": 0x80, "ff": 0xFF}    # biased 255, 0 (signed -128), 127 (signed -1)


def steps_per_unit(geo):
    return GEO[geo]["B"] // GEO[geo]["segs"]


def units_per_wave(geo):
    """3 * ceil(255 / s) + 2: a wave flushes inside its loop at least three
    times (it flushes once more than 255 - s steps are held: every
    floor((255 - s) / s) + 1 <= ceil(255 / s) units)."""
    s = steps_per_unit(geo)
    return 3 * -(-BYTE_EVERY // s) + 2


def units_between_flushes(steps, own_geo):
    """Units of `steps` steps a wave of geometry own_geo runs from one in-loop
    flush to the next: tri_body adds the unit's steps to since_flush and
    flushes at the top of a unit once since_flush > 255 - kBlock / kSegs."""
    return (BYTE_EVERY - steps_per_unit(own_geo)) // steps + 1


def followup_units_per_wave(first_geo):
    """The wide follow-up stage behind `first_geo`, every read deferred: it walks
    the first stage's units (B reads each, compacted: nr = B), so a unit is
    ceil(B / 4) steps of wide's 4 reads (steps_of); since_flush grows by that
    and the flush line is 255 - 60 / 4 = 240.  Behind hex: 12 steps a unit,
    a flush every 21 units (12 * 21 = 252 > 240); 3 * 21 + 2 = 65 units."""
    steps = -(-GEO[first_geo]["B"] // GEO["wide"]["segs"])
    return 3 * units_between_flushes(steps, "wide") + 2


def _freeze(r):
    for a in (r.seq, r.qual, r.idx):
        a.setflags(write=False)
    return r


def _from_lengths(ln):
    idx = np.zeros(len(ln) + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    return idx


def per_read(values, ln):
    return np.repeat(np.asarray(values), ln)


def positions(ln):
    """Position within its read of every byte."""
    ln = np.asarray(ln, np.int64)
    return np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)


# ---------------------------------------------------------------------------
# (a) counters at capacity
# ---------------------------------------------------------------------------

def capacity_lengths(n_reads, length, ragged):
    """Full length, or cycling 1 .. length (lanes filled unevenly; the last
    lane of a segment borrows from the next)."""
    i = np.arange(n_reads, dtype=np.int64)
    return 1 + i % length if ragged else np.full(n_reads, length, np.int64)


def negative_pattern(n_reads, B, mul=5, mod=3):
    """Reads whose quality is 0x80 in the half-failing form: not aligned to the unit."""
    i = np.arange(n_reads, dtype=np.int64)
    return (i * mul + i // B) % mod == 0


def sparse_failures(n_reads, B, add=3):
    """One read per unit, at a position that moves through the unit: 29 places
    on from one unit of a wave to its next (7 per unit, 4 waves, + 1), and 29
    is coprime to 3, 4 and 6: it visits every segment."""
    i = np.arange(n_reads, dtype=np.int64)
    u = i // B
    return i % B == (u * 7 + u // WAVES + add) % B


def peak_count(counted, B, segs, n_waves, line, steps=None):
    """How high a lane's byte counter for the batch's letter gets, at the
    least: counted[i] says read i holds the letter and passes.  A wave runs
    units w, w + n_waves, ...; step t of a unit holds reads segs t .. segs t +
    segs - 1, one per segment; it flushes at the top of a unit once it holds
    more than `line` steps (tri_body: since_flush).  Reads that fail are left
    out altogether (the pass-first kernels never add them; the others hold them
    on top of this until their unit ends), so the true peak is no lower."""
    per_unit = np.asarray(counted).reshape(-1, B // segs, segs).sum(axis=1)   # [unit][segment]
    steps = B // segs if steps is None else steps
    peak = 0
    for w in range(n_waves):
        held, since = np.zeros(segs, np.int64), 0
        for u in range(w, len(per_unit), n_waves):
            if since > line:
                held[:], since = 0, 0
            held += per_unit[u]
            since += steps
            peak = max(peak, int(held.max()))
    return peak


def capacity_reads(ln, letter, qbyte, negative=None, ends=None):
    """ln: lengths; letter: one byte, or one per read; qbyte: the quality byte;
    negative: reads with 0x80 instead; ends: reads whose first 3 and last 5
    quality bytes are 0x80 (what an edit trims from a passing read)."""
    ln = np.asarray(ln, np.int64)
    n = len(ln)
    letters = np.broadcast_to(np.asarray(letter, np.uint8), (n,))
    q = np.full(n, qbyte, np.uint8)
    if negative is not None:
        q = np.where(negative, np.uint8(0x80), q)
    seq = per_read(letters, ln).astype(np.uint8)
    qual = per_read(q, ln).astype(np.uint8)
    if ends is not None:
        j, nn = positions(ln), per_read(ln, ln)
        qual[per_read(ends, ln) & ((j < 3) | (j >= nn - 5))] = 0x80
    return _freeze(O.Reads(np.ascontiguousarray(seq), np.ascontiguousarray(qual), _from_lengths(ln)))


def assert_pass_and_fail_in_every_unit(mask, B):
    m = np.asarray(mask).reshape(-1, B)
    assert m.any(axis=1).all() and not m.all(axis=1).any()


def units_of_waves(n_units, n_waves):
    """Units each wave runs: wave w takes units w, w + n_waves, ..."""
    return np.bincount(np.arange(n_units) % n_waves, minlength=n_waves)


# the ways a failed read leaves the counters (part a, half-failing form):
# name -> (mates, options, edit, where the expected mask comes from)
WAYS = {
    "pf": (1, dict(read_quality_range="0,"), False, "c2"),
    "pf_noor": (1, dict(read_quality_range="0,", max_N=4), False, "oracle"),
    "window": (1, dict(read_quality_range="0,", left_length=12, left_quality_range="0,", right_length=20,
                       right_quality_range="0,200"), False, "oracle"),
    "edit": (1, dict(read_quality_range="0,", left_length=10, left_quality_range="0,", right_length=30,
                     right_quality_range="0,"), True, "oracle"),
    "pe_c2": (2, dict(read_quality_range="0,"), False, "c2"),
    "pe_noor": (2, dict(read_quality_range="0,", max_N=4), False, "oracle"),
}


def way_params(way, lmax):
    nm, opts, edit, _ = WAYS[way]
    p = H.edit_params(lmax=lmax, stats=True, **opts) if edit else H.stats_params(lmax=lmax, **opts)
    p.paired = nm - 1
    return p


def expect_variant(way, geo, name):
    """The first stage's name for a way on a geometry (hpgq_engine_geo.hip, desc())."""
    assert geo in name, name
    if way in ("pf", "plain"):
        ok = "engine_tri_kernel<" in name and ", 1, filter, " in name
    elif way == "pf_noor":
        ok = "engine_tri_x_kernel<" in name and ", 1, " in name and name.endswith(", noor>")
    elif way == "window":
        ok = "engine_tri_x_kernel<" in name and ", 1, " in name and name.endswith(", window>")
    elif way == "edit":   # hex: the trims at the step (ST); tri, wide: the unit-prologue trims
        ok = "engine_tri_kernel<" in name and ", 1, edit, " in name and name.endswith(", st>") == (geo == "hex")
    elif way == "pe_c2":
        ok = "engine_tri_kernel<" in name and ", 2, filter, " in name
    elif way == "pe_noor":
        ok = "engine_tri_x_kernel<" in name and ", 2, " in name and name.endswith(", noor>")
    else:
        raise KeyError(way)
    assert ok, (way, geo, name)


DENSITIES = ("third", "sparse")
NEAR_FULL = BYTE_EVERY - 16   # what "at capacity" asks of a sparse batch's byte counters (peak_count)


def half_failing_mates(way, B, n_reads, length, density="third"):
    """The mates of a half-failing batch.  Mate 1 is all G, mate 2 all T; a
    noor way also holds reads of N alone (they fail max_N); the edit way gives
    every other read low-quality ends, so passing reads are trimmed too.
    density "third": about one read in three (mate 2: four) has quality 0x80,
    so a byte counter holds about two thirds of the steps since its flush;
    "sparse": ONE failing read (pair: by mate 1 and mate 2 in turn) a unit, in
    a noor way a read of N instead in two units of four, so the counters a
    failed read is kept out of or taken back from are within 16 of full
    (peak_count)."""
    nm = WAYS[way][0]
    ln = capacity_lengths(n_reads, length, False)
    i = np.arange(n_reads, dtype=np.int64)
    mates = []
    for m in range(nm):
        letter = np.full(n_reads, ord("G") if m == 0 else ord("T"), np.uint8)
        if density == "sparse":
            neg = sparse_failures(n_reads, B)
            if nm == 2:   # one failing pair a unit: mate 1's fault in even units, mate 2's in odd ones
                neg = neg & ((i // B) % 2 == m)
            if way.endswith("noor"):
                of_n = neg & ((i // B // 2) % 2 == 1)
                letter[of_n] = ord("N")
                neg = neg & ~of_n
        else:
            neg = negative_pattern(n_reads, B) if m == 0 else negative_pattern(n_reads, B, mul=3, mod=4)
            if way.endswith("noor"):
                letter[(i * 3 + i // B) % (5 + 2 * m) == 1] = ord("N")   # (3: coprime to 5 and 7)
        ends = (i % 2 == 1) if way == "edit" else None
        mates.append(capacity_reads(ln, letter, 0x7F, negative=neg, ends=ends))
    return tuple(mates)


# ---------------------------------------------------------------------------
# (b) every quotient edge of a length
# ---------------------------------------------------------------------------

def edge_sums(n):
    """The biased sums of length n that hold every edge of sb / n: the ends,
    around the zero mean (128 n), and for a spread of quotients q the
    remainders 0, 1, just below / at / above the half, n - 1."""
    s = {0, 1, n - 1, n, 128 * n - 1, 128 * n, 128 * n + 1, 255 * n - 1, 255 * n}
    for q in (0, 1, 60, 127, 128, 200, 254):
        for r in (0, 1, -(-n // 2) - 1, -(-n // 2), n // 2 + 1, n - 1):
            s.add(q * n + r)
    return sorted(v for v in s if 0 <= v <= 255 * n)


def gc_counts(n):
    """Every G+C count for a segmented read; for a longer one the ends and both
    sides of every step of floor(100 gc / n)."""
    if n <= GEO["wide"]["pos"]:
        return list(range(n + 1))
    s = {0, 1, 2, n - 1, n}
    for k in range(1, 101):
        first = -(-k * n // 100)          # the smallest gc with 100 gc / n >= k
        s.update((first - 1, first))
    return sorted(v for v in s if 0 <= v <= n)


def _sum_reads(ln, sb):
    """Reads of lengths ln with biased quality sums sb, spread unevenly over the
    bytes: sb // n everywhere, one more on sb % n bytes (rotated by the read's
    number), and a zero-sum wiggle of up to +-3 on byte pairs where the range
    0 .. 255 leaves room."""
    ln, sb = np.asarray(ln, np.int32), np.asarray(sb, np.int32)   # (int32 throughout: tens of millions of bytes)
    i = np.arange(len(ln), dtype=np.int32)
    j, nn, ii = positions(ln).astype(np.int32), per_read(ln, ln), per_read(i, ln)
    base = per_read(sb // ln, ln)
    b = base + ((j + ii) % nn < per_read(sb % ln, ln))
    w = np.maximum(np.minimum(np.minimum(1 + ii % 3, base), 254 - base), 0)
    w[j >= (nn & ~1)] = 0          # whole pairs only
    w[j % 2 == 1] *= -1
    b += w
    assert b.min() >= 0 and b.max() <= 255
    seq = np.frombuffer(b"ACGT", np.uint8)[(j + ii) % 4]
    seq[(j % 11 == 3) & (j // 11 < per_read((i // 5) % 4, ln))] = ord("N")
    return seq, (b ^ 0x80).astype(np.uint8)


def _gc_reads(ln, gc, first):
    """Reads of lengths ln holding gc bases of C and G (a rotated block,
    alternating), the rest A, T and N; a quality level per read."""
    ln, gc = np.asarray(ln, np.int64), np.asarray(gc, np.int64)
    i = first + np.arange(len(ln), dtype=np.int64)
    j, nn, ii = positions(ln), per_read(ln, ln), per_read(i, ln)
    is_gc = (j + ii) % nn < per_read(gc, ln)
    seq = np.where(is_gc, np.frombuffer(b"CG", np.uint8)[j % 2], np.frombuffer(b"ATN", np.uint8)[j % 3])
    qual = (33 + 2 + ii % 40 + (j * 3) % 5).astype(np.uint8)
    return seq.astype(np.uint8), qual


@functools.lru_cache(maxsize=2)
def edge_reads(lengths, full=()):
    """One read per edge sum of every length (every sum 0 .. 255 n for the
    lengths in `full`), then one read per G+C count of every length."""
    ln_s, sb_s = [], []
    for n in lengths:
        sums = range(255 * n + 1) if n in full else edge_sums(n)
        ln_s += [n] * len(sums)
        sb_s += list(sums)
    ln_g, gc_g = [], []
    for n in lengths:
        g = gc_counts(n)
        ln_g += [n] * len(g)
        gc_g += g
    s1, q1 = _sum_reads(ln_s, sb_s)
    s2, q2 = _gc_reads(ln_g, gc_g, len(ln_s))
    ln = np.array(ln_s + ln_g, np.int64)
    assert int(ln.sum()) < 2 ** 31
    r = O.Reads(np.ascontiguousarray(np.concatenate([s1, s2])), np.ascontiguousarray(np.concatenate([q1, q2])),
                _from_lengths(ln))
    return _freeze(r)


def biased_sums(reads):
    """(sb, n) per read, from the bytes alone."""
    n = np.diff(reads.idx).astype(np.int64)
    cs = np.zeros(len(reads.qual) + 1, np.int64)
    np.cumsum(reads.qual ^ 0x80, out=cs[1:])
    a = reads.idx[:-1].astype(np.int64)
    return cs[a + n] - cs[a], n


def gc_of(reads):
    n = np.diff(reads.idx).astype(np.int64)
    cs = np.zeros(len(reads.seq) + 1, np.int64)
    np.cumsum((reads.seq == ord("C")) | (reads.seq == ord("G")), out=cs[1:])
    a = reads.idx[:-1].astype(np.int64)
    return cs[a + n] - cs[a]


def assert_edges_present(reads, lengths, full=()):
    """From the inputs alone: every length has a tie 2 rem = n (even n), a
    negative mean (sb < 128 n), the largest remainder, both ends of the sums,
    G+C = 0 and G+C = n; the lengths in `full` have every sum."""
    sb, n = biased_sums(reads)
    gc = gc_of(reads)
    rem = sb % n
    for L in lengths:
        at = n == L
        assert at.any(), L
        s, r = sb[at], rem[at]
        if L % 2 == 0:
            assert (2 * r == L).any(), ("tie", L)
            assert ((2 * r == L) & (s < 128 * L)).any() and ((2 * r == L) & (s > 128 * L)).any(), ("tie, both signs", L)
        assert (s < 128 * L).any() and (s >= 128 * L).any(), ("sign", L)
        assert (r == L - 1).any() and (r == 0).any(), ("rem", L)
        assert s.min() == 0 and s.max() == 255 * L, ("ends", L)
        assert gc[at].min() == 0 and gc[at].max() == L, ("gc", L)
        if L in full:
            assert np.array_equal(np.unique(s), np.arange(255 * L + 1)), ("every sum", L)


def full_lengths(pos):
    return (1, 2, 3, pos - 1, pos)


FOLLOW_WIDE_LENGTHS = (157, 158, 200, 251, 252)
CATCH_ALL_LENGTHS = (253, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024)
LONG_MERGE_LENGTHS = (151, 152, 253, 1025, 4097)
LONG_MERGE_LMAX = 150


# ---------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------

_expected_cache = {}


def expected_of(key, p, mates, source, lmax=None):
    """expected(), computed once for the tests that follow one another on `key`."""
    if key not in _expected_cache:
        _expected_cache.clear()
        _expected_cache[key] = expected(p, mates, source, lmax)
    return _expected_cache[key]


def expected(p, mates, source, lmax=None):
    """-> (mask, trim, counters, oracle's (mask, counters)).  The mask is
    c2_mask's where the filter is C2's (source "c2"), every read without a
    filter ("all"), else the oracle's; the trim words are the oracle's; the
    counters are exact_ref's over them, one set per mate, at `lmax` (p.lmax
    when None; the oracle's are always at p.lmax)."""
    m_o, t_o, c_o = O.run(p, *mates)
    if source == "c2":
        mask = np.ones(mates[0].n, np.uint8)
        for r in mates:
            mask &= X.c2_mask(r, p.phred, p.min_read_length, p.max_read_length, p.min_read_quality, p.max_read_quality)
    elif source == "all":
        assert not p.filter_on
        mask = np.ones(mates[0].n, np.uint8)
    else:
        mask = m_o
    n = mates[0].n
    sets = [X.counters(r, p.lmax if lmax is None else lmax, mask, t_o[m * n:(m + 1) * n] if p.edit_on else None)
            for m, r in enumerate(mates)]
    out = (mask, t_o, np.concatenate(sets), (m_o, c_o))
    for a in (mask, t_o, out[2], m_o, c_o):
        a.setflags(write=False)
    return out


# ---- (a) -------------------------------------------------------------------

def capacity_batch_size(geo):
    return WAVES * units_per_wave(geo) * GEO[geo]["B"]


@functools.lru_cache(maxsize=2)
def uniform_case(geo, letter, qname, ragged=False):
    g = GEO[geo]
    ln = capacity_lengths(capacity_batch_size(geo), g["pos"], ragged)
    return H.stats_params(lmax=g["pos"]), (capacity_reads(ln, LETTERS[letter], QBYTES[qname]),), "all"


@functools.lru_cache(maxsize=2)
def half_case(way, geo, density="third"):
    g = GEO[geo]
    mates = half_failing_mates(way, g["B"], capacity_batch_size(geo), g["pos"], density)
    return way_params(way, g["pos"]), mates, WAYS[way][3]


def half_case_peak(geo, mates, mask):
    """peak_count of a first-stage half-failing batch: the lowest over the mates."""
    g = GEO[geo]
    line = BYTE_EVERY - steps_per_unit(geo)
    return min(peak_count((r.seq[r.idx[:-1]] == (ord("G"), ord("T"))[m]) & (mask != 0), g["B"], g["segs"], WAVES, line)
               for m, r in enumerate(mates))


FOLLOW_FIRST = "hex"
FOLLOW_KINDS = ("G-7f", "N-80", "other-ff", "half", "sparse")


@functools.lru_cache(maxsize=2)
def follow_case(kind):
    """Route hex, lmax 252, every read 252 bases: the whole batch goes to the
    wide follow-up stage."""
    B = GEO[FOLLOW_FIRST]["B"]
    n = WAVES * followup_units_per_wave(FOLLOW_FIRST) * B
    ln = capacity_lengths(n, 252, False)
    if kind in ("half", "sparse"):
        neg = negative_pattern(n, B) if kind == "half" else sparse_failures(n, B)
        return H.stats_params(lmax=252, read_quality_range="0,"), (capacity_reads(ln, ord("G"), 0x7F, negative=neg),), "c2"
    letter, q = kind.split("-")
    return H.stats_params(lmax=252), (capacity_reads(ln, LETTERS[letter], QBYTES[q]),), "all"


def follow_case_peak(mates, mask):
    """peak_count of the wide follow-up behind FOLLOW_FIRST: its units are the
    first stage's, 4 reads a step, the flush line wide's own."""
    B, segs = GEO[FOLLOW_FIRST]["B"], GEO["wide"]["segs"]
    return peak_count(mask != 0, B, segs, WAVES, BYTE_EVERY - steps_per_unit("wide"), steps=-(-B // segs))


CATCH_ALL_KINDS = ("G-7f", "T-80", "half")


@functools.lru_cache(maxsize=2)
def catch_all_case(lmax, kind):
    """Route single: 64-read units, one read per wave at a time.  Five units a
    wave: 320 reads, of which the half-failing form passes two in three."""
    n = WAVES * 5 * CATCH_ALL_UNIT
    ln = capacity_lengths(n, lmax, False)
    if kind == "half":
        return (H.stats_params(lmax=lmax, read_quality_range="0,"),
                (capacity_reads(ln, ord("G"), 0x7F, negative=negative_pattern(n, CATCH_ALL_UNIT)),), "c2")
    letter, q = kind.split("-")
    return H.stats_params(lmax=lmax), (capacity_reads(ln, LETTERS[letter], QBYTES[q]),), "all"


RAGGED = (("G", "7f"), ("C", "80"), ("N", "ff"), ("other", "7f"))


def capacity_cases():
    """Every part (a) input: (id, builder, arguments)."""
    out = []
    for geo in GEO:
        out += [(f"uniform-{geo}-{l}-{q}", uniform_case, (geo, l, q)) for l in LETTERS for q in QBYTES]
        out += [(f"ragged-{geo}-{l}-{q}", uniform_case, (geo, l, q, True)) for l, q in RAGGED]
        out += [(f"half-{geo}-{w}-{d}", half_case, (w, geo, d)) for w in WAYS for d in DENSITIES]
    out += [(f"follow-{k}", follow_case, (k,)) for k in FOLLOW_KINDS]
    out += [(f"catchall-{lmax}-{k}", catch_all_case, (lmax, k)) for lmax in (252, 1024) for k in CATCH_ALL_KINDS]
    return out


# ---- (b) -------------------------------------------------------------------

def edge_case(lengths, lmax, full=()):
    """(the reads are shared by the tests that run one after the other on them, and read-only)"""
    return H.stats_params(lmax=lmax), (edge_reads(tuple(lengths), tuple(full)),), "all"


def edge_cases():
    """Every part (b) input: (id, lengths, lmax, full)."""
    out = [(f"edges-{geo}", tuple(range(1, g["pos"] + 1)), g["pos"], full_lengths(g["pos"])) for geo, g in GEO.items()]
    out.append(("edges-follow-wide", FOLLOW_WIDE_LENGTHS, 252, ()))
    out.append(("edges-catch-all", CATCH_ALL_LENGTHS, 1024, ()))
    out.append(("edges-long-merge", LONG_MERGE_LENGTHS, LONG_MERGE_LMAX, ()))
    return out
