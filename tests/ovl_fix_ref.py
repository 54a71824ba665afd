"""Reference for `edit --correct-overlap` and `--insert-size`, written from
DESIGN.md §2.14 alone: pure Python, a loop over the facing positions; no code
shared with the product (tests only).  tests/ovl_ref.py gives F*, the cuts and
the pair builders.

With F = F* > 0, lo = max(0, F - n2), hi = min(n1, F) and k in [lo, hi), byte
s1[k] faces s2[j], j = F - 1 - k.  q1 = Q1[k] - phred, q2 = Q2[j] - phred (the
quality bytes unsigned).  At a position that does not match (both bytes one of
A C G T and the one the other's complement):
  1. s1[k] a base, q1 >= high, q2 <= low:  s2[j] := comp(s1[k]), Q2[j] := Q1[k];
  2. else s2[j] a base, q2 >= high, q1 <= low:  s1[k] := comp(s2[j]), Q1[k] := Q2[j];
  3. else nothing.
F* comes from the uncorrected bytes; the correction acts on the kept reads."""
import numpy as np

import ovl_ref as R

BINS = 1025
DEFAULT = (33, 30, 14)                                # phred, high, low


def correct(s1, q1, s2, q2, F, phred=33, high=30, low=14):
    """(s1, q1, s2, q2, [bases corrected in mate 1, in mate 2]) of one pair whose F* is F."""
    a, qa, b, qb = bytearray(s1), bytearray(q1), bytearray(s2), bytearray(q2)
    done = [0, 0]
    if F > 0:
        n1, n2 = len(a), len(b)
        for k in range(max(0, F - n2), min(n1, F)):
            j = F - 1 - k
            if R.COMP.get(a[k]) == b[j]:              # (COMP.get of a non-base is None: never equal)
                continue
            v1, v2 = qa[k] - phred, qb[j] - phred
            if a[k] in R.COMP and v1 >= high and v2 <= low:
                b[j], qb[j] = R.COMP[a[k]], qa[k]
                done[1] += 1
            elif b[j] in R.COMP and v2 >= high and v1 <= low:
                a[k], qa[k] = R.COMP[b[j]], qb[j]
                done[0] += 1
    return bytes(a), bytes(qa), bytes(b), bytes(qb), done


def hist_of(inserts):
    """u64 [1025]: hist[F*] over the analysed pairs, -1 in no bin."""
    h = np.zeros(BINS, np.uint64)
    for f in inserts:
        if f >= 0:
            h[int(f)] += 1
    return h


class Fixed:
    """What cut and correction make of two batches (O.Reads): an ovl_ref.Cut
    (.cut: insert, pos, idx, info, and the kept bytes before the correction), the
    kept bytes after it (.seq / .qual per mate), the three scalars (.fix) and the
    histogram of one find pass (.hist)."""

    def __init__(self, r1, r2, min_overlap=30, M=5, phred=33, high=30, low=14, cut=None):
        self.cut = cut if cut is not None else R.Cut(r1, r2, min_overlap, M)
        c = self.cut
        self.seq = [bytearray(bytes(x)) for x in c.seq]
        self.qual = [bytearray(bytes(x)) for x in c.qual]
        pairs, bases = 0, [0, 0]
        for i, F in enumerate(c.insert.tolist()):
            if F <= 0:
                continue
            (a0, a1), (b0, b1) = (int(c.idx[0][i]), int(c.idx[0][i + 1])), (int(c.idx[1][i]), int(c.idx[1][i + 1]))
            s1, q1, s2, q2, done = correct(self.seq[0][a0:a1], self.qual[0][a0:a1], self.seq[1][b0:b1], self.qual[1][b0:b1],
                                           F, phred, high, low)
            self.seq[0][a0:a1], self.qual[0][a0:a1], self.seq[1][b0:b1], self.qual[1][b0:b1] = s1, q1, s2, q2
            pairs += sum(done) > 0
            bases = [x + y for x, y in zip(bases, done)]
        self.seq = [np.frombuffer(bytes(x), np.uint8) for x in self.seq]
        self.qual = [np.frombuffer(bytes(x), np.uint8) for x in self.qual]
        self.fix = dict(corrected_pairs=pairs, corrected_bases=bases)
        self.hist = hist_of(c.insert.tolist())


def add_fix(infos):
    return dict(corrected_pairs=sum(i["corrected_pairs"] for i in infos),
                corrected_bases=[sum(i["corrected_bases"][m] for i in infos) for m in range(2)])


def fix_records(rec1, rec2, min_overlap=30, M=5, phred=33, high=30, low=14):
    """Two lists of (name, seq, qual, ...) cut by §2.13 and corrected by §2.14:
    (the records, §2.13's scalars, the three scalars, the histogram)."""
    out, ins = ([], []), []
    pairs, bases = 0, [0, 0]
    for a, b in zip(rec1, rec2):
        F = R.find(a[1], b[1], min_overlap, M)
        ins.append(F)
        c1, c2 = R.cuts(len(a[1]), len(b[1]), F)
        s1, q1, s2, q2, done = correct(a[1][:c1], a[2][:c1], b[1][:c2], b[2][:c2], F, phred, high, low)
        out[0].append((a[0], s1, q1, *a[3:]))
        out[1].append((b[0], s2, q2, *b[3:]))
        pairs += sum(done) > 0
        bases = [x + y for x, y in zip(bases, done)]
    info = R.info_of([len(r[1]) for r in rec1], [len(r[1]) for r in rec2], ins, min_overlap, M)
    return out, info, dict(corrected_pairs=pairs, corrected_bases=bases), hist_of(ins)


def render_correct(info, fix):
    """The bytes of <base>.overlap.correct.data."""
    p = int(info["pairs"])
    pct = 100.0 * fix["corrected_pairs"] / p if p else 0.0
    return (b"# Pairs\tOverlapping\tCorrected pairs\t% corrected\tBases corrected 1\tBases corrected 2\n" +
            ("%d\t%d\t%d\t%.2f\t%d\t%d\n" % (p, info["overlapping"], fix["corrected_pairs"], pct, fix["corrected_bases"][0],
                                           fix["corrected_bases"][1])).encode())


def render_inserts(info, hist):
    """The bytes of <base>.insert.size.data."""
    h = [int(x) for x in hist]
    assert len(h) == BINS
    sizes = [f for f in range(1, BINS) if h[f]]
    with_ov = sum(h[1:])
    out = b"# Pairs\tSkipped\tWithout overlap\tWith overlap\tMin\tMedian\tMax\tMean\n"
    head = "%d\t%d\t%d\t%d\t" % (info["pairs"], info["skipped"], h[0], with_ov)
    if not sizes:
        return out + (head + "0\t0\t0\t0.00\n").encode() + b"# Insert size\tPairs\t% of overlapping\n"
    lo, hi = sizes[0], sizes[-1]
    median = next(F for F in range(1, BINS) if 2 * sum(h[1:F + 1]) >= with_ov)
    mean = sum(f * h[f] for f in sizes) / with_ov
    out += (head + "%d\t%d\t%d\t%.2f\n" % (lo, median, hi, mean)).encode()
    out += b"# Insert size\tPairs\t% of overlapping\n"
    for F in range(lo, hi + 1):
        out += ("%d\t%d\t%.2f\n" % (F, h[F], 100.0 * h[F] / with_ov)).encode()
    return out


# -- pairs with qualities: (s1, q1, s2, q2) --------------------------------------------------------

def between(n, i, phred=33, high=30, low=14):
    """n quality bytes that neither win nor lose (all of them `high` where nothing lies between)."""
    span = high - low - 1
    return bytes(phred + (low + 1 + (7 * k + 3 * i) % span if span > 0 else high) for k in range(n))


def clean(rng, n1, n2, F, i=0, **th):
    """A pair from a fragment of F bases without a disagreement."""
    s1, s2 = R.pair_of(rng, n1, n2, F)
    return s1, between(n1, i, **th), s2, between(n2, i + 1, **th)


def plant(pair, F, off, winner, win_q, lose_q, lose_byte=None, win_byte=None):
    """The pair with a disagreement at offset `off` of the overlap: the winner
    (mate 1 or 2) keeps its base (or takes win_byte) at the quality BYTE win_q,
    the byte that faces it becomes another base (or lose_byte) at the quality
    byte lose_q."""
    s1, q1, s2, q2 = (bytearray(x) for x in pair)
    k = max(0, F - len(s2)) + off
    j = F - 1 - k
    assert 0 <= k < len(s1) and 0 <= j < len(s2)
    (ws, wq, wi), (ls, lq, li) = ((s1, q1, k), (s2, q2, j)) if winner == 1 else ((s2, q2, j), (s1, q1, k))
    ls[li] = R.flip(bytes(ls), li)[li] if lose_byte is None else lose_byte
    if win_byte is not None:
        ws[wi] = win_byte
    wq[wi], lq[li] = win_q, lose_q
    return bytes(s1), bytes(q1), bytes(s2), bytes(q2)


POSITION_SHAPES = [(150, 100), (150, 150), (150, 230), (300, 290), (512, 512), (512, 600)]


def position_pairs(seed=21):
    """One disagreement per pair at the offsets a lane, a load step or the overlap
    begins or ends at, each once with mate 1 and once with mate 2 as the winner;
    then mates of 40 and 70 bases at every F.  phred 33, thresholds 30 / 14."""
    rng = np.random.default_rng(seed)
    out = []
    for n, F in POSITION_SHAPES:
        ov = min(n, F) - max(0, F - n)
        for off in sorted({o for o in (0, 1, 3, 4, 63, 64, 252, 255, 256, 259, ov - 1) if o < ov}):
            for winner in (1, 2):
                out.append(plant(clean(rng, n, n, F, len(out)), F, off, winner, 33 + 40, 33 + 2))
    for F in range(30, 40 + 70 - 30 + 1):
        ov = min(40, F) - max(0, F - 70)
        for winner in (1, 2):
            out.append(plant(clean(rng, 40, 70, F, len(out)), F, (0, ov - 1, ov // 2)[F % 3], winner, 33 + 30, 33 + 14))
    return out


def threshold_pairs(phred, high, low, seed=22):
    """The winner at high - 1 and high, the loser at low and low + 1, both
    directions; the loser's quality byte below phred, the winner's 255."""
    rng = np.random.default_rng(seed + phred + high)
    th = dict(phred=phred, high=high, low=low)
    out = []
    for winner in (1, 2):
        for wq in (high - 1, high):
            for lq in (low, low + 1):
                out.append(plant(clean(rng, 90, 80, 70, len(out), **th), 70, 5 + len(out), winner, phred + wq, phred + lq))
        for wq, lq in ((255, phred - 1), (255, 0), (phred + high, phred - 1), (255, phred + low), (255, phred + low + 1)):
            out.append(plant(clean(rng, 90, 80, 70, len(out), **th), 70, 5 + len(out), winner, wq, lq))
    return out


def byte_pairs(seed=23):
    """The loser takes every byte value against each base as the winner, five
    disagreements per pair, both directions; then winners that are no upper-case
    base, at high quality, facing a base of low quality and facing themselves."""
    rng = np.random.default_rng(seed)
    out = []
    todo = [(v, w) for w in b"ACGT" for v in range(256)]
    for winner in (1, 2):
        for g in range(0, len(todo), 5):
            p = clean(rng, 90, 80, 70, len(out))
            for t, (v, w) in enumerate(todo[g:g + 5]):
                # the winner's base w: what faces it is v, so v is a match only where it is w's complement
                p = plant(p, 70, 3 + 13 * t, winner, 33 + 40, 33 + 3, lose_byte=v, win_byte=w)
            out.append(p)
    for winner in (1, 2):
        for v in (ord("N"), ord("a"), ord("c"), ord("g"), ord("t"), ord("n"), 0x00, 0xFF):
            p = clean(rng, 90, 80, 70, len(out))
            p = plant(p, 70, 10, winner, 33 + 40, 33 + 3, lose_byte=None, win_byte=v)       # faces a base of low quality
            p = plant(p, 70, 30, winner, 33 + 40, 33 + 3, lose_byte=v, win_byte=v)          # faces itself
            p = plant(p, 70, 50, winner, 33 + 40, 33 + 40, lose_byte=v, win_byte=v)         # both of high quality
            out.append(p)
    return out


def several_pairs(min_overlap, M, seed=24):
    """Exactly M disagreements, all correctable: towards mate 2, towards mate 1,
    alternating; then a mixture of correctable and not."""
    rng = np.random.default_rng(seed + M)
    n, F = 150, 110
    out = []
    spots = [int(x) for x in rng.permutation(F)[:M]]
    for way in ((1,), (2,), (1, 2)):
        p = clean(rng, n, n, F, len(out))
        for t, off in enumerate(spots):
            p = plant(p, F, off, way[t % len(way)], 33 + 35, 33 + 10)
        out.append(p)
    p = clean(rng, n, n, F, len(out))
    kinds = [(33 + 35, 33 + 10), (33 + 35, 33 + 20), (33 + 29, 33 + 3), (33 + 40, 33 + 40), (33 + 2, 33 + 2), (33 + 30, 33 + 14)]
    for t, off in enumerate(spots):
        p = plant(p, F, off, 1 + t % 2, *kinds[t % len(kinds)])
    out.append(p)
    return out


def untouched_pairs(seed=25):
    """Pairs the correction must not touch -- unrelated mates, a mate of 513
    bases, mates of 0 .. 8 bases -- each between two corrected pairs whose
    corrections lie at the first and the last facing position."""
    rng = np.random.default_rng(seed)

    def corrected(i):
        p = clean(rng, 60 + i % 7, 50 + i % 5, 45 + i % 3, i)
        F = 45 + i % 3
        p = plant(p, F, 0, 1 + i % 2, 33 + 40, 33 + 2)
        return plant(p, F, F - 1, 2 - i % 2, 33 + 40, 33 + 2)

    def plain(n1, n2, i):
        # qualities that would win and lose everywhere, were the pair analysed
        return R.acgt(rng, n1), bytes([33 + 40]) * n1, R.acgt(rng, n2), bytes([33 + 2]) * n2

    quiet = [plain(80, 90, 0), plain(513, 100, 1), plain(100, 513, 2)]
    quiet += [plain(a, b, a + b) for a in range(9) for b in (0, 1, 2, 3, a, 8)]
    # a read-through of 513 bases: skipped although its mates would overlap
    s1, s2 = R.pair_of(rng, 513, 513, 100)
    quiet.append((s1, bytes([33 + 40]) * 513, R.flip(s2, 50), bytes([33 + 2]) * 513))
    out = [corrected(0)]
    for i, q in enumerate(quiet):
        out += [q, corrected(i + 1)]
    return out


def random_case(n=600, seed=11):
    """ovl_ref.random_pairs with the quality 33 + (7 j + 3 i) % 41 of read i at position j."""
    out = []
    for i, (s1, s2) in enumerate(R.random_pairs(n, seed)):
        out.append((s1, bytes(33 + (7 * j + 3 * i) % 41 for j in range(len(s1))),
                    s2, bytes(33 + (7 * j + 3 * i) % 41 for j in range(len(s2)))))
    return out
