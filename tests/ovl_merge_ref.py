"""Reference for `edit --merge-overlap`, written from DESIGN.md §2.15 alone: pure
Python, a loop over the merged read's positions; no code shared with the
product (tests only).  tests/ovl_ref.py gives F* and the pair builders.

A pair with F = F* > 0 becomes one read m[0, F), QM[0, F); every other pair
passes through uncut.  lo = max(0, F - n2), hi = min(n1, F), j = F - 1 - p;
rc(b) is b's complement for A C G T and b itself for every other byte.
  p <  lo: m[p] = s1[p],     QM[p] = Q1[p]
  p >= hi: m[p] = rc(s2[j]), QM[p] = Q2[j]
  otherwise (a facing position):
    1. both bytes bases and complementary: m[p] = s1[p], QM[p] = max(Q1[p], Q2[j])
    2. else mate 2 wins iff s2[j] is a base and (s1[p] is none or Q2[j] > Q1[p]):
       m[p] = comp(s2[j]), QM[p] = Q2[j], resolved[1] += 1
    3. else m[p] = s1[p], QM[p] = Q1[p], resolved[0] += 1
The quality bytes compare unsigned; a tie goes to mate 1."""
import numpy as np

import ovl_ref as R
import ovl_fix_ref as X                               # (its pair builders only)

BINS = 1025


def merge(s1, q1, s2, q2, F):
    """(m, QM, [resolved by mate 1, by mate 2]) of one pair whose F* is F (F <= 0: empty)."""
    s1, q1, s2, q2 = bytes(s1), bytes(q1), bytes(s2), bytes(q2)
    m, qm, res = bytearray(), bytearray(), [0, 0]
    if F <= 0:
        return b"", b"", res
    n1, n2 = len(s1), len(s2)
    lo, hi = max(0, F - n2), min(n1, F)
    assert lo < hi
    for p in range(F):
        j = F - 1 - p
        if p < lo:
            m.append(s1[p])
            qm.append(q1[p])
        elif p >= hi:
            m.append(R.COMP.get(s2[j], s2[j]))
            qm.append(q2[j])
        elif s1[p] in R.COMP and R.COMP[s1[p]] == s2[j]:
            m.append(s1[p])
            qm.append(max(q1[p], q2[j]))
        elif s2[j] in R.COMP and (s1[p] not in R.COMP or q2[j] > q1[p]):
            m.append(R.COMP[s2[j]])
            qm.append(q2[j])
            res[1] += 1
        else:
            m.append(s1[p])
            qm.append(q1[p])
            res[0] += 1
    return bytes(m), bytes(qm), res


def hist_of(inserts):
    h = np.zeros(BINS, np.uint64)
    for f in inserts:
        if f >= 0:
            h[int(f)] += 1
    return h


def info_of(inserts, resolved):
    return dict(merged_pairs=sum(f > 0 for f in inserts), merged_bases=sum(f for f in inserts if f > 0),
                resolved=[int(resolved[0]), int(resolved[1])])


def add_info(infos):
    return dict(merged_pairs=sum(i["merged_pairs"] for i in infos), merged_bases=sum(i["merged_bases"] for i in infos),
                resolved=[sum(i["resolved"][m] for i in infos) for m in range(2)])


class _Out:
    """A compacted batch: idx int32 [k + 1] from 0, seq, qual u8."""

    def __init__(self, seqs, quals):
        self.n = len(seqs)
        self.idx = np.zeros(self.n + 1, np.int32)
        if self.n:
            self.idx[1:] = np.cumsum([len(s) for s in seqs])
        self.seq = np.frombuffer(b"".join(seqs) + b"\1", np.uint8)[:-1].copy()
        self.qual = np.frombuffer(b"".join(quals) + b"\1", np.uint8)[:-1].copy()


class Merged:
    """What the merge makes of two batches (O.Reads): insert int32 [n], the three
    compacted batches (.out[0], .out[1]: the unmerged pairs' mates; .merged),
    §2.13's scalars of the find pass (.info), the four scalars (.merge) and the
    histogram of one find pass (.hist)."""

    def __init__(self, r1, r2, min_overlap=30, M=5):
        assert r1.n == r2.n
        n = r1.n
        blob = [[bytes(np.asarray(x, np.uint8)) for x in (r.seq, r.qual)] for r in (r1, r2)]
        ix = [[int(x) for x in r.idx] for r in (r1, r2)]
        ins, res = [], [0, 0]
        keep = ([], [], [], [])            # seq1, qual1, seq2, qual2 of the unmerged pairs
        ms, mq = [], []
        for i in range(n):
            s1, q1 = (blob[0][k][ix[0][i]:ix[0][i + 1]] for k in range(2))
            s2, q2 = (blob[1][k][ix[1][i]:ix[1][i + 1]] for k in range(2))
            F = R.find(s1, s2, min_overlap, M)
            ins.append(F)
            if F > 0:
                m, qm, r = merge(s1, q1, s2, q2, F)
                assert len(m) == len(qm) == F <= 1016
                ms.append(m)
                mq.append(qm)
                res = [a + b for a, b in zip(res, r)]
            else:
                for lst, x in zip(keep, (s1, q1, s2, q2)):
                    lst.append(x)
        self.insert = np.array(ins, np.int32).reshape(n)
        self.out = [_Out(keep[0], keep[1]), _Out(keep[2], keep[3])]
        self.merged = _Out(ms, mq)
        lens = [np.diff(ix[0]).tolist(), np.diff(ix[1]).tolist()]
        self.info = R.info_of(lens[0], lens[1], ins, min_overlap, M)
        self.merge = info_of(ins, res)
        self.hist = hist_of(ins)


def merge_records(rec1, rec2, min_overlap=30, M=5):
    """Two lists of (name, seq, qual, ...): (the unmerged pairs' records of mate 1,
    of mate 2, the merged records under mate 1's name, §2.13's scalars, the four
    scalars, the histogram)."""
    out1, out2, merged, ins, res = [], [], [], [], [0, 0]
    for a, b in zip(rec1, rec2):
        F = R.find(a[1], b[1], min_overlap, M)
        ins.append(F)
        if F > 0:
            m, qm, r = merge(a[1], a[2], b[1], b[2], F)
            merged.append((a[0], m, qm, *a[3:]))
            res = [x + y for x, y in zip(res, r)]
        else:
            out1.append(a)
            out2.append(b)
    info = R.info_of([len(r[1]) for r in rec1], [len(r[1]) for r in rec2], ins, min_overlap, M)
    return out1, out2, merged, info, info_of(ins, res), hist_of(ins)


def render(info, merge_info):
    """The bytes of <base>.overlap.merge.data."""
    p = int(info["pairs"])
    pct = 100.0 * merge_info["merged_pairs"] / p if p else 0.0
    return (b"# Pairs\tOverlapping\tMerged\t% merged\tMerged bases\tResolved by mate 1\tResolved by mate 2\n" +
            ("%d\t%d\t%d\t%.2f\t%d\t%d\t%d\n" % (p, info["overlapping"], merge_info["merged_pairs"], pct,
                                               merge_info["merged_bases"], merge_info["resolved"][0],
                                               merge_info["resolved"][1])).encode())


# -- pairs with qualities: (s1, q1, s2, q2) --------------------------------------------------------

def tie_pairs(seed=41):
    """Disagreements at equal quality bytes (mate 1 wins), one byte apart (the
    greater wins), with the extreme bytes 0x00 and 0xFF, and losers that are N,
    lower case, 0x00 or 0xFF in either mate, inside and outside the overlap."""
    rng = np.random.default_rng(seed)
    out = []
    for winner in (1, 2):
        for wq, lq in ((60, 60), (61, 60), (0, 0), (255, 255), (255, 254), (1, 0), (128, 127)):
            out.append(X.plant(X.clean(rng, 90, 80, 70, len(out)), 70, 7 + len(out), winner, wq, lq))
        for v in (ord("N"), ord("a"), ord("t"), 0x00, 0xFF):
            # the loser is no base: the other mate's base wins whatever the qualities
            out.append(X.plant(X.clean(rng, 90, 80, 70, len(out)), 70, 11, winner, 40, 90, lose_byte=v))
            # neither is a base: mate 1's byte stays
            out.append(X.plant(X.clean(rng, 90, 80, 70, len(out)), 70, 23, winner, 40, 90, lose_byte=v, win_byte=v))
    # such bytes outside the overlap: mate 1's head and mate 2's head of a pair with F > n
    for v in (ord("N"), ord("a"), 0x00, 0xFF):
        s1, q1, s2, q2 = (bytearray(x) for x in X.clean(rng, 80, 80, 100, len(out)))
        s1[3], s2[5], q1[4], q2[6] = v, v, v, v
        out.append((bytes(s1), bytes(q1), bytes(s2), bytes(q2)))
    return out
