"""Reference for `edit --clip-overlap`, written from DESIGN.md §2.13 alone: pure
Python, a loop over the candidate insert lengths from the top; no code shared
with the product (tests only).  Also the pairs the CPU and GPU tests share.

A pair is mate 1 s1[0, n1) and mate 2 s2[0, n2).  For a candidate F,
lo = max(0, F - n2), hi = min(n1, F), ov = hi - lo, and s1[k] faces
s2[F - 1 - k] for k in [lo, hi).  A position matches iff both bytes are one of
A C G T and the one is the other's complement.  F is admissible iff
ov >= min_overlap and the positions that do not match are at most M.  F* is the
greatest admissible F, 0 if none, -1 if a mate is longer than 512."""
import numpy as np

MAX_LEN = 512
COMP = {65: 84, 84: 65, 67: 71, 71: 67}          # A<->T, C<->G
BASES = np.frombuffer(b"ACGT", np.uint8)


def find(s1, s2, min_overlap=30, M=5):
    """F*, 0 or -1 of the two byte strings."""
    s1, s2 = bytes(s1), bytes(s2)
    n1, n2 = len(s1), len(s2)
    if n1 > MAX_LEN or n2 > MAX_LEN:
        return -1
    for F in range(n1 + n2 - min_overlap, min_overlap - 1, -1):
        lo, hi = max(0, F - n2), min(n1, F)
        if hi - lo < min_overlap:
            continue
        mism = 0
        for k in range(lo, hi):
            if COMP.get(s1[k]) != s2[F - 1 - k]:      # (COMP.get of a non-base is None: never equal)
                mism += 1
                if mism > M:
                    break
        if mism <= M:
            return F
    return 0


def cuts(n1, n2, F):
    """(c1, c2): the bytes each mate keeps."""
    return (min(n1, F), min(n2, F)) if F > 0 else (n1, n2)


def info_of(lens1, lens2, inserts, min_overlap, M):
    c = [cuts(a, b, f) for a, b, f in zip(lens1, lens2, inserts)]
    return dict(pairs=len(inserts), skipped=sum(f < 0 for f in inserts), overlapping=sum(f > 0 for f in inserts),
                clipped=sum(x < a or y < b for (x, y), a, b in zip(c, lens1, lens2)),
                bases_removed=[sum(a - x for (x, _), a in zip(c, lens1)), sum(b - y for (_, y), b in zip(c, lens2))],
                min_overlap=min_overlap, max_mismatches=M)


class Cut:
    """What the overlap cut makes of two batches (O.Reads): insert int32 [n], per
    mate pos u32 [n], idx int32 [n + 1] from 0 and the kept sequence and quality
    bytes, and the scalars."""

    def __init__(self, r1, r2, min_overlap=30, M=5):
        assert r1.n == r2.n
        blob = [bytes(np.asarray(r.seq, np.uint8)) for r in (r1, r2)]
        ix = [[int(x) for x in r.idx] for r in (r1, r2)]
        n = r1.n
        self.insert = np.zeros(n, np.int32)
        self.pos = [np.zeros(n, np.uint32), np.zeros(n, np.uint32)]
        keep = [np.zeros(len(b), bool) for b in blob]
        for i in range(n):
            s = [blob[m][ix[m][i]:ix[m][i + 1]] for m in range(2)]
            F = find(s[0], s[1], min_overlap, M)
            self.insert[i] = F
            for m, c in enumerate(cuts(len(s[0]), len(s[1]), F)):
                self.pos[m][i] = c
                keep[m][ix[m][i]:ix[m][i] + c] = True
        self.idx, self.seq, self.qual = [], [], []
        for m, r in enumerate((r1, r2)):
            idx = np.zeros(n + 1, np.int32)
            idx[1:] = np.cumsum(self.pos[m].astype(np.int64))
            self.idx.append(idx)
            self.seq.append(np.asarray(r.seq, np.uint8)[keep[m]])
            self.qual.append(np.asarray(r.qual, np.uint8)[keep[m]])
        self.lens = [np.diff(ix[0]), np.diff(ix[1])]
        self.info = info_of(self.lens[0].tolist(), self.lens[1].tolist(), self.insert.tolist(), min_overlap, M)

    def head(self, n):
        """The same for the batches' first n pairs (nothing computed again)."""
        h = object.__new__(Cut)
        h.insert, h.pos, h.lens = self.insert[:n], [p[:n] for p in self.pos], [x[:n] for x in self.lens]
        h.idx = [i[:n + 1] for i in self.idx]
        h.seq = [s[:int(i[-1])] for s, i in zip(self.seq, h.idx)]
        h.qual = [q[:int(i[-1])] for q, i in zip(self.qual, h.idx)]
        h.info = info_of(h.lens[0].tolist(), h.lens[1].tolist(), h.insert.tolist(), self.info["min_overlap"],
                         self.info["max_mismatches"])
        return h


def add(infos):
    """The scalars of several batches (or workers, or shards): plain sums."""
    out = dict(infos[0], bases_removed=list(infos[0]["bases_removed"]))
    for i in infos[1:]:
        for k in ("pairs", "skipped", "overlapping", "clipped"):
            out[k] += i[k]
        out["bases_removed"] = [x + y for x, y in zip(out["bases_removed"], i["bases_removed"])]
    return out


def _pct(num, den):
    return 100.0 * num / den if den else 0.0


def render(info):
    """The bytes of <base>.overlap.clip.data."""
    p = int(info["pairs"])
    return (b"# Pairs\tSkipped\tOverlapping\t% overlapping\tClipped\t% clipped\tBases removed 1\tBases removed 2\n" +
            ("%d\t%d\t%d\t%.2f\t%d\t%.2f\t%d\t%d\n" % (p, info["skipped"], info["overlapping"], _pct(info["overlapping"], p),
                                                     info["clipped"], _pct(info["clipped"], p), info["bases_removed"][0],
                                                     info["bases_removed"][1])).encode())


def cut_records(rec1, rec2, min_overlap=30, M=5):
    """Two lists of (name, seq, qual, ...) cut by the rule, and the scalars."""
    out, ins = ([], []), []
    for a, b in zip(rec1, rec2):
        F = find(a[1], b[1], min_overlap, M)
        ins.append(F)
        for m, (r, c) in enumerate(zip((a, b), cuts(len(a[1]), len(b[1]), F))):
            out[m].append((r[0], r[1][:c], r[2][:c], *r[3:]))
    return out, info_of([len(r[1]) for r in rec1], [len(r[1]) for r in rec2], ins, min_overlap, M)


# -- pairs ----------------------------------------------------------------------------------------

def acgt(rng, n):
    return bytes(BASES[rng.integers(0, 4, size=n)])


def revcomp(s):
    return bytes(COMP[b] for b in reversed(bytes(s)))


def pair_of(rng, n1, n2, F, tail1=None, tail2=None):
    """A pair of n1 and n2 bases from a fragment of F bases: mate 1 reads it
    forwards, mate 2 its reverse complement; a mate longer than the fragment
    goes on with random bases (tail1 / tail2: those bases instead)."""
    frag = acgt(rng, F)
    s1, s2 = frag[:n1], revcomp(frag)[:n2]
    if n1 > F:
        s1 += (tail1 if tail1 is not None else acgt(rng, n1 - F))[:n1 - F]
    if n2 > F:
        s2 += (tail2 if tail2 is not None else acgt(rng, n2 - F))[:n2 - F]
    assert len(s1) == n1 and len(s2) == n2
    return s1, s2


def flip(s, at):
    """s with the base at `at` replaced by another base."""
    s = bytearray(s)
    s[at] = {65: 67, 67: 65, 71: 84, 84: 71}[s[at]]
    return bytes(s)


def mismatch_in_overlap(s1, s2, F, ks):
    """The pair with mate 1 changed at the overlap's positions ks (offsets into [lo, hi))."""
    lo = max(0, F - len(s2))
    for k in ks:
        s1 = flip(s1, lo + k)
    return s1, s2


def edge_pairs(min_overlap, M, seed=5):
    """[(s1, s2)] of the issue's edge list for one parameter set (lengths up to 70
    unless the case is about length)."""
    rng = np.random.default_rng(seed)
    mo = min_overlap
    out = []
    if mo <= 40:
        # every F, mates of 40 and 70 bases
        for n1, n2 in ((40, 70), (70, 40), (40, 40), (70, 70)):
            for F in range(mo, n1 + n2 - mo + 1):
                out.append(pair_of(rng, n1, n2, F))
        # ov = min_overlap - 1 at both ends of the range
        for n1, n2 in ((40, 70), (70, 40)):
            out += [pair_of(rng, n1, n2, mo - 1), pair_of(rng, n1, n2, n1 + n2 - mo + 1)]
    # exactly M and M + 1 mismatches at the first, last and every 32nd position of the overlap
    for n, F in ((150, 100), (150, 150), (150, 230), (300, 290), (512, 512)):
        ov = min(n, F) - max(0, F - n)
        if ov < mo:
            continue
        at = sorted({0, ov - 1, *range(32, ov - 1, 32), *range(31, ov - 1, 32)})
        at += [k for k in range(1, ov - 1, 2) if k not in at]       # (more than those: every other position)
        for count in (M, M + 1):
            for first in (at[:count], at[-count:] if count else []):
                out.append(mismatch_in_overlap(*pair_of(rng, n, n, F), F, first))
    # lengths
    for n in (31, 32, 33, 63, 64, 65, 511, 512):
        if n < mo:
            out.append(pair_of(rng, n, n, n))
            continue
        out += [pair_of(rng, n, n, n), pair_of(rng, n, n, max(mo, n - 7)), pair_of(rng, n, 70, max(mo, min(n, 70) - 3)),
                pair_of(rng, 70, n, max(mo, min(n, 70) - 3)), pair_of(rng, n, n, 2 * n - mo)]
    # skipped
    out += [pair_of(rng, 513, 100, 90), pair_of(rng, 100, 513, 90), pair_of(rng, 70000, 150, 120)]
    # candidate counts 63, 64, 65, 128, 129: n1 + n2 - 2 mo + 1 of them, the match at the top, at the bottom, nowhere
    for cnt in (63, 64, 65, 128, 129):
        total = cnt - 1 + 2 * mo
        n1 = total // 2
        n2 = total - n1
        if max(n1, n2) > MAX_LEN:
            continue
        out += [pair_of(rng, n1, n2, total - mo), pair_of(rng, n1, n2, mo), (acgt(rng, n1), acgt(rng, n2)),
                pair_of(rng, n1, n2, total - mo - 63), pair_of(rng, n1, n2, total - mo - 64)]
    # N, lower case and other byte values facing themselves and facing a base
    if mo <= 60:
        for v in (ord("N"), ord("a"), ord("c"), ord("g"), ord("t"), ord("n"), 0, 0x20, 0x45, 0x55, 0x80, 0xC1, 0xD4, 0xFF):
            for count in (M, M + 1):
                s1, s2 = pair_of(rng, 100, 100, 80)
                a, b = bytearray(s1), bytearray(s2)
                for k in range(count):          # s1[k] faces s2[79 - k]
                    at = 3 + 7 * k
                    a[at] = v
                    if k % 2 == 0:
                        b[79 - at] = v            # the byte faces itself
                out.append((bytes(a), bytes(b)))
    # a tandem repeat admissible at several F: the greatest wins
    unit = b"ACGTTGCA"
    rep = unit * 16
    out += [(rep[:100], revcomp(rep[:100])), (rep[:100], revcomp(rep[:84])), (b"AT" * 40, b"AT" * 40)]
    # reads of 0 .. 8 bases
    for a in range(9):
        for b in (0, a, 8, 50):
            out.append((acgt(rng, a), acgt(rng, b)))
    out += [pair_of(rng, 8, 8, 8), pair_of(rng, 8, 50, 8)]
    return out


def random_pairs(n, seed, L=(20, 160)):
    """n pairs: two in three from a fragment shorter than the reads' sum, a few
    mismatches and Ns in some, the rest unrelated."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        n1, n2 = int(rng.integers(L[0], L[1])), int(rng.integers(L[0], L[1]))
        if i % 3 != 2:
            F = int(rng.integers(20, n1 + n2))
            s1, s2 = pair_of(rng, n1, n2, F)
            if i % 4 == 0:
                for _ in range(int(rng.integers(0, 8))):
                    s1 = flip(s1, int(rng.integers(0, n1)))
            if i % 10 == 0:
                at = int(rng.integers(0, n2))
                s2 = s2[:at] + b"N" + s2[at + 1:]
        else:
            s1, s2 = acgt(rng, n1), acgt(rng, n2)
        out.append((s1, s2))
    return out
