"""Reference for `edit --clip-adapters`, written from DESIGN.md §2.12 alone: pure
Python, bytes.find for whole occurrences and a suffix / prefix comparison for a
read that ends inside the adapter; no code shared with the product (tests only).

Probe a of K bytes matches at j of a read s of n bytes iff, with m = min(K, n - j),
s[j:j + m] == probe[:m] and (m == K or m >= min_overlap).  c is the lowest such j
over all probes (n: none); the winner is the lowest probe that matches at c
(0xFF: none)."""
import numpy as np

NONE = 0xFF


def find(s, probes, min_overlap=8):
    """(c, winner) of the bytes s."""
    s = bytes(s)
    n = len(s)
    c, who = n, NONE
    for a, p in enumerate(probes):
        p = bytes(p)
        at = []
        j = s.find(p)
        if j >= 0:
            at.append(j)
        for m in range(min(len(p) - 1, n), min_overlap - 1, -1):    # the longest overlap starts lowest
            if s[n - m:] == p[:m]:
                at.append(n - m)
                break
        if at and min(at) < c:                                      # (a tie keeps the lower probe)
            c, who = min(at), a
    return c, who


class Clipped:
    """What the clip makes of a batch: pos u32 [n], probe u8 [n], idx int32 [n + 1]
    from 0, the kept sequence and quality bytes, and the scalars."""

    def __init__(self, reads, probes, min_overlap=8):
        blob = bytes(np.asarray(reads.seq, np.uint8))
        idx = [int(x) for x in reads.idx]
        n = len(idx) - 1
        self.pos = np.zeros(n, np.uint32)
        self.probe = np.zeros(n, np.uint8)
        keep = np.zeros(len(blob), bool)
        for i in range(n):
            c, who = find(blob[idx[i]:idx[i + 1]], probes, min_overlap)
            self.pos[i], self.probe[i] = c, who
            keep[idx[i]:idx[i] + c] = True
        self.idx = np.zeros(n + 1, np.int32)
        self.idx[1:] = np.cumsum(self.pos.astype(np.int64))
        self.seq = np.asarray(reads.seq, np.uint8)[keep]
        self.qual = np.asarray(reads.qual, np.uint8)[keep]
        lens = np.diff(np.asarray(idx, np.int64))
        self.info = dict(reads=n, clipped=int((self.pos < lens).sum()), bases_removed=int((lens - self.pos).sum()),
                         by_probe=[int((self.probe == a).sum()) for a in range(len(probes))], nprobes=len(probes),
                         min_overlap=min_overlap)


def add(infos):
    """The scalars of several batches (or workers, or shards): plain sums."""
    out = dict(infos[0], by_probe=list(infos[0]["by_probe"]))
    for i in infos[1:]:
        for k in ("reads", "clipped", "bases_removed"):
            out[k] += i[k]
        out["by_probe"] = [x + y for x, y in zip(out["by_probe"], i["by_probe"])]
    return out


def _pct(num, den):
    return 100.0 * num / den if den else 0.0


def render(info, names):
    """The bytes of <base>.adapter.clip.data."""
    reads = int(info["reads"])
    out = [b"# Reads\tClipped\t% clipped\tBases removed\n",
           ("%d\t%d\t%.2f\t%d\n" % (reads, info["clipped"], _pct(info["clipped"], reads), info["bases_removed"])).encode(),
           b"# Adapter\tReads\t% of reads\n"]
    for name, won in zip(names, info["by_probe"]):
        out.append(bytes(name) + ("\t%d\t%.2f\n" % (won, _pct(won, reads))).encode())
    return b"".join(out)


def clip_records(records, probes, min_overlap=8):
    """[(name, seq, qual)] cut by the rule, and the scalars."""
    out, pos, who = [], [], []
    for name, s, q in records:
        c, a = find(s, probes, min_overlap)
        out.append((name, s[:c], q[:c]))
        pos.append(c)
        who.append(a)
    info = dict(reads=len(records), clipped=sum(c < len(r[1]) for c, r in zip(pos, records)),
                bases_removed=sum(len(r[1]) - c for c, r in zip(pos, records)),
                by_probe=[who.count(a) for a in range(len(probes))], nprobes=len(probes), min_overlap=min_overlap)
    return out, info
