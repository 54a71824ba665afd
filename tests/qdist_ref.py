"""Reference for `stats --quality-dist`, written from DESIGN.md §2.8 alone: pure
numpy and Python integers, no code shared with the product (tests only).

Table: every base j of every counted read adds 1 to hist[j][b], b the raw
quality byte as an unsigned index; as many rows as the longest counted read.
Quantiles: per position, over the bytes in ascending SIGNED order (128..255
before 0..127), the smallest Q = (signed char)b - phred whose cumulative count
reaches max(1, ceil(num * c / den))."""
import numpy as np

QUANTILES = ((1, 10), (1, 4), (1, 2), (3, 4), (9, 10))
HEADER = b"# Position\tCount\tMin\tP10\tQ1\tMedian\tQ3\tP90\tMax\n"


def table(qual, idx, mask=None):
    """(npos, 256) u64 over the reads with mask[i] == 1 (all without a mask)."""
    idx = np.asarray(idx, dtype=np.int64)
    lens = np.diff(idx)
    keep = np.ones(len(lens), bool) if mask is None else (np.asarray(mask) == 1)
    npos = int(lens[keep].max()) if keep.any() else 0
    hist = np.zeros((npos, 256), dtype=np.uint64)
    if npos == 0:
        return hist
    starts, lk = idx[:-1][keep], lens[keep]
    total = int(lk.sum())
    if total == 0:
        return hist
    # position of every counted base within its read, and where its byte is
    first = np.repeat(np.cumsum(lk) - lk, lk)
    pos = np.arange(total, dtype=np.int64) - first
    src = np.repeat(starts, lk) + pos
    np.add.at(hist, (pos, np.asarray(qual)[src].astype(np.int64)), np.uint64(1))
    return hist


def table_of(reads, mask=None):
    return table(reads.qual, reads.idx, mask)


def add(tables):
    """Sum of tables of different heights."""
    npos = max([t.shape[0] for t in tables] + [0])
    out = np.zeros((npos, 256), dtype=np.uint64)
    for t in tables:
        out[:t.shape[0]] += t
    return out


def quantile_row(row, phred):
    """[c, min, p10, q1, median, q3, p90, max] of one position (Python ints)."""
    counts = [int(x) for x in row]
    c = sum(counts)
    if c == 0:
        return [0] * 8
    order = list(range(128, 256)) + list(range(0, 128))
    present = [b for b in order if counts[b]]

    def q_of(b):
        return (b - 256 if b >= 128 else b) - phred

    out = [c, q_of(present[0])]
    for num, den in QUANTILES:
        rank = max(1, -((-num * c) // den))
        cum = 0
        for b in order:
            cum += counts[b]
            if cum >= rank:
                out.append(q_of(b))
                break
    out.append(q_of(present[-1]))
    return out


def quantiles(hist, phred):
    """(npos, 8) object array of Python ints (counts may reach 2^64 - 1)."""
    return [quantile_row(hist[p], phred) for p in range(hist.shape[0])]


def render(hist, phred):
    """The bytes of <base>.quality.dist.per.nt.data."""
    lines = [HEADER]
    for p, r in enumerate(quantiles(hist, phred)):
        lines.append(("\t".join(str(x) for x in [p + 1] + r) + "\n").encode())
    return b"".join(lines)


def parse_dump(blob, mates=1):
    """--quality-dist-out: per mate [npos u64 | hist u64 [npos][256]]."""
    a = np.frombuffer(blob, dtype=np.uint64)
    out, o = [], 0
    for _ in range(mates):
        npos = int(a[o])
        out.append(a[o + 1:o + 1 + npos * 256].reshape(npos, 256).copy())
        o += 1 + npos * 256
    assert o == len(a), (o, len(a))
    return out
