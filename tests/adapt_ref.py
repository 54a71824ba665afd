"""Reference for `stats --adapters`, written from DESIGN.md §2.11 alone: pure
Python, bytes.find per read and probe, no code shared with the product (tests
only).

A probe occurs at j of a read iff the read's bytes [j, j + K) equal the probe's
as they stand.  For every counted read (mask[i] == 1; all without a mask) and
every probe that occurs in it, first[a][p] += 1 at the lowest such p.  reads:
the counted reads; with_any: those with at least one probe; npos: the longest
counted read."""
import numpy as np

DEFAULTS = [
    (b"Illumina Universal Adapter", b"AGATCGGAAGAG"),
    (b"Illumina Small RNA 3' Adapter", b"TGGAATTCTCGG"),
    (b"Illumina Small RNA 5' Adapter", b"GATCGTCGGACT"),
    (b"Nextera Transposase Sequence", b"CTGTCTCTTATA"),
    (b"PolyA", b"AAAAAAAAAAAA"),
    (b"PolyG", b"GGGGGGGGGGGG"),
]
DEFAULT_PROBES = [p for _, p in DEFAULTS]


def table(seq, idx, probes, mask=None):
    """(first u64 (nprobes, npos), dict(reads, with_any, nprobes, npos))."""
    blob = bytes(np.asarray(seq, dtype=np.uint8))
    idx = [int(x) for x in idx]
    probes = [bytes(p) for p in probes]
    hits, reads, with_any, npos = [], 0, 0, 0
    for i in range(len(idx) - 1):
        if mask is not None and int(mask[i]) != 1:
            continue
        s = blob[idx[i]:idx[i + 1]]
        reads += 1
        npos = max(npos, len(s))
        found = False
        for a, p in enumerate(probes):
            j = s.find(p)
            if j >= 0:
                hits.append((a, j))
                found = True
        with_any += found
    first = np.zeros((len(probes), npos), dtype=np.uint64)
    for a, j in hits:
        first[a, j] += np.uint64(1)
    return first, dict(reads=reads, with_any=with_any, nprobes=len(probes), npos=npos)


def table_of(reads, probes, mask=None):
    return table(reads.seq, reads.idx, probes, mask)


def add(results):
    """The merge of shards: first row by row at the longer npos, the scalars added."""
    npos = max([r[1]["npos"] for r in results] + [0])
    nprobes = results[0][1]["nprobes"]
    first = np.zeros((nprobes, npos), dtype=np.uint64)
    info = dict(reads=0, with_any=0, nprobes=nprobes, npos=npos)
    for f, i in results:
        first[:, :f.shape[1]] += f
        info["reads"] += i["reads"]
        info["with_any"] += i["with_any"]
    return first, info


def render(first, info, names):
    """The bytes of <base>.adapter.content.data (first: rows of Python ints or u64)."""
    reads, with_any = int(info["reads"]), int(info["with_any"])
    out = [b"# Reads\tWith adapter\t% with adapter\n",
           ("%d\t%d\t%.2f\n" % (reads, with_any, 100.0 * with_any / reads if reads else 0.0)).encode(),
           b"# Position" + b"".join(b"\t" + bytes(n) for n in names) + b"\n"]
    cum = [0] * len(names)
    for p in range(int(info["npos"])):
        cells = []
        for a in range(len(names)):
            cum[a] = (cum[a] + int(first[a][p])) % (1 << 64)
            cells.append("%.4f" % (100.0 * cum[a] / reads if reads else 0.0))
        out.append(("%d\t" % (p + 1) + "\t".join(cells) + "\n").encode())
    return b"".join(out)


def parse_dump(blob, mates=1):
    """--adapters-out: per mate [nprobes u64 | npos u64 | reads u64 | with_any u64
    | first u64 [nprobes][npos]] -> [(first, info)]."""
    a = np.frombuffer(blob, dtype=np.uint64)
    out, o = [], 0
    for _ in range(mates):
        nprobes, npos, reads, with_any = (int(x) for x in a[o:o + 4])
        first = a[o + 4:o + 4 + nprobes * npos].reshape(nprobes, npos).copy()
        out.append((first, dict(reads=reads, with_any=with_any, nprobes=nprobes, npos=npos)))
        o += 4 + nprobes * npos
    assert o == len(a), (o, len(a))
    return out
