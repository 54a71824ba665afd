"""Reference for `stats --duplication`, written from DESIGN.md §2.9 alone: Python
integers and dicts, no code shared with the product (tests only).

Fingerprint (mod 2^64): G = 0x9E3779B97F4A7C15; mix(x): x ^= x >> 30; x *=
0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.  For n
bytes s, w_j = the little-endian 8-byte word s[8j .. 8j+8), zero padded, j <
ceil(n / 8); S = sum mix(w_j + (j+1) G); fp = mix(S ^ n G), 1 if that is 0.

The table is counted twice: by fingerprint and by the sequence BYTES.  `table`
asserts that no two different sequences share a fingerprint, so for its inputs
"equal to the reference" and "exact" are the same statement."""
import numpy as np

M = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
BOUNDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)
LABELS = ("1", "2", "3", "4", "5", "6", "7", "8", "9", ">=10", ">=50", ">=100", ">=500", ">=1000", ">=5000",
          ">=10000")
HEADER1 = b"# Reads\tDistinct\tHighest count\t% distinct\n"
HEADER2 = b"# Level\tSequences\tReads\t% of sequences\t% of reads\n"


def mix(x):
    x &= M
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def fingerprint(s):
    s = bytes(s)
    n = len(s)
    total = 0
    for j in range((n + 7) // 8):
        w = int.from_bytes(s[8 * j:8 * j + 8].ljust(8, b"\0"), "little")
        total = (total + mix(w + (j + 1) * G)) & M
    fp = mix(total ^ ((n * G) & M))
    return fp if fp else 1


def sequences(seq, idx, mask=None):
    """The counted reads' sequences as bytes objects."""
    raw = np.asarray(seq, dtype=np.uint8).tobytes()
    idx = [int(x) for x in idx]
    return [raw[idx[i]:idx[i + 1]] for i in range(len(idx) - 1) if mask is None or int(mask[i]) == 1]


def table(seqs):
    """{fingerprint: count} of a list of bytes objects; asserts that the count
    by bytes says the same (no two different sequences with one fingerprint)."""
    by_bytes = {}
    for s in seqs:
        by_bytes[s] = by_bytes.get(s, 0) + 1
    out = {}
    for s, c in by_bytes.items():
        fp = fingerprint(s)
        assert fp not in out, "two different sequences with one fingerprint: not a valid test input"
        out[fp] = c
    return out


def table_of(reads, mask=None):
    return table(sequences(reads.seq, reads.idx, mask))


def merge(tables):
    out = {}
    for t in tables:
        for k, c in t.items():
            out[k] = out.get(k, 0) + c
    return out


def arrays(tab):
    """(keys ascending, counts in key order) as u64 arrays."""
    keys = sorted(tab)
    return np.array(keys, dtype=np.uint64), np.array([tab[k] for k in keys], dtype=np.uint64)


def level_of(c):
    lv = 0
    for i, lo in enumerate(BOUNDS):
        if c >= lo:
            lv = i
    return lv


def levels(counts):
    """dict as hpgfastq's: sums mod 2^64, zeros are no sequence."""
    out = dict(reads=0, distinct=0, max_count=0, distinct_at=[0] * 16, reads_at=[0] * 16)
    for c in counts:
        c = int(c)
        if c == 0:
            continue
        lv = level_of(c)
        out["distinct_at"][lv] += 1
        out["reads_at"][lv] = (out["reads_at"][lv] + c) & M
        out["distinct"] += 1
        out["reads"] = (out["reads"] + c) & M
        out["max_count"] = max(out["max_count"], c)
    return out


def levels_of_table(tab):
    return levels(tab.values())


def _pct(a, b):
    return "%.2f" % (100.0 * a / b if b else 0.0)


def render(lv):
    """The bytes of <base>.duplication.data."""
    lines = [HEADER1, ("%d\t%d\t%d\t%s\n" % (lv["reads"], lv["distinct"], lv["max_count"],
                                              _pct(lv["distinct"], lv["reads"]))).encode(), HEADER2]
    for i, name in enumerate(LABELS):
        lines.append(("%s\t%d\t%d\t%s\t%s\n" % (name, lv["distinct_at"][i], lv["reads_at"][i],
                                                _pct(lv["distinct_at"][i], lv["distinct"]),
                                                _pct(lv["reads_at"][i], lv["reads"]))).encode())
    return b"".join(lines)


def parse_dump(blob, mates=1):
    """--duplication-out: per mate [n u64 | n keys ascending | n counts in key order]."""
    a = np.frombuffer(blob, dtype=np.uint64)
    out, o = [], 0
    for _ in range(mates):
        n = int(a[o])
        out.append((a[o + 1:o + 1 + n].copy(), a[o + 1 + n:o + 1 + 2 * n].copy()))
        o += 1 + 2 * n
    assert o == len(a), (o, len(a))
    return out
