"""Reference for `stats --overrepresented`, written from DESIGN.md §2.10 alone:
Python dicts and sorted(), no code shared with the product (tests only).

Two reads are the same sequence iff their bytes are equal; the reference counts
by BYTES.  `count_map` asserts through dup_ref.table that no two different
sequences of its input share a fingerprint, so for its inputs "equal to the
reference" and "exact" are the same statement.

The list: the entries with count >= min_count, count descending, ties by
fingerprint ascending (unsigned), cut to the first n.  The file: a header line,
then per entry rank (from 1), count, 100 * count / reads with four decimals
(0.0000 when reads is 0), length, and the sequence's bytes as they stand."""
import dup_ref

HEADER = b"# Rank\tCount\t% of reads\tLength\tSequence\n"


def count_map(seqs):
    """{bytes: count} of a list of bytes objects."""
    by_bytes = {}
    for s in seqs:
        by_bytes[s] = by_bytes.get(s, 0) + 1
    by_key = dup_ref.table(seqs)           # asserts: one fingerprint per sequence
    assert len(by_key) == len(by_bytes)
    for s, c in by_bytes.items():
        assert by_key[dup_ref.fingerprint(s)] == c
    return by_bytes


def select_pairs(pairs, n, min_count=1):
    """pairs: iterable of (key, count).  -> ([(key, count)] the first n, total)."""
    hits = [(int(k), int(c)) for k, c in pairs if int(k) != 0 and int(c) >= min_count]
    hits.sort(key=lambda kc: (-kc[1], kc[0]))
    return hits[:n], len(hits)


def select(seqs, n, min_count=1):
    """-> ([(key, count, bytes)] the first n in list order, total)."""
    cm = count_map(seqs)
    by_key = {dup_ref.fingerprint(s): s for s in cm}
    hits, total = select_pairs(((k, cm[s]) for k, s in by_key.items()), n, min_count)
    return [(k, c, by_key[k]) for k, c in hits], total


def kept(seqs, threshold):
    """(sequences with count >= threshold, the sum of their lengths)."""
    cm = count_map(seqs)
    hit = [s for s, c in cm.items() if c >= threshold]
    return len(hit), sum(len(s) for s in hit)


def render(entries, reads):
    """The bytes of <base>.overrepresented.data: entries [(key, count, bytes)] in list order."""
    out = [HEADER]
    for rank, (_, c, s) in enumerate(entries, 1):
        pct = 100.0 * c / reads if reads else 0.0
        out.append(("%d\t%d\t%.4f\t%d\t" % (rank, c, pct, len(s))).encode() + bytes(s) + b"\n")
    return b"".join(out)


def render_reads(seqs, n, min_count):
    """The file of a run over the counted reads `seqs`."""
    entries, _ = select(seqs, n, min_count)
    return render(entries, len(seqs))
