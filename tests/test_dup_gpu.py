"""`stats --duplication` on the GPU: hpgq_dup_* (gfx950) against tests/dup_ref.py,
bit for bit.  A lane owns 16 bytes, a segment of 10
lanes one read (160 bytes per pass), a read longer than 2048 the whole wave
(1024 bytes per pass); the table keeps its load at or below 1/2."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import dup_ref

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150, 159, 160, 161, 250, 511, 512, 513, 1000, 5003, 70001]
LEAD = 5   # data_indices are absolute: the first read starts here, not at 0


def _dev(seqs, mask=None, offset=0):
    """Device copies of a list of bytes objects.  The sequence pointer is
    `offset` bytes into a larger (256-byte aligned) buffer; LEAD garbage bytes
    come before the first read and HPGQ_DEVICE_SLACK nonzero garbage bytes
    after the last; only the sequence pointer of the batch is set."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(len(seqs) + offset)
    idx = np.zeros(len(seqs) + 1, dtype=np.int64)
    idx[1:] = np.cumsum([len(s) for s in seqs])
    assert idx[-1] + LEAD < 2 ** 31
    body = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:-1]
    buf = np.concatenate([rng.integers(1, 256, size=offset + LEAD, dtype=np.uint8), body,
                          rng.integers(1, 256, size=H.DEVICE_SLACK, dtype=np.uint8)])
    t = dict(seq=torch.from_numpy(buf).to(dev), idx=torch.from_numpy((idx + LEAD).astype(np.int32)).to(dev))
    if mask is not None:
        t["mask"] = torch.from_numpy(np.asarray(mask, dtype=np.uint8)).to(dev)
    torch.cuda.synchronize()
    assert t["seq"].data_ptr() % 8 == 0
    t["batch"] = H.engine.device_batch(len(seqs), t["seq"].data_ptr() + offset, 0, t["idx"].data_ptr())
    return t


def _count(d, seqs, mask=None, offset=0, keep=None):
    t = _dev(seqs, mask, offset)
    d.count_device(t["batch"], t["mask"].data_ptr() if mask is not None else None)
    if keep is None:
        d.sync()
    else:
        keep.append(t)


def _check(d, want):
    """Export and levels of the table against a reference {fingerprint: count}."""
    keys, counts = d.export()
    wk, wc = dup_ref.arrays(want)
    np.testing.assert_array_equal(keys, wk)
    np.testing.assert_array_equal(counts, wc)
    assert d.levels() == dup_ref.levels_of_table(want)


def _masked(seqs, mask):
    return [s for s, m in zip(seqs, mask) if m == 1]


def _distinct(rng, n, lo, hi, alphabet=b"ACGTN"):
    """n different sequences of lo..hi bytes."""
    out, seen = [], set()
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    while len(out) < n:
        s = letters[rng.integers(0, len(letters), size=int(rng.integers(lo, hi + 1)))].tobytes()
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


@pytest.fixture(scope="module")
def edge_reads():
    """Three reads of every length, all 256 byte values, in a shuffled order
    (so the reads of one wave step differ in length), with their fingerprints."""
    rng = np.random.default_rng(41)
    seqs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in LENGTHS for _ in range(3)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    return seqs, np.array([dup_ref.fingerprint(s) for s in seqs], dtype=np.uint64)


@pytest.mark.parametrize("offset", range(8))
def test_fingerprints_per_read(edge_reads, offset):
    seqs, want = edge_reads
    with H.Duplication(log2_slots=4) as d:
        t = _dev(seqs, offset=offset)
        np.testing.assert_array_equal(d.fingerprints(t["batch"]), want)
        assert d.levels()["reads"] == 0          # nothing was inserted


def test_host_and_device_fingerprints_agree(edge_reads):
    seqs, want = edge_reads
    assert [H.dup_fingerprint(s) for s in seqs] == [int(x) for x in want]


@pytest.fixture(scope="module")
def mixed_reads():
    """20,000 reads drawn from 3,000 sequences, levels 1 .. >=100 all populated."""
    rng = np.random.default_rng(42)
    base = _distinct(rng, 2990, 1, 300)
    x, y = base[0] + b"ACGTACGTAC", base[1] + b"TTTTTTTTTTTTTTTTTTTT"
    special = [b"",                          # empty reads
               x, x[:-5],                    # one a prefix of the other
               y, y + b"\0", y + b"\0\0",    # the same bytes followed by NULs
               x[:-1] + b"G", x[:-1] + b"T",  # differ in the last byte only
               b"\0", b"\0" * 8]
    seqs = special + base
    assert len(seqs) == 3000 and len(set(seqs)) == 3000
    mult = rng.integers(1, 10, size=3000)
    mult[:10] = [7, 150, 120, 60, 55, 30, 12, 10, 3, 2]
    mult[10:20] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    assert mult.sum() < 20000
    mult[1] += 20000 - mult.sum()
    order = rng.permutation(np.repeat(np.arange(3000), mult))
    reads = [seqs[i] for i in order]
    want = dup_ref.table(reads)
    lv = dup_ref.levels_of_table(want)
    assert lv["reads"] == 20000 and lv["distinct"] == 3000 and all(lv["distinct_at"][:12])
    return reads, want


def test_levels_and_export(mixed_reads):
    reads, want = mixed_reads
    with H.Duplication(log2_slots=10) as d:
        _count(d, reads, offset=3)
        _check(d, want)
        assert H.dup_levels_of(d.export()[1]) == d.levels()


def test_one_hot_sequence():
    rng = np.random.default_rng(43)
    hot, *single = _distinct(rng, 101, 150, 150)
    reads = [hot] * 50000 + single
    reads = [reads[i] for i in rng.permutation(len(reads))]
    want = dup_ref.table(reads)
    with H.Duplication(log2_slots=12) as d:
        _count(d, reads)
        _check(d, want)
        lv = d.levels()
        assert lv["max_count"] == 50000 and lv["distinct_at"][15] == 1 and lv["distinct_at"][0] == 100


def test_growth_keeps_counts():
    """From 2^4 slots: a ramp of small batches (one growth each), then three
    batches of 5,000 mostly distinct reads: at least 8 rehashes, counts kept."""
    rng = np.random.default_rng(44)
    pool = _distinct(rng, 61100, 30, 40)
    ramp = [pool[:9], pool[9:25], pool[25:60], pool[60:130], pool[130:270], pool[270:550], pool[550:1100]]
    big = [[pool[int(i)] for i in rng.integers(1100 + 20000 * k, 1100 + 20000 * (k + 1), size=5000)] for k in range(3)]
    big[1][:50] = big[0][:50]                    # some sequences of an earlier batch again
    big[2][:50] = pool[:50]
    keep, seen = [], []
    with H.Duplication(log2_slots=4, log2_max_slots=20) as d:
        for batch in ramp + big:
            _count(d, batch, keep=keep)
            seen += batch
        d.sync()
        want = dup_ref.table(seen)
        assert len(want) > 10000
        _check(d, want)
        log2, rehashes = d.info()
        assert rehashes >= 8 and (1 << log2) >= 2 * len(want)


def test_cap_is_nomem_then_reset():
    rng = np.random.default_rng(45)
    reads = _distinct(rng, 1000, 30, 40)
    with H.Duplication(log2_slots=6, log2_max_slots=8) as d:
        _count(d, reads[:100])
        t = _dev(reads)
        with pytest.raises(H.HpgqError) as e:
            d.count_device(t["batch"], None)
        assert e.value.code == H.E_NOMEM
        _check(d, dup_ref.table(reads[:100]))    # the table is as it was
        d.reset()
        small = reads[:60] + reads[:20]
        _count(d, small)
        _check(d, dup_ref.table(small))


def test_probe_chains_through_import():
    """300 keys with one home slot, cap - 3 of a 2^10-slot table: the chain
    wraps.  200 of them again (their counts double in place; 500 keys are the
    most the host's bound lets 1024 slots take), a count of 2^33 twice, then
    all 300 again: the bound cannot know they are there already, so the table
    grows once and the wrapped chain is rehashed with its counts."""
    cap = 1 << 10
    rng = np.random.default_rng(46)
    high = rng.permutation(1 << 20)[:300].astype(np.uint64) + np.uint64(1)
    keys = (high << np.uint64(10)) | np.uint64(cap - 3)
    counts = rng.integers(1, 1000, size=300).astype(np.uint64)
    want = {int(k): int(c) for k, c in zip(keys, counts)}
    with H.Duplication(log2_slots=10, log2_max_slots=12) as d:
        d.import_(keys, counts)
        _check(d, want)
        assert d.info() == (10, 0)
        d.import_(keys[199::-1], counts[199::-1])
        for k, c in zip(keys[:200], counts[:200]):
            want[int(k)] += int(c)
        _check(d, want)
        assert d.info() == (10, 0)
        big = np.array([(7 << 10) | 5], dtype=np.uint64)
        for _ in range(2):
            d.import_(big, np.array([1 << 33], dtype=np.uint64))
        want[int(big[0])] = 1 << 34
        _check(d, want)
        assert d.info() == (10, 0)
        d.import_(keys, counts)
        for k, c in zip(keys, counts):
            want[int(k)] += int(c)
        _check(d, want)
        assert d.info() == (11, 1)
        more = ((high + np.uint64(1 << 21)) << np.uint64(10)) | np.uint64(cap - 3)   # 300 other keys, same chain
        d.import_(more, counts)
        want.update({int(k): int(c) for k, c in zip(more, counts)})
        _check(d, want)
        assert d.info() == (11, 1)
        for bad in ((np.array([0], np.uint64), np.array([1], np.uint64)),
                    (np.array([9], np.uint64), np.array([0], np.uint64))):
            with pytest.raises(H.HpgqError) as e:
                d.import_(*bad)
            assert e.value.code == H.E_INVALID
        _check(d, want)


def test_mask_batches_and_reset():
    rng = np.random.default_rng(47)
    pool = _distinct(rng, 800, 0, 200)
    batches = [[pool[int(i)] for i in rng.integers(0, 800, size=2000)] for _ in range(3)]
    masks = [(rng.random(2000) < 0.6).astype(np.uint8) for _ in range(3)]
    masks[1][:] = 0                                      # one batch all masked out
    masks[2][7] = 2                                      # (only mask == 1 counts)
    want = dup_ref.table([s for b, m in zip(batches, masks) for s in _masked(b, m)])
    keep = []
    with H.Duplication(log2_slots=8) as d:
        for b, m in zip(batches, masks):
            _count(d, b, m, offset=1, keep=keep)
        d.count_device(H.engine.device_batch(0, 0, 0, 0), None)   # one batch empty
        d.sync()
        _check(d, want)
        d.reset()
        _count(d, batches[0], masks[0])
        _check(d, dup_ref.table(_masked(batches[0], masks[0])))
        d.reset()
        _check(d, {})


def test_several_groups_per_workgroup(mixed_reads):
    reads, want = mixed_reads
    with H.Duplication(log2_slots=6) as d:
        d.set_max_workgroups(2)
        _count(d, reads, offset=6)
        _check(d, want)


def test_merge_of_half_tables(mixed_reads):
    reads, want = mixed_reads
    with H.Duplication(log2_slots=8) as a, H.Duplication(log2_slots=8) as b, H.Duplication(log2_slots=4) as c:
        _count(a, reads[:9000])
        _count(b, reads[9000:], offset=2)
        ea, eb = a.export(), b.export()
        assert set(ea[0]) & set(eb[0])                   # one sequence may be in both halves
        c.import_(*ea)
        c.import_(*eb)
        _check(c, want)
        a.import_(*eb)
        _check(a, want)


def _engine_dev(reads):
    import torch
    dev = torch.device("cuda", 0)
    pad = np.zeros(H.DEVICE_SLACK, np.uint8)
    t = dict(seq=torch.from_numpy(np.concatenate([reads.seq, pad])).to(dev),
             qual=torch.from_numpy(np.concatenate([reads.qual, pad])).to(dev),
             idx=torch.from_numpy(reads.idx).to(dev))
    t["batch"] = H.engine.device_batch(reads.n, t["seq"].data_ptr(), t["qual"].data_ptr(), t["idx"].data_ptr())
    return t


def _with_duplicates(reads, rng):
    """The same batch with a third of its reads replaced by copies of others."""
    pairs = reads.pairs()
    for i in rng.integers(0, len(pairs), size=len(pairs) // 3):
        pairs[int(i)] = pairs[int(rng.integers(0, 200))]
    return O.Reads.from_pairs(pairs)


def test_on_the_engines_stream_with_its_mask():
    import torch
    reads = _with_duplicates(O.synth(20_000, seed=51, L=150), np.random.default_rng(51))
    p = H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,")
    m_o, _, _ = O.run(p, reads)
    assert 0 < int(m_o.sum()) < reads.n
    t = _engine_dev(reads)
    mask = torch.zeros(reads.n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with H.Engine(p) as e, H.Duplication(log2_slots=10, stream=e.stream) as d:
        e.run_device(t["batch"], None, mask.data_ptr(), None)
        d.count_device(t["batch"], mask.data_ptr())      # no sync between: the stream orders them
        d.sync()
        np.testing.assert_array_equal(mask.cpu().numpy(), m_o)
        want = dup_ref.table_of(reads, m_o)
        assert max(want.values()) > 10
        _check(d, want)


def test_paired_two_tables_one_pair_mask():
    import torch
    rng = np.random.default_rng(52)
    r1 = _with_duplicates(O.synth(10_000, seed=52, L=150), rng)
    r2 = _with_duplicates(O.synth(10_000, seed=152, L=150, trunc_pct=30), rng)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    m_o, _, _ = O.run(p, r1, r2)
    assert 0 < int(m_o.sum()) < r1.n
    t1, t2 = _engine_dev(r1), _engine_dev(r2)
    mask = torch.zeros(r1.n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with H.Engine(p) as e, H.Duplication(log2_slots=10, stream=e.stream) as d1, \
            H.Duplication(log2_slots=10, stream=e.stream) as d2:
        e.run_device(t1["batch"], t2["batch"], mask.data_ptr(), None)
        d1.count_device(t1["batch"], mask.data_ptr())
        d2.count_device(t2["batch"], mask.data_ptr())
        d1.sync()
        _check(d1, dup_ref.table_of(r1, m_o))
        _check(d2, dup_ref.table_of(r2, m_o))
