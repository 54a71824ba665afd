"""`stats --overrepresented` on the GPU: hpgq_dup_keep_sequences / _top /
_sequence (gfx950) against tests/overrep_ref.py, byte for byte (DESIGN.md
§2.10, §4.12).  After every batch's insert a lane per read looks its key up;
a key at or above the threshold without a representative is claimed once and
its bytes are copied into the table's arena by the whole wave, 16 bytes per
lane per pass."""
import ctypes as C

import numpy as np
import pytest

import hpgfastq as H
import dup_ref
import overrep_ref

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


def _count(d, seqs, mask=None, offset=0):
    t = _dev(seqs, mask, offset)
    d.count_device(t["batch"], t["mask"].data_ptr() if mask is not None else None)
    d.sync()


def _check_counts(d, want):
    keys, counts = d.export()
    wk, wc = dup_ref.arrays(want)
    np.testing.assert_array_equal(keys, wk)
    np.testing.assert_array_equal(counts, wc)
    assert d.levels() == dup_ref.levels_of_table(want)


def _check_kept(d, reads, threshold):
    """Every sequence with count >= threshold is held with its bytes, no other one is."""
    cm = overrep_ref.count_map(reads)
    assert d.kept() == overrep_ref.kept(reads, threshold)
    for s, c in cm.items():
        assert d.sequence(dup_ref.fingerprint(s)) == (s if c >= threshold else None), (len(s), c)


def _distinct(rng, n, lo, hi, alphabet=b"ACGTN"):
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
    """One sequence of every length (all 256 byte values), three times each, shuffled."""
    rng = np.random.default_rng(81)
    one = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in LENGTHS]
    assert one[0] == b"" and dup_ref.fingerprint(one[0]) == 1
    seqs = [s for s in one for _ in range(3)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    longest = max(range(len(seqs)), key=lambda i: len(seqs[i]))
    last = seqs[:longest] + seqs[longest + 1:] + [seqs[longest]]     # its copy ends at the batch's last byte
    assert len(last[-1]) == 70001
    overrep_ref.count_map(seqs)
    return seqs, last


@pytest.mark.parametrize("longest_last", [False, True])
@pytest.mark.parametrize("offset", range(8))
def test_every_length_and_alignment(edge_reads, offset, longest_last):
    seqs = edge_reads[1 if longest_last else 0]
    with H.Duplication(log2_slots=8) as d:
        d.keep_sequences(3)
        _count(d, seqs, offset=offset)
        assert d.kept() == (22, sum(LENGTHS))
        for s in set(seqs):
            assert d.sequence(dup_ref.fingerprint(s)) == s, len(s)


@pytest.fixture(scope="module")
def hot_reads():
    """20,000 reads, 60 % of them one sequence; of the others some occur once."""
    rng = np.random.default_rng(82)
    hot, *pool = _distinct(rng, 6001, 30, 200)
    reads = [hot] * 12000 + [pool[int(i)] for i in rng.integers(0, 6000, size=8000)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    n2, _ = overrep_ref.kept(reads, 2)
    assert 1000 < n2 < len(overrep_ref.count_map(reads)) - 1000
    return reads


@pytest.mark.parametrize("max_wg", [0, 1, 2])
def test_one_copy_per_key_under_contention(hot_reads, max_wg):
    with H.Duplication(log2_slots=12) as d:
        d.keep_sequences(2)
        d.set_max_workgroups(max_wg)
        _count(d, hot_reads, offset=1)
        assert d.kept() == overrep_ref.kept(hot_reads, 2)
        cm = overrep_ref.count_map(hot_reads)
        some = sorted(cm, key=lambda s: -cm[s])[:40] + [s for s in cm if cm[s] == 1][:40]
        for s in some:
            assert d.sequence(dup_ref.fingerprint(s)) == (s if cm[s] >= 2 else None)


def test_threshold_crossed_across_batches():
    rng = np.random.default_rng(83)
    x, y, *fill = _distinct(rng, 42, 100, 160)
    kx, ky = dup_ref.fingerprint(x), dup_ref.fingerprint(y)
    with H.Duplication(log2_slots=8) as d:
        d.keep_sequences(3)
        for b in range(4):
            batch = fill[10 * b:10 * b + 10] + [x] + ([y] if b < 2 else [])
            _count(d, [batch[i] for i in rng.permutation(len(batch))], offset=b)
            assert d.sequence(kx) == (None if b < 2 else x), b
            assert d.sequence(ky) is None
        assert d.kept() == (1, len(x))
        keys, counts = d.top(2)
        assert list(keys) == [kx, ky] and list(counts) == [4, 2]


def test_masked_reads_are_neither_counted_nor_kept():
    rng = np.random.default_rng(84)
    a, b, c = _distinct(rng, 3, 150, 150)
    reads = [a, a, a, a, b, b, b, b, c, c, c]
    mask = [1, 0, 2, 1, 0, 0, 2, 0, 1, 1, 1]      # a: 2 counted of 4, b: none, c: 3
    with H.Duplication(log2_slots=6) as d:
        d.keep_sequences(3)
        _count(d, reads, mask, offset=3)
        _check_counts(d, dup_ref.table([a, a, c, c, c]))
        assert d.sequence(dup_ref.fingerprint(a)) is None
        assert d.sequence(dup_ref.fingerprint(b)) is None
        assert d.sequence(dup_ref.fingerprint(c)) == c
        assert d.kept() == (1, 150)


def test_growth_carries_representatives():
    rng = np.random.default_rng(85)
    pool = _distinct(rng, 3000, 20, 90)
    order = rng.permutation(np.repeat(np.arange(3000), 4))
    seen, carried = [], False
    with H.Duplication(log2_slots=4, log2_max_slots=20) as d:
        d.keep_sequences(2)
        for b in range(6):
            kept_before, grown_before = d.kept()[0], d.info()[1]
            had = [s for s, c in overrep_ref.count_map(seen).items() if c >= 2][:150] if seen else []
            batch = [pool[int(i)] for i in order[2000 * b:2000 * b + 2000]]
            _count(d, batch, offset=b)
            seen += batch
            carried |= kept_before > 0 and d.info()[1] > grown_before
            for s in had:                         # kept before this batch (and its growth): still there
                assert d.sequence(dup_ref.fingerprint(s)) == s
        assert carried and d.info()[1] >= 2
        _check_counts(d, dup_ref.table(seen))
        _check_kept(d, seen, 2)
        assert d.kept() == (3000, sum(len(s) for s in pool))


def test_import_makes_no_representative():
    s = b"ACGTTGCA" * 9
    key = dup_ref.fingerprint(s)
    with H.Duplication(log2_slots=6) as d:
        d.keep_sequences(3)
        d.import_([key], [10])
        assert d.sequence(key) is None and d.kept() == (0, 0)
        _count(d, [s])
        assert d.sequence(key) == s and d.kept() == (1, len(s))
        _check_counts(d, {key: 11})


def test_shards_keep_at_the_ceiling_of_k_over_w():
    rng = np.random.default_rng(86)
    x, y, *fill = _distinct(rng, 12, 80, 150)
    kx, ky = dup_ref.fingerprint(x), dup_ref.fingerprint(y)
    ra = [x, x, x, y, y] + fill[:5]
    rb = [x, x, y, y] + fill[5:]
    with H.Duplication(log2_slots=6) as a, H.Duplication(log2_slots=6) as b:
        a.keep_sequences(3)                       # ceil(5 / 2)
        b.keep_sequences(3)
        _count(a, [ra[i] for i in rng.permutation(len(ra))])
        _count(b, [rb[i] for i in rng.permutation(len(rb))], offset=2)
        b.import_(*a.export())
        keys, counts = b.top(10, 5)
        assert list(keys) == [kx] and list(counts) == [5] and b.count_at_least(5) == 1
        assert b.sequence(kx) is None and a.sequence(kx) == x
        assert a.sequence(ky) is None and b.sequence(ky) is None
        _check_counts(b, dup_ref.table(ra + rb))


@pytest.fixture(scope="module")
def mixed_reads():
    """20,000 reads drawn from 3,000 sequences, counts from 1 to past 100, many ties."""
    rng = np.random.default_rng(87)
    seqs = [b"", b"\0", b"\0" * 8] + _distinct(rng, 2997, 1, 300)
    mult = rng.integers(1, 10, size=3000)
    mult[:10] = [7, 150, 120, 60, 55, 30, 12, 10, 3, 2]
    mult[1] += 20000 - mult.sum()
    order = rng.permutation(np.repeat(np.arange(3000), mult))
    reads = [seqs[i] for i in order]
    assert len(reads) == 20000 and len(overrep_ref.count_map(reads)) == 3000
    return reads


@pytest.mark.parametrize("keeping", [True, False])
def test_top_against_reference(mixed_reads, keeping):
    with H.Duplication(log2_slots=10) as d:
        if keeping:
            d.keep_sequences(10)
        _count(d, mixed_reads, offset=5)
        for n, m in ((1, 1), (20, 1), (50, 10), (10 ** 6, 2), (5, 10 ** 9)):
            want, total = overrep_ref.select(mixed_reads, n, m)
            keys, counts = d.top(n, m)
            assert d.count_at_least(m) == total, (n, m)
            assert [(int(k), int(c)) for k, c in zip(keys, counts)] == [(k, c) for k, c, _ in want], (n, m)
            for k, _, s in want[:30] if keeping and m >= 10 else []:
                assert d.sequence(k) == s
        k2, c2, t2 = H.dup_top_of(*d.export(), 50, 10)
        keys, counts = d.top(50, 10)
        assert list(k2) == list(keys) and list(c2) == list(counts) and t2 == d.count_at_least(10)


def test_state_and_errors():
    rng = np.random.default_rng(88)
    reads = _distinct(rng, 5, 40, 60) * 2
    key = dup_ref.fingerprint(reads[0])
    n = C.c_int64(0)
    with H.Duplication(log2_slots=6) as d:
        with pytest.raises(H.HpgqError) as e:
            d.sequence(key)                                # keeping off
        assert e.value.code == H.E_STATE
        _count(d, reads)
        with pytest.raises(H.HpgqError) as e:
            d.keep_sequences(2)                            # not empty
        assert e.value.code == H.E_STATE
        d.reset()
        for bad in ((1, 0), (1, (1 << 40) + 1)):
            assert H.lib.hpgq_dup_keep_sequences(d._h, *bad) == H.E_INVALID
        d.keep_sequences(2, 1 << 16)
        _count(d, reads, offset=1)
        assert d.kept() == (5, sum(len(s) for s in reads[:5]))
        buf = C.create_string_buffer(8)
        assert H.lib.hpgq_dup_sequence(d._h, key, buf, 8, C.byref(n)) == H.E_INVALID and n.value == len(reads[0])
        assert H.lib.hpgq_dup_sequence(d._h, key ^ 1, None, 0, C.byref(n)) == 0 and n.value == -1   # an absent key
        assert H.lib.hpgq_dup_top(d._h, 0, None, None, 0, C.byref(C.c_size_t(0))) == H.E_INVALID
        d.reset()                                          # drops the representatives, keeps the settings
        assert d.kept() == (0, 0) and d.sequence(key) is None
        _count(d, reads, offset=2)
        assert d.sequence(key) == reads[0]
        d.reset()
        d.keep_sequences(0)                                # off again
        with pytest.raises(H.HpgqError) as e:
            d.sequence(key)
        assert e.value.code == H.E_STATE


def test_arena_overflow_is_sticky_and_harmless():
    rng = np.random.default_rng(89)
    pool = _distinct(rng, 20, 150, 150)
    reads = [pool[i] for i in rng.permutation(np.repeat(np.arange(20), 3))]
    want = dup_ref.table(reads)
    with H.Duplication(log2_slots=8) as d:
        d.keep_sequences(3, 1000)
        t = _dev(reads)
        d.count_device(t["batch"], None)
        with pytest.raises(H.HpgqError) as e:
            d.sync()
        assert e.value.code == H.E_NOMEM
        _check_counts(d, want)
        keys, counts = d.top(100, 3)
        assert sorted(int(k) for k in keys) == sorted(want) and set(int(c) for c in counts) == {3}
        with pytest.raises(H.HpgqError) as e:
            d.sequence(dup_ref.fingerprint(pool[0]))
        assert e.value.code == H.E_NOMEM
        assert d.kept()[0] < 20                            # what fitted, no more than the budget
        assert d.kept()[1] <= 1000
        d.reset()
        d.keep_sequences(3, 1 << 20)
        _count(d, reads, offset=4)
        _check_kept(d, reads, 3)
        assert d.kept() == (20, 3000)


def test_keeping_off_changes_nothing(mixed_reads):
    with H.Duplication(log2_slots=10) as d:
        _count(d, mixed_reads, offset=3)
        _check_counts(d, dup_ref.table(mixed_reads))
        assert d.kept() == (0, 0)
