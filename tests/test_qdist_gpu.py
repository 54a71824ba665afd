"""`stats --quality-dist` on the GPU: hpgq_qdist_* (gfx950) against
tests/qdist_ref.py, cell for cell.  The tile is P = 256
positions, the on-chip window 64 byte values from `base`."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import qdist_ref

pytestmark = pytest.mark.gpu

P = 256
FILL = 0xEE   # the bytes around the reads: a value the reads of most tests never hold


def _dev(reads, mask=None, offset=0, shift=0):
    """Device copies as tests/test_kmers_gpu.py::_dev makes them.  `offset` bytes
    lead the data (data_indices start there); `shift` moves the quality pointer
    itself off its alignment.  The bytes before, and HPGQ_DEVICE_SLACK after,
    are FILL: counted nowhere."""
    import torch
    dev = torch.device("cuda", 0)
    lead = np.full(offset + shift, FILL, np.uint8)
    pad = np.full(H.DEVICE_SLACK, FILL, np.uint8)
    t = dict(qual=torch.from_numpy(np.concatenate([lead, reads.qual, pad])).to(dev),
             idx=torch.from_numpy((reads.idx + offset).astype(np.int32)).to(dev))
    if mask is not None:
        t["mask"] = torch.from_numpy(mask).to(dev)
    torch.cuda.synchronize()
    t["batch"] = H.engine.device_batch(reads.n, 0, t["qual"].data_ptr() + shift, t["idx"].data_ptr())
    return t


def _count(q, reads, mask=None, offset=0, shift=0, keep=None):
    t = _dev(reads, mask, offset, shift)
    if keep is not None:
        keep.append(t)
    q.count_device(t["batch"], t["mask"].data_ptr() if mask is not None else None)
    if keep is None:
        q.sync()
    return t


def _reads(rng, lens, lo=0, hi=256):
    lens = np.asarray(lens, dtype=np.int64)
    idx = np.zeros(len(lens) + 1, dtype=np.int32)
    idx[1:] = np.cumsum(lens)
    qual = rng.integers(lo, hi, size=max(int(idx[-1]), 1), dtype=np.uint8)[:int(idx[-1])]
    return O.Reads(np.full(len(qual), ord("A"), np.uint8), qual, idx)


@pytest.fixture(scope="module")
def edge_reads():
    rng = np.random.default_rng(11)
    reads = _reads(rng, rng.integers(0, P + 41, size=3000))   # lengths 0 .. P + 40, all 256 byte values
    reads_max = _reads(rng, [P + 40, 0, 1, P, P - 1, P + 1])
    both = O.Reads.from_pairs(reads.pairs() + reads_max.pairs())
    return both, qdist_ref.table_of(both)


@pytest.mark.parametrize("rows", [P - 1, P, P + 1])
@pytest.mark.parametrize("offset", [0, 1, 2, 3, 13])
def test_edge_lengths_and_alignments(edge_reads, offset, rows):
    reads, want = edge_reads
    assert want.shape[0] == P + 40
    with H.QualityDist(rows, base=33) as q:
        q.reserve_length(P + 40)
        _count(q, reads, offset=offset)
        np.testing.assert_array_equal(q.hist(), want)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_quality_pointer(edge_reads, shift):
    reads, want = edge_reads
    with H.QualityDist(P + 40, base=64) as q:
        _count(q, reads, offset=2, shift=shift)
        np.testing.assert_array_equal(q.hist(), want)


def test_short_reads():
    rng = np.random.default_rng(12)
    reads = _reads(rng, rng.choice([0, 1, 3, 4, 5, 7], size=500))
    with H.QualityDist(8, base=33) as q:
        _count(q, reads, offset=3)
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(reads))


def test_realistic_values_any_window():
    rng = np.random.default_rng(13)
    reads = _reads(rng, [150] * 20000, 33, 74)
    want = qdist_ref.table_of(reads)
    for base in (33, 64, 0):   # 64 and 0: most bytes are outside the window
        with H.QualityDist(150, base=base) as q:
            _count(q, reads)
            np.testing.assert_array_equal(q.hist(), want, err_msg=f"base {base}")


def test_hot_cell():
    reads = _reads(np.random.default_rng(14), [150] * 70000, 70, 71)
    with H.QualityDist(150, base=33) as q:
        _count(q, reads)
        got = q.hist()
    want = np.zeros((150, 256), np.uint64)
    want[:, 70] = 70000
    np.testing.assert_array_equal(got, want)


def test_mask_batches_and_reset():
    rng = np.random.default_rng(15)
    batches = [_reads(rng, rng.integers(0, 160, size=2000)) for _ in range(3)]
    masks = [(rng.random(2000) < 0.6).astype(np.uint8) for _ in range(3)]
    masks[1][:] = 0                                      # one batch all masked out
    masks[2][7] = 2                                      # (only mask == 1 counts)
    empty = _reads(rng, [])
    want = qdist_ref.add([qdist_ref.table_of(b, m) for b, m in zip(batches, masks)])
    keep = []
    with H.QualityDist(160, base=33) as q:
        for b, m in zip(batches, masks):
            _count(q, b, m, offset=13, keep=keep)
        q.count_device(H.engine.device_batch(0, 0, 0, 0), None)   # one batch empty
        _count(q, empty, np.zeros(0, np.uint8), keep=keep)
        q.sync()
        np.testing.assert_array_equal(q.hist(), want)
        q.reset()
        _count(q, batches[0], masks[0])
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(batches[0], masks[0]))
        q.reset()
        assert q.hist().shape == (0, 256)


def test_growth_keeps_counts():
    rng = np.random.default_rng(16)
    short = _reads(rng, [150] * 3000, 33, 74)
    long_ = _reads(rng, list(rng.integers(500, 901, size=400)) + [1500])
    m = np.ones(long_.n, np.uint8)
    m[-1] = 0                                            # the longest read is masked out
    want = qdist_ref.add([qdist_ref.table_of(short), qdist_ref.table_of(long_, m)])
    keep = []
    with H.QualityDist(150, base=33) as q:
        _count(q, short, keep=keep)
        q.reserve_length(900)
        q.reserve_length(10)                             # never shrinks
        _count(q, long_, m, offset=1, keep=keep)
        q.sync()
        got = q.hist()
    assert got.shape[0] == int(np.diff(long_.idx)[:-1].max()) <= 900
    np.testing.assert_array_equal(got, want)


def test_clipping_is_an_error_until_reset():
    rng = np.random.default_rng(17)
    reads = _reads(rng, [40, 101, 100])
    with H.QualityDist(100, base=33) as q:
        _count(q, reads, np.array([1, 0, 1], np.uint8))  # the read of 101 masked out: no error
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(reads, np.array([1, 0, 1], np.uint8)))
        t = _count(q, reads, keep=[])
        for call in (q.sync, q.hist, q.sync):
            with pytest.raises(H.HpgqError) as e:
                call()
            assert e.value.code == H.E_READ_TOO_LONG
        del t
        q.reset()
        fits = _reads(rng, [100, 99, 0, 100])
        _count(q, fits)
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(fits))


def test_several_groups_per_workgroup():
    rng = np.random.default_rng(18)
    reads = _reads(rng, rng.integers(1, 301, size=5000))
    with H.QualityDist(300, base=33) as q:
        q.set_max_workgroups(2)
        _count(q, reads, offset=1)
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(reads))


def _engine_dev(reads):
    import torch
    dev = torch.device("cuda", 0)
    pad = np.zeros(H.DEVICE_SLACK, np.uint8)
    t = dict(seq=torch.from_numpy(np.concatenate([reads.seq, pad])).to(dev),
             qual=torch.from_numpy(np.concatenate([reads.qual, pad])).to(dev),
             idx=torch.from_numpy(reads.idx).to(dev))
    t["batch"] = H.engine.device_batch(reads.n, t["seq"].data_ptr(), t["qual"].data_ptr(), t["idx"].data_ptr())
    return t


def test_on_the_engines_stream_with_its_mask():
    import torch
    reads = O.synth(50_000, seed=21, L=150)
    p = H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,")
    m_o, _, _ = O.run(p, reads)
    assert 0 < int(m_o.sum()) < reads.n
    t = _engine_dev(reads)
    mask = torch.zeros(reads.n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with H.Engine(p) as e, H.QualityDist(150, base=33, stream=e.stream) as q:
        e.run_device(t["batch"], None, mask.data_ptr(), None)
        q.count_device(t["batch"], mask.data_ptr())      # no sync between: the stream orders them
        q.sync()
        np.testing.assert_array_equal(mask.cpu().numpy(), m_o)
        np.testing.assert_array_equal(q.hist(), qdist_ref.table_of(reads, m_o))


def test_paired_two_tables_one_pair_mask():
    import torch
    r1 = O.synth(20_000, seed=22, L=150)
    r2 = O.synth(20_000, seed=122, L=150, trunc_pct=30)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    m_o, _, _ = O.run(p, r1, r2)
    assert 0 < int(m_o.sum()) < r1.n
    t1, t2 = _engine_dev(r1), _engine_dev(r2)
    mask = torch.zeros(r1.n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with H.Engine(p) as e, H.QualityDist(150, stream=e.stream) as q1, H.QualityDist(150, stream=e.stream) as q2:
        e.run_device(t1["batch"], t2["batch"], mask.data_ptr(), None)
        q1.count_device(t1["batch"], mask.data_ptr())
        q2.count_device(t2["batch"], mask.data_ptr())
        q1.sync()
        np.testing.assert_array_equal(q1.hist(), qdist_ref.table_of(r1, m_o))
        np.testing.assert_array_equal(q2.hist(), qdist_ref.table_of(r2, m_o))
