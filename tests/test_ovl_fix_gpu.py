"""`edit --correct-overlap` and `--insert-size` on the GPU: ovl_fix_kernel and
ovl_hist_kernel (gfx950) through the hpgq_ovl handle against tests/ovl_fix_ref.py
(DESIGN.md §2.14, §4.17).  Every comparison is exact: both mates' kept sequence
and quality bytes after the correction, idx_out, zeros from idx_out[n] through
the slack, the inputs, §2.13's six scalars, the correction's three, the histogram.

A lane of the fix kernel holds four positions of mate 1, a load step 256; the
facing bytes of mate 2 come from two dwords, the lower of which lies before the
kept buffer for the first pair's last positions.  Every batch goes up through
hostile_lib.device_batch; the kept batches lie in buffers the handle owns and
zeroes when it makes them, so every handle whose slack is checked is fresh."""
import ctypes as C

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import ovl_ref as R
import ovl_fix_ref as X
import hostile_lib as HL

pytestmark = pytest.mark.gpu

POISON = 0xA5
# (seq shift of mate 1, of mate 2): every alignment 0 .. 3 of each mate
ALIGNS = [(a, b) for a in range(4) for b in range(4)]
_hip = None


def _fetch(ptr, nbytes):
    """nbytes of device memory at ptr (the stream that wrote them is idle)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")   # (the runtime torch has loaded)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert _hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out[:nbytes]


def _reads(seqs, quals):
    idx = np.zeros(len(seqs) + 1, dtype=np.int32)
    idx[1:] = np.cumsum([len(s) for s in seqs])
    flat = [np.frombuffer(b"".join(x) + b"\1", dtype=np.uint8)[:-1].copy() for x in (seqs, quals)]
    assert len(flat[0]) == len(flat[1])
    return O.Reads(flat[0], flat[1], idx)


def _mates(pairs):
    """Two batches of [(s1, q1, s2, q2)]."""
    return _reads([p[0] for p in pairs], [p[1] for p in pairs]), _reads([p[2] for p in pairs], [p[3] for p in pairs])


def _head(reads, n):
    end = int(reads.idx[n])
    return O.Reads(reads.seq[:end], reads.qual[:end], reads.idx[:n + 1])


def _upload(r1, r2, case=0, leads=(0, 0)):
    a1, a2 = ALIGNS[case % len(ALIGNS)]
    return [HL.device_batch(r, lead=lead, seq_shift=sh, qual_shift=(sh + 1 + m) % 4)
            for m, (r, lead, sh) in enumerate(zip((r1, r2), leads, (a1, a2)))]


def _clip(ov, t, r1, r2, cut, seq, qual):
    """hpgq_ovl_batch_device: idx_out as the cut's, the kept bytes `seq` / `qual`
    per mate, zeros behind them as far as the input's bytes and the slack reach,
    the inputs as they were."""
    n = r1.n
    out = ov.clip_batch(t[0].batch, t[1].batch)
    ov.sync()
    for m, (o, r) in enumerate(zip(out, (r1, r2))):
        assert o.num_reads == n
        idx = _fetch(o.data_indices, 4 * (n + 1)).view(np.int32)
        np.testing.assert_array_equal(idx, cut.idx[m], err_msg=f"idx_out of mate {m + 1}")
        kept, held = int(cut.idx[m][-1]), len(r.seq)
        for name, ptr, w in (("seq", o.seq, seq[m]), ("qual", o.quality, qual[m])):
            got = _fetch(ptr, held + H.DEVICE_SLACK)
            np.testing.assert_array_equal(got[:kept], w, err_msg=f"{name}_out of mate {m + 1}")
            assert not got[kept:].any(), f"{name}_out of mate {m + 1}: a store behind idx_out[n]"
    for x in t:
        HL.inputs_unchanged(x)


def _fix_info(fix, th, on=True):
    return dict(fix, on=on, phred=th[0], high=th[1], low=th[2])


def _fresh(r1, r2, want, mo=30, M=5, th=X.DEFAULT, *, case=0, leads=(0, 0), max_wg=0):
    """One hpgq_ovl_batch_device on a new handle with both switches on: the bytes and every scalar."""
    with H.OverlapClip(mo, M, correct=th, inserts=True) as ov:
        ov.set_max_workgroups(max_wg)
        _clip(ov, _upload(r1, r2, case, leads), r1, r2, want.cut, want.seq, want.qual)
        assert ov.info() == want.cut.info                                # §2.13's scalars: as without the switches
        assert ov.correct_info() == _fix_info(want.fix, th)
        np.testing.assert_array_equal(ov.inserts(), want.hist)


def _case(pairs, mo=30, M=5, th=X.DEFAULT):
    r1, r2 = _mates(pairs)
    return r1, r2, X.Fixed(r1, r2, mo, M, *th)


# -- 1. positions: one disagreement per pair, both directions, every alignment -------------------

@pytest.fixture(scope="module")
def positions():
    pairs = X.position_pairs()
    r1, r2, want = _case(pairs)
    # by the reference: every pair at its F, one base corrected in each, half of them in either mate
    k = 0
    for n, F in X.POSITION_SHAPES:
        ov = min(n, F) - max(0, F - n)
        cnt = 2 * len({o for o in (0, 1, 3, 4, 63, 64, 252, 255, 256, 259, ov - 1) if o < ov})
        assert want.cut.insert[k:k + cnt].tolist() == [F] * cnt
        k += cnt
    assert want.cut.insert[k:].tolist() == [F for F in range(30, 81) for _ in range(2)]
    assert want.fix == dict(corrected_pairs=len(pairs), corrected_bases=[len(pairs) // 2, len(pairs) // 2])
    assert any(not np.array_equal(a, b) for a, b in zip(want.seq + want.qual, want.cut.seq + want.cut.qual))
    return r1, r2, want


@pytest.mark.parametrize("align", range(16))
def test_positions(positions, align):
    r1, r2, want = positions
    _fresh(r1, r2, want, case=align, leads=(align % 5, (3 * align) % 7))


# -- 2. thresholds ---------------------------------------------------------------------------------

@pytest.mark.parametrize("phred", [33, 64])
@pytest.mark.parametrize("high,low", [(30, 14), (1, 0), (93, 92)])
def test_thresholds(phred, high, low):
    th = (phred, high, low)
    pairs = X.threshold_pairs(*th)
    r1, r2, want = _case(pairs, th=th)
    assert want.cut.insert.tolist() == [70] * len(pairs)
    # (tests/test_ovl_fix_cpu.py::test_thresholds counts them by hand)
    assert want.fix["corrected_pairs"] == 2 * (5 + (high == low + 1)) and want.fix["corrected_bases"][0] == want.fix["corrected_bases"][1]
    _fresh(r1, r2, want, th=th, case=phred + high, leads=(1, 2))


# -- 3. bytes ----------------------------------------------------------------------------------------

def test_every_byte_value():
    pairs = X.byte_pairs()
    r1, r2, want = _case(pairs)
    assert want.cut.insert.tolist() == [70] * len(pairs)
    assert want.fix == dict(corrected_pairs=2 * 205, corrected_bases=[4 * 255, 4 * 255])
    # the pairs whose winner is no upper-case base stay as they are
    for m in range(2):
        at = int(want.cut.idx[m][-17])
        np.testing.assert_array_equal(want.seq[m][at:], want.cut.seq[m][at:])
        np.testing.assert_array_equal(want.qual[m][at:], want.cut.qual[m][at:])
    _fresh(r1, r2, want, case=7, leads=(2, 5))


# -- 4. several per pair ----------------------------------------------------------------------------

@pytest.mark.parametrize("mo,M", [(30, 5), (64, 40)])
def test_several_per_pair(mo, M):
    pairs = X.several_pairs(mo, M)
    r1, r2, want = _case(pairs, mo, M)
    assert want.cut.insert.tolist() == [110] * 4
    mixed = want.fix["corrected_bases"][0] + want.fix["corrected_bases"][1] - 3 * M
    assert want.fix["corrected_pairs"] == 4 and 0 < mixed < M
    _fresh(r1, r2, want, mo, M, case=M, leads=(3, 0))


# -- 5. untouched pairs ------------------------------------------------------------------------------

def test_untouched_pairs():
    pairs = X.untouched_pairs()
    r1, r2, want = _case(pairs)
    ins = want.cut.insert.tolist()
    assert ins[0::2] == [45 + i % 3 for i in range(len(ins[0::2]))] and set(ins[1::2]) == {0, -1} and ins.count(-1) == 3
    half = len(ins[0::2])
    assert want.fix == dict(corrected_pairs=half, corrected_bases=[half, half])
    # kept reads of 0 .. 3 bytes lie between corrected ones
    for m in range(2):
        assert {0, 1, 2, 3} <= set(np.diff(want.cut.idx[m])[1::2].tolist())
    for case in (0, 5, 10):
        _fresh(r1, r2, want, case=case, leads=(case % 3, case % 2))


# -- 6. waves and grid -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_case():
    r1, r2 = _mates(X.random_case(600, seed=11))
    cut = R.Cut(r1, r2, 30, 5)
    want = X.Fixed(r1, r2, cut=cut)
    # the case cannot pass with nothing corrected: by the reference
    assert min(want.fix["corrected_bases"]) >= 5 and cut.info["overlapping"] > 200
    return r1, r2, cut


@pytest.mark.parametrize("n,max_wg", [(15, 0), (16, 0), (17, 0), (128, 0), (129, 0), (600, 0), (600, 1)])
def test_random_pairs(random_case, n, max_wg):
    r1, r2, cut = random_case
    h1, h2 = _head(r1, n), _head(r2, n)
    want = X.Fixed(h1, h2, cut=cut.head(n))
    if n == 600:
        assert want.fix["corrected_bases"] == [10, 14] and want.fix["corrected_pairs"] == 11
    _fresh(h1, h2, want, case=n + max_wg, leads=(n % 4, max_wg), max_wg=max_wg)


# -- 7. switches --------------------------------------------------------------------------------------

def test_switches(random_case):
    r1, r2, cut = random_case
    on = X.Fixed(r1, r2, cut=cut)
    other = X.Fixed(r1, r2, 30, 5, 33, 20, 19, cut=cut)
    assert other.fix["corrected_pairs"] > on.fix["corrected_pairs"]
    zero = dict(corrected_pairs=0, corrected_bases=[0, 0])
    t = _upload(r1, r2, 6, (1, 3))
    n = r1.n
    # off, as after open: the bytes of the cut alone, no scalar, an empty histogram
    with H.OverlapClip(30, 5) as ov:
        _clip(ov, t, r1, r2, cut, cut.seq, cut.qual)
        assert ov.correct_info() == _fix_info(zero, X.DEFAULT, on=False) and not ov.inserts().any()
        assert ov.info() == cut.info and ov.last_inserts_ptr() is None
    with H.OverlapClip(30, 5, correct=X.DEFAULT) as ov:
        # the find alone never corrects: its outputs as without the switch, the three scalars 0
        gi, g1, g2 = (HL.Guarded(4 * n, 4, POISON) for _ in range(3))
        ov.find(t[0].batch, t[1].batch, gi.ptr, g1.ptr, g2.ptr)
        ov.find(t[0].batch, t[1].batch, None, None, None)
        ov.sync()
        np.testing.assert_array_equal(gi.check().view(np.int32), cut.insert)
        np.testing.assert_array_equal(g1.check().view(np.uint32), cut.pos[0])
        np.testing.assert_array_equal(g2.check().view(np.uint32), cut.pos[1])
        assert ov.correct_info() == _fix_info(zero, X.DEFAULT)
        for x in t:
            HL.inputs_unchanged(x)
        ov.reset()
        # on, off, on with other thresholds: each call as its switch says; the scalars add up
        _clip(ov, t, r1, r2, cut, on.seq, on.qual)
        assert ov.correct_info() == _fix_info(on.fix, X.DEFAULT)
        # the F* it worked from stay readable until the next call
        np.testing.assert_array_equal(_fetch(ov.last_inserts_ptr(), 4 * n).view(np.int32), cut.insert)
        ov.find(t[0].batch, t[1].batch)
        assert ov.last_inserts_ptr() is None
        ov.reset()
        _clip(ov, t, r1, r2, cut, on.seq, on.qual)
        ov.set_correct(None)
        _clip(ov, t, r1, r2, cut, cut.seq, cut.qual)
        assert ov.correct_info() == _fix_info(on.fix, X.DEFAULT, on=False)
        with pytest.raises(H.HpgqError):
            ov.set_correct((33, 14, 14))
        ov.set_correct((33, 20, 19))
        _clip(ov, t, r1, r2, cut, other.seq, other.qual)
        _clip(ov, t, r1, r2, cut, other.seq, other.qual)
        assert ov.correct_info() == _fix_info(X.add_fix([on.fix, other.fix, other.fix]), (33, 20, 19))
        assert ov.info() == R.add([cut.info] * 4) and not ov.inserts().any()
        ov.reset()
        assert ov.correct_info() == _fix_info(zero, (33, 20, 19))       # the switch and the parameters stay
        _clip(ov, t, r1, r2, cut, other.seq, other.qual)
        assert ov.correct_info() == _fix_info(other.fix, (33, 20, 19)) and ov.info() == cut.info


# -- 8. histogram --------------------------------------------------------------------------------------

def _plain(pairs):
    return [(a, b"I" * len(a), b, b"I" * len(b)) for a, b in pairs]


def test_histogram_every_insert_size_once():
    rng = np.random.default_rng(31)
    pairs = _plain([R.pair_of(rng, 40, 70, F) for F in range(30, 81)])
    r1, r2, want = _case(pairs)
    assert want.hist[30:81].tolist() == [1] * 51 and int(want.hist.sum()) == 51
    _fresh(r1, r2, want, case=3, leads=(1, 1))


def test_histogram_one_bin_many_pairs():
    """4,096 pairs at one F: every workgroup adds to the same cell."""
    rng = np.random.default_rng(32)
    one = R.pair_of(rng, 40, 40, 35)
    assert R.find(*one, 30, 5) == 35
    r1, r2 = _mates(_plain([one] * 4096))
    t = _upload(r1, r2, 9, (0, 2))
    for max_wg in (0, 1):
        with H.OverlapClip(30, 5, inserts=True) as ov:
            ov.set_max_workgroups(max_wg)
            ov.find(t[0].batch, t[1].batch)
            np.testing.assert_array_equal(ov.inserts(), X.hist_of([35] * 4096))
            assert ov.info()["overlapping"] == 4096


def test_histogram_ends_switch_and_reset():
    rng = np.random.default_rng(33)
    pairs = _plain([R.pair_of(rng, 8, 8, 8), R.pair_of(rng, 512, 512, 1016), (R.acgt(rng, 60), R.acgt(rng, 60)), (b"", b"ACGT"),
                    R.pair_of(rng, 513, 100, 90), R.pair_of(rng, 100, 513, 90), R.pair_of(rng, 512, 512, 1016)])
    r1, r2, want = _case(pairs, 8, 0)
    assert want.cut.insert.tolist() == [8, 1016, 0, 0, -1, -1, 1016]
    h = np.zeros(X.BINS, np.uint64)
    h[[0, 8, 1016]] = 2, 1, 2
    np.testing.assert_array_equal(want.hist, h)                         # bins 8 and 1016, bin 0, the skipped pairs in none
    _fresh(r1, r2, want, 8, 0, case=12, leads=(2, 0))
    t = _upload(r1, r2, 4, (3, 1))
    ins = HL.Guarded(4 * r1.n, 4, POISON)
    with H.OverlapClip(8, 0) as ov:
        ov.find(t[0].batch, t[1].batch)                                  # off: nothing is counted
        ov.clip_batch(t[0].batch, t[1].batch)
        assert not ov.inserts().any()
        ov.count_inserts(True)
        ov.find(t[0].batch, t[1].batch)                                  # F* in the handle's buffer
        ov.find(t[0].batch, t[1].batch, ins.ptr)                         # F* in the caller's
        ov.clip_batch(t[0].batch, t[1].batch)
        np.testing.assert_array_equal(ov.inserts(), 3 * h)
        np.testing.assert_array_equal(ins.check().view(np.int32), want.cut.insert)
        ov.count_inserts(False)
        ov.find(t[0].batch, t[1].batch)
        np.testing.assert_array_equal(ov.inserts(), 3 * h)
        assert ov.info() == R.add([want.cut.info] * 6)
        ov.reset()
        assert not ov.inserts().any()
        ov.count_inserts(True)
        ov.clip_batch(t[0].batch, t[1].batch)
        np.testing.assert_array_equal(ov.inserts(), h)
    for x in t:
        HL.inputs_unchanged(x)


def test_empty_batch_with_both_switches():
    with H.OverlapClip(correct=X.DEFAULT, inserts=True) as ov:
        empty = H.engine.device_batch(0, 0, 0, 0)
        ov.find(empty, empty)
        out = ov.clip_batch(empty, empty)
        assert out[0].num_reads == out[1].num_reads == 0
        assert ov.correct_info() == _fix_info(dict(corrected_pairs=0, corrected_bases=[0, 0]), X.DEFAULT)
        assert not ov.inserts().any()
