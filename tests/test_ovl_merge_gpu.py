"""`edit --merge-overlap` on the GPU: ovl_plan_kernel, ovl_compact_kernel and
ovl_merge_kernel (gfx950) through hpgq_ovl_merge_device against
tests/ovl_merge_ref.py.  Every comparison is exact:
the three compacted batches' data_indices, sequence and quality bytes, zeros
from data_indices[num_reads] through the slack, the inputs, §2.13's six
scalars, the merge's four, the histogram, the F* the handle keeps, and the
correction's scalars, which stay zero with the correction switched on.

A lane of the merge kernel holds four positions of the merged read, a step 256;
its bytes move by the output offset's residue to aligned dwords, the first and
the last of which are stored byte by byte.  The facing bytes of mate 2 come from
two dwords, the lower of which lies before the buffer for the first pair's last
positions.  Every batch goes up through hostile_lib.device_batch; the outputs
lie in buffers the handle owns and zeroes when it makes them, so every handle
whose slack is checked is fresh."""
import ctypes as C

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import ovl_ref as R
import ovl_fix_ref as X
import ovl_merge_ref as G
import hostile_lib as HL

pytestmark = pytest.mark.gpu

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
    if seqs:
        idx[1:] = np.cumsum([len(s) for s in seqs])
    flat = [np.frombuffer(b"".join(x) + b"\1", dtype=np.uint8)[:-1].copy() for x in (seqs, quals)]
    assert len(flat[0]) == len(flat[1])
    return O.Reads(flat[0], flat[1], idx)


def _mates(pairs):
    """Two batches of [(s1, q1, s2, q2)]."""
    return _reads([p[0] for p in pairs], [p[1] for p in pairs]), _reads([p[2] for p in pairs], [p[3] for p in pairs])


def _upload(r1, r2, case=0, leads=(0, 0)):
    a1, a2 = ALIGNS[case % len(ALIGNS)]
    return [HL.device_batch(r, lead=lead, seq_shift=sh, qual_shift=(sh + 1 + m) % 4)
            for m, (r, lead, sh) in enumerate(zip((r1, r2), leads, (a1, a2)))]


def _merge(ov, t, r1, r2, want, fresh=True):
    """hpgq_ovl_merge_device: the three batches as the reference's, zeros behind
    them as far as the inputs' bytes and the slack reach (fresh: the handle's
    first call, its buffers still as it zeroed them), the F* the handle keeps,
    the inputs as they were."""
    n = r1.n
    outs = ov.merge_batch(t[0].batch, t[1].batch)
    ov.sync()
    room = (len(r1.seq), len(r2.seq), len(r1.seq) + len(r2.seq))
    for name, o, w, held in zip(("mate 1", "mate 2", "merged"), outs, (*want.out, want.merged), room):
        assert o.num_reads == w.n, name
        idx = _fetch(o.data_indices, 4 * (w.n + 1)).view(np.int32)
        np.testing.assert_array_equal(idx, w.idx, err_msg=f"data_indices of {name}")
        end = int(w.idx[-1])
        for what, ptr, bytes_ in (("seq", o.seq, w.seq), ("qual", o.quality, w.qual)):
            got = _fetch(ptr, held + H.DEVICE_SLACK)
            np.testing.assert_array_equal(got[:end], bytes_, err_msg=f"{what} of {name}")
            assert not (fresh and got[end:].any()), f"{what} of {name}: a store behind data_indices[num_reads]"
    if n:
        np.testing.assert_array_equal(_fetch(ov.last_inserts_ptr(), 4 * n).view(np.int32), want.insert)
    for x in t:
        HL.inputs_unchanged(x)
    return outs


ZERO_FIX = dict(corrected_pairs=0, corrected_bases=[0, 0])


def _fix_info(th, on=True):
    return dict(ZERO_FIX, on=on, phred=th[0], high=th[1], low=th[2])


def _fresh(r1, r2, want, mo=30, M=5, *, case=0, leads=(0, 0), max_wg=0, correct=X.DEFAULT):
    """One hpgq_ovl_merge_device on a new handle with both switches on: the bytes and every scalar."""
    with H.OverlapClip(mo, M, correct=correct, inserts=True) as ov:
        ov.set_max_workgroups(max_wg)
        _merge(ov, _upload(r1, r2, case, leads), r1, r2, want)
        assert ov.info() == want.info
        assert ov.merge_info() == want.merge
        assert ov.correct_info() == _fix_info(correct)                   # the merge never corrects
        np.testing.assert_array_equal(ov.inserts(), want.hist)


def _case(pairs, mo=30, M=5):
    r1, r2 = _mates(pairs)
    return r1, r2, G.Merged(r1, r2, mo, M)


# -- 1. geometry: the three ranges, every alignment ---------------------------------------------------

@pytest.fixture(scope="module")
def positions():
    """ovl_fix_ref's shapes (read-through, F = n, F > n, 512 / 512 at F = 1016 is
    below) with a disagreement at the offsets a lane, a step or the overlap
    begins or ends at, both winners; then mates of 40 and 70 bases at every F."""
    planted = X.position_pairs()
    rng = np.random.default_rng(90)
    # three merged reads of 31, 34 and 33 bases first: the offsets behind them take every residue
    pairs = [X.clean(rng, 40, 45, F, F) for F in (31, 34, 33)] + planted
    r1, r2, want = _case(pairs)
    assert (want.insert > 0).all() and want.merge["merged_pairs"] == len(pairs)
    assert want.merge["resolved"] == [len(planted) // 2, len(planted) // 2]
    assert {int(x) % 4 for x in want.merged.idx[:-1]} == {0, 1, 2, 3}    # every residue of the merged output offset
    return r1, r2, want


@pytest.mark.parametrize("align", range(16))
def test_positions(positions, align):
    r1, r2, want = positions
    _fresh(r1, r2, want, case=align, leads=(align % 5, (3 * align) % 7))


def test_longest_and_step_crossings():
    """512 / 512 at F = 1016 (lo = 504, hi = 512), F of 255, 256, 257 and 260 with
    mates of 200 and 180 bases (n1 != n2), hostile quality bytes."""
    rng = np.random.default_rng(91)
    pairs = []
    for n1, n2, F in ((512, 512, 1016), (200, 180, 255), (200, 180, 256), (180, 200, 257), (200, 180, 260), (512, 512, 1016),
                      (512, 300, 520), (300, 512, 520), (512, 512, 512), (512, 512, 513)):
        s1, s2 = R.pair_of(rng, n1, n2, F)
        pairs.append((s1, bytes(rng.integers(0, 256, n1, dtype=np.uint8)), s2, bytes(rng.integers(0, 256, n2, dtype=np.uint8))))
    r1, r2, want = _case(pairs, 8, 0)
    assert want.insert.tolist() == [1016, 255, 256, 257, 260, 1016, 520, 520, 512, 513]
    for case in (0, 6, 11, 13):
        _fresh(r1, r2, want, 8, 0, case=case, leads=(case % 3, case % 4))


def test_short_merged_reads_side_by_side():
    """min_overlap = 8: merged reads of 8 .. 11 bases back to back share output
    dwords; none may be written by its neighbour."""
    rng = np.random.default_rng(92)
    pairs = []
    lengths, seen, o = [], set(), 0
    while len(seen) < 16:                               # every length at every residue of its output offset
        F = next((f for f in (8, 9, 10, 11) if (o % 4, f) not in seen), 9)
        seen.add((o % 4, F))
        lengths.append(F)
        o += F
    assert len(lengths) < 40
    for k, F in enumerate(lengths):
        n1, n2 = F + k % 3, F + (k // 3) % 2
        s1, s2 = R.pair_of(rng, n1, n2, F, tail1=b"A" * 8, tail2=b"C" * 8)
        pairs.append((s1, bytes(rng.integers(0, 256, n1, dtype=np.uint8)), s2, bytes(rng.integers(0, 256, n2, dtype=np.uint8))))
    s1, s2 = R.pair_of(rng, 8, 8, 8)
    pairs.append((s1, b"IIIIIIII", s2, b"JJJJJJJJ"))
    r1, r2, want = _case(pairs, 8, 0)
    assert (want.insert > 0).all() and {8, 9, 10, 11} == set(want.insert.tolist())
    assert {(int(o) % 4, int(f)) for o, f in zip(want.merged.idx[:-1], want.insert)} == {(r, f) for r in range(4) for f in (8, 9, 10, 11)}
    for case in (0, 5, 10, 15):
        _fresh(r1, r2, want, 8, 0, case=case, leads=(case % 2, case % 3))


# -- 2. bytes -----------------------------------------------------------------------------------------

def test_every_byte_value_and_ties():
    pairs = X.byte_pairs() + G.tie_pairs() + X.threshold_pairs(33, 30, 14)
    r1, r2, want = _case(pairs)
    assert (want.insert > 0).all() and min(want.merge["resolved"]) > 1000
    _fresh(r1, r2, want, case=7, leads=(2, 5))
    _fresh(r1, r2, want, case=9, leads=(0, 0), correct=(64, 1, 0))


# -- 3. the mix of merged, unmerged and skipped pairs ---------------------------------------------------

def _pool(seed=93):
    rng = np.random.default_rng(seed)

    def qual(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))

    def merged(i):
        n1, n2 = 40 + i % 37, 35 + (i * 5) % 41
        F = 30 + (i * 11) % (n1 + n2 - 59)
        p = X.clean(rng, n1, n2, F, i)
        if i % 3 == 0:
            ov = min(n1, F) - max(0, F - n2)
            p = X.plant(p, F, (i * 7) % ov, 1 + i % 2, 33 + 40, 33 + 2, lose_byte=[None, ord("N"), 0, 255][i % 4])
        return p

    def unmerged(i):
        n1, n2 = (i * 3) % 50, (i * 7) % 45                            # (reads of 0 .. 3 bytes among them)
        if i % 9 == 4:
            n1, n2 = 60, 70
        return R.acgt(rng, n1), qual(n1), R.acgt(rng, n2), qual(n2)

    def skipped(i):
        s1, s2 = R.pair_of(rng, 513, 100, 90)
        return (s1, qual(513), s2, qual(100)) if i % 2 else (s2, qual(100), s1, qual(513))

    return merged, unmerged, skipped


MIXES = {
    "all": "m" * 50, "none": "u" * 50, "alternating": "mu" * 30 + "m", "one_merged": "m", "one_unmerged": "u",
    "one_skipped": "s", "skipped_between": "msmmsmusm", "unmerged_ends": "u" + "m" * 20 + "u",
    "runs_17": ("m" * 17 + "u" * 17) * 2 + "m" * 3, "runs_130": "m" * 130 + "u" * 130 + "mmmmm" + "u" * 4,
}


@pytest.fixture(scope="module")
def mixes():
    merged, unmerged, skipped = _pool()
    out = {}
    for name, pattern in MIXES.items():
        pairs = [dict(m=merged, u=unmerged, s=skipped)[c](i) for i, c in enumerate(pattern)]
        r1, r2, want = _case(pairs)
        assert [f > 0 for f in want.insert.tolist()] == [c == "m" for c in pattern], name
        assert [f < 0 for f in want.insert.tolist()] == [c == "s" for c in pattern], name
        out[name] = (r1, r2, want)
    return out


@pytest.mark.parametrize("name", list(MIXES))
def test_mix(mixes, name):
    r1, r2, want = mixes[name]
    k = len(name)
    _fresh(r1, r2, want, case=k, leads=(0, 0) if k % 2 else (3, 1))


def test_one_workgroup(mixes):
    """The grid-stride loops: every kernel of the call in one workgroup."""
    for name in ("runs_130", "runs_17"):
        r1, r2, want = mixes[name]
        _fresh(r1, r2, want, case=3, leads=(1, 2), max_wg=1)


def test_empty_batch():
    with H.OverlapClip(correct=X.DEFAULT, inserts=True) as ov:
        empty = H.engine.device_batch(0, 0, 0, 0)
        outs = ov.merge_batch(empty, empty)
        ov.sync()
        for o in outs:
            assert o.num_reads == 0 and _fetch(o.data_indices, 4).view(np.int32)[0] == 0
        assert ov.merge_info() == dict(merged_pairs=0, merged_bases=0, resolved=[0, 0])
        assert ov.info()["pairs"] == 0 and not ov.inserts().any()


# -- 4. waves ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_case():
    return X.random_case(600, seed=11)


@pytest.mark.parametrize("n,max_wg", [(15, 0), (16, 0), (17, 0), (128, 0), (129, 0), (600, 0), (600, 1)])
def test_random_pairs(random_case, n, max_wg):
    r1, r2, want = _case(random_case[:n])
    if n == 600:
        assert want.merge["merged_pairs"] > 200 and min(want.merge["resolved"]) >= 5 and want.out[0].n > 100
    _fresh(r1, r2, want, case=n + max_wg, leads=(n % 4, max_wg), max_wg=max_wg)


# -- 5. one handle, several calls ---------------------------------------------------------------------------

def test_calls_add_up_and_follow_a_clip(mixes, random_case):
    r1, r2, want = mixes["alternating"]
    s1, s2, other = _case(random_case[:100])
    cut = R.Cut(s1, s2, 30, 5)
    t, u = _upload(r1, r2, 2, (1, 0)), _upload(s1, s2, 13, (0, 3))
    with H.OverlapClip(30, 5) as ov:
        assert ov.last_inserts_ptr() is None
        _merge(ov, t, r1, r2, want)
        assert ov.merge_info() == want.merge and ov.info() == want.info and not ov.inserts().any()
        _merge(ov, u, s1, s2, other, fresh=False)                       # larger: the buffers grow
        _merge(ov, t, r1, r2, want, fresh=False)
        assert ov.merge_info() == G.add_info([want.merge, other.merge, want.merge])
        assert ov.info() == R.add([want.info, other.info, want.info])
        ov.reset()
        assert ov.merge_info() == dict(merged_pairs=0, merged_bases=0, resolved=[0, 0])
        # after a clip_batch on the same handle: the kept buffers are shared
        out = ov.clip_batch(u[0].batch, u[1].batch)
        ov.sync()
        for m in range(2):
            np.testing.assert_array_equal(_fetch(out[m].seq, int(cut.idx[m][-1])), cut.seq[m])
        assert ov.last_inserts_ptr() is None
        _merge(ov, u, s1, s2, other, fresh=False)
        assert ov.merge_info() == other.merge and ov.info() == R.add([cut.info, other.info])
        assert ov.correct_info() == _fix_info(X.DEFAULT, on=False)
        # and a clip after the merge
        out = ov.clip_batch(u[0].batch, u[1].batch)
        ov.sync()
        for m in range(2):
            np.testing.assert_array_equal(_fetch(out[m].quality, int(cut.idx[m][-1])), cut.qual[m])


# -- 6. invalid arguments ---------------------------------------------------------------------------------

def test_invalid_arguments(mixes):
    r1, r2, want = mixes["alternating"]
    t = _upload(r1, r2)
    f = H.lib.hpgq_ovl_merge_device
    with H.OverlapClip(30, 5) as ov:
        a, b, m = H.Batch(), H.Batch(), H.Batch()
        m1, m2 = C.byref(t[0].batch), C.byref(t[1].batch)
        assert f(ov._h, m1, m2, C.byref(a), C.byref(b), None) == -1     # a NULL merged
        assert f(ov._h, m1, m2, None, C.byref(b), C.byref(m)) == -1 and f(ov._h, m1, m2, C.byref(a), None, C.byref(m)) == -1
        assert f(ov._h, m1, m2, C.byref(a), C.byref(a), C.byref(m)) == -1
        assert f(ov._h, m1, m2, C.byref(a), C.byref(b), C.byref(a)) == -1
        assert f(ov._h, None, m2, C.byref(a), C.byref(b), C.byref(m)) == -1
        short = H.engine.device_batch(r2.n - 1, t[1].batch.seq, t[1].batch.quality, t[1].batch.data_indices)
        assert f(ov._h, m1, C.byref(short), C.byref(a), C.byref(b), C.byref(m)) == -1   # differing num_reads
        noq = H.engine.device_batch(r2.n, t[1].batch.seq, 0, t[1].batch.data_indices)
        assert f(ov._h, m1, C.byref(noq), C.byref(a), C.byref(b), C.byref(m)) == -1
        with pytest.raises(H.HpgqError):
            ov.merge_batch(t[0].batch, short)
        # offsets that claim more than INT32_MAX bytes for both mates together: refused from the offsets alone,
        # before anything is allocated or launched (no byte of such a batch is ever read)
        import torch
        far = torch.tensor([0, 2 ** 30 + 8], dtype=torch.int32, device="cuda")
        huge = H.engine.device_batch(1, t[0].batch.seq, t[0].batch.quality, far.data_ptr())
        assert f(ov._h, C.byref(huge), C.byref(huge), C.byref(a), C.byref(b), C.byref(m)) == -1
        assert ov.merge_info() == dict(merged_pairs=0, merged_bases=0, resolved=[0, 0]) and ov.info()["pairs"] == 0
        # the outputs may be the inputs' structs
        i1, i2 = (H.engine.device_batch(x.batch.num_reads, x.batch.seq, x.batch.quality, x.batch.data_indices) for x in t)
        assert f(ov._h, C.byref(i1), C.byref(i2), C.byref(i1), C.byref(i2), C.byref(m)) == 0
        ov.sync()
        assert (i1.num_reads, i2.num_reads, m.num_reads) == (want.out[0].n, want.out[1].n, want.merged.n)
        assert ov.merge_info() == want.merge
    for x in t:
        HL.inputs_unchanged(x)
