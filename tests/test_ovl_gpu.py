"""`edit --clip-overlap` on the GPU: hpgq_ovl_* (gfx950) against tests/ovl_ref.py:
insert length, both cut positions, both kept batches (offsets and both byte
ranges) and the scalars.  A block of the find kernel
covers 64 candidate insert lengths, a load step 256 bases of a mate.

Every batch goes up through hostile_lib.device_batch.  The outputs of
hpgq_ovl_find_device lie in hostile_lib.Guarded buffers: poison stays where
nothing belongs, both bands stay intact.  The kept batches of
hpgq_ovl_batch_device lie in buffers the handle owns, which it zeroes when it
makes them: every handle here is fresh when its kept bytes are compared, no
sequence or quality byte of these batches is 0, and the bytes from idx_out[n]
to the end of what the input held, and the slack behind them, must still be 0."""
import ctypes as C

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import ovl_ref as R
import hostile_lib as HL

pytestmark = pytest.mark.gpu

POISON = 0xA5
PARAMS = [(8, 0), (30, 5), (512, 255)]
# (seq shift of mate 1, of mate 2): every alignment 0 .. 3 of each mate, handed out in turn
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


def _reads(seqs, plain_quality=False):
    """A batch of the byte strings; quality depends on read and position, reaches past 127 and is never 0."""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    idx = np.zeros(len(seqs) + 1, dtype=np.int32)
    idx[1:] = np.cumsum(lens)
    seq = np.frombuffer(b"".join(seqs) + b"\1", dtype=np.uint8)[:-1].copy()
    i = np.repeat(np.arange(len(seqs)), lens)
    j = np.arange(len(seq)) - np.repeat(idx[:-1].astype(np.int64), lens)
    if plain_quality:
        qual = (33 + (j * 7 + i * 3) % 41).astype(np.uint8)
    else:
        qual = (((j * 37 + i * 101 + 7) & 0xFF) | 1).astype(np.uint8)
    return O.Reads(seq, qual, idx)


def _mates(pairs, **kw):
    return _reads([a for a, _ in pairs], **kw), _reads([b for _, b in pairs], **kw)


def _head(reads, n):
    end = int(reads.idx[n])
    return O.Reads(reads.seq[:end], reads.qual[:end], reads.idx[:n + 1])


def _check(ov, r1, r2, want, *, case=0, leads=(0, 0), slack=("hostile", "hostile"), scalars=True):
    """hpgq_ovl_find_device into guarded buffers and hpgq_ovl_batch_device on a
    handle that has cut nothing yet, everything against `want`.  slack: what
    lies behind each mate's data (hostile_lib.device_batch's slack_fill)."""
    a1, a2 = ALIGNS[case % len(ALIGNS)]
    t = [HL.device_batch(r, lead=lead, seq_shift=sh, qual_shift=(sh + 1 + m) % 4, slack_fill=slack[m])
         for m, (r, lead, sh) in enumerate(zip((r1, r2), leads, (a1, a2)))]
    n = r1.n
    gi, g1, g2 = (HL.Guarded(4 * n, 4, POISON) for _ in range(3))
    ov.find(t[0].batch, t[1].batch, gi.ptr, g1.ptr, g2.ptr)
    ov.sync()
    np.testing.assert_array_equal(gi.check().view(np.int32), want.insert, err_msg="insert")
    np.testing.assert_array_equal(g1.check().view(np.uint32), want.pos[0], err_msg="pos1")
    np.testing.assert_array_equal(g2.check().view(np.uint32), want.pos[1], err_msg="pos2")
    out = ov.clip_batch(t[0].batch, t[1].batch)
    ov.sync()
    for m, (o, r) in enumerate(zip(out, (r1, r2))):
        assert o.num_reads == n
        idx = _fetch(o.data_indices, 4 * (n + 1)).view(np.int32)
        np.testing.assert_array_equal(idx, want.idx[m], err_msg=f"idx_out of mate {m + 1}")
        kept, held = int(want.idx[m][-1]), len(r.seq)
        for name, ptr, w in (("seq", o.seq, want.seq[m]), ("qual", o.quality, want.qual[m])):
            got = _fetch(ptr, held + H.DEVICE_SLACK)
            np.testing.assert_array_equal(got[:kept], w, err_msg=f"{name}_out of mate {m + 1}")
            assert not got[kept:].any(), f"{name}_out of mate {m + 1}: a store behind idx_out[n]"
    for x in t:
        HL.inputs_unchanged(x)
    if scalars:
        assert ov.info() == R.add([want.info, want.info])                # (the find and the cut both count)
    return t


def _fresh(pairs, mo, M, **kw):
    r1, r2 = _mates(pairs)
    want = R.Cut(r1, r2, mo, M)
    with H.OverlapClip(mo, M) as ov:
        _check(ov, r1, r2, want, **kw)
    return want


# -- 1. the edge list, every parameter set, every alignment of each mate -----------------------

@pytest.fixture(scope="module")
def edges():
    out = {}
    for mo, M in PARAMS:
        pairs = R.edge_pairs(mo, M)
        r1, r2 = _mates(pairs)
        out[mo, M] = (pairs, r1, r2, R.Cut(r1, r2, mo, M))
    return out


def test_the_edge_list_means_what_it_says(edges):
    """By the reference: every F of the 40/70 mates is found, M mismatches pass and
    M + 1 do not, the long mates are skipped, the repeat's greatest F wins."""
    pairs, r1, r2, want = edges[30, 5]
    ins = want.insert.tolist()
    k = 0
    for n1, n2 in ((40, 70), (70, 40), (40, 40), (70, 70)):
        span = list(range(30, n1 + n2 - 30 + 1))
        assert ins[k:k + len(span)] == span, (n1, n2)
        k += len(span)
    assert ins[k:k + 4] == [0, 0, 0, 0]                                  # ov = min_overlap - 1
    assert want.info["skipped"] == 3 and ins.count(-1) == 3
    unit = b"ACGTTGCA" * 16
    at = pairs.index((unit[:100], R.revcomp(unit[:100])))
    for k, true_f in ((at, 100), (at + 1, 84)):                          # admissible at every F = true_f + 8 j with ov >= 30
        assert ins[k] > true_f and (ins[k] - true_f) % 8 == 0 and R.find(*pairs[k], 30, 0) == ins[k]
    for mo, M in PARAMS[:2]:
        w = edges[mo, M][3]
        assert w.info["overlapping"] > 20 and w.info["clipped"] > 8, (mo, M)
    # (512, 255): only two whole mates of 512 bases can overlap, and nothing is ever cut
    ins = edges[512, 255][3].insert.tolist()
    assert ins.count(512) >= 3 and set(ins) == {512, 0, -1} and edges[512, 255][3].info["clipped"] == 0
    # exactly M and M + 1 mismatches, by hand on one pair
    rng = np.random.default_rng(1)
    s1, s2 = R.pair_of(rng, 150, 150, 100)
    ov_at = [0, 99, 32, 64, 96, 31]
    assert R.find(*R.mismatch_in_overlap(s1, s2, 100, ov_at[:5]), 30, 5) == 100
    assert R.find(*R.mismatch_in_overlap(s1, s2, 100, ov_at), 30, 5) != 100


@pytest.mark.parametrize("align", range(16))
@pytest.mark.parametrize("params", PARAMS)
def test_edge_list(edges, params, align):
    _, r1, r2, want = edges[params]
    with H.OverlapClip(*params) as ov:
        _check(ov, r1, r2, want, case=align, leads=(align % 5, (3 * align) % 7))


# -- 2. mismatches at the first, last and every 32nd position -----------------------------------

@pytest.mark.parametrize("n,F", [(150, 100), (150, 150), (150, 230), (300, 290), (512, 512), (512, 600)])
def test_mismatch_positions(n, F):
    """One mismatch more than M at a time: M at the positions a word ends or
    begins at, and the one more at each such position in turn."""
    mo, M = 30, 5
    rng = np.random.default_rng(n + F)
    ov = min(n, F) - max(0, F - n)
    at = sorted({0, ov - 1, *range(32, ov - 1, 32), *range(31, ov - 1, 32)})
    pairs = []
    for start in range(0, len(at) - M, 2):
        s1, s2 = R.pair_of(rng, n, n, F)
        pairs.append(R.mismatch_in_overlap(s1, s2, F, at[start:start + M]))
        pairs.append(R.mismatch_in_overlap(s1, s2, F, at[start:start + M + 1]))
    want = _fresh(pairs, mo, M, case=n % 16, leads=(1, 2))
    ins = want.insert.tolist()
    assert ins[0::2] == [F] * (len(pairs) // 2) and F not in ins[1::2]


# -- 3. block edges ------------------------------------------------------------------------------

@pytest.mark.parametrize("mo", [8, 30])
def test_candidate_block_edges(mo):
    """63, 64, 65, 128 and 129 candidates, the one admissible F at each of them."""
    rng = np.random.default_rng(7 + mo)
    pairs, expect = [], []
    for cnt in (63, 64, 65, 128, 129):
        total = cnt - 1 + 2 * mo
        n1 = total // 2 + 3
        n2 = total - n1
        for F in range(mo, total - mo + 1):
            pairs.append(R.pair_of(rng, n1, n2, F))
            expect.append(F)
    want = _fresh(pairs, mo, 0, case=5, leads=(3, 0))
    # (a random fragment may be admissible at a greater F by chance at 8 bases: never at a smaller one)
    assert all(f >= e for f, e in zip(want.insert.tolist(), expect))
    assert sum(f == e for f, e in zip(want.insert.tolist(), expect)) > len(expect) * 9 // 10


# -- 4. hostile bytes ----------------------------------------------------------------------------

@pytest.mark.parametrize("params", [(8, 0), (30, 5)])
def test_every_byte_value(params):
    """Each byte value in the overlap, facing itself and facing a base: a
    mismatch unless it is the base that belongs there."""
    mo, M = params
    rng = np.random.default_rng(11)
    pairs = []
    for v in range(256):
        s1, s2 = R.pair_of(rng, 90, 80, 70)
        a, b = bytearray(s1), bytearray(s2)
        for k in range(M + 1):                                           # M + 1 of them: one too many unless v matches
            at = 2 + 11 * k
            a[at] = v
            if v % 2:
                b[69 - at] = v                                           # the byte faces itself
        pairs.append((bytes(a), bytes(b)))
        a = bytearray(s1)
        for k in range(M):                                               # M of them: still admissible
            a[3 + 13 * k] = v
        pairs.append((bytes(a), s2))
    want = _fresh(pairs, mo, M, case=9, leads=(2, 5))
    ins = want.insert.tolist()
    assert ins[1::2] == [70] * 256 and ins[0::2].count(70) <= 4          # (only A C G T can be the base that belongs there)


# -- 5. what follows a read has no influence -----------------------------------------------------

def test_match_that_continues_past_the_read():
    """The match would go on in the next read's bytes and in the slack: the pair
    is what its offsets say."""
    rng = np.random.default_rng(13)
    frag = R.acgt(rng, 60)
    rc = R.revcomp(frag)
    # pair 0: mate 1 holds 25 bases of the fragment and the next read goes on with it (25 < 30: no overlap);
    # pair 2: the same for mate 2; pair 4 ends both batches: 18 bases face each other, 34 with the slack's 8
    pairs = [(frag[:25], rc[:60]), (frag[25:60], R.acgt(rng, 40)), (frag[:40], rc[:25]), (R.acgt(rng, 33), rc[25:60]),
             (frag[:29], rc[20:49])]
    assert R.find(frag, rc, 30, 0) == 60 and R.find(frag[:37], rc[20:57], 30, 0) == 40
    r1, r2 = _mates(pairs)
    want = R.Cut(r1, r2, 30, 0)
    assert want.insert.tolist() == [0, 0, 0, 0, 0]
    for case in (6, 11):
        with H.OverlapClip(30, 0) as ov:
            _check(ov, r1, r2, want, case=case, leads=(3, 1), slack=(frag[29:37], rc[49:57]))


# -- 6. short reads and the empty batch -----------------------------------------------------------

def test_short_reads_and_empty_batch():
    rng = np.random.default_rng(17)
    pairs = [(R.acgt(rng, a), R.acgt(rng, b)) for a in range(9) for b in (0, 1, a, 8, 50)]
    pairs += [R.pair_of(rng, 8, 8, 8), R.pair_of(rng, 8, 50, 8), R.pair_of(rng, 50, 8, 8), (b"", b"")]
    want = _fresh(pairs, 8, 0, case=3, leads=(1, 0))
    assert want.insert.tolist()[-4:-1] == [8, 8, 8] and want.pos[1][-3] == 8 and want.info["clipped"] == 2
    _fresh([(b"", b"")] * 3, 8, 0)
    with H.OverlapClip() as ov:
        empty = H.engine.device_batch(0, 0, 0, 0)
        ov.find(empty, empty, None, None, None)
        out = ov.clip_batch(empty, empty)
        assert out[0].num_reads == out[1].num_reads == 0
        assert _fetch(out[0].data_indices, 4).view(np.int32)[0] == 0 == _fetch(out[1].data_indices, 4).view(np.int32)[0]
        z = ov.info()
        assert z == dict(pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0], min_overlap=30, max_mismatches=5)
        one = HL.device_batch(_reads([b"ACGT"]))
        with pytest.raises(H.HpgqError) as e:                            # differing num_reads
            ov.find(one.batch, empty, None, None, None)
        assert e.value.code == -1


# -- 7. random pairs, few workgroups --------------------------------------------------------------

SIZES = [0, 1, 15, 16, 17, 127, 128, 129, 4000, 20000]


@pytest.fixture(scope="module")
def random_case():
    pairs = R.random_pairs(20000, 91, L=(20, 120))
    r1, r2 = _mates(pairs)
    want = R.Cut(r1, r2, 30, 5)
    # a kernel that finds nothing does not pass: by the reference's results
    assert want.info["overlapping"] * 3 >= want.info["pairs"] and want.info["clipped"] * 3 >= want.info["overlapping"]
    return r1, r2, want


@pytest.mark.parametrize("n", SIZES)
def test_random_pairs(random_case, n):
    r1, r2, want = random_case
    h1, h2, w = _head(r1, n), _head(r2, n), want.head(n)
    if n >= 127:
        assert w.info["overlapping"] * 3 >= n and w.info["clipped"] * 3 >= w.info["overlapping"]
    case = SIZES.index(n)
    for k, max_wg in enumerate((0, 1, 2)):
        with H.OverlapClip(30, 5) as ov:
            ov.set_max_workgroups(max_wg)
            _check(ov, h1, h2, w, case=case * 3 + k, leads=(case % 4, k))


# -- 8. scalars ------------------------------------------------------------------------------------

def test_scalars_accumulate_and_reset(random_case):
    r1, r2, want = random_case
    a, b = (_head(r1, 3000), _head(r2, 3000), want.head(3000)), (_head(r1, 777), _head(r2, 777), want.head(777))
    import torch
    with H.OverlapClip(30, 5) as ov:
        zero = dict(a[2].info, pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0])
        assert ov.info() == zero
        keep = []
        for x in (a, b, a):
            t = [HL.device_batch(r, lead=1 + m) for m, r in enumerate(x[:2])]
            keep.append(t)
            ins = torch.empty(x[0].n, dtype=torch.int32, device="cuda")
            ov.find(t[0].batch, t[1].batch, ins.data_ptr(), None, None)  # the inserts only
            ov.sync()
        assert ov.info() == R.add([a[2].info, b[2].info, a[2].info])
        np.testing.assert_array_equal(ins.cpu().numpy(), a[2].insert)
        ov.reset()
        assert ov.info() == zero
        ov.find(keep[1][0].batch, keep[1][1].batch, None, None, None)    # no output at all: the scalars still count
        assert ov.info() == b[2].info
    for t in keep:
        for x in t:
            HL.inputs_unchanged(x)


# -- 9. into the engine ---------------------------------------------------------------------------

def test_cut_then_engine():
    """hpgq_ovl_batch_device's batches through hpgq_run_device (paired edit +
    filter + stats): counters, mask and trims as the oracle's on the reference's
    kept reads.  The outputs replace the inputs' structs."""
    import torch
    pairs = R.random_pairs(3000, 93, L=(60, 151))
    r1, r2 = _mates(pairs, plain_quality=True)
    want = R.Cut(r1, r2, 30, 5)
    kept = [O.Reads(want.seq[m], want.qual[m], want.idx[m]) for m in range(2)]
    assert 500 < want.info["clipped"] < 2500
    p = HL.params("paired", 150)
    m_o, t_o, c_o = O.run(p, kept[0], kept[1])
    assert 0 < int(m_o.sum()) < r1.n and np.count_nonzero(t_o) > 100
    t = [HL.device_batch(r1, lead=5, seq_shift=1, qual_shift=3), HL.device_batch(r2, lead=2, seq_shift=2, qual_shift=0)]
    mask = torch.full((r1.n,), POISON, dtype=torch.uint8, device="cuda")
    trim = torch.full((2 * r1.n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with H.Engine(p) as e, H.OverlapClip(30, 5, stream=e.stream) as ov:
        b = [H.engine.device_batch(r1.n, x.batch.seq, x.batch.quality, x.batch.data_indices) for x in t]
        H.check(H.lib.hpgq_ovl_batch_device(ov._h, C.byref(b[0]), C.byref(b[1]), C.byref(b[0]), C.byref(b[1])),
                "the inputs' structs as outputs")
        assert b[0].num_reads == r1.n and b[0].seq != t[0].batch.seq and b[1].seq != t[1].batch.seq
        e.run_device(b[0], b[1], mask.data_ptr(), trim.data_ptr())
        e.sync()
        ctr = e.counters()
        assert ov.info() == want.info
    np.testing.assert_array_equal(mask.cpu().numpy(), m_o)
    np.testing.assert_array_equal(trim.cpu().numpy().view(np.uint32), t_o)
    np.testing.assert_array_equal(ctr, c_o)
    for x in t:
        HL.inputs_unchanged(x)
