"""`edit --clip-adapters` on the GPU: hpgq_clip_* (gfx950) against
tests/clip_ref.py: clip position, winning probe, output offsets, both output
byte ranges and the scalars.  A step of the find kernel
covers 244 starts (probes of up to 13 bases) or 224 (longer ones).  Every batch
goes up through hostile_lib.device_batch, every output of hpgq_clip_device lies
in a hostile_lib.Guarded buffer: poison stays behind the written bytes, both
bands stay intact.  Quality bytes depend on read and position and reach past
127, so a byte in the wrong place shows."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import clip_ref
import hostile_lib as HL
from adapt_ref import DEFAULT_PROBES as DEF
from test_adapt_gpu import _set32, _planted_batch, _plant, _acgt

pytestmark = pytest.mark.gpu

POISON = 0xA5
K = 12
# unequal (seq_shift, qual_shift), and the outputs' alignments, handed out in turn
SHIFTS = [(s, q) for s in range(4) for q in range(4) if s != q]
ALIGNS = [(s, q) for s in range(4) for q in range(4)]


def _reads(seqs, plain_quality=False):
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    idx = np.zeros(len(seqs) + 1, dtype=np.int32)
    idx[1:] = np.cumsum(lens)
    seq = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:-1].copy()
    i = np.repeat(np.arange(len(seqs)), lens)
    j = np.arange(len(seq)) - np.repeat(idx[:-1].astype(np.int64), lens)
    if plain_quality:
        qual = (33 + (j * 7 + i * 3) % 41).astype(np.uint8)
    else:
        qual = ((j * 37 + i * 101 + 7) & 0xFF).astype(np.uint8)
    return O.Reads(seq, qual, idx)


def _clip(cl, reads, want, *, lead=0, shifts=(0, 1), aligns=(0, 0), lead_fill="hostile", slack_fill="hostile",
          scalars=True):
    """hpgq_clip_device into guarded buffers, everything against `want`."""
    t = HL.device_batch(reads, lead=lead, seq_shift=shifts[0], qual_shift=shifts[1], lead_fill=lead_fill,
                        slack_fill=slack_fill)
    n, nbytes = reads.n, len(reads.seq)
    gs, gq = HL.Guarded(nbytes, aligns[0], POISON), HL.Guarded(nbytes, aligns[1], POISON)
    gi, gp, gw = HL.Guarded(4 * (n + 1), 4, POISON), HL.Guarded(4 * n, 4, POISON), HL.Guarded(n, 1, POISON)
    cl.clip_device(t.batch, gs.ptr, gq.ptr, gi.ptr, gp.ptr, gw.ptr)
    cl.sync()
    np.testing.assert_array_equal(gp.check().view(np.uint32), want.pos, err_msg="pos")
    np.testing.assert_array_equal(gw.check(), want.probe, err_msg="probe")
    np.testing.assert_array_equal(gi.check().view(np.int32), want.idx, err_msg="idx_out")
    kept = int(want.idx[-1])
    for name, g, w in (("seq", gs, want.seq), ("qual", gq, want.qual)):
        got = g.check()
        np.testing.assert_array_equal(got[:kept], w, err_msg=name + "_out")
        assert (got[kept:] == POISON).all(), name + "_out: a store behind idx_out[n]"
    HL.inputs_unchanged(t)
    if scalars:
        assert cl.info() == want.info
    return t


def _fresh(reads, probes, min_overlap, **kw):
    want = clip_ref.Clipped(reads, probes, min_overlap)
    with H.AdapterClip(probes, min_overlap) as cl:
        _clip(cl, reads, want, **kw)
    return want


# -- 1. every start, every alignment ------------------------------------------------------------

L1 = 296
OVERLAPS = [1, 5, 8, 11, 12, 32]


@pytest.fixture(scope="module")
def every_start():
    seqs = []
    for p in DEF:
        assert len(p) == K
        seqs += [_plant(b"N" * L1, s, p) for s in range(L1 - K + 1)]     # whole at every start 0 .. 284
        seqs += [b"N" * (L1 - m) + p[:m] for m in range(K - 1, 0, -1)]   # its first 11 .. 1 bases at the end
    reads = _reads(seqs)
    wants = {mo: clip_ref.Clipped(reads, DEF, mo) for mo in OVERLAPS}
    # the recipe means what it says: every start is a clip position, and the overlaps count from min_overlap on
    w = wants[1]
    assert set(w.pos.tolist()) == set(range(L1)) and w.info["clipped"] == reads.n
    for mo in OVERLAPS:
        assert wants[mo].info["clipped"] == len(DEF) * (L1 - K + 1 + max(0, K - mo))
    return reads, wants


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 13])
@pytest.mark.parametrize("min_overlap", OVERLAPS)
def test_every_start_every_alignment(every_start, min_overlap, lead):
    reads, wants = every_start
    case = OVERLAPS.index(min_overlap) * 5 + [0, 1, 2, 3, 13].index(lead)
    with H.AdapterClip(None, min_overlap) as cl:
        _clip(cl, reads, wants[min_overlap], lead=lead, shifts=SHIFTS[case % len(SHIFTS)], aligns=ALIGNS[case % len(ALIGNS)])


# -- 2. near misses -----------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap", [3, 8])
def test_near_misses(min_overlap):
    p = DEF[0]
    seqs = []
    for part in (K, 9, 5):                                               # a whole window, two that the read ends in
        for at in range(part):
            for v in range(256):
                if v != p[at]:
                    seqs.append(b"N" * 5 + _plant(p[:part], at, bytes([v])) + (b"N" * 5 if part == K else b""))
    reads = _reads(seqs)
    want = _fresh(reads, DEF, min_overlap, lead=1, shifts=(2, 3), aligns=(1, 3))
    # next to none of them matches: what does is another probe's start, or a shorter overlap behind the changed byte
    assert want.info["clipped"] < reads.n // 4


# -- 3. the read's end --------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap", [1, 4, 5, 8, 12])
def test_reads_end(min_overlap):
    """Read i ends in p[:cut], read i + 1 starts with p[cut:]: no whole match over
    the boundary, an overlap iff cut >= min_overlap.  The last read ends on the
    data's last byte and the slack goes on with the probe."""
    seqs, expect = [], []
    for p in DEF[:4]:
        for cut in range(1, K):
            seqs += [b"N" * 20 + p[:cut], p[cut:] + b"N" * 20]
            expect += [20 if cut >= min_overlap else 20 + cut, K - cut + 20]
    cut = 4
    rest = DEF[0][cut:]
    seqs.append(b"N" * 9 + DEF[0][:cut])
    expect.append(9 if cut >= min_overlap else 9 + cut)
    reads = _reads(seqs)
    want = _fresh(reads, DEF[:4], min_overlap, lead=3, shifts=(3, 0), aligns=(2, 1), lead_fill=rest, slack_fill=rest)
    np.testing.assert_array_equal(want.pos, expect)


# -- 4. step edges ------------------------------------------------------------------------------

def _edge_reads(probes, edges, rng):
    seqs = []
    for p in probes:
        for e in edges:
            for fill in (b"N", None):
                body = (lambda n: fill * n) if fill else (lambda n: _acgt(rng, n))
                seqs.append(body(e) + p + body(30))                      # whole, at the edge
                seqs.append(body(e) + p)                                 # whole, the read ends with it
                seqs.append(body(e) + p[:9])                             # the read ends inside it
                seqs.append(body(e) + p[:4])
                seqs.append(body(e))                                     # the read ends at the edge
    return seqs


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_step_edges(name):
    rng = np.random.default_rng(41)
    if name == "narrow":
        probes, edges = DEF, (243, 244, 245, 487, 488)
    else:
        probes, edges = [_acgt(rng, 32), DEF[0], _acgt(rng, 8)], (223, 224, 225, 447, 448)
    seqs = _edge_reads(probes, edges, rng)
    while True:                                                          # 70,000 bases, the only hit a 9-base overlap at the end
        long_ = _acgt(rng, 70000 - 9) + probes[0][:9]
        if clip_ref.find(long_, probes, 4)[0] == 70000 - 9:
            break
    seqs.append(long_)
    reads = _reads(seqs)
    for mo in (4, 8):
        want = _fresh(reads, probes, mo, lead=2, shifts=(1, 2), aligns=(3, 0))
        assert want.pos[-1] == 70000 - 9 and want.info["clipped"] > len(seqs) // 2


# -- 5. who wins --------------------------------------------------------------------------------

def test_who_wins():
    long_ = b"ACGGTCATTGCAAC"
    tail = b"ACGTACGTTTAG"                                               # ends in AG: the start of DEF[0]
    cases = [
        # probes, min_overlap, read, c, winner
        ([long_, long_[:10], long_, DEF[1]], 8, b"N" * 7 + long_ + b"N" * 9, 7, 0),
        ([long_[:10], long_, long_[:10]], 8, b"N" * 7 + long_ + b"N" * 9, 7, 0),
        ([long_, long_[:10]], 8, b"N" * 7 + long_[:12], 7, 0),           # both run off the end: the lower one
        ([long_, long_[:10]], 11, b"N" * 7 + long_[:10], 7, 1),          # 10 < 11: only the whole shorter one
        (DEF, 8, b"N" * 20 + DEF[1] + b"N" * 28 + DEF[0] + b"N", 20, 1),
        (DEF, 8, b"G" * 12 + b"A" * 12, 0, 5),
        ([b"CACACACACA", b"ACACACACAC"], 8, b"NN" + b"ACACACACACA", 2, 1),   # two starts of one lane
        ([b"CACACACACA", b"ACACACACAC"], 8, b"NNN" + b"ACACACACACA", 3, 1),  # two lanes
        ([tail, DEF[0]], 2, b"N" * 20 + tail, 20, 0),                    # the overlap AG at 30 loses
        ([tail, DEF[0]], 1, b"N" * 20 + tail + b"A", 20, 0),
        ([tail, DEF[0]], 1, b"N" * 20 + tail[1:] + b"A", 29, 1),             # no whole match: the overlap AGA
        ([tail, DEF[0]], 2, b"NNNNNAG", 5, 1),
        ([tail, DEF[0]], 1, b"NNNNNA", 5, 0),                            # A starts both: the lower one
    ]
    for probes, mo, read, c, who in cases:
        assert clip_ref.find(read, probes, mo) == (c, who), read
        reads = _reads([b"N" * 30, read, b"", read, b"ACGT" * 70 + read])
        want = _fresh(reads, probes, mo, lead=1, shifts=(1, 3), aligns=(2, 2))
        assert (int(want.pos[1]), int(want.probe[1])) == (c, who)


# -- 6. short reads -----------------------------------------------------------------------------

@pytest.mark.parametrize("min_overlap", [1, 4, 8])
def test_short_reads(min_overlap):
    rng = np.random.default_rng(43)
    seqs = [DEF[a][:m] for a in range(len(DEF)) for m in range(0, K + 1)]       # a probe's start of each length, and the probe
    seqs += [b"N" + DEF[a][:m] for a in range(len(DEF)) for m in range(0, K + 1)]
    seqs += [DEF[2] + b"AC", b"", b"", b"N"]
    for i in range(400):
        seqs.append(_acgt(rng, int(rng.integers(0, 15))))
    assert {len(s) for s in seqs} == set(range(15))
    reads = _reads(seqs)
    want = _fresh(reads, DEF, min_overlap, lead=3, shifts=(2, 1), aligns=(1, 0))
    assert int((want.pos == 0).sum()) >= len(DEF) * (K + 1 - min_overlap)


# -- 7. probe sets ------------------------------------------------------------------------------

def _planted(probes, n, seed):
    """test_adapt_gpu's planted reads, every 13th ending inside a probe."""
    base = _planted_batch(probes, n=n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    seqs = []
    for i in range(base.n):
        s = base.read(i)[0]
        if i % 13 == 0:
            p = probes[i % len(probes)]
            m = int(rng.integers(1, len(p)))
            s = s[:len(s) - m] + p[:m]
        seqs.append(s)
    return _reads(seqs)


@pytest.fixture(scope="module")
def set_cases():
    out = {}
    for name, probes, n in (("default", DEF, 20000), ("32", _set32(), 5000)):
        reads = _planted(probes, n, 44)
        want = clip_ref.Clipped(reads, probes, 6)
        assert want.info["clipped"] > n // 5 and min(want.info["by_probe"][:6]) > 0
        out[name] = (probes, reads, want)
    return out


@pytest.mark.parametrize("name", ["default", "32"])
def test_probe_sets(set_cases, name):
    probes, reads, want = set_cases[name]
    with H.AdapterClip(probes, 6) as cl:
        _clip(cl, reads, want, lead=1, shifts=(1, 2), aligns=(3, 1))


@pytest.mark.parametrize("max_wg", [1, 2])
@pytest.mark.parametrize("name", ["default", "32"])
def test_few_workgroups(set_cases, name, max_wg):
    probes, reads, want = set_cases[name]
    with H.AdapterClip(probes, 6) as cl:
        cl.set_max_workgroups(max_wg)
        _clip(cl, reads, want, shifts=(3, 2), aligns=(0, 2))


# -- 8. compaction ------------------------------------------------------------------------------

KEPT = [0, 1, 2, 3, 4, 5, 0, 0, 1, 37, 2, 150, 3, 3, 1, 1, 2, 0, 5, 263, 4]


def _compaction_reads(n, kind):
    """kind 'mixed': read i keeps KEPT[i % ..] bases, every seventh read all of
    its own; 'none': no probe anywhere; 'all': every read starts with one."""
    seqs = []
    for i in range(n):
        body = (b"ACGT" * 70)[i % 4:][:KEPT[(i * 5 + i // 21) % len(KEPT)]]
        p = DEF[i % 4]
        if kind == "none" or (kind == "mixed" and i % 7 == 3):
            seqs.append(body)
        elif kind == "all":
            seqs.append(p + body)
        else:
            seqs.append(body + p + b"ACGT" * (i % 3))
    return _reads(seqs)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 127, 128, 129, 20000])
def test_compaction(n):
    case = [0, 1, 15, 16, 17, 127, 128, 129, 20000].index(n)
    reads = _compaction_reads(n, "mixed")
    want = clip_ref.Clipped(reads, DEF, 8)
    if n >= 15:
        assert {0, 1, 2, 3, 4, 5} <= set(want.pos.tolist()) and 0 < want.info["clipped"] < n
    with H.AdapterClip() as cl:
        for k, max_wg in enumerate((0, 1, 2)):
            cl.set_max_workgroups(max_wg)
            _clip(cl, reads, want, lead=case % 4, shifts=SHIFTS[(case + 5 * k) % len(SHIFTS)],
                  aligns=ALIGNS[(case * 3 + 5 * k + 1) % len(ALIGNS)], scalars=False)
        got = cl.info()
    assert got == clip_ref.add([want.info] * 3)


@pytest.mark.parametrize("kind", ["none", "all"])
def test_compaction_nothing_and_everything(kind):
    reads = _compaction_reads(1000, kind)
    want = clip_ref.Clipped(reads, DEF, 8)
    if kind == "none":
        np.testing.assert_array_equal(want.idx, reads.idx)
        np.testing.assert_array_equal(want.qual, reads.qual)
    else:
        assert not want.idx.any() and want.seq.size == 0                 # (_clip: every output byte is still poison)
    for a in range(4):
        with H.AdapterClip() as cl:
            _clip(cl, reads, want, lead=a, shifts=SHIFTS[a * 3], aligns=(a, 3 - a))


# -- 9. scalars ---------------------------------------------------------------------------------

def test_scalars_accumulate_and_reset(set_cases):
    probes, reads, want = set_cases["32"]
    other = _compaction_reads(300, "mixed")
    want2 = clip_ref.Clipped(other, probes, 6)
    import torch
    with H.AdapterClip(probes, 6) as cl:
        assert cl.info() == dict(want.info, reads=0, clipped=0, bases_removed=0, by_probe=[0] * 32)
        keep = [HL.device_batch(r, lead=1) for r in (reads, other, reads)]
        for t in keep:
            pos = torch.empty(t.batch.num_reads, dtype=torch.int32, device="cuda")
            cl.find(t.batch, pos.data_ptr())                             # positions only, no probe output
            cl.sync()
        cl.find(H.engine.device_batch(0, 0, 0, 0), None)                 # an empty batch
        assert cl.info() == clip_ref.add([want.info, want2.info, want.info])
        np.testing.assert_array_equal(pos.cpu().numpy().view(np.uint32), want.pos)
        cl.reset()
        assert cl.info()["reads"] == 0 and not any(cl.info()["by_probe"])
        _clip(cl, other, want2)
    for t in keep:
        HL.inputs_unchanged(t)


# -- 10. into the engine ------------------------------------------------------------------------

def test_clip_then_engine():
    """hpgq_clip_batch_device's batch through hpgq_run_device (edit + filter +
    stats): counters, mask and trims as the oracle's on clip_ref's kept reads."""
    import torch
    import ctypes as C
    base = _planted(DEF, 3000, 45)
    seqs = [base.read(i)[0] for i in range(base.n)]
    seqs[7] = DEF[3] + seqs[7][K:]                                       # clipped to nothing
    reads = _reads(seqs, plain_quality=True)
    want = clip_ref.Clipped(reads, DEF, 5)
    kept = O.Reads(want.seq, want.qual, want.idx)
    assert 500 < want.info["clipped"] < 2500 and (want.pos == 0).any()
    p = HL.params("edit", 150)
    m_o, t_o, c_o = O.run(p, kept)
    assert 0 < int(m_o.sum()) < reads.n and np.count_nonzero(t_o) > 100
    t = HL.device_batch(reads, lead=5, seq_shift=1, qual_shift=3)
    mask = torch.full((reads.n,), POISON, dtype=torch.uint8, device="cuda")
    trim = torch.full((reads.n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with H.Engine(p) as e, H.AdapterClip(None, 5, stream=e.stream) as cl:
        out = H.engine.device_batch(reads.n, t.batch.seq, t.batch.quality, t.batch.data_indices)
        H.check(H.lib.hpgq_clip_batch_device(cl._h, C.byref(out), C.byref(out)), "in and out the same struct")
        assert out.num_reads == reads.n and out.seq != t.batch.seq
        e.run_device(out, None, mask.data_ptr(), trim.data_ptr())
        e.sync()
        ctr = e.counters()
        assert cl.info() == want.info
    np.testing.assert_array_equal(mask.cpu().numpy(), m_o)
    np.testing.assert_array_equal(trim.cpu().numpy().view(np.uint32), t_o)
    np.testing.assert_array_equal(ctr, c_o)
    HL.inputs_unchanged(t)
