"""The engine's kernels on hostile bytes, writing into guarded, poisoned outputs
(tests/hostile_lib.py), bit for bit against the CPU oracle.

  * the atlas (every byte value at every residue, first, last, four in a
    dword, whole reads of it, the N and C/G look-alikes) through every first
    stage (routes hex, tri, wide) and the catch-all alone (single); an atlas
    with reads of 151, 200, 300 and 1,100 bases and units of deferred reads of
    157..300 through the automatic chain at lmax 150 (hex, then the catch-all
    as follow-up stage, then the long-read tail) and at lmax 1024 (hex, the
    wide geometry as follow-up stage for 157..252 bases, the catch-all, the
    tail), the stage names asserted; each with five option sets: stats; the
    C2 filter; max_N / max_out_of_quality on top; edit with both windows; mate
    pairs (mate 2: the atlas reversed);
  * device path, the sequence and quality pointers at different residues
    mod 4, garbage that counts before the first read and in the slack;
  * mask_out and trim_out lie between guard bands and are pre-filled with
    0xA5: every mask byte must come back 0 or 1 and every trim word the
    oracle's (the zeros of failing, untrimmed and empty reads are stores
    too); without edit the trim words are untouched; either output may be
    NULL; the inputs are unchanged afterwards;
  * a window past the batch's last read adds nothing (hostile against zero slack);
  * the host path's reused staging slots deliver no stale mask or trim, and
    no trim at all without edit;
  * hpgq_synth_device writes exactly its reads' bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import hostile_lib as HL
import hpgfastq as H
import oracle_lib as O
from test_filter_bounds_gpu import LENGTHS

pytestmark = pytest.mark.gpu

POS = {"hex": 156, "tri": 160, "wide": 252}
# case -> (atlas of HL.ATLAS_SETS, the route the engine is forced to).  "auto" (lmax 150): hex,
# then the catch-all, then the tail; "chain" (lmax 1024, no adaptive choice): hex, the wide
# follow-up stage, the catch-all, the tail
ROUTES = {"hex": ("hex", "hex"), "tri": ("tri", "tri"), "wide": ("wide", "wide"), "single": ("wide", "single"),
          "auto": ("auto", "auto"), "chain": ("chain", "auto_fixed")}
POISON = 0xA5


def _lmax(route):
    return HL.ATLAS_SETS[ROUTES[route][0]][2]


@functools.lru_cache(maxsize=None)
def _atlas_of(name):
    lengths, units, _ = HL.ATLAS_SETS[name]
    reads, planted = HL.atlas(lengths, deferred_units=units)
    assert reads.n % 64 == 1 and all(reads.n % s for s in (3, 4, 6))     # no multiple of a segment count
    assert len(set(zip(planted[:, 2].tolist(), (planted[:, 1] % 4).tolist()))) == 1024
    return reads, planted


@functools.lru_cache(maxsize=None)
def _mate2_of(name):
    return HL.reverse(_atlas_of(name)[0])


def _atlas(route):
    name = ROUTES[route][0]
    return _atlas_of("auto" if name == "chain" else name)      # (the same reads)


def _mates(route, nm):
    name = ROUTES[route][0]
    name = "auto" if name == "chain" else name
    return (_atlas_of(name)[0],) + ((_mate2_of(name),) if nm == 2 else ())


def _freeze(res):
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _oracle(route, config, lmax=None):
    p = HL.params(config, lmax or _lmax(route))
    return _freeze(O.run(p, *_mates(route, 2 if p.paired else 1)))


def _merged_max(p, mates, mask, trim):
    """The longest merged window: what lmax_ext must be."""
    best = p.lmax
    n = mates[0].n
    for m, r in enumerate(mates):
        t = trim[m * n:(m + 1) * n].astype(np.int64) if p.edit_on else np.zeros(n, np.int64)
        w = np.diff(r.idx) - (t & 0xFFFF) - (t >> 16)
        best = max(best, int(w[mask == 1].max(initial=0)))
    return best


def _expect_kernel(e, route, config, nm):
    """The chain's stage names, as tests/test_followup_units_gpu.py::_expect_chain reads them."""
    st = e.kernel_chain.split(" -> ")
    edit, noor = config in ("edit", "paired"), config == "noor"
    catch_all = f"hpgq::engine_kernel<{nm}, 5, true> (follow-up)"
    if route == "single":
        assert len(st) == 1 and st[0].startswith(f"hpgq::engine_kernel<{nm}, "), e.kernel_chain
        return
    assert " | adaptive" not in e.kernel_chain, e.kernel_chain
    geo = "hex" if route in ("auto", "chain") else route
    assert "engine_tri" in st[0] and geo in st[0] and "follow" not in st[0] and f", {nm}, " in st[0], e.kernel_chain
    assert st[0] == e.kernel_name
    assert ("noor" in st[0]) == noor and ("edit" in st[0]) == edit, e.kernel_chain
    if route == "auto":        # lmax 150 with stats: no read lies between hex and the wide geometry
        assert st[1:] == [catch_all], e.kernel_chain
    elif route == "chain":
        assert len(st) == 3 and st[2] == catch_all, e.kernel_chain
        assert "engine_tri" in st[1] and "wide" in st[1] and ", follow" in st[1] and f", {nm}, " in st[1], e.kernel_chain
        assert ("noor" in st[1]) == noor and ("edit" in st[1]) == edit, e.kernel_chain


def _differ(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:8]}: gpu {got[bad[:8]]} oracle {want[bad[:8]]}"


def _run(route, config, outputs=("mask", "trim"), counters=True):
    p = HL.params(config, _lmax(route))
    nm = 2 if p.paired else 1
    mates = _mates(route, nm)
    n = mates[0].n
    m_o, t_o, c_o = _oracle(route, config)
    if config != "stats":
        assert 0 < int(m_o.sum()) < n
    if p.edit_on:
        assert (t_o == 0).any() and (t_o & 0xFFFF).any() and (t_o >> 16).any()
        assert (t_o[:n][np.diff(mates[0].idx) == 0] == 0).all() and (np.diff(mates[0].idx) == 0).sum() >= 3
    # mate 1: 5 garbage bytes lead, pointers at residues 1 and 3; mate 2: none, residues 2 and 1
    dev = [HL.device_batch(r, lead=lead, seq_shift=ss, qual_shift=qs)
           for r, (lead, ss, qs) in zip(mates, ((5, 1, 3), (0, 2, 1)))]
    gm = HL.Guarded(n, 1, POISON) if "mask" in outputs else None
    gt = HL.Guarded(4 * n * nm, 4, POISON) if "trim" in outputs else None
    assert gm is None or gm.ptr % 2 == 1
    assert gt is None or gt.ptr % 4 == 0
    with H.Engine(p, route=ROUTES[route][1]) as e:
        _expect_kernel(e, route, config, nm)
        e.run_device(dev[0].batch, dev[1].batch if nm == 2 else None, gm.ptr if gm else None, gt.ptr if gt else None)
        e.sync()
        ctr = e.counters()
        ext, L = e.counters_ext()
    what = f"{route} {config} {'+'.join(outputs)}"
    if gm:
        mask = gm.check()
        assert np.isin(mask, (0, 1)).all(), f"{what}: mask bytes {np.unique(mask)} (0xA5: never stored)"
        _differ(mask, m_o, what + " mask")
    if gt:
        trim = gt.check()
        if p.edit_on:
            _differ(trim.view(np.uint32), t_o, what + " trim")
        else:
            assert (trim == POISON).all(), f"{what}: trim_out written without edit"
    for t in dev:
        HL.inputs_unchanged(t)
    if counters:
        _differ(ctr, c_o, what + " counters")
        assert L == _merged_max(p, mates, m_o, t_o), what
        c_x = _oracle(route, config, L)[2] if L != p.lmax else c_o
        _differ(ext, c_x, what + f" full-length counters (lmax_ext {L})")
    return L


@pytest.mark.parametrize("config", HL.CONFIGS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_atlas_through_every_kernel(route, config):
    L = _run(route, config)
    if route in ("auto", "chain") and config in ("stats", "c2"):
        assert L == 1100      # a read of 1,100 bases passed: the long-read tail took it


@pytest.mark.parametrize("outputs", [("mask",), ("trim",), ()])
@pytest.mark.parametrize("config", ["c2", "edit", "paired"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_either_output_may_be_null(route, config, outputs):
    _run(route, config, outputs)


STAGE_LENGTHS = {   # case -> the read lengths each stage after the first takes (with stats on)
    "auto": {"the catch-all": (151, 300), "the tail": (1100, 1100)},
    "chain": {"the wide follow-up": (157, 252), "the catch-all": (253, 300), "the tail": (1100, 1100)},
}


@pytest.mark.parametrize("route", sorted(STAGE_LENGTHS))
def test_planted_bytes_reach_every_later_stage(route):
    """From the lengths and the oracle alone: every byte value is planted in a
    read of each later stage's lengths, in passing and in failing reads.  (That
    the chain has exactly these stages is _expect_kernel's assertion.)"""
    reads, planted = _atlas(route)
    ln = np.diff(reads.idx)
    m_o = _oracle(route, "c2")[0]
    for stage, (lo, hi) in STAGE_LENGTHS[route].items():
        rows = planted[(ln[planted[:, 0]] >= lo) & (ln[planted[:, 0]] <= hi)]
        assert set(rows[:, 2].tolist()) == set(range(256)), (stage, len(set(rows[:, 2].tolist())))
        assert 0 < int(m_o[rows[:, 0]].sum()) < len(rows), stage


# ---------------------------------------------------------------------------
# the slack counts if touched
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ends_at_batch_end(geo):
    """Reads of mixed lengths; the last one ACGT... of the geometry's longest
    length, ending at the batch end."""
    reads, _ = HL.atlas(LENGTHS[geo], dense=False)
    L = POS[geo]
    last = (np.frombuffer(b"ACGT", np.uint8)[np.arange(L) % 4].tobytes(), bytes([33 + 30]) * L)
    return O.Reads.from_pairs(reads.pairs()[:700] + [last])


@pytest.mark.parametrize("config", ["stats", "noor", "edit"])
@pytest.mark.parametrize("route", ["hex", "tri", "wide", "single"])
def test_slack_is_not_counted(route, config):
    geo = "wide" if route == "single" else route
    reads = _ends_at_batch_end(geo)
    p = HL.params(config, POS[geo])
    m_o, t_o, c_o = O.run(p, reads)
    assert m_o[-1] == 1
    got = {}
    for slack in ("hostile", "zero"):
        t = HL.device_batch(reads, lead=3, seq_shift=3, qual_shift=2, slack_fill=slack)
        gm, gt = HL.Guarded(reads.n, 3, POISON), HL.Guarded(4 * reads.n, 4, POISON)
        with H.Engine(p, route=route) as e:
            e.run_device(t.batch, None, gm.ptr, gt.ptr)
            e.sync()
            got[slack] = e.counters()
        _differ(gm.check(), m_o, f"{route} {config} {slack} slack: mask")
        trim = gt.check()
        if p.edit_on:
            _differ(trim.view(np.uint32), t_o, f"{route} {config} {slack} slack: trim")
        else:
            assert (trim == POISON).all(), f"{route} {config} {slack} slack: trim_out written without edit"
        HL.inputs_unchanged(t)
    _differ(got["hostile"], got["zero"], f"{route} {config}: hostile against zero slack")
    _differ(got["hostile"], c_o, f"{route} {config}: counters")


# ---------------------------------------------------------------------------
# the host path's staging slots
# ---------------------------------------------------------------------------

def _slot_reads(kind, seed, n=1000):
    """pass: 100 bases of Q 30 with 1..9 low bases on the left and 1..20 on the
    right (trimmed on both sides, passes); fail: 30 bases of Q 30 (untrimmed,
    fails the length range); empty."""
    i = np.arange(n)
    L = {"pass": 100, "fail": 30, "empty": 0}[kind]
    seq = np.frombuffer(b"ACGT", np.uint8)[(np.arange(n * L) + seed) % 4].copy()
    qual = np.full(n * L, 33 + 30, np.uint8).reshape(n, L)
    if kind == "pass":
        j = np.arange(L)
        left, right = 1 + (i * 7 + seed) % 9, 1 + (i * 11 + seed) % 20
        qual[(j[None, :] < left[:, None]) | (j[None, :] >= L - right[:, None])] = 33 + 3
    return O.Reads(seq, np.ascontiguousarray(qual.reshape(-1)), (np.arange(n + 1) * L).astype(np.int32))


@pytest.mark.parametrize("sync_each", [True, False])
def test_host_path_delivers_no_stale_slot(sync_each):
    p = HL.params("edit", 150)
    kinds = ("pass", "pass", "fail", "fail", "empty", "empty")
    batches = [_slot_reads(k, s) for s, k in enumerate(kinds)]
    wants = [O.run(p, r) for r in batches]
    for k, (m_o, t_o, _) in zip(kinds, wants):
        assert (m_o == (k == "pass")).all()
        assert ((t_o & 0xFFFF) > 0).all() and ((t_o >> 16) > 0).all() if k == "pass" else (t_o == 0).all()
    assert (wants[0][1] != wants[1][1]).any()
    outs = []
    with H.Engine(p) as e:
        for r in batches:
            mask = np.full(r.n, 7, np.uint8)
            trim = np.full(r.n, 0x07070707, np.uint32)
            b = r.batch()
            e.run_host(b, None, mask, trim)
            outs.append((mask, trim, b))
            if sync_each:
                e.sync()
        e.sync()
        ctr = e.counters()
    for k, ((mask, trim, _), (m_o, t_o, _c)) in enumerate(zip(outs, wants)):
        _differ(mask, m_o, f"batch {k} ({kinds[k]}) mask")
        _differ(trim, t_o, f"batch {k} ({kinds[k]}) trim")
    _differ(ctr, sum(w[2] for w in wants), "counters of the six batches")


@pytest.mark.parametrize("route", ["hex", "single"])
def test_host_path_leaves_trims_alone_without_edit(route):
    """trim_out is edit's output.  Without edit no kernel owes it a store, so
    the host path must not copy the slot's bytes (the batch before last's
    inputs) into the caller's array."""
    p = HL.params("c2", 150)
    batches = [_slot_reads(k, s) for s, k in enumerate(("pass", "fail", "pass", "fail"))]
    outs = []
    with H.Engine(p, route=route) as e:
        for r in batches:
            mask, trim, b = np.full(r.n, 7, np.uint8), np.full(r.n, 0x07070707, np.uint32), r.batch()
            e.run_host(b, None, mask, trim)
            outs.append((mask, trim, b))
        e.sync()
    for k, (r, (mask, trim, _)) in enumerate(zip(batches, outs)):
        _differ(mask, O.run(p, r)[0], f"{route} batch {k} mask")
        assert (trim == 0x07070707).all(), f"{route} batch {k}: trim_out written without edit"


# ---------------------------------------------------------------------------
# hpgq_synth_device
# ---------------------------------------------------------------------------

def test_synth_device_writes_its_reads_and_nothing_else():
    import torch
    n = 2000
    s = H.Synth(7, 150, 50, 5, 4, 33, 0)
    want = O.synth(n, seed=7, L=150, trunc_pct=50, bad_pct=5, n_per_1024=4)
    idx = np.zeros(n + 1, np.int32)
    H.check(H.lib.hpgq_synth_indices_host(C.byref(s), 0, n, idx.ctypes.data_as(C.c_void_p)), "hpgq_synth_indices_host")
    np.testing.assert_array_equal(idx, want.idx)
    assert len(set(np.diff(idx).tolist())) > 50      # truncated reads: the reads start at every residue
    nb = int(idx[-1])
    gs, gq = HL.Guarded(nb, 1, POISON), HL.Guarded(nb, 3, POISON)
    d_idx = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    H.check(H.lib.hpgq_synth_device(C.byref(s), 0, n, gs.ptr, gq.ptr, d_idx.data_ptr(), None), "hpgq_synth_device")
    torch.cuda.synchronize()
    _differ(gs.check(), want.seq, "synthetic bases")
    _differ(gq.check(), want.qual, "synthetic qualities")
    np.testing.assert_array_equal(d_idx.cpu().numpy(), idx)
