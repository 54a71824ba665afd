"""Follow-up stages over several units per wave, every variant.

A follow-up stage (the wide segmented kernel over what the first stage
deferred, the catch-all over what is left, the catch-all again as the
long-read tail's second pass) walks the FIRST stage's units: wave gw of nw
takes units gw, gw + nw, ... and skips those without a deferred read.  What
a wave carries from one unit to the next (the pipeline slot and read-table
parity, the compaction scratch, the prefetched offsets, the rewritten
deferral word) only matters once a wave runs a second unit, which a batch of
a few thousand reads never gives a grid of thousands of waves.  So these
tests cap the grid (hpgq_debug_set_max_workgroups(2): 8 waves) and give
every wave 7 or more units of every kind; three cases at the natural grid
(3 * the widest stage's waves + 5 units) show that the cap hides nothing.

Every comparison is bit for bit against the CPU oracle: the mask, both
mates' trim words with edit, the counters.  Inputs are built explicitly and
keyed on the first-stage unit u = i // B (B: 48 hex, 54 tri, 60 wide) through
(u + shift) % 7; 7 is coprime to every wave count in use, so each wave meets
every class:

  class 0, 5  no deferred read (the iterator skips the unit)
  class 1     one read at position 0, 200 bases (to wide)
  class 2     positions 1, B/2, B-1 with 157, 252 and 253 bases (two to
              wide, one to the catch-all; the top bit of the unit's mask)
  class 3     the whole unit, 157 .. 252 bases
  class 4     two reads of 300 and 1000 bases (the wide stage defers its
              whole unit again: nothing to stream)
  class 6     B-1 reads alternating wide (157 .. 252) and catch-all
              (253 .. 300) lengths, the one left of zero length

The other reads have 20 .. 60 bases, some none.  The batch ends in a short
unit of class 2, so its last read is a deferred one.  In paired cases mate 2
follows the same pattern three classes on: a pair is deferred when either
mate is long, and the mates disagree on which.  At the natural grid a wave
has three units only, so there every unit also holds one read of catch-all
length (`dense`); the units to skip are the capped matrix's business.

Before a GPU result is looked at each test asserts, from the lengths, the
stages' deferral rule and the oracle alone: (a) every wave of every follow-up
stage (hpgq_debug_stage_waves) has at least 3 units holding a read deferred
to that stage; (b) those reads both pass and fail; (c) with edit their trim
words are both zero and non-zero; (d) the planned chain is the intended one.
"""
import functools

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

BLOCK = {"hex": 48, "tri": 54, "wide": 60}    # reads per unit of a first stage
POS = {"hex": 156, "tri": 160, "wide": 252}   # the longest read a geometry holds
CAP_UNITS = 8 * 7 + 3                         # full units of a capped batch (8 waves: 7 or 8 units each)
C2 = dict(read_quality_range="20,", read_length_range="50,")
TRIMS = dict(left_length=10, left_quality_range="20,", right_length=30, right_quality_range="20,")


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _batch_size(B, full_units):
    """`full_units` whole units and a short one of B/2 + 1 reads."""
    return B * full_units + B // 2 + 1


def _shift_for(B, n, last_class=2):
    """The class shift that gives the batch's last unit `last_class`."""
    return (last_class - (n - 1) // B) % 7


def _lengths(B, n, shift, dense=False, long=True, short=(20, 60), scale=None):
    """Read lengths of the class pattern (explicit, no random draw).
    scale: (lo, hi) squeezes the deferred lengths into lo .. hi (the tail test)."""
    i = np.arange(n, dtype=np.int64)
    u, pos = i // B, i % B
    nu = np.minimum(B, n - u * B)   # reads of the read's own unit (the last one is short)
    cls = (u + shift) % 7
    ln = short[0] + (i * 11) % (short[1] - short[0] + 1)
    if short[0] >= 20:
        ln[(i * 5) % 23 == 3] = 0
    if not long:
        return ln
    if scale is None:
        wide_len = 157 + (i * 29) % 96     # 157 .. 252
        call_len = 253 + (i * 31) % 48     # 253 .. 300
        one, three, two = 200, (157, 252, 253), (300, 1000)
    else:
        lo, hi = scale
        wide_len = lo + (i * 29) % (hi - lo + 1)
        call_len = lo + (i * 31) % (hi - lo + 1)
        one, three, two = (lo + hi) // 2, (lo, hi - 1, hi), (lo + 1, hi)
    ln[(cls == 1) & (pos == 0)] = one
    c = cls == 2
    ln[c & (pos == 1)] = three[0]
    ln[c & (pos == nu // 2)] = three[1]
    ln[c & (pos == nu - 1)] = three[2]
    c = cls == 3
    ln[c] = wide_len[c]
    c = cls == 4
    ln[c & (pos == 3)] = two[0]
    ln[c & (pos == nu - 2)] = two[1]
    c = cls == 6
    ln[c] = np.where(pos % 2 == 1, wide_len, call_len)[c]
    ln[c & (pos == 0)] = 0
    if dense:   # every unit: one read of catch-all length
        c = pos == (u * 5 + 2) % nu
        ln[c] = (253 + (u * 17) % 200)[c]
    return ln


_BASES = np.frombuffer(b"ACGT" * 18 + b"ACN", np.uint8)   # 1 N in 75: ~2 per 150 bases


def _fill(ln, B, seed):
    """Bases and qualities for the lengths `ln`: a quality level per read
    around the filter's Phred 20 with jitter, every fifth read with
    low-quality ends (the trims)."""
    n = len(ln)
    idx = np.zeros(n + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    nb = int(idx[-1])
    rng = np.random.default_rng(seed)
    seq = _BASES[rng.integers(0, len(_BASES), nb, dtype=np.uint8)]
    i = np.arange(n)
    level = (33 + 12 + (i * 7 + i // B) % 20).astype(np.uint8)
    qual = np.repeat(level, ln) + rng.integers(0, 9, nb, dtype=np.uint8)
    sel = np.nonzero((i % 5 == 2) & (ln > 0))[0]
    a, e, L = idx[sel].astype(np.int64), idx[sel + 1].astype(np.int64), ln[sel]
    for k in range(9):
        qual[(a + k)[k < np.minimum(L // 3, 9)]] = 33 + 3
    for k in range(25):
        qual[(e - 1 - k)[k < np.minimum(L // 4, 25)]] = 33 + 4
    r = O.Reads(np.ascontiguousarray(seq), np.ascontiguousarray(qual), idx)
    for arr in (r.seq, r.qual, r.idx):
        arr.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _mate(B, n, shift, mate, dense=False, long=True):
    """Mate `mate` of a batch: mate 2 runs three classes ahead of mate 1."""
    return _fill(_lengths(B, n, shift + 3 * mate, dense, long), B, 11 + 100 * mate + shift)


def _mates(B, n, shift, nm, dense=False, long=True):
    return [_mate(B, n, shift, m, dense, long) for m in range(nm)]


# ---------------------------------------------------------------------------
# options, the oracle, the deferral rule
# ---------------------------------------------------------------------------

def _params(kind, lmax, paired, scans="none", stats=True):
    """kind: filter (C2's flags; stats on top unless stats=False) or edit;
    scans: the segmented kernels' extra scans (none, noor, window, both)."""
    flags = dict(C2)
    if scans in ("noor", "both"):
        flags.update(max_N=4, max_out_of_quality=50)
    win = scans in ("window", "both")
    if kind == "filter":
        if win:
            flags.update(left_length=12, left_quality_range="24,", right_length=20, right_quality_range="10,38")
        p = H.stats_params(lmax=lmax, **flags) if stats else H.filter_params(lmax=lmax, **flags)
    else:
        p = H.edit_params(lmax=lmax, stats=stats, **TRIMS, **flags)
        if win:   # (edit's own options switch the filter's windows off: set them on the struct)
            p.filter_on = 1
            p.left_length, p.min_left_quality, p.max_left_quality = 12, 24, H.MAX_VALUE
            p.right_length, p.min_right_quality, p.max_right_quality = 20, 10, 38
    p.paired = paired
    return p


def _freeze(res):
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _oracle(kind, lmax, paired, scans, stats, B, n, shift, dense=False, long=True):
    """The reference result, computed once and shared (read-only)."""
    return _freeze(O.run(_params(kind, lmax, paired, scans, stats), *_mates(B, n, shift, 1 + paired, dense, long)))


def _stage_rules(e, geo, p, has2, chain=0):
    """[(stage, waves, defer limit of the stage before)] of the chain's
    follow-up stages; asserts which stages the chain has."""
    B = BLOCK[geo]
    lim = (lambda pos: min(pos, p.lmax)) if p.stats_on else (lambda pos: pos)
    w1, b1 = e.stage_waves(1, chain)
    assert b1 == B
    rules = []
    if has2:
        w, b = e.stage_waves(2, chain)
        assert b == B
        rules.append((2, w, lim(POS[geo])))
    else:
        with pytest.raises(H.HpgqError):
            e.stage_waves(2, chain)
    w, b = e.stage_waves(3, chain)
    assert b == B
    rules.append((3, w, lim(POS["wide"]) if has2 else lim(POS[geo])))
    return w1, rules


def _conditions(rules, B, mates, want, edit, min_units=3):
    """(a), (b), (c) on the lengths and the oracle result alone."""
    m_o, t_o, _ = want
    n = mates[0].n
    longest = np.max([np.diff(r.idx) for r in mates], axis=0)
    for stage, nw, limit in rules:
        d = longest > limit   # a pair goes on when either mate is too long
        if min_units:
            per_wave = np.bincount(np.unique(np.nonzero(d)[0] // B) % nw, minlength=nw)
            assert per_wave.min() >= min_units, (stage, nw, int(per_wave.min()), int(per_wave.argmin()))
        assert 0 < int(m_o[d].sum()) < int(d.sum()), (stage, "the deferred reads all pass or all fail")
        if edit:
            t = t_o.reshape(len(mates), n)[:, d]
            assert (t == 0).any() and (t != 0).any(), (stage, "the deferred reads' trims are all zero or all set")


def _expect_chain(e, geo, nm, kind, scans, has2):
    """(d): the chain's stage names."""
    assert " | adaptive" not in e.kernel_chain, e.kernel_chain
    st = e.kernel_chain.split(" -> ")
    assert len(st) == (3 if has2 else 2), e.kernel_chain
    assert "engine_tri" in st[0] and geo in st[0] and "follow" not in st[0] and f", {nm}, " in st[0], e.kernel_chain
    if has2:
        s2 = st[1]
        assert "engine_tri" in s2 and "wide" in s2 and ", follow" in s2 and f", {nm}, " in s2, e.kernel_chain
        assert ("edit" in s2) == (kind == "edit"), e.kernel_chain
        assert ("noor" in s2) == (scans in ("noor", "both")), e.kernel_chain
        assert ("window" in s2) == (scans in ("window", "both")), e.kernel_chain
    assert f"engine_kernel<{nm}, 5, true> (follow-up)" in st[-1], e.kernel_chain


def _same(mask, trim, ctr, want, edit, what):
    m_o, t_o, c_o = want
    diffs = []
    bad = np.nonzero(mask != m_o)[0]
    if bad.size:
        diffs.append(f"{bad.size} of {mask.size} masks differ, first at reads {bad[:8]}")
    bad = np.nonzero(trim != t_o)[0] if edit else bad[:0]
    if bad.size:
        diffs.append(f"{bad.size} trim words differ, first at {bad[:8]}")
    bad = np.nonzero(ctr != c_o)[0] if ctr is not None else bad[:0]
    if bad.size:
        diffs.append(f"{bad.size} counters differ, first at {bad[:8]} gpu={ctr[bad[:8]]} oracle={c_o[bad[:8]]}")
    assert not diffs, f"{what}: " + "; ".join(diffs)


def _to_device(torch, r):
    pad = np.zeros(H.DEVICE_SLACK, np.uint8)
    t = [torch.from_numpy(np.concatenate([r.seq, pad])).cuda(), torch.from_numpy(np.concatenate([r.qual, pad])).cuda(),
         torch.from_numpy(r.idx.copy()).cuda()]
    return t, H.engine.device_batch(r.n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def _run(e, mates, path):
    """One batch through the host or the device path -> mask, trim."""
    if path == "host":
        args = [a for r in mates for a in (r.seq, r.qual, r.idx)]
        return e.process(*args)
    torch = pytest.importorskip("torch")
    n = mates[0].n
    dev = [_to_device(torch, r) for r in mates]
    dm = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dt = torch.zeros(n * len(mates), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.run_device(dev[0][1], dev[1][1] if len(mates) > 1 else None, dm.data_ptr(), dt.data_ptr())
    e.sync()
    return dm.cpu().numpy(), dt.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------
# the capped matrix
# ---------------------------------------------------------------------------

# (route, lmax, mates, kind, scans, stats, has a wide follow-up)
MATRIX = (
    # all 16 wide follow-up variants
    [("hex", 1024, nm, kind, scans, True, True) for nm in (1, 2) for kind in ("filter", "edit")
     for scans in ("none", "noor", "window", "both")]
    # behind tri (units of 54, the `held` mask); behind wide (units of 60, no stage 2, pending_clear2)
    + [("tri", 1024, nm, kind, "none", True, True) for nm in (1, 2) for kind in ("filter", "edit")]
    + [("wide", 1024, nm, kind, "none", True, False) for nm in (1, 2) for kind in ("filter", "edit")]
    # lmax 150: hex hands straight to the catch-all
    + [("hex", 150, 2, "filter", "none", True, False), ("hex", 150, 1, "edit", "none", True, False),
       ("hex", 150, 2, "edit", "none", True, False)]
    # stats off: the deferral limit is the geometry's own, so hex -> wide -> catch-all at lmax 150 too
    + [("hex", 150, 1, "filter", "none", False, True), ("hex", 150, 1, "edit", "none", False, True)]
)


def _case_id(c):
    route, lmax, nm, kind, scans, stats, _ = c
    return f"{route}-{lmax}-{'pe' if nm == 2 else 'se'}-{kind}-{scans}{'' if stats else '-nostats'}"


@pytest.mark.parametrize("case", MATRIX, ids=_case_id)
def test_capped_grid(case):
    route, lmax, nm, kind, scans, stats, has2 = case
    B = BLOCK[route]
    n = _batch_size(B, CAP_UNITS)
    shift = _shift_for(B, n)
    p = _params(kind, lmax, nm - 1, scans, stats)
    mates = _mates(B, n, shift, nm)
    want = _oracle(kind, lmax, nm - 1, scans, stats, B, n, shift)
    assert np.diff(mates[0].idx)[-1] > POS["wide"]   # the batch's last read is a deferred one
    with H.Engine(p, route=route) as e:
        e.set_max_workgroups(2)
        _expect_chain(e, route, nm, kind, scans, has2)
        w1, rules = _stage_rules(e, route, p, has2)
        assert w1 == 8 and all(w == 8 for _, w, _ in rules), (w1, rules)
        _conditions(rules, B, mates, want, kind == "edit")
        mask, trim = _run(e, mates, "host")
        _same(mask, trim, e.counters(), want, kind == "edit", _case_id(case))


def test_grid_cap_entry_points():
    """The cap survives hpgq_debug_set_route and hpgq_reset, 0 lifts it, and
    bad arguments are HPGQ_E_INVALID."""
    p = H.stats_params(lmax=1024, **C2)
    with H.Engine(p) as e:
        full = [e.stage_waves(s) for s in (1, 2, 3, 4)]
        assert [b for _, b in full] == [48, 48, 48, 64] and all(w >= 8 and w % 4 == 0 for w, _ in full), full
        assert e.stage_waves(1, chain=1)[1] == 60   # the adaptive wide-first chain
        with pytest.raises(H.HpgqError):
            e.stage_waves(2, chain=1)
        e.set_max_workgroups(2)
        assert [e.stage_waves(s)[0] for s in (1, 2, 3, 4)] == [8] * 4
        e.set_route("wide")
        e.reset()
        assert [e.stage_waves(s) for s in (1, 3, 4)] == [(8, 60), (8, 60), (8, 64)]
        for bad in ((2, 0), (0, 0), (5, 0), (1, 1), (1, -1)):   # (stage, chain) this ctx does not have
            with pytest.raises(H.HpgqError) as ei:
                e.stage_waves(*bad)
            assert ei.value.code == -1
        assert H.lib.hpgq_debug_set_max_workgroups(e._h, -1) == -1
        assert H.lib.hpgq_debug_set_max_workgroups(None, 0) == -1
        assert e.stage_waves(1)[0] == 8   # (a rejected value changes nothing)
        e.set_max_workgroups(0)
        e.set_route("auto")
        assert [e.stage_waves(s) for s in (1, 2, 3, 4)] == full


# ---------------------------------------------------------------------------
# call-to-call state: bits1 / bits2, the unit_and mask, PEND1 / PEND2 by
# parity, follow_up_idle
# ---------------------------------------------------------------------------

SEQ_FLAGS = {"c2": ("filter", 0), "pe_edit": ("edit", 1)}


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("flags", sorted(SEQ_FLAGS))
@pytest.mark.parametrize("route,cap", [("hex", 2), ("auto", 0)])
def test_call_sequence_on_one_context(route, cap, flags, path):
    """A: the pattern; B: the classes one on (every stale mask word disagrees
    with the new one); C: no deferred read (the follow-up stages exit idle);
    D: a third of the size (stale words lie past its units); E: A again.
    Capped on route hex; uncapped on route auto, where whichever chain the
    adaptive choice picks must be exact."""
    kind, paired = SEQ_FLAGS[flags]
    B, lmax, nm = BLOCK["hex"], 1024, 1 + paired
    n = _batch_size(B, CAP_UNITS)
    n_d = _batch_size(B, CAP_UNITS // 3)
    s = _shift_for(B, n)
    calls = [("A", n, s, True), ("B", n, s + 1, True), ("C", n, s, False), ("D", n_d, _shift_for(B, n_d), True),
             ("E", n, s, True)]
    p = _params(kind, lmax, paired)
    with H.Engine(p, route=route) as e:
        e.set_max_workgroups(cap)
        if cap:
            _expect_chain(e, "hex", nm, kind, "none", True)
            _, rules = _stage_rules(e, "hex", p, True)
        total = np.zeros(H.counters_len(lmax) * nm, np.uint64)
        for name, n_c, shift, long in calls:
            mates = _mates(B, n_c, shift, nm, long=long)
            want = _oracle(kind, lmax, paired, "none", True, B, n_c, shift, long=long)
            longest = np.max([np.diff(r.idx) for r in mates], axis=0)
            if not long:
                assert longest.max() <= POS["hex"]
            elif cap:   # (D has under three units a wave: conditions (b), (c) only)
                _conditions(rules, B, mates, want, kind == "edit", min_units=3 if n_c == n else 0)
            mask, trim = _run(e, mates, path)
            _same(mask, trim, None, want, kind == "edit", f"call {name}")
            total += want[2]
        ctr = e.counters()
    bad = np.nonzero(ctr != total)[0]
    assert bad.size == 0, f"{bad.size} accumulated counters differ, first at {bad[:8]}: {ctr[bad[:8]]} vs {total[bad[:8]]}"


# ---------------------------------------------------------------------------
# the long-read tail's second pass (hpgq_sync -> resolve): units of 64
# ---------------------------------------------------------------------------

TAIL_LMAX = 64


@functools.lru_cache(maxsize=None)
def _tail_mates(shift, paired):
    """64 * 59 - 5 reads of 10 .. 64 bases; the pattern's deferred reads have
    65 .. 400 (one, three, two, 63 and 64 of them a unit).  Paired: only one
    mate of a pair is long, mate 1 in even units and mate 2 in odd ones."""
    n = 64 * CAP_UNITS - 5
    out = []
    for m in range(1 + paired):
        ln = _lengths(64, n, shift + 3 * m, short=(10, 64), scale=(65, 400))
        if paired:
            short = _lengths(64, n, shift, long=False, short=(10, 64))
            ln = np.where((np.arange(n) // 64) % 2 == m, ln, short)
        out.append(_fill(ln, 64, 31 + 100 * m + shift))
    return out


def _add(results):
    return sum(r[2].astype(np.uint64) for r in results)


@pytest.mark.parametrize("paired", [0, 1])
def test_tail_second_pass(paired):
    torch = pytest.importorskip("torch")
    p = H.stats_params(lmax=TAIL_LMAX, read_quality_range="20,")
    p.paired = paired
    batches = [_tail_mates(s, paired) for s in (0, 1)]
    wants = [O.run(p, *mates) for mates in batches]
    # the longest merged read: what lmax_ext must be, and where the oracle counts every position
    L = max(int(np.diff(r.idx)[w[0] == 1].max()) for mates, w in zip(batches, wants) for r in mates)
    assert L > 300
    px = H.Params.from_buffer_copy(p)
    px.lmax = L
    wants_x = [O.run(px, *mates) for mates in batches]
    with H.Engine(p) as e:
        e.set_max_workgroups(2)
        st = e.kernel_chain.split(" -> ")
        assert len(st) == 2 and "hex" in st[0] and f"engine_kernel<{1 + paired}, 5, true> (follow-up)" in st[1], \
            e.kernel_chain
        nw, ur = e.stage_waves(4)
        assert (nw, ur) == (8, 64)
        for mates, w in zip(batches, wants):   # the unreserved tail ends at lmax: reads past it take the second pass
            _conditions([(4, nw, TAIL_LMAX)], 64, mates, w, False)
        keep, outs = [], []
        for mates in batches:   # two batches before one sync
            dev = [_to_device(torch, r) for r in mates]
            dm = torch.zeros(mates[0].n, dtype=torch.uint8, device="cuda")
            keep.append(dev)
            outs.append(dm)
            torch.cuda.synchronize()
            e.run_device(dev[0][1], dev[1][1] if paired else None, dm.data_ptr(), None)
        e.sync()
        dense = e.counters()
        ext, L_g = e.counters_ext()
    for k, (dm, w) in enumerate(zip(outs, wants)):
        np.testing.assert_array_equal(dm.cpu().numpy(), w[0], err_msg=f"batch {k}")
    np.testing.assert_array_equal(dense, _add(wants))
    assert L_g == L
    c_x = _add(wants_x)
    assert all(int(c_x[m * H.counters_len(L) + H.S_LONG_READS]) == 0 for m in range(1 + paired))
    bad = np.nonzero(ext != c_x)[0]
    assert bad.size == 0, f"{bad.size} full-length counters differ, first at {bad[:8]}: {ext[bad[:8]]} vs {c_x[bad[:8]]}"


# ---------------------------------------------------------------------------
# the natural grid
# ---------------------------------------------------------------------------

# (id, route, first geometry, mates, kind)
NATURAL = [("c2-auto_fixed", "auto_fixed", "hex", 1, "filter"), ("pe-edit-hex", "hex", "hex", 2, "edit"),
           ("se-edit-tri", "tri", "tri", 1, "edit")]


@pytest.mark.parametrize("case", NATURAL, ids=[c[0] for c in NATURAL])
def test_natural_grid(case):
    """No cap: 3 * (the widest stage's waves) + 5 units, the last one short."""
    _, route, geo, nm, kind = case
    lmax, B = 1024, BLOCK[geo]
    p = _params(kind, lmax, nm - 1)
    with H.Engine(p, route=route) as e:
        _expect_chain(e, geo, nm, kind, "none", True)
        w1, rules = _stage_rules(e, geo, p, True)
        n_units = 3 * max([w1] + [w for _, w, _ in rules]) + 5
        n = _batch_size(B, n_units - 1)
        shift = _shift_for(B, n)
        mates = _mates(B, n, shift, nm, dense=True)
        want = _oracle(kind, lmax, nm - 1, "none", True, B, n, shift, dense=True)
        _conditions(rules, B, mates, want, kind == "edit")
        mask, trim = _run(e, mates, "host")
        _same(mask, trim, e.counters(), want, kind == "edit", case[0])
