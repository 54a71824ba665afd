"""The engine kernels at counter capacity and at every rounding edge, bit for
bit against the plain exact reference (tests/exact_ref.py; inputs from
tests/capacity_lib.py; tests/test_exact_ref_cpu.py shows on the CPU that the
oracle agrees with the reference on the same inputs).

Expected values: the mask is exact_ref.c2_mask where the filter is C2's
(length and read quality ranges), every read where there is no filter, the
oracle's otherwise; the trim words are the oracle's; the counters are
exact_ref.counters over them.  No tolerance anywhere.

(a) Counters at capacity through several flushes.  The grid is capped at one
workgroup (4 waves) and every wave gets at least 3 * ceil(255 / s) + 2 units
(s: steps per unit), so it flushes its packed counters inside its loop three
times and holds them full in between: every base of a batch is one letter
(A, C, G, T, N, '.') and every quality byte one of 0x7F, 0x80, 0xFF (biased
255, 0, 127).  Batches: tri 10,152 reads of 160, hex 18,816 of 156, wide
12,720 of 252.
  * uniform: full-length reads; ragged: lengths cycling 1 .. kPos;
  * half-failing: 0x7F and 0x80 reads in a pattern not aligned to the unit,
    read_quality_range "0,", through each way a failed read leaves the
    counters: the pass-first kernels (pf) and their noor variant (reads of N
    alone fail max_N too), a left / right window filter (take-back), edit
    with a filter (hex: the trims at the step; passing reads are trimmed too),
    paired C2 (undo per step; either mate fails) and paired with max_N
    (take-back of both mates).  Two densities: "third", about one failing read
    in three (a byte counter then holds some 170 of 255), and "sparse", one
    failing read or pair a unit at a position that moves through the
    segments, which keeps the counters a read is kept out of or taken back
    from within 16 of full (capacity_lib.peak_count, asserted);
  * the wide follow-up stage (uniform, third, sparse): route hex, lmax 252,
    12,480 reads of 252 bases, all deferred.  It walks hex's units of 48 reads: 12 steps of 4 reads, and
    tri_body (FOLLOW) flushes once since_flush > 255 - 60 / 4 = 240, i.e.
    every 21 units; 3 * 21 + 2 = 65 units a wave;
  * the catch-all alone (route single, lmax 252 and 1024): 320 reads a wave,
    at least 200 of them passing: its 6-bit fields flush every 63.

(b) Every quotient edge of every length.  Natural grid, no filter.  Per
length n one read per biased sum in capacity_lib.edge_sums(n) (ties, the zero
mean, the largest remainders, both ends), every sum 0 .. 255 n for n in {1,
2, 3, kPos - 1, kPos}, and one read per G+C count: tri 102 K reads (15 MB),
hex 99 K (14 MB), wide 172 K (39 MB).  The same edge set runs through the wide follow-up
(lengths 157 .. 252), the catch-all (253 .. 1024; as the chain's last stage and
alone) and long_merge (lmax 150, lengths 151 .. 4097; counters_ext against the
reference at lmax_ext; host path, device path with and without
reserve_length).

Before a GPU result is looked at every case asserts the kernel variant from
the chain's names, (a) the units or passing reads per wave, (b) that every
edge class is present in its input.

Measured on an MI355X: every case under 0.2 s but the three first-stage edge
batches (wide, the slowest: 1.8 s, nearly all of it building the 39 MB input
and its reference on the host; the engine call is 10 ms).  A build with the
in-loop flush 16 steps late, the catch-all's flush at 66 and the rounding
ties moved fails every case here except those whose counters cannot overflow
(batches of N or '.' whose quality byte is not the largest, and the "third"
density).
"""
import time

import numpy as np
import pytest

import capacity_lib as CL
import exact_ref as X
import hpgfastq as H

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# running and comparing
# ---------------------------------------------------------------------------

def _to_device(torch, r):
    pad = np.zeros(H.DEVICE_SLACK, np.uint8)
    t = [torch.from_numpy(np.concatenate([r.seq, pad])).cuda(), torch.from_numpy(np.concatenate([r.qual, pad])).cuda(),
         torch.from_numpy(r.idx.copy()).cuda()]
    return t, H.engine.device_batch(r.n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def _run(e, mates, path="host"):
    """One batch -> (mask, trim, seconds)."""
    t0 = time.perf_counter()
    if path == "host":
        args = [a for r in mates for a in (r.seq, r.qual, r.idx)]
        mask, trim = e.process(*args)
        return mask, trim, time.perf_counter() - t0
    import torch   # (a missing torch fails the case: nothing here skips)
    n = mates[0].n
    dev = [_to_device(torch, r) for r in mates]
    dm = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dtr = torch.zeros(n * len(mates), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run_device(dev[0][1], dev[1][1] if len(mates) > 1 else None, dm.data_ptr(), dtr.data_ptr())
    e.sync()   # (the batch stays valid up to here: the long-read tail's second pass reads it)
    seconds = time.perf_counter() - t0
    return dm.cpu().numpy(), dtr.cpu().numpy().view(np.uint32), seconds


def _diff(got, want, what):
    bad = np.nonzero(got != want)[0]
    return [f"{bad.size} {what} differ, first at {bad[:8]}: gpu {got[bad[:8]]} exact {want[bad[:8]]}"] if bad.size else []


def _same(name, p, mates, want, mask, trim, ctr, seconds):
    m_x, t_x, c_x = want[:3]
    print(f"{name}: {mates[0].n} reads x {len(mates)}, {sum(len(r.seq) for r in mates)} bases, engine call {seconds:.3f} s")
    d = _diff(mask, m_x, "masks")
    if p.edit_on:
        d += _diff(trim, t_x, "trim words")
    d += _diff(ctr, c_x, "counters")
    assert not d, f"{name}: " + "; ".join(d)


def _cap_one_workgroup(e, stage, unit_reads):
    e.set_max_workgroups(1)
    assert e.stage_waves(stage) == (CL.WAVES, unit_reads), e.stage_waves(stage)
    return CL.WAVES


def _stages(e):
    return e.kernel_chain.split(" | adaptive: ")[0].split(" -> ")


# ---------------------------------------------------------------------------
# (a) counters at capacity
# ---------------------------------------------------------------------------

def _first_stage_capacity(name, geo, way, p, mates, source, density=None):
    g = CL.GEO[geo]
    want = CL.expected_of(name, p, mates, source)
    ln = [np.diff(r.idx) for r in mates]
    assert all(int(x.max()) <= g["pos"] for x in ln)           # nothing is deferred
    with H.Engine(p, route=geo) as e:
        CL.expect_variant(way, geo, e.kernel_name)
        nw = _cap_one_workgroup(e, 1, g["B"])
        n_units = -(-mates[0].n // g["B"])
        per_wave = CL.units_of_waves(n_units, nw)
        assert per_wave.min() >= CL.units_per_wave(geo), (per_wave, CL.units_per_wave(geo))
        assert CL.units_per_wave(geo) >= 3 * CL.units_between_flushes(CL.steps_per_unit(geo), geo) + 2
        if way != "plain":   # reads pass and fail in every unit; sparse: from counters within 16 of full
            CL.assert_pass_and_fail_in_every_unit(want[0], g["B"])
            assert density != "sparse" or CL.half_case_peak(geo, mates, want[0]) >= CL.NEAR_FULL
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(name, p, mates, want, mask, trim, ctr, dt)
    return ctr


@pytest.mark.parametrize("qname", list(CL.QBYTES))
@pytest.mark.parametrize("letter", list(CL.LETTERS))
@pytest.mark.parametrize("geo", list(CL.GEO))
def test_uniform_reads_fill_every_counter(geo, letter, qname):
    p, mates, source = CL.uniform_case(geo, letter, qname)
    r = mates[0]
    assert mates[0].n == CL.capacity_batch_size(geo) and (np.diff(r.idx) == CL.GEO[geo]["pos"]).all()
    assert (r.seq == CL.LETTERS[letter]).all() and (r.qual == CL.QBYTES[qname]).all()
    if (letter, qname) == ("G", "7f"):   # both fields of the wave scan's packed word are maximal
        assert ((r.qual ^ 0x80) == 255).all() and (r.seq == ord("G")).all()
    ctr = _first_stage_capacity(f"uniform-{geo}-{letter}-{qname}", geo, "plain", p, mates, source)
    if qname == "80":
        assert H.engine.summary(ctr, p.lmax)["mean_quality_raw"] == -128.0


@pytest.mark.parametrize("letter,qname", CL.RAGGED, ids=[f"{l}-{q}" for l, q in CL.RAGGED])
@pytest.mark.parametrize("geo", list(CL.GEO))
def test_ragged_reads(geo, letter, qname):
    p, mates, source = CL.uniform_case(geo, letter, qname, True)
    ln = np.diff(mates[0].idx)
    assert set(ln.tolist()) == set(range(1, CL.GEO[geo]["pos"] + 1))
    _first_stage_capacity(f"ragged-{geo}-{letter}-{qname}", geo, "plain", p, mates, source)


@pytest.mark.parametrize("density", CL.DENSITIES)
@pytest.mark.parametrize("way", list(CL.WAYS))
@pytest.mark.parametrize("geo", list(CL.GEO))
def test_failed_reads_leave_full_counters(geo, way, density):
    p, mates, source = CL.half_case(way, geo, density)
    assert len(mates) == CL.WAYS[way][0]
    if len(mates) == 2:   # different letters, and either mate may be the failing one
        assert (mates[0].seq == ord("G")).any() and (mates[1].seq == ord("T")).any()
        neg = [(r.qual[r.idx[:-1]] == 0x80) for r in mates]
        assert (neg[0] & ~neg[1]).any() and (~neg[0] & neg[1]).any()
        assert density == "sparse" or (neg[0] & neg[1]).any()
    _first_stage_capacity(f"half-{geo}-{way}-{density}", geo, way, p, mates, source, density)


@pytest.mark.parametrize("kind", CL.FOLLOW_KINDS)
def test_wide_follow_up_at_capacity(kind):
    p, mates, source = CL.follow_case(kind)
    name = f"follow-{kind}"
    first = CL.GEO[CL.FOLLOW_FIRST]
    want = CL.expected_of(name, p, mates, source)
    ln = np.diff(mates[0].idx)
    assert (ln > first["pos"]).all() and (ln <= CL.GEO["wide"]["pos"]).all()   # hex defers all, wide holds all
    with H.Engine(p, route=CL.FOLLOW_FIRST) as e:
        st = _stages(e)
        assert len(st) == 3 and CL.FOLLOW_FIRST in st[0], e.kernel_chain
        assert "engine_tri_kernel<" in st[1] and st[1].endswith("filter, wide, follow>"), e.kernel_chain
        nw = _cap_one_workgroup(e, 2, first["B"])
        n_units = mates[0].n // first["B"]
        need = CL.followup_units_per_wave(CL.FOLLOW_FIRST)
        assert need == 65 and CL.units_of_waves(n_units, nw).min() >= need
        if kind in ("half", "sparse"):
            CL.assert_pass_and_fail_in_every_unit(want[0], first["B"])
            assert kind != "sparse" or CL.follow_case_peak(mates, want[0]) >= CL.NEAR_FULL
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(name, p, mates, want, mask, trim, ctr, dt)


@pytest.mark.parametrize("kind", CL.CATCH_ALL_KINDS)
@pytest.mark.parametrize("lmax", [252, 1024])
def test_catch_all_alone_at_capacity(lmax, kind):
    p, mates, source = CL.catch_all_case(lmax, kind)
    name = f"catchall-{lmax}-{kind}"
    want = CL.expected_of(name, p, mates, source)
    assert (np.diff(mates[0].idx) == lmax).all()
    with H.Engine(p, route="single") as e:
        st = _stages(e)
        assert len(st) == 1 and st[0].startswith(f"hpgq::engine_kernel<1, {1 if lmax == 252 else 5}, "), e.kernel_chain
        nw = _cap_one_workgroup(e, 1, CL.CATCH_ALL_UNIT)
        unit = np.arange(mates[0].n) // CL.CATCH_ALL_UNIT
        passing = np.bincount(unit % nw, weights=want[0], minlength=nw)
        assert passing.min() >= 200 > 3 * CL.FLUSH_EVERY, passing
        if kind == "half":
            assert 0 < int(want[0].sum()) < mates[0].n
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(name, p, mates, want, mask, trim, ctr, dt)
    if kind.endswith("-80"):
        assert H.engine.summary(ctr, lmax)["mean_quality_raw"] == -128.0


# ---------------------------------------------------------------------------
# (b) every quotient edge of every length
# ---------------------------------------------------------------------------

def _edge_inputs(name, lengths, lmax, full=()):
    p, mates, source = CL.edge_case(lengths, lmax, full)
    CL.assert_edges_present(mates[0], lengths, full)
    assert not p.filter_on
    return p, mates, CL.expected_of(name, p, mates, source)


@pytest.mark.parametrize("geo", list(CL.GEO))
def test_edges_first_stage(geo):
    pos = CL.GEO[geo]["pos"]
    name = f"edges-{geo}"
    p, mates, want = _edge_inputs(name, tuple(range(1, pos + 1)), pos, CL.full_lengths(pos))
    with H.Engine(p, route=geo) as e:
        CL.expect_variant("plain", geo, e.kernel_name)
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(name, p, mates, want, mask, trim, ctr, dt)


@pytest.mark.parametrize("route", ["hex", "auto"])
def test_edges_wide_follow_up(route):
    """Route hex at lmax 252 defers every read of 157 .. 252 bases to the wide
    follow-up.  Route auto at lmax 252 plans wide FIRST (plan_chain: an lmax of
    157 .. 252 says the reads are that long), so the same reads meet the wide
    first stage there: asserted as such."""
    name = "edges-follow-wide"
    p, mates, want = _edge_inputs(name, CL.FOLLOW_WIDE_LENGTHS, 252)
    assert int(np.diff(mates[0].idx).min()) > CL.GEO["hex"]["pos"]
    with H.Engine(p, route=route) as e:
        st = _stages(e)
        if route == "hex":
            assert len(st) == 3 and "hex" in st[0] and st[1].endswith("filter, wide, follow>"), e.kernel_chain
        else:
            assert len(st) == 2 and st[0].endswith("filter, wide>") and "follow" not in st[0], e.kernel_chain
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(f"{name}-{route}", p, mates, want, mask, trim, ctr, dt)


@pytest.mark.parametrize("route", ["auto", "single"])
def test_edges_catch_all(route):
    name = "edges-catch-all"
    p, mates, want = _edge_inputs(name, CL.CATCH_ALL_LENGTHS, 1024)
    assert int(np.diff(mates[0].idx).min()) > CL.GEO["wide"]["pos"]     # no segmented kernel holds one
    with H.Engine(p, route=route) as e:
        st = _stages(e)
        if route == "auto":
            assert len(st) == 3 and st[-1] == "hpgq::engine_kernel<1, 5, true> (follow-up)", e.kernel_chain
        else:
            assert len(st) == 1 and st[0].startswith("hpgq::engine_kernel<1, 5, "), e.kernel_chain
        mask, trim, dt = _run(e, mates)
        ctr = e.counters()
    _same(f"{name}-{route}", p, mates, want, mask, trim, ctr, dt)


@pytest.mark.parametrize("path", ["host", "device", "device_reserved"])
def test_edges_long_merge(path):
    """lmax 150: every read is longer, so the catch-all merges it by long_merge
    (positions < 150 on chip, the rest and the length into the long-read
    tail).  The dense counters against the reference at lmax 150, counters_ext
    against the reference at lmax_ext = 4097."""
    name = "edges-long-merge"
    lmax, longest = CL.LONG_MERGE_LMAX, max(CL.LONG_MERGE_LENGTHS)
    p, mates, want = _edge_inputs(name, CL.LONG_MERGE_LENGTHS, lmax)
    assert int(np.diff(mates[0].idx).min()) > lmax
    want_ext = X.counters(mates[0], longest)
    assert int(want[2][X.S_LONG_READS]) == mates[0].n and int(want_ext[X.S_LONG_READS]) == 0
    with H.Engine(p) as e:
        st = _stages(e)
        assert len(st) == 2 and "hex" in st[0] and st[1] == "hpgq::engine_kernel<1, 5, true> (follow-up)", e.kernel_chain
        if path == "device_reserved":
            e.reserve_length(longest)
        mask, trim, dt = _run(e, mates, "host" if path == "host" else "device")
        ctr = e.counters()
        ext, L = e.counters_ext()
    _same(f"{name}-{path}", p, mates, want, mask, trim, ctr, dt)
    assert L == longest
    d = _diff(ext, want_ext, "full-length counters")
    assert not d, f"{name}-{path}: {d[0]}"
