"""The CPU oracle (oracle/hpgq_oracle.c) against the plain exact reference
(tests/exact_ref.py) on every input of tests/test_capacity_gpu.py, bit for
bit, without a GPU: the counters of O.run(...) equal exact_ref.counters(...)
over the expected mask and the oracle's trim words, and where the filter is
C2's the oracle's mask equals exact_ref.c2_mask.  So the inputs, the oracle
and the reference agree before any kernel is involved, and the oracle's
rounding and floor, written with the kernels' integer expressions, are pinned
by a reference written from the definitions.

exact_ref's own checks against fractions.Fraction (every n <= 40 and S) and its
hand-written example are collected here too.
"""
import numpy as np
import pytest

import capacity_lib as CL
import exact_ref as X
import hpgfastq as H
import oracle_lib as O
from exact_ref import test_counters_by_hand, test_floor_fx16, test_round_half_away_is_round  # noqa: F401


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:8]}: oracle {got[bad[:8]]} exact {want[bad[:8]]}"


CAPACITY = CL.capacity_cases()


@pytest.mark.parametrize("case", CAPACITY, ids=[c[0] for c in CAPACITY])
def test_oracle_equals_exact_at_capacity(case):
    name, build, args = case
    p, mates, source = build(*args)
    mask, _, ctr, (m_o, c_o) = CL.expected(p, mates, source)
    _same(m_o, mask, f"{name} mask")
    _same(c_o, ctr, f"{name} counters")
    if name.startswith("half"):   # (the GPU test asserts the same before it runs)
        CL.assert_pass_and_fail_in_every_unit(mask, CL.GEO[args[1]]["B"])
        peak = CL.half_case_peak(args[1], mates, mask)
        print(f"{name}: a byte counter reaches at least {peak}")
        assert args[2] != "sparse" or peak >= CL.NEAR_FULL
    elif name in ("follow-half", "follow-sparse"):
        CL.assert_pass_and_fail_in_every_unit(mask, CL.GEO[CL.FOLLOW_FIRST]["B"])
        peak = CL.follow_case_peak(mates, mask)
        print(f"{name}: a byte counter reaches at least {peak}")
        assert name != "follow-sparse" or peak >= CL.NEAR_FULL
    elif name.endswith("half"):
        assert 0 < int(mask.sum()) < mask.size
    if name.endswith("-80"):   # every quality byte 0x80: the summary's mean quality is exactly -128
        assert H.engine.summary(c_o, p.lmax)["mean_quality_raw"] == -128.0


EDGES = CL.edge_cases()


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_oracle_equals_exact_at_the_edges(case):
    name, lengths, lmax, full = case
    p, mates, source = CL.edge_case(lengths, lmax, full)
    CL.assert_edges_present(mates[0], lengths, full)
    mask, _, ctr, (m_o, c_o) = CL.expected(p, mates, source)
    _same(m_o, mask, f"{name} mask")
    _same(c_o, ctr, f"{name} counters")
    longest = max(lengths)
    if longest > lmax:   # long_merge: the set an lmax of the longest read holds
        px = H.Params.from_buffer_copy(p)
        px.lmax = longest
        _, _, c_x = O.run(px, *mates)
        _same(c_x, X.counters(mates[0], longest), f"{name} counters at lmax_ext")
        assert int(c_x[X.S_LONG_READS]) == 0 and int(c_o[X.S_LONG_READS]) == mates[0].n


def test_c2_mask_by_hand():
    """Lengths 0, 2, 3 and 4 around min_len 2 and max_len 3; sums on and off both bounds."""
    q = lambda *v: [33 + x for x in v]   # noqa: E731
    reads = O.Reads.from_pairs([(b"", b""), (b"AC", bytes(q(20, 20))), (b"AC", bytes(q(20, 19))),
                                (b"ACG", bytes(q(30, 30, 30))), (b"ACG", bytes(q(30, 30, 31))),
                                (b"ACGT", bytes(q(25, 25, 25, 25))), (b"AC", bytes([0x80, 0xFF]))])
    assert X.c2_mask(reads, 33, 2, 3, 20, 30).tolist() == [0, 1, 0, 1, 0, 0, 0]
    assert X.c2_mask(reads, 33, 0, 100000, -200, 100000).tolist() == [1] * 7
