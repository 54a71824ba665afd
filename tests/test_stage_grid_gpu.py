"""The persistent grid of every stage of the kernel chain.

A stage launches as many workgroups as stay resident: CUs x workgroups per CU,
the latter from the kernel's registers and the LDS bytes of its layout
(hpgq_engine_lds.h).  A byte count that drifts from the layout's slack-carrying
value, or a chain wired to the wrong stage, shows here as another grid before
it shows anywhere as a slower run.  Contexts are opened and asked
(hpgq_debug_stage_waves); nothing is launched.

TABLE: workgroups per CU and unit size of stages 1..4 (first stage, wide
follow-up, catch-all follow-up, the long-read tail's second pass), measured
on an MI355X (256 CUs) at commit 547bfb6, the last one whose host computed
the LDS bytes by hand.  It agrees with the waves in that commit's message:
single-end hex 4096/4096/3072, tri filter 5120/4096/3072, tri edit
4096/4096/3072, wide 4096 (edit 3072)/-/3072; paired hex 3072/3072/2048, tri
filter 4096, tri edit 2048, wide 3072 (edit 2048) -- waves = 4 x 256 x
workgroups per CU.
"""
import pytest

import hpgfastq as H

pytestmark = pytest.mark.gpu

C2 = dict(read_quality_range="20,", read_length_range="50,")
TRIMS = dict(left_length=10, left_quality_range="20,", right_length=30, right_quality_range="20,")

# (mates, kind, first geometry) -> {lmax: [(workgroups per CU, reads per unit) or None, stages 1..4]}
TABLE = {
    (1, "filter", "hex"): {150: [(4, 48), None, (3, 48), (3, 64)], 1024: [(4, 48), (4, 48), (3, 48), (3, 64)]},
    (1, "filter", "tri"): {150: [(5, 54), None, (3, 54), (3, 64)], 1024: [(5, 54), (4, 54), (3, 54), (3, 64)]},
    (1, "filter", "wide"): {150: [(4, 60), None, (3, 60), (3, 64)], 1024: [(4, 60), None, (3, 60), (3, 64)]},
    (1, "edit", "hex"): {150: [(4, 48), None, (3, 48), (3, 64)], 1024: [(4, 48), (4, 48), (3, 48), (3, 64)]},
    (1, "edit", "tri"): {150: [(4, 54), None, (3, 54), (3, 64)], 1024: [(4, 54), (4, 54), (3, 54), (3, 64)]},
    (1, "edit", "wide"): {150: [(3, 60), None, (3, 60), (3, 64)], 1024: [(3, 60), None, (3, 60), (3, 64)]},
    (2, "filter", "hex"): {150: [(3, 48), None, (2, 48), (2, 64)], 1024: [(3, 48), (3, 48), (2, 48), (2, 64)]},
    (2, "filter", "tri"): {150: [(4, 54), None, (2, 54), (2, 64)], 1024: [(4, 54), (3, 54), (2, 54), (2, 64)]},
    (2, "filter", "wide"): {150: [(3, 60), None, (2, 60), (2, 64)], 1024: [(3, 60), None, (2, 60), (2, 64)]},
    (2, "edit", "hex"): {150: [(3, 48), None, (2, 48), (2, 64)], 1024: [(3, 48), (3, 48), (2, 48), (2, 64)]},
    (2, "edit", "tri"): {150: [(2, 54), None, (2, 54), (2, 64)], 1024: [(2, 54), (3, 54), (2, 54), (2, 64)]},
    (2, "edit", "wide"): {150: [(2, 60), None, (2, 60), (2, 64)], 1024: [(2, 60), None, (2, 60), (2, 64)]},
}
# the catch-all alone (route "single"): stage 1 and the second pass only
ALONE = {(1, 150): [(5, 64), None, None, (3, 64)], (1, 1024): [(3, 64), None, None, (3, 64)],
         (2, 150): [(4, 64), None, None, (2, 64)], (2, 1024): [(2, 64), None, None, (2, 64)]}


def _params(kind, lmax, nm):
    p = H.stats_params(lmax=lmax, **C2) if kind == "filter" else H.edit_params(lmax=lmax, stats=True, **TRIMS, **C2)
    p.paired = nm - 1
    return p


def _stages(e, cus, chain=0):
    out = []
    for stage in (1, 2, 3, 4):
        try:
            waves, unit = e.stage_waves(stage, chain)
        except H.HpgqError as err:
            assert err.code == -1
            out.append(None)
            continue
        assert waves % (4 * cus) == 0, (stage, waves, cus)
        out.append((waves // (4 * cus), unit))
    return out


@pytest.fixture(scope="module")
def cus():
    torch = pytest.importorskip("torch")
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", sorted(TABLE), ids=lambda c: f"{'pe' if c[0] == 2 else 'se'}-{c[1]}-{c[2]}")
def test_stage_grids(cus, case):
    nm, kind, route = case
    for lmax, want in TABLE[case].items():
        with H.Engine(_params(kind, lmax, nm), route=route) as e:
            assert _stages(e, cus) == want, (case, lmax, e.kernel_chain)
            assert len(e.kernel_chain.split(" -> ")) == sum(s is not None for s in want[:3]), e.kernel_chain


def test_adaptive_and_catch_all_alone(cus):
    """The default route at lmax 1024 keeps a second, wide-first chain; the
    catch-all alone has a first stage and the second pass only."""
    for nm in (1, 2):
        for kind in ("filter", "edit"):
            with H.Engine(_params(kind, 1024, nm)) as e:
                assert _stages(e, cus, 0) == TABLE[(nm, kind, "hex")][1024]
                assert _stages(e, cus, 1) == TABLE[(nm, kind, "wide")][1024]
                assert " | adaptive: " in e.kernel_chain
        for lmax in (150, 1024):
            with H.Engine(_params("filter", lmax, nm), route="single") as e:
                assert _stages(e, cus) == ALONE[(nm, lmax)], (nm, lmax)
                assert " -> " not in e.kernel_chain
