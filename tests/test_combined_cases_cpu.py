"""The case table of the combined tests (tests/combined_lib.py) covers what it is
meant to cover: asserted on the table itself, with the oracle and the references
alone, before any GPU run, so that a table which hides a failure fails here.

The table has 48 library stats cases and 8 library clip cases
(tests/test_combined_gpu.py), 24 CLI `stats` cases and 12 CLI `edit` cases
(tests/test_cli_combined_gpu.py).  For the stats cases of each layer taken
separately: every add-on in a third of the cases; every pair of add-ons together
with a filter and without; every add-on with phred64, with counted reads longer
than the case's lmax and (but for kmers and cg) with paired input; at least half
of the filter cases pass some reads and fail others, between 5 % and 95 % of
them; no drawn add-on's output is trivial.  The edit cases: every clip form,
every input layout, a read clipped to nothing that then fails the length filter,
a clipped read trimmed on both sides, and 0 < clipped < n in every one."""
import itertools

import numpy as np
import pytest

import combined_lib as CL


def _facts(c):
    share = float(np.mean(c.mask == 1))
    return dict(addons=set(c.addons), filter=c.filter, phred=int(c.p.phred), paired=c.nm == 2,
                long=c.longest_counted > c.p.lmax, share=share, trivial=c.nontrivial(), info=CL.summary(c),
                cli=None if c.layer == "lib" else dict(layout=c.layout, lmax=c.cli_lmax, chunk_mb=c.chunk_mb, workers=c.workers,
                                                       own=c.own, text=[2 * int(r.idx[-1]) + 10 * r.n for r in c.mates]))


@pytest.fixture(scope="module")
def lib_stats():
    return [_facts(CL.lib_case(i)) for i in range(CL.N_LIB)]


@pytest.fixture(scope="module")
def cli_stats():
    return [_facts(CL.cli_case(i)) for i in range(CL.N_CLI)]


def _check_stats_layer(cases):
    n = len(cases)
    for a in CL.ADDONS:
        with_a = [c for c in cases if a in c["addons"]]
        assert 3 * len(with_a) >= n, (a, len(with_a), n)
        assert any(c["phred"] == 64 for c in with_a), f"{a} never with phred64"
        assert any(c["long"] for c in with_a), f"{a} never with counted reads longer than lmax"
        if a not in ("kmers", "cg"):
            assert any(c["paired"] for c in with_a), f"{a} never with paired input"
        else:
            assert not any(c["paired"] for c in with_a), f"{a} on pairs: the CLI refuses it"
    for a, b in itertools.combinations(CL.ADDONS, 2):
        for filt in (False, True):
            assert any({a, b} <= c["addons"] and c["filter"] == filt for c in cases), (a, b, "filter" if filt else "no filter")
    assert {len(c["addons"]) for c in cases} >= {2, 3, 4, 5, 6}
    filtered = [c for c in cases if c["filter"]]
    mixed = [c for c in filtered if 0.0 < c["share"] < 1.0]
    assert filtered and 2 * len(mixed) >= len(filtered)
    for c in mixed:
        assert 0.05 <= c["share"] <= 0.95, (c["share"], c["info"])
    for c in cases:
        assert not c["trivial"], (c["trivial"], c["info"])
        assert len(c["addons"]) >= 2, c["info"]


def test_library_stats_cases(lib_stats):
    _check_stats_layer(lib_stats)


def test_cli_stats_cases(cli_stats):
    _check_stats_layer(cli_stats)
    cli = [c["cli"] for c in cli_stats]
    assert {c["layout"] for c in cli} == set(CL.LAYOUTS)
    assert {c["lmax"] for c in cli} == set(CL.CLI_LMAX)
    assert {c["chunk_mb"] for c in cli} == {1, 256} and {c["workers"] for c in cli} == {1, 2}
    with_adapt = [c["cli"]["own"] for c in cli_stats if "adapt" in c["addons"]]
    assert any(with_adapt) and not all(with_adapt)
    # every mate's text (two lines of its bases, and the header and '+' lines) is more than one 1 MB unit
    for c in cli_stats:
        assert min(c["cli"]["text"]) > 1.5 * (1 << 20), c["info"]


def _check_clip_cases(cases):
    assert {c.form for c in cases} == set(CL.FORMS)
    for c in cases:
        for cut in c.cut:
            assert 0 < cut.info["clipped"] < c.mates[0].n, CL.summary(c)
    assert any(c.nothing_then_too_short() for c in cases)
    assert any(c.clipped_then_trimmed_both_sides() for c in cases)
    assert any(c.filter for c in cases) and any(c.p.phred == 64 for c in cases)


def test_cli_edit_cases():
    cases = [CL.cli_edit_case(i) for i in range(CL.N_CLI_EDIT)]
    _check_clip_cases(cases)
    assert {c.layout for c in cases} == set(CL.LAYOUTS)
    assert {(c.layout, c.workers) for c in cases} == set(itertools.product(CL.LAYOUTS, (1, 2)))


def test_library_clip_cases():
    cases = [CL.lib_clip_case(i) for i in range(CL.N_LIB_CLIP)]
    _check_clip_cases(cases)
    assert {c.nm for c in cases} == {1, 2}
    assert {c.cmd for c in cases} == {"edit", "edit_stats"}
    assert {c.route for c in cases} >= {"auto", "tri", "wide", "single"}


def test_the_draw_is_reproducible():
    CL.lib_case.cache_clear()
    a = CL.lib_case(5)
    CL.lib_case.cache_clear()
    b = CL.lib_case(5)
    assert a is not b and a.addons == b.addons and a.attempt == b.attempt
    np.testing.assert_array_equal(a.mates[0].seq, b.mates[0].seq)
    np.testing.assert_array_equal(a.counters, b.counters)
