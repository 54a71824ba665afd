"""`edit --correct-overlap` and `--insert-size` without a GPU:
hpgq_ovl_correct against tests/ovl_fix_ref.py on the edge list of §2.13 and on
the threshold, byte and position cases the GPU test shares, hand-checked pairs,
the argument checks, the flag rules through the CLI (all end before any device
call), and the reference's two renderers on histograms written by hand."""
import ctypes as C

import numpy as np
import pytest

import hpgfastq as H
import ovl_ref as R
import ovl_fix_ref as X
from cli_lib import run_cli, print_params

THRESHOLDS = [(33, 30, 14), (33, 1, 0), (33, 93, 92), (64, 30, 14), (64, 1, 0), (64, 93, 92)]


def _same(pair, F, phred=33, high=30, low=14):
    want = X.correct(*pair, F, phred, high, low)
    got = H.ovl_correct(*pair, F, phred, high, low)
    assert got == want, (pair, F, phred, high, low)
    return want[4]


def test_edge_list_against_reference():
    """§2.13's edge pairs (skipped ones and pairs without an overlap among them)
    under qualities that win at some positions and lose at others."""
    pairs = R.edge_pairs(30, 5)
    done, touched, quiet = [0, 0], 0, 0
    for i, (s1, s2) in enumerate(pairs):
        q1 = bytes(33 + (40, 2, 20, 35, 14, 30)[(k + i) % 3 + 3 * (k % 2)] for k in range(len(s1)))
        q2 = bytes(33 + (3, 41, 0, 31)[(k + k // 7) % 4] for k in range(len(s2)))
        F = R.find(s1, s2, 30, 5)
        d = _same((s1, q1, s2, q2), F)
        if F <= 0:
            assert d == [0, 0]
            quiet += 1
        touched += sum(d) > 0
        done = [x + y for x, y in zip(done, d)]
    # not vacuous, by the reference: at least 5 bases corrected in each mate, and many pairs that stay as they are
    assert min(done) >= 5 and touched >= 5 and quiet > 30, (done, touched, quiet)


@pytest.mark.parametrize("phred,high,low", THRESHOLDS)
def test_thresholds(phred, high, low):
    pairs = X.threshold_pairs(phred, high, low)
    fired = [sum(_same(p, 70, phred, high, low)) for p in pairs]
    assert set(fired) == {0, 1}
    # by hand, per direction: of high - 1 / high against low / low + 1 only (high, low) fires; where high = low + 1 the
    # pair (high - 1, low + 1) is (low, high), the other mate's win
    per_way = 1 + (high == low + 1) + 4
    assert sum(fired) == 2 * per_way


def test_bytes_positions_and_several():
    done = [0, 0]
    for p in X.byte_pairs():
        d = _same(p, 70)
        done = [x + y for x, y in zip(done, d)]
    # per direction 4 winners x 256 values, all but the one that matches: the loser's byte plays no part
    assert done == [4 * 255, 4 * 255]
    for p in X.position_pairs():
        F = R.find(p[0], p[2], 30, 5)
        assert sum(_same(p, F)) == 1
    for mo, M in ((30, 5), (64, 40)):
        pairs = X.several_pairs(mo, M)
        got = [_same(p, R.find(p[0], p[2], mo, M)) for p in pairs]
        assert got[0] == [0, M] and got[1] == [M, 0] and got[2] == [M // 2, M - M // 2] and 0 < sum(got[3]) < M
    for p in X.untouched_pairs() + X.random_case(200):
        _same(p, R.find(p[0], p[2], 30, 5))


def test_by_hand():
    """tests/ovl_fix_ref.py itself, and the library, on pairs worked out by hand."""
    frag = b"ACGGTCATTGCAACGTTAGCATCGGATCAATGCCTA"                   # 36 bases
    rc = R.revcomp(frag)
    hi, lo, mid = bytes([33 + 30]), bytes([33 + 14]), bytes([33 + 20])
    for f in (X.correct, H.ovl_correct):
        # F = 36, mates of 30: k in [6, 30) faces j = 35 - k; s1[10] wrong at low quality, s2[25] right at high quality
        s1 = R.flip(frag[:30], 10)
        q1, q2 = mid * 10 + lo + mid * 19, mid * 25 + hi + mid * 4
        assert f(s1, q1, rc[:30], q2, 36) == (frag[:30], mid * 10 + hi + mid * 19, rc[:30], q2, [1, 0])
        # the other way round: mate 2 takes comp(s1[10]) and its quality byte
        want2 = rc[:25] + bytes([R.COMP[s1[10]]]) + rc[26:30]
        assert f(s1, mid * 10 + hi + mid * 19, rc[:30], mid * 25 + lo + mid * 4, 36) == \
            (s1, mid * 10 + hi + mid * 19, want2, mid * 25 + hi + mid * 4, [0, 1])
        # one short of either threshold, both high, both low: nothing
        for a, b in ((bytes([33 + 29]), lo), (hi, bytes([33 + 15])), (hi, hi), (lo, lo), (mid, mid)):
            for x, y in ((a, b), (b, a)):
                pair = (s1, mid * 10 + x + mid * 19, rc[:30], mid * 25 + y + mid * 4)
                assert f(*pair, 36) == (*pair, [0, 0])
        # a disagreement outside [lo, hi) -- s1[3] faces nothing -- and F <= 0: nothing
        pair = (R.flip(frag[:30], 3), lo * 30, rc[:30], hi * 30)
        assert f(*pair, 36) == (*pair, [0, 0])
        for F in (0, -1):
            pair = (s1, lo * 30, rc[:30], hi * 30)
            assert f(*pair, F) == (*pair, [0, 0])
        # N at high quality wins nothing, N at low quality loses; a quality byte below phred counts as low
        sn = frag[:10] + b"N" + frag[11:30]
        pair = (sn, mid * 10 + hi + mid * 19, rc[:30], mid * 25 + lo + mid * 4)
        assert f(*pair, 36) == (*pair, [0, 0])
        assert f(sn, mid * 10 + b"\x05" + mid * 19, rc[:30], q2, 36) == (frag[:30], mid * 10 + hi + mid * 19, rc[:30], q2, [1, 0])
        # both rules could fire at no position: rule 1 comes first where q1 >= high and q2 <= low, else rule 2
        assert f(s1, hi * 30, rc[:30], lo * 30, 36)[4] == [0, 1] and f(s1, lo * 30, rc[:30], hi * 30, 36)[4] == [1, 0]


def test_invalid_arguments():
    """-2 from the host function and HPGQ_E_INVALID from hpgq_ovl_set_correct
    before any device call, for every rule of §2.14."""
    s, q = b"ACGTACGTACGTACGT", b"I" * 16
    bad = [(33, 14, 14), (33, 10, 14), (33, 94, 14), (33, 30, -1), (33, -3, -5), (-1, 30, 14), (256, 30, 14), (33, 0, 0)]

    def call(s1, q1, n1, s2, q2, n2, F, phred=33, high=30, low=14):
        return H.lib.hpgq_ovl_correct(s1, q1, n1, s2, q2, n2, F, phred, high, low, None)

    buf = [C.create_string_buffer(x, 16) for x in (s, q, s, q)]
    for phred, high, low in bad:
        assert call(buf[0], buf[1], 16, buf[2], buf[3], 16, 16, phred, high, low) == -2, (phred, high, low)
        assert call(buf[0], buf[1], 16, buf[2], buf[3], 16, 0, phred, high, low) == -2, (phred, high, low)
        with pytest.raises(H.HpgqError):
            H.ovl_correct(s, q, s, q, 16, phred, high, low)
    for phred, high, low in ((33, 30, 14), (0, 1, 0), (255, 93, 92), (64, 93, 0)):
        assert call(buf[0], buf[1], 16, buf[2], buf[3], 16, 16, phred, high, low) >= 0
    # an F the rule cannot return for these lengths: fewer than 8 facing bytes, a mate longer than 512
    for F in (1, 7, 25, 26, 32, 1000):
        assert call(buf[0], buf[1], 16, buf[2], buf[3], 16, F) == -2, F
    for F in (8, 16, 24, 0, -1, -7):
        assert call(buf[0], buf[1], 16, buf[2], buf[3], 16, F) == 0, F
    long = C.create_string_buffer(b"A" * 513, 513)
    assert call(long, long, 513, buf[2], buf[3], 16, 16) == -2 and call(long, long, 513, buf[2], buf[3], 16, -1) == 0
    assert call(None, buf[1], 16, buf[2], buf[3], 16, 16) == -2 and call(buf[0], buf[1], 16, buf[2], None, 16, 16) == -2
    assert call(None, None, 0, None, None, 0, 0) == 0
    with pytest.raises(ValueError):
        H.ovl_correct(s, q[:5], s, q, 16)
    # the handle's entry points on a NULL handle
    hist = np.zeros(H.OVL_INSERT_BINS, np.uint64)
    info = H.OvlCorrectInfo()
    assert H.lib.hpgq_ovl_set_correct(None, 1, 33, 30, 14) == -1 and H.lib.hpgq_ovl_count_inserts(None, 1) == -1
    assert H.lib.hpgq_ovl_read_correct(None, C.byref(info)) == -1 and H.lib.hpgq_ovl_read_inserts(None, hist.ctypes.data) == -1
    # a handle, where there is a device: the rules before any device call, and the switches' state
    h = C.c_void_p()
    if H.lib.hpgq_ovl_open(C.byref(h), 0, 30, 5, None) == 0:
        for phred, high, low in bad:
            assert H.lib.hpgq_ovl_set_correct(h, 1, phred, high, low) == -1
        assert H.lib.hpgq_ovl_read_correct(h, None) == -1 and H.lib.hpgq_ovl_read_inserts(h, None) == -1
        H.lib.hpgq_ovl_close(h)


# -- the flag rules, through the CLI ----------------------------------------------------------------

EDIT = ["--left-length", "5", "--left-quality-range", "20,"]
NEW_FLAGS = (["--correct-overlap"], ["--correct-overlap-high", "20"], ["--correct-overlap-low=3"], ["--insert-size"])
NEED = "\nError: --correct-overlap, --correct-overlap-high, --correct-overlap-low and --insert-size need --clip-overlap\n"


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]), ("stats", [])])
def test_flags_rejected_on_stats_and_filter(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r/1\nACGT\n+\nIIII\n@r/2\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in NEW_FLAGS:
        r = run_cli([cmd, "-f", fq, "--interleaved", "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        name = "insert-size" if extra[0] == "--insert-size" else "correct-overlap"
        assert r.stderr == f"hpg-fastq: --{name} is an option of the edit command, not of {cmd}\n"
        assert r.stdout == "" and list(out.iterdir()) == []


@pytest.mark.parametrize("extra", NEW_FLAGS)
def test_flags_need_clip_overlap(tmp_path, extra):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, *extra], check=False)
    assert r.returncode == 1 and NEED in r.stdout and "Usage:" in r.stdout


@pytest.mark.parametrize("extra", NEW_FLAGS[1:3])
def test_value_flags_need_the_flag(tmp_path, extra):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, "--clip-overlap", *extra],
                check=False)
    assert r.returncode == 1
    assert "\nError: --correct-overlap-high and --correct-overlap-low need --correct-overlap\n" in r.stdout


@pytest.mark.parametrize("flag,value", [("high", "0"), ("high", "94"), ("high", "x"), ("high", ""), ("high", "-1"),
                                        ("low", "-1"), ("low", "93"), ("low", "3x")])
def test_value_ranges(tmp_path, flag, value):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, "--clip-overlap",
                 "--correct-overlap", f"--correct-overlap-{flag}={value}"], check=False)
    rng = "1..93" if flag == "high" else "0..92"
    assert r.returncode != 0 and f"Error: --correct-overlap-{flag} must be an integer in {rng}" in r.stdout


@pytest.mark.parametrize("high,low", [(30, 30), (14, None), (None, 30), (1, 0 + 1), (20, 92)])
def test_low_below_high(tmp_path, high, low):
    flags = ["--clip-overlap", "--correct-overlap"]
    flags += ["--correct-overlap-high", str(high)] if high is not None else []
    flags += ["--correct-overlap-low", str(low)] if low is not None else []
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, *flags], check=False)
    assert r.returncode == 1 and "Usage:" in r.stdout
    assert f"\nError: --correct-overlap-low ({14 if low is None else low}) must be below --correct-overlap-high " \
           f"({30 if high is None else high})\n" in r.stdout


def test_flags_parse_on_edit_and_change_no_parameter(tmp_path):
    flags = ["-f", str(tmp_path / "in.fq"), "--interleaved", *EDIT, "--read-quality-range", "20,", "--lmax", "150"]
    plain = print_params("edit", *flags)
    assert plain["paired"] == 1
    for extra in (["--correct-overlap"], ["--insert-size"], ["--correct-overlap", "--insert-size"],
                  ["--correct-overlap", "--correct-overlap-high", "1", "--correct-overlap-low", "0"],
                  ["--correct-overlap", "--correct-overlap-high=93", "--correct-overlap-low=92"],
                  ["--correct-overlap", "--correct-overlap-low=29"], ["--correct-overlap", "--correct-overlap-high=15"]):
        assert print_params("edit", *flags, "--clip-overlap", *extra) == plain
    assert print_params("edit", *flags, "--quality-encoding", "phred64", "--clip-overlap", "--correct-overlap")["phred"] == 64


def test_help_shows_the_flags():
    r = run_cli(["edit", "--help"], check=False)
    for flag in ("--correct-overlap ", "--correct-overlap-high=<int>", "--correct-overlap-low=<int>", "--insert-size "):
        assert flag in r.stdout, flag
    for cmd in ("stats", "filter"):
        out = run_cli([cmd, "--help"], check=False).stdout
        assert "--correct-overlap" not in out and "--insert-size" not in out


# -- the reference's renderers, on histograms written by hand ---------------------------------------

HEAD1 = b"# Pairs\tSkipped\tWithout overlap\tWith overlap\tMin\tMedian\tMax\tMean\n"
HEAD2 = b"# Insert size\tPairs\t% of overlapping\n"


def _hist(cells):
    h = np.zeros(X.BINS, np.uint64)
    for f, c in cells.items():
        h[f] = c
    return h


def test_render_inserts_by_hand():
    info = dict(pairs=7, skipped=2, overlapping=0)
    assert X.render_inserts(info, _hist({})) == HEAD1 + b"7\t2\t0\t0\t0\t0\t0\t0.00\n" + HEAD2
    assert X.render_inserts(info, _hist({0: 5})) == HEAD1 + b"7\t2\t5\t0\t0\t0\t0\t0.00\n" + HEAD2
    # one bin
    assert X.render_inserts(dict(pairs=4, skipped=0), _hist({0: 1, 100: 3})) == \
        HEAD1 + b"4\t0\t1\t3\t100\t100\t100\t100.00\n" + HEAD2 + b"100\t3\t100.00\n"
    # bins 8 and 1016: every row between them, zeros included; 2 * 1 >= 3 is false at 8, so the median is 1016
    got = X.render_inserts(dict(pairs=3, skipped=0), _hist({8: 1, 1016: 2}))
    rows = got.split(b"\n")
    assert got.startswith(HEAD1 + b"3\t0\t0\t3\t8\t1016\t1016\t680.00\n" + HEAD2 + b"8\t1\t33.33\n9\t0\t0.00\n")
    assert got.endswith(b"1015\t0\t0.00\n1016\t2\t66.67\n") and len(rows) == 3 + 1009 + 1
    # an even total whose median falls between two bins: the lower one (2 * 2 >= 4 at 50)
    got = X.render_inserts(dict(pairs=10, skipped=1), _hist({0: 5, 50: 2, 53: 2}))
    assert got == HEAD1 + b"10\t1\t5\t4\t50\t50\t53\t51.50\n" + HEAD2 + b"50\t2\t50.00\n51\t0\t0.00\n52\t0\t0.00\n53\t2\t50.00\n"
    # an odd total
    got = X.render_inserts(dict(pairs=5, skipped=0), _hist({40: 1, 41: 1, 45: 3}))
    assert got.startswith(HEAD1 + b"5\t0\t0\t5\t40\t45\t45\t43.20\n")
    np.testing.assert_array_equal(X.hist_of([5, 0, -1, 5, 1016, 0, 0]), _hist({0: 3, 5: 2, 1016: 1}))


def test_render_correct_by_hand():
    head = b"# Pairs\tOverlapping\tCorrected pairs\t% corrected\tBases corrected 1\tBases corrected 2\n"
    info = dict(pairs=3, overlapping=2)
    assert X.render_correct(info, dict(corrected_pairs=1, corrected_bases=[2, 5])) == head + b"3\t2\t1\t33.33\t2\t5\n"
    assert X.render_correct(dict(pairs=0, overlapping=0), dict(corrected_pairs=0, corrected_bases=[0, 0])) == \
        head + b"0\t0\t0\t0.00\t0\t0\n"
