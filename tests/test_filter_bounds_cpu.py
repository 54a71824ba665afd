"""The segmented kernels' per-read filter bounds and mask-free quality sums
(hpg-fastq_amd/csrc/hpgq_engine_kernel.h: filter_bounds, in_filter_bounds,
quality_q02), checked on the CPU: tests/filter_bounds/ compiles the header's
host side (UBSan) and compares

(a) for every read length n in 0..252 and every segment sum S in 0..255 n the
    packed test lo16 <= S <= hi16 with the filter's predicate
    (!filter) || (min_len <= n <= max_len && lo_r n <= S <= hi_r n) in 64-bit
    arithmetic, over a grid of mean bounds (0, Phred 20 at offset 33, Phred 41
    at offset 64, 255, 256, 300, 65535, 2^31 - 1 and a negative lower bound), the
    length ranges [0, 0], [50, 150], [1, 2^31 - 1] and the empty [200, 100],
    with the filter on and off;
(b) the packed words the kernels' comments name (never-pass, always-pass, a
    plain pair);
(c) the quality sums of 255 steps (the most between two flushes) kept as
    a += word and q13 += b1 | b3 << 16: q02 recovered as a - (q13 << 8) against
    direct per-position sums, for random bytes, all 0xFF, all 0x00, and with
    half of the steps subtracted again (the kernels' take-back paths).
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

NEG = -7
LO_R = [NEG, 0, 128 + 33 + 20, 128 + 64 + 41, 255, 256, 300, 65535, 2 ** 31 - 1]
HI_R = [0, 128 + 33 + 20, 128 + 64 + 41, 255, 256, 300, 65535, 2 ** 31 - 1]
RANGES = [(0, 0), (50, 150), (1, 2 ** 31 - 1), (200, 100)]
COMPARED = sum(255 * n + 1 for n in range(253))   # every (n, S)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("filter_bounds")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "filter_bounds"), f"OUT={out}"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(out / "filter_bounds_main")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert not r.stderr, r.stderr
    rows = [line.split() for line in r.stdout.splitlines()]
    bad = [row for row in rows if row[-1] != "0"]
    assert r.returncode == (1 if bad else 0), (r.returncode, bad[:5])
    return rows


def test_packed_bounds_equal_the_predicate(lines):
    """(a)"""
    got = {tuple(int(x) for x in row[1:6]): (int(row[6]), int(row[7])) for row in lines if row[0] == "B"}
    want = {(f, lo_len, hi_len, lo, hi) for f in (0, 1) for lo_len, hi_len in RANGES for lo in LO_R for hi in HI_R}
    assert set(got) == want
    for key, (compared, bad) in got.items():
        assert compared == COMPARED, key
        assert bad == 0, (key, bad)


def test_named_words(lines):
    """(b)"""
    assert [row for row in lines if row[0] == "W"] == [["W", "0"]]


def test_quality_sums_without_the_mask(lines):
    """(c)"""
    q = {row[1]: (int(row[2]), int(row[3])) for row in lines if row[0] == "Q"}
    names = {"ones", "zeros", "one_step"} | {f"{k}{i}" for k in ("random", "undo") for i in range(64)}
    assert set(q) == names
    for name, (steps, bad) in q.items():
        assert steps == (1 if name == "one_step" else 255), name
        assert bad == 0, (name, bad)
