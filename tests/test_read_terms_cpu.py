"""The unit epilogues' per-read quotients (hpg-fastq_amd/csrc/
hpgq_engine_kernel.h: div_len, meanq_terms_rc, meanq_terms), checked on the
CPU: tests/read_terms/ compiles the header's host side (UBSan) and compares
them with 64-bit / __int128 arithmetic written from the definitions (the
nearest integer to S / n with halves away from zero, floor(65536 S / n),
floor(100 gc / n)):

(a) meanq_terms_rc, with rtab built by the kernel's own expression, for every
    read length n in 1..252 and every biased sum sb in 0..255 n; the G+C bin
    div_len(100 gc, ...) for every gc in 0..n;
(b) meanq_terms (the catch-all's, plain division) for every n in 1..1024 and
    every sb in 0..255 n;
(c) div_len's stated bound: per n the largest numerator the epilogue can form
    (max(255 n, (n - 1) << 16)) satisfies x (n - 1) < 2^32 and divides exactly.
    The first x above it that does not is printed per n: the margin, reported
    and not asserted beyond lying above the numerator;
(d) the pairs of (a) hold every edge class: ties 2 rem = n, sb < 128 n
    (a negative mean), rem = n - 1, and n = 1.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

PAIRS_252 = sum(255 * n + 1 for n in range(1, 253))      # 8,129,142
PAIRS_1024 = sum(255 * n + 1 for n in range(1, 1025))    # 133,825,024
PAIRS_GC = sum(n + 1 for n in range(1, 253))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("read_terms")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "read_terms"), f"OUT={out}"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(out / "read_terms_main")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert not r.stderr, r.stderr     # (no UBSan report)
    rows = [line.split() for line in r.stdout.splitlines()]
    for row in rows:
        if row[0] in "RGME":
            print(" ".join(row))
    bad = [row for row in rows if row[0] in "RGME" and row[-1] != "0"]
    assert r.returncode == (1 if bad else 0), (r.returncode, bad[:5])
    return rows


def _line(lines, tag):
    (row,) = [row for row in lines if row[0] == tag]
    return row


def test_meanq_terms_rc_every_pair(lines):
    """(a)"""
    assert _line(lines, "R") == ["R", "meanq_terms_rc", str(PAIRS_252), "0"]
    assert PAIRS_252 > 8_100_000


def test_gc_bin_every_pair(lines):
    """(a)"""
    assert _line(lines, "G") == ["G", "div_len_gc", str(PAIRS_GC), "0"]


def test_meanq_terms_every_pair(lines):
    """(b)"""
    assert _line(lines, "M") == ["M", "meanq_terms", str(PAIRS_1024), "0"]
    assert PAIRS_1024 > 133_000_000


def test_div_len_bound(lines):
    """(c)"""
    assert _line(lines, "E") == ["E", "div_len_epilogue_max", "252", "0"]
    x = {int(r[1]): (int(r[2]), int(r[3])) for r in lines if r[0] == "X"}
    assert sorted(x) == list(range(1, 253))
    for n, (x_max, first_bad) in x.items():
        assert x_max == max(255 * n, (n - 1) << 16) and x_max * (n - 1) < 2 ** 32, n
        assert first_bad == 0 or first_bad > x_max, (n, x_max, first_bad)   # (0: exact below 2^32)
    tight = min((fb / xm, n) for n, (xm, fb) in x.items() if fb)
    print(f"div_len: the smallest margin is at n = {tight[1]}: first inexact x = {x[tight[1]][1]}, "
          f"{tight[0]:.4f} x the epilogue's largest numerator {x[tight[1]][0]}")


def test_edge_classes_present(lines):
    """(d)"""
    _, _, ties, neg, rem_max, n_one = _line(lines, "C")
    assert int(ties) == 255 * 126                    # even n: sb = q n + n / 2, q in 0..254
    assert int(neg) == sum(128 * n for n in range(1, 253))
    assert int(rem_max) == sum(255 if n > 1 else 256 for n in range(1, 253))
    assert int(n_one) == 256
