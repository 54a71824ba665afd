"""`stats --overrepresented` without a GPU: hpgq_dup_top_of
against tests/overrep_ref.py, the report writer's bytes, the option rules, the
argument checks of the new entry points, and the same host code under ASan +
UBSan in a stand-alone program (tests/sanitize/overrep_main.c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hpgfastq as H
import dup_ref
import overrep_ref
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIG = (1 << 64) - 1


def _random_pairs():
    rng = np.random.default_rng(71)
    keys = np.unique(rng.integers(1, 1 << 63, size=5200, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[:5000]
    keys = keys[rng.permutation(5000)]
    counts = rng.integers(1, 40, size=5000).astype(np.uint64)      # many ties
    return [int(k) for k in keys], [int(c) for c in counts]


RK, RC = _random_pairs()
# (keys, counts, cap, min_count, why)
CASES = [
    ([], [], 5, 1, "empty input"),
    ([], [], 0, 1, "empty input, cap 0"),
    ([9, 3, BIG, 1 << 63, 7], [4, 4, 4, 4, 4], 5, 1, "all counts equal: by key only, unsigned"),
    ([9, 3, BIG, 1 << 63, 7], [4, 4, 4, 4, 4], 3, 4, "all counts equal, cut inside the tie"),
    ([5, 6, 7], [10, 20, 30], 3, 31, "min_count above every count"),
    ([5, 6, 7, 8], [10, 20, 30, 20], 0, 1, "cap 0"),
    ([5, 6, 7, 8], [10, 20, 30, 20], 1, 1, "cap 1"),
    ([5, 6, 7, 8], [10, 20, 30, 20], 100, 15, "cap more than total"),
    ([1, 2, 3, 4, 5], [BIG, BIG - 1, 1 << 63, BIG, (1 << 63) - 1], 4, 1 << 63, "counts near 2^64"),
    ([1, 2, 3], [BIG, BIG - 1, 5], 3, BIG, "min_count 2^64 - 1"),
    (RK, RC, 5000, 1, "5,000 random pairs, all"),
    (RK, RC, 37, 30, "5,000 random pairs, a cut inside a tie"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_top_of_against_reference(case):
    keys, counts, cap, min_count, why = CASES[case]
    want, total = overrep_ref.select_pairs(zip(keys, counts), cap, min_count)
    k, c, t = H.dup_top_of(keys, counts, cap, min_count)
    assert t == total, why
    assert [(int(a), int(b)) for a, b in zip(k, c)] == want, why


def test_the_tie_cases_do_tie():
    """The cases mean what they say: the cut of the random case falls inside a tie."""
    want, total = overrep_ref.select_pairs(zip(RK, RC), 38, 30)
    assert total > 38 and want[36][1] == want[37][1] and want[36][0] < want[37][0]
    want, _ = overrep_ref.select_pairs(zip(*CASES[2][:2]), 5, 1)
    assert [k for k, _ in want] == [3, 7, 9, 1 << 63, BIG]


def test_top_of_argument_checks():
    t = C.c_size_t(0)
    one = np.array([1], dtype=np.uint64)
    p = one.ctypes.data_as(C.c_void_p)
    assert H.lib.hpgq_dup_top_of(None, None, 1, 1, None, None, 0, C.byref(t)) == -1
    assert H.lib.hpgq_dup_top_of(p, p, 1, 0, None, None, 0, C.byref(t)) == -1
    assert H.lib.hpgq_dup_top_of(p, p, 1, 1, None, None, 0, None) == -1
    assert H.lib.hpgq_dup_top_of(p, p, 1, 1, p, None, 1, C.byref(t)) == -1
    assert H.lib.hpgq_dup_top_of(None, None, 0, 1, None, None, 0, C.byref(t)) == 0 and t.value == 0
    assert H.lib.hpgq_dup_keep_sequences(None, 1, 1) == -1
    assert H.lib.hpgq_dup_top(None, 1, None, None, 0, C.byref(t)) == -1
    assert H.lib.hpgq_dup_sequence(None, 1, None, 0, None) == -1
    assert H.lib.hpgq_dup_debug_kept(None, None, None) == -1
    assert H.lib.hpgq_dup_debug_last_keep_time(None, None) == -1


def test_reference_by_hand():
    """tests/overrep_ref.py itself on a few reads worked out by hand."""
    seqs = [b"ACGT", b"AC\tT", b"ACGT", b"", b"", b"AC\tT", b"ACGT", b"G"]
    assert overrep_ref.count_map(seqs) == {b"ACGT": 3, b"AC\tT": 2, b"": 2, b"G": 1}
    got, total = overrep_ref.select(seqs, 10, 2)
    assert total == 3 and got[0] == (dup_ref.fingerprint(b"ACGT"), 3, b"ACGT")
    # the two with count 2: by fingerprint ascending; the empty read's is 1
    assert got[1] == (1, 2, b"") and got[2] == (dup_ref.fingerprint(b"AC\tT"), 2, b"AC\tT")
    assert overrep_ref.select(seqs, 1, 1) == ([got[0]], 4)
    assert overrep_ref.kept(seqs, 2) == (3, 8)
    assert overrep_ref.render(got, 8) == (b"# Rank\tCount\t% of reads\tLength\tSequence\n"
                                          b"1\t3\t37.5000\t4\tACGT\n2\t2\t25.0000\t0\t\n3\t2\t25.0000\t4\tAC\tT\n")
    assert overrep_ref.render([], 0) == overrep_ref.HEADER
    assert overrep_ref.render(got[:1], 0).endswith(b"1\t3\t0.0000\t4\tACGT\n")


INPUTS = {"se": lambda f: ["-f", f], "pair": lambda f: ["--fq1", f, "--fq2", f + "2"],
          "interleaved": lambda f: ["-f", f, "--interleaved"]}


@pytest.mark.parametrize("inputs", sorted(INPUTS))
def test_option_parses_on_stats_and_changes_no_parameter(tmp_path, inputs):
    files = INPUTS[inputs](str(tmp_path / "in.fq"))
    flags = files + ["--read-quality-range", "20,", "--lmax", "150"]
    got = print_params("stats", *flags, "--overrepresented", "--overrepresented-min-count", "8",
                       "--overrepresented-top=50", "--overrepresented-bytes", "4096")
    assert got == print_params("stats", *flags)


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]),
                                       ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
def test_option_rejected_on_filter_and_edit(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in (["--overrepresented"], ["--overrepresented-min-count", "5"], ["--overrepresented-top", "5"],
                  ["--overrepresented-bytes", "5"]):
        r = run_cli([cmd, "-f", fq, "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        assert len(r.stderr.strip().splitlines()) == 1 and "--overrepresented" in r.stderr
        assert r.stdout == "" and list(out.iterdir()) == []


@pytest.mark.parametrize("extra", [["--overrepresented-min-count", "5"], ["--overrepresented-top", "5"],
                                   ["--overrepresented-bytes", "5"],
                                   ["--overrepresented", "--overrepresented-min-count", "0"],
                                   ["--overrepresented", "--overrepresented-min-count", "-3"],
                                   ["--overrepresented", "--overrepresented-min-count", "x"],
                                   ["--overrepresented", "--overrepresented-top", "0"],
                                   ["--overrepresented", "--overrepresented-top", "100001"],
                                   ["--overrepresented", "--overrepresented-bytes", "0"],
                                   ["--overrepresented", "--overrepresented-bytes", str((1 << 40) + 1)]])
def test_bad_values_are_errors(tmp_path, extra):
    r = run_cli(["stats", "-f", tmp_path / "in.fq", "--print-params", *extra], check=False)
    assert r.returncode != 0 and "Error: " in r.stdout and "overrepresented" in r.stdout


def test_help_shows_the_flags():
    r = run_cli(["stats", "--help"], check=False)
    for flag in ("--overrepresented ", "--overrepresented-min-count=<int>", "--overrepresented-top=<int>",
                 "--overrepresented-bytes=<int>"):
        assert flag in r.stdout, flag
    r = run_cli(["filter", "--help"], check=False)
    assert "--overrepresented" not in r.stdout


# the rendered files: (base, reads, [(count, bytes)])
RENDER = [
    ("tab.fq", 1000, [(700, b"ACGT\tACGT\t"), (3, b"\t"), (1, b"N" * 150)]),
    ("empty.fq", 7, [(4, b""), (3, b"A")]),
    ("noreads.fq", 0, [(5, b"ACGT"), (5, b"")]),
    ("none.fq", 12, []),
    ("third.fq", 3, [(1, bytes(range(256)))]),
]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """csrc/hpgq_dup_post.cpp and host/hpgq_report_overrep.c with their own main
    (nothing loaded into Python), built with ASan + UBSan and run once."""
    tmp = tmp_path_factory.mktemp("overrep_san")
    exe, obj = tmp / "overrep_main", tmp / "dup_post.o"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hpg-fastq_amd", "host")]
    for cmd in (["g++", *san, "-std=c++17", *inc, "-c", os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_dup_post.cpp"),
                 "-o", str(obj)],
                ["gcc", *san, "-std=gnu11", "-Wall", *inc, os.path.join(HERE, "sanitize", "overrep_main.c"),
                 os.path.join(ROOT, "hpg-fastq_amd", "host", "hpgq_report_overrep.c"), str(obj), "-o", str(exe),
                 "-lstdc++"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    lines = []
    for keys, counts, cap, min_count, _ in CASES:
        want, total = overrep_ref.select_pairs(zip(keys, counts), cap, min_count)
        nums = [len(keys), cap, min_count] + [x for kc in zip(keys, counts) for x in kc] + [total, len(want)] + \
            [x for kc in want for x in kc]
        lines.append("T " + " ".join(map(str, nums)) + "\n")
    for base, reads, entries in RENDER:
        words = [base, reads, len(entries)] + [x for c, s in entries for x in (c, len(s), s.hex() or "-")]
        lines.append("R " + " ".join(map(str, words)) + "\n")
    (tmp / "cases.txt").write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp / "cases.txt"), str(tmp)], capture_output=True, text=True, timeout=300, env=env)
    return r, len(lines), tmp


def test_host_code_under_asan_ubsan(sanitized):
    r, ncases, _ = sanitized
    assert r.returncode == 0 and f"overrep_main: ok {ncases} cases" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("case", range(len(RENDER)))
def test_rendered_file_bytes(sanitized, case):
    """host/hpgq_report_overrep.c's file against overrep_ref.render: a sequence
    holding a tab, a zero-length sequence, reads == 0, no entry at all, every
    byte value."""
    r, _, tmp = sanitized
    assert r.returncode == 0, r.stdout + r.stderr
    base, reads, entries = RENDER[case]
    want = overrep_ref.render([(0, c, s) for c, s in entries], reads)
    assert (tmp / (base + ".overrepresented.data")).read_bytes() == want
    assert want.count(b"\n") >= 1 + len(entries)
