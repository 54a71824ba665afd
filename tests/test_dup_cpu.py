"""`stats --duplication` without a GPU: the host-only half of the
C-ABI (hpgq_dup_fingerprint, hpgq_dup_levels_of) against the known answers and
tests/dup_ref.py, the report writer's bytes, the option rules, the argument
checks of hpgq_dup_open, and the same host code under ASan + UBSan in a
stand-alone program (tests/sanitize/dup_main.c)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hpgfastq as H
import dup_ref
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KAT = json.load(open(os.path.join(HERE, "golden", "dup_kat.json")))
BOUNDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000]


def _kat_bytes(k):
    return bytes.fromhex(k["hex"]) * k["times"]


@pytest.mark.parametrize("case", range(len(KAT["fingerprints"])))
def test_fingerprint_known_answers(case):
    k = KAT["fingerprints"][case]
    s, want = _kat_bytes(k), int(k["fp"], 16)
    assert H.dup_fingerprint(s) == want, k["why"]
    assert dup_ref.fingerprint(s) == want, k["why"]


def test_kat_file_is_the_issues_table():
    got = {(_kat_bytes(k), int(k["fp"], 16)) for k in KAT["fingerprints"]}
    assert got == {(b"", 0x1), (b"A", 0xfd9a76e08e39350f), (b"A\0", 0xd7cff870de333766),
                   (b"ACGTACGT", 0x70c3c801724b0972), (b"ACGTACGTA", 0x32572c6db4b65288),
                   (b"N" * 150, 0x123fedd1b5aab34a)}


def test_fingerprint_every_length_to_600():
    """Every length 0 .. 600 of one random buffer (all byte values), at a start
    that moves, so every word count and every tail length is met."""
    rng = np.random.default_rng(61)
    buf = rng.integers(0, 256, size=1300, dtype=np.uint8).tobytes()
    seen = set()
    for n in range(601):
        s = buf[n:n + n]
        fp = H.dup_fingerprint(s)
        assert fp == dup_ref.fingerprint(s), n
        assert fp != 0
        seen.add(fp)
    assert len(seen) == 601


def test_fingerprint_sees_length_case_and_padding():
    fps = [H.dup_fingerprint(s) for s in (b"ACGT", b"acgt", b"ACGT\0", b"ACGT\0\0\0\0", b"ACGN", b"ACG", b"")]
    assert len(set(fps)) == len(fps)
    # the same words in another order are another sequence
    assert H.dup_fingerprint(b"AAAAAAAACCCCCCCC") != H.dup_fingerprint(b"CCCCCCCCAAAAAAAA")


@pytest.mark.parametrize("case", range(len(KAT["levels"])))
def test_levels_known_answers(case):
    k = KAT["levels"][case]
    assert H.dup_levels_of(k["counts"]) == k["want"], k["why"]
    assert dup_ref.levels(k["counts"]) == k["want"], k["why"]


def test_levels_at_every_bound():
    assert H.dup_level_bounds() == BOUNDS == list(dup_ref.BOUNDS)
    for i, lo in enumerate(BOUNDS):
        for c in (lo - 1, lo, lo + 1):
            got = H.dup_levels_of([c])
            assert got == dup_ref.levels([c]), c
            if c:
                want_level = i - 1 if c < lo else (i + 1 if i + 1 < 16 and c >= BOUNDS[i + 1] else i)
                assert got["distinct_at"][want_level] == 1 and got["reads_at"][want_level] == c, (c, got)
            else:
                assert got["distinct"] == 0 and got["reads"] == 0
    every = [c for lo in BOUNDS for c in (lo - 1, lo, lo + 1)]
    assert H.dup_levels_of(every) == dup_ref.levels(every)


def test_levels_counts_near_2_64_and_empty():
    big = (1 << 64) - 1
    for counts in ([big], [big - 1, 1], [1 << 63, (1 << 63) - 1], [big, 7, 10000], []):
        got = H.dup_levels_of(counts)
        assert got == dup_ref.levels(counts), counts
    assert H.dup_levels_of([big])["reads_at"][15] == big
    assert H.dup_levels_of([big, 7, 10000])["reads"] == (big + 10007) % (1 << 64)   # (sums are mod 2^64)
    assert H.dup_levels_of([]) == dict(reads=0, distinct=0, max_count=0, distinct_at=[0] * 16, reads_at=[0] * 16)
    lv = H.DupLevels()
    assert H.lib.hpgq_dup_levels_of(None, 3, C.byref(lv)) == -1
    assert H.lib.hpgq_dup_levels_of(None, 0, None) == -1


def test_reference_by_hand():
    """tests/dup_ref.py itself on a few reads worked out by hand."""
    seq = np.frombuffer(b"xxACGTACGTAAC", dtype=np.uint8)       # two bytes before the first read
    idx = np.array([2, 6, 10, 10, 11, 12, 13], dtype=np.int32)  # ACGT ACGT "" A A C
    seqs = dup_ref.sequences(seq, idx)
    assert seqs == [b"ACGT", b"ACGT", b"", b"A", b"A", b"C"]
    t = dup_ref.table(seqs)
    assert t == {dup_ref.fingerprint(b"ACGT"): 2, 1: 1, 0xfd9a76e08e39350f: 2, dup_ref.fingerprint(b"C"): 1}
    t = dup_ref.table(dup_ref.sequences(seq, idx, np.array([1, 0, 1, 2, 1, 0], np.uint8)))
    assert t == {dup_ref.fingerprint(b"ACGT"): 1, 1: 1, 0xfd9a76e08e39350f: 1}
    lv = dup_ref.levels_of_table(dup_ref.table(seqs))
    assert dup_ref.render(lv) == (
        b"# Reads\tDistinct\tHighest count\t% distinct\n6\t4\t2\t66.67\n"
        b"# Level\tSequences\tReads\t% of sequences\t% of reads\n"
        b"1\t2\t2\t50.00\t33.33\n2\t2\t4\t50.00\t66.67\n" +
        b"".join(b"%s\t0\t0\t0.00\t0.00\n" % n.encode() for n in dup_ref.LABELS[2:]))
    keys, counts = dup_ref.arrays(t)
    blob = np.concatenate([[np.uint64(len(keys))], keys, counts]).astype(np.uint64).tobytes()
    ((k2, c2),) = dup_ref.parse_dump(blob)
    assert list(k2) == sorted(t) and [int(c) for c in c2] == [t[int(k)] for k in k2]


def test_open_argument_checks():
    h = C.c_void_p()
    for lo, hi in ((3, 20), (0, 20), (-1, 20), (20, 19), (4, 35), (35, 35), (20, 3)):
        assert H.lib.hpgq_dup_open(C.byref(h), 0, lo, hi, None) == -1, (lo, hi)
    assert H.lib.hpgq_dup_open(None, 0, 20, 32, None) == -1
    for fn in (H.lib.hpgq_dup_sync, H.lib.hpgq_dup_reset):
        assert fn(None) == -1
    assert H.lib.hpgq_dup_debug_set_max_workgroups(None, 2) == -1
    assert H.lib.hpgq_dup_count_device(None, None, None) == -1
    assert H.lib.hpgq_dup_levels(None, None) == -1
    assert H.lib.hpgq_dup_export(None, None, None, 0, None) == -1
    assert H.lib.hpgq_dup_import(None, None, None, 0) == -1
    assert H.lib.hpgq_dup_debug_fingerprints(None, None, None) == -1
    assert H.lib.hpgq_dup_debug_info(None, None, None) == -1
    assert H.lib.hpgq_dup_debug_set_timing(None, 1) == -1
    assert H.lib.hpgq_dup_debug_last_times(None, None, None) == -1
    H.lib.hpgq_dup_close(None)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device path")
def test_open_fails_loudly_without_device():
    with pytest.raises(H.HpgqError) as e:
        H.Duplication()
    assert e.value.code == -5


INPUTS = {"se": lambda f: ["-f", f], "pair": lambda f: ["--fq1", f, "--fq2", f + "2"],
          "interleaved": lambda f: ["-f", f, "--interleaved"]}


@pytest.mark.parametrize("inputs", sorted(INPUTS))
def test_option_parses_on_stats_and_changes_no_parameter(tmp_path, inputs):
    files = INPUTS[inputs](str(tmp_path / "in.fq"))
    kw = dict(lmax=150, read_quality_range="20,", quality_encoding="phred64")
    flags = files + ["--read-quality-range", "20,", "--lmax", "150", "--quality-encoding", "phred64"]
    got = print_params("stats", *flags, "--duplication", "--duplication-out", str(tmp_path / "d.bin"))
    assert got == print_params("stats", *flags)
    twin = H.stats_params(**kw).as_dict()                 # the Python twin of the option rules
    if inputs != "se":
        twin["paired"] = 1
    assert got == twin


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]),
                                       ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
def test_option_rejected_on_filter_and_edit(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in (["--duplication"], ["--duplication-out", str(tmp_path / "d.bin")]):
        r = run_cli([cmd, "-f", fq, "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        assert len(r.stderr.strip().splitlines()) == 1 and "--duplication" in r.stderr
        assert r.stdout == "" and list(out.iterdir()) == [] and not (tmp_path / "d.bin").exists()


def test_help_shows_the_flags():
    r = run_cli(["stats", "--help"], check=False)
    assert "--duplication " in r.stdout and "--duplication-out=<file>" in r.stdout
    r = run_cli(["filter", "--help"], check=False)
    assert "--duplication" not in r.stdout


LEVEL_CASES = [k["counts"] for k in KAT["levels"]] + [
    [(1 << 64) - 1, 7, 10000], [lo + d for lo in BOUNDS for d in (-1, 0, 1)],
    [1] * 700 + [2] * 30 + [3, 3, 12, 12, 12, 51, 777, 20000]]   # the last one is rendered


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """csrc/hpgq_dup_post.cpp and host/hpgq_report_dup.c with their own main
    (nothing loaded into Python), built with ASan + UBSan and run once."""
    tmp = tmp_path_factory.mktemp("dup_san")
    exe, obj = tmp / "dup_main", tmp / "dup_post.o"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hpg-fastq_amd", "host")]
    for cmd in (["g++", *san, "-std=c++17", *inc, "-c", os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_dup_post.cpp"),
                 "-o", str(obj)],
                ["gcc", *san, "-std=gnu11", "-Wall", *inc, os.path.join(HERE, "sanitize", "dup_main.c"),
                 os.path.join(ROOT, "hpg-fastq_amd", "host", "hpgq_report_dup.c"), str(obj), "-o", str(exe), "-lstdc++"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    rng = np.random.default_rng(62)
    lines = []
    seqs = [_kat_bytes(k) for k in KAT["fingerprints"]] + \
        [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (1, 7, 8, 9, 15, 16, 17, 64, 65, 151, 600)]
    for s in seqs:
        lines.append(f"F {len(s)} {s.hex() or '-'} {dup_ref.fingerprint(s):x}\n")
    for counts in LEVEL_CASES:
        lv = dup_ref.levels(counts)
        nums = list(counts) + [lv["reads"], lv["distinct"], lv["max_count"]] + lv["distinct_at"] + lv["reads_at"]
        lines.append(f"L {len(counts)} " + " ".join(map(str, nums)) + "\n")
    (tmp / "cases.txt").write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp / "cases.txt"), str(tmp), "in.fq"], capture_output=True, text=True,
                       timeout=300, env=env)
    return r, len(lines), tmp


def test_host_code_under_asan_ubsan(sanitized):
    r, ncases, _ = sanitized
    assert r.returncode == 0 and f"dup_main: ok {ncases} cases" in r.stdout, r.stdout + r.stderr


def test_rendered_file_bytes(sanitized):
    """host/hpgq_report_dup.c's file against dup_ref.render, percentages with
    thirds and a level of one sequence in 738."""
    r, _, tmp = sanitized
    assert r.returncode == 0, r.stdout + r.stderr
    want = dup_ref.render(dup_ref.levels(LEVEL_CASES[-1]))
    assert (tmp / "in.fq.duplication.data").read_bytes() == want
    assert want.count(b"\n") == 19 and b"\n>=10000\t1\t20000\t" in want
