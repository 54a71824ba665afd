"""`edit --clip-overlap` without a GPU: hpgq_ovl_find against
tests/ovl_ref.py on the edge list and on random pairs, hand-checked cases, the
argument checks of hpgq_ovl_find and hpgq_ovl_open, the flag rules through the
CLI, and the host function together with the kernel's lane arithmetic under
ASan + UBSan in a stand-alone program (tests/sanitize/ovl_main.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

import hpgfastq as H
import ovl_ref as R
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PARAMS = [(8, 0), (30, 5), (512, 255)]
BAD_PARAMS = [(7, 0), (513, 5), (30, -1), (30, 256), (30, 30), (8, 8), (30, 31), (0, 0), (-5, 0)]


def _cases(edge_seed=5, nrandom=1500):
    """[(min_overlap, M, s1, s2)]"""
    out = []
    for mo, M in PARAMS:
        out += [(mo, M, a, b) for a, b in R.edge_pairs(mo, M, edge_seed)]
    for i, (a, b) in enumerate(R.random_pairs(nrandom, 81)):
        mo, M = [(8, 0), (30, 5), (12, 2), (20, 19)][i % 4]
        out.append((mo, M, a, b))
    # long mates for the widest parameters: a read-through, an overlap, nothing
    import numpy as np
    rng = np.random.default_rng(82)
    for F in (512, 700, 300):
        a, b = R.pair_of(rng, 512, 512, F)
        out += [(512, 255, a, b), (30, 5, a, b)]
    return out


def test_find_against_reference():
    cases = _cases()
    found = cut = 0
    for mo, M, a, b in cases:
        want = R.find(a, b, mo, M)
        assert H.ovl_find(a, b, mo, M) == want, (mo, M, a, b)
        found += want > 0
        cut += want > 0 and R.cuts(len(a), len(b), want) != (len(a), len(b))
    assert found > len(cases) // 3 and cut > found // 3


def test_reference_by_hand():
    """tests/ovl_ref.py itself, and the library, on pairs worked out by hand."""
    frag = b"ACGGTCATTGCAACGTTAGCATCGGATCAATGCCTA"                   # 36 bases
    rc = b"TAGGCATTGATCCGATGCTAACGTTGCAATGACCGT"
    assert R.revcomp(frag) == rc
    for f in (R.find, H.ovl_find):
        # read-through: the fragment's first 20 bases, then adapter, in both mates
        s1, s2 = frag[:20] + b"GGGGGGGGGG", R.revcomp(frag[:20]) + b"TTTTTTTTTT"
        assert f(s1, s2, 8, 0) == 20 and R.cuts(30, 30, 20) == (20, 20)
        # the mates overlap by 24 of the 36 bases: found, nothing cut
        assert f(frag[:30], rc[:30], 8, 0) == 36 and R.cuts(30, 30, 36) == (30, 30)
        # one mismatch
        bad = R.flip(s1, 4)
        assert f(bad, s2, 8, 0) == 0 and f(bad, s2, 8, 1) == 20
        # N faces N: a mismatch; lower case too
        assert f(b"ACGTNACGTAC", b"GTACGTNACGT", 8, 0) == 0 and f(b"ACGTNACGTAC", b"GTACGTNACGT", 8, 1) == 11
        assert f(b"acgtacgtac", b"gtacgtacgt", 8, 7) == 0
        # ov = min_overlap - 1
        assert f(frag[:9], R.revcomp(frag[:9]), 10, 0) == 0 and f(frag[:10], R.revcomp(frag[:10]), 10, 0) == 10
        # AT repeat: admissible at every even F up to 2 n - 8; the greatest wins, nothing is cut
        assert f(b"AT" * 10, b"AT" * 10, 8, 0) == 32
        # a mate of 513 bases
        assert f(b"A" * 513, b"T" * 20, 8, 0) == -1 and f(b"A" * 20, b"T" * 513, 8, 0) == -1
        assert f(b"", b"", 8, 0) == 0 and f(b"ACGTACGT", b"", 8, 0) == 0
    i = dict(pairs=3, skipped=1, overlapping=2, clipped=1, bases_removed=[10, 7])
    assert R.render(i) == (b"# Pairs\tSkipped\tOverlapping\t% overlapping\tClipped\t% clipped\tBases removed 1\tBases removed 2\n"
                           b"3\t1\t2\t66.67\t1\t33.33\t10\t7\n")
    z = dict(pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0])
    assert R.render(z).endswith(b"\n0\t0\t0\t0.00\t0\t0.00\t0\t0\n")


def _open(mo, M):
    h = C.c_void_p()
    rc = H.lib.hpgq_ovl_open(C.byref(h), 0, mo, M, None)
    if h.value:
        H.lib.hpgq_ovl_close(h)
    return rc


def test_invalid_arguments():
    """-2 from the host function, HPGQ_E_INVALID from hpgq_ovl_open before any
    device call (there is no device here), for every rule of §2.13."""
    s = b"ACGTACGTACGTACGT"
    for mo, M in BAD_PARAMS:
        assert H.lib.hpgq_ovl_find(s, len(s), s, len(s), mo, M) == -2, (mo, M)
        assert _open(mo, M) == -1, (mo, M)
        with pytest.raises(H.HpgqError):
            H.ovl_find(s, s, mo, M)
    assert H.lib.hpgq_ovl_find(None, 5, s, len(s), 8, 0) == -2 and H.lib.hpgq_ovl_find(s, len(s), None, 5, 8, 0) == -2
    assert H.lib.hpgq_ovl_find(None, 0, None, 0, 8, 0) == 0
    assert H.lib.hpgq_ovl_open(None, 0, 30, 5, None) == -1
    # parameters that follow the rules get as far as the device (0 with one, HPGQ_E_NO_DEVICE without)
    for mo, M in PARAMS + [(8, 7), (256, 255)]:
        assert H.lib.hpgq_ovl_find(s, len(s), s, len(s), mo, M) >= 0
        assert _open(mo, M) in (0, -5)
    b = H.Batch()
    for f, args in (("sync", ()), ("reset", ()), ("read", (None,)), ("debug_set_max_workgroups", (1,)),
                    ("find_device", (C.byref(b), C.byref(b), None, None, None)),
                    ("batch_device", (C.byref(b), C.byref(b), C.byref(b), C.byref(b)))):
        assert getattr(H.lib, "hpgq_ovl_" + f)(None, *args) == -1, f
    H.lib.hpgq_ovl_close(None)


# -- the flag rules, through the CLI (all end before any device call) ----------------------------

EDIT = ["--left-length", "5", "--left-quality-range", "20,"]
OVL_FLAGS = (["--clip-overlap"], ["--clip-overlap-min", "20"], ["--clip-overlap-mismatches", "2"])


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]), ("stats", [])])
def test_flags_rejected_on_stats_and_filter(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r/1\nACGT\n+\nIIII\n@r/2\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in OVL_FLAGS:
        r = run_cli([cmd, "-f", fq, "--interleaved", "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        assert r.stderr == f"hpg-fastq: --clip-overlap is an option of the edit command, not of {cmd}\n"
        assert r.stdout == "" and list(out.iterdir()) == []


@pytest.mark.parametrize("extra", OVL_FLAGS[1:])
def test_value_flags_need_the_flag(tmp_path, extra):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, *extra], check=False)
    assert r.returncode != 0 and "Error: --clip-overlap-min and --clip-overlap-mismatches need --clip-overlap" in r.stdout


def test_single_end_input_is_rejected(tmp_path):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--print-params", *EDIT, "--clip-overlap"], check=False)
    assert r.returncode != 0
    assert "\nError: --clip-overlap needs paired-end input (--fq1/--fq2 or --interleaved)\n" in r.stdout
    assert "Usage:" in r.stdout


@pytest.mark.parametrize("flag,value", [("min", "7"), ("min", "513"), ("min", "x"), ("min", ""), ("min", "-1"),
                                        ("mismatches", "-1"), ("mismatches", "256"), ("mismatches", "3x")])
def test_value_ranges(tmp_path, flag, value):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, "--clip-overlap",
                 f"--clip-overlap-{flag}={value}"], check=False)
    rng = "8..512" if flag == "min" else "0..255"
    assert r.returncode != 0 and f"Error: --clip-overlap-{flag} must be an integer in {rng}" in r.stdout


@pytest.mark.parametrize("mo,M", [(8, 8), (30, 30), (30, 200), (None, 30)])
def test_mismatches_below_the_minimum(tmp_path, mo, M):
    flags = ["--clip-overlap", "--clip-overlap-mismatches", str(M)] + (["--clip-overlap-min", str(mo)] if mo else [])
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, *flags], check=False)
    assert r.returncode != 0 and "Error: --clip-overlap-mismatches" in r.stdout and "must be below --clip-overlap-min" in r.stdout
    assert "Usage:" in r.stdout


def test_nothing_to_edit_rule_stays(tmp_path):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", "--clip-overlap"], check=False)
    assert r.returncode != 0 and "Error: Nothing to edit, no edit options specified !" in r.stdout


def test_flags_parse_on_edit_and_change_no_parameter(tmp_path):
    for inputs in (["-f", str(tmp_path / "in.fq"), "--interleaved"], ["--fq1", str(tmp_path / "a.fq"), "--fq2", str(tmp_path / "b.fq")]):
        flags = [*inputs, *EDIT, "--read-quality-range", "20,", "--lmax", "150"]
        plain = print_params("edit", *flags)
        assert plain["paired"] == 1
        assert print_params("edit", *flags, "--clip-overlap") == plain
        for mo, M in (("8", "0"), ("30", "5"), ("512", "255"), ("9", "8")):
            assert print_params("edit", *flags, "--clip-overlap", "--clip-overlap-min", mo, "--clip-overlap-mismatches", M) == plain
        assert print_params("edit", *flags, "--clip-overlap", "--clip-adapters", "--clip-min-overlap", "5") == plain


def test_help_shows_the_flags():
    r = run_cli(["edit", "--help"], check=False)
    for flag in ("--clip-overlap ", "--clip-overlap-min=<int>", "--clip-overlap-mismatches=<int>"):
        assert flag in r.stdout, flag
    for cmd in ("stats", "filter"):
        assert "--clip-overlap" not in run_cli([cmd, "--help"], check=False).stdout


# -- the host function and the kernel's lane arithmetic under ASan + UBSan -----------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/hpgq_ovl_post.cpp and csrc/hpgq_ovl_lane.h with their own main:
    nothing loaded into Python."""
    exe = tmp_path / "ovl_main"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    r = subprocess.run(["g++", *san, "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(HERE, "sanitize", "ovl_main.cpp"),
                        os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_ovl_post.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hexed = lambda b: b.hex() or "-"    # noqa: E731
    lines = []
    for mo, M, a, b in _cases(edge_seed=6, nrandom=600):
        lines.append(f"{mo} {M} {hexed(a)} {hexed(b)} {R.find(a, b, mo, M)}")
    for mo, M in BAD_PARAMS:
        lines.append(f"{mo} {M} {hexed(b'ACGTACGTAC')} {hexed(b'GTACGTACGT')} -2")
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"ovl_main: ok {len(lines)} cases" in r.stdout, r.stdout + r.stderr
