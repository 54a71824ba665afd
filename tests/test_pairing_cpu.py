"""Paired-end input without a GPU: hpgq_fastq_record_prefix (libhpgq host code,
HIP-free) at every cut point, the same sweep as a stand-alone C program under
ASan + UBSan, and the CLI's paired options (--fq1/--fq2, --interleaved)."""
import os
import subprocess

import pytest

import hpgfastq as H
from cli_lib import print_params, run_cli
from fastq_io import to_fastq
from test_parse_cpu import _reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_prefix(text, max_records):
    """The first min(max_records, whole records) four-line records of `text`
    by a Python line splitter: (bytes, records)."""
    lines = text.split(b"\n")[:-1]   # the '\n'-terminated lines
    k = min(max_records, len(lines) // 4)
    return sum(len(ln) + 1 for ln in lines[:4 * k]), k


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("plus_header", [False, True])
def test_record_prefix_every_cut(crlf, plus_header):
    reads = _reads()
    quals = [reads.read(i)[1] for i in range(reads.n)]
    assert any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
    text, ends = to_fastq(reads, crlf=crlf, plus_header=plus_header)
    for n in range(0, len(text) + 1):
        for mx in (0, 1, 3, 10**9):
            assert H.record_prefix(text[:n], mx) == ref_prefix(text[:n], mx), (n, mx)
    # the whole text: every record, ending where to_fastq says they end
    assert H.record_prefix(text, 10**9) == (len(text), reads.n)
    assert H.record_prefix(text, 3) == (ends[2], 3)
    assert H.lib.hpgq_fastq_count_lines(text, len(text)) == 4 * reads.n


def test_record_prefix_standalone_under_asan_ubsan(tmp_path):
    """tests/sanitize/prefix_main.c + the HIP-free source, compiled with gcc
    alone (no libhpgq, no Python in the process) and run directly."""
    exe = tmp_path / "prefix_main"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "sanitize", "prefix_main.c"),
                        os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_fastq_text.c"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "prefix_main: ok" in r.stdout, r.stdout + r.stderr


def test_strerror_pairing():
    assert H.E_PAIRING == -10
    assert H.lib.hpgq_strerror(-10) == b"mate pairs out of step"


# ---- options -----------------------------------------------------------------
@pytest.mark.parametrize("cmd,extra", [("stats", []), ("filter", ["--max-N", "1"]),
                                       ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
@pytest.mark.parametrize("form", [["--fq1", "a_1.fq", "--fq2", "a_2.fq"],
                                  ["--fastq1", "a_1.fq", "--fastq2", "a_2.fq"],
                                  ["--interleaved", "-f", "a.fq"]])
def test_print_params_paired(cmd, extra, form):
    d = print_params(cmd, *form, *extra)
    assert d["paired"] == 1
    single = print_params(cmd, "-f", "a.fq", *extra)
    assert single["paired"] == 0
    assert {k: v for k, v in d.items() if k != "paired"} == {k: v for k, v in single.items() if k != "paired"}


def test_print_params_single_end_unchanged():
    r = run_cli(["stats", "--print-params", "-f", "a.fq", "--read-quality-range", "20,"])
    assert r.stdout == (
        "phred=33 lmax=1024 stats_on=1 filter_on=1 edit_on=0 paired=0\n"
        "min_read_length=0 max_read_length=100000 min_read_quality=20 max_read_quality=100000\n"
        "max_out_of_quality=100000 left_length=0 min_left_quality=0 max_left_quality=100000\n"
        "right_length=0 min_right_quality=0 max_right_quality=100000 max_N=100000\n"
        "edit_left_length=0 edit_min_left_quality=0 edit_max_left_quality=100000\n"
        "edit_right_length=0 edit_min_right_quality=0 edit_max_right_quality=100000\n")


REJECTED = [
    (["--fq1", "a_1.fq"], "--fq1 and --fq2 must be given together"),
    (["--fq2", "a_2.fq"], "--fq1 and --fq2 must be given together"),
    (["--fq1", "a_1.fq", "--fq2", "a_2.fq", "-f", "a.fq"], "cannot be combined with -f or --interleaved"),
    (["--fq1", "a_1.fq", "--fq2", "a_2.fq", "--interleaved"], "cannot be combined with -f or --interleaved"),
    (["--fq1", "a_1.fq", "--interleaved", "-f", "a.fq"], "cannot be combined with -f or --interleaved"),
    (["--interleaved"], "--interleaved needs the input file (-f)"),
    (["--fq1", "a_1.fq", "--fq2", "a_2.fq", "--kmers"], "not available for paired-end input"),
    (["--fq1", "a_1.fq", "--fq2", "a_2.fq", "--cg"], "not available for paired-end input"),
    (["--interleaved", "-f", "a.fq", "--kmers"], "not available for paired-end input"),
    (["--interleaved", "-f", "a.fq", "--chaos-game"], "not available for paired-end input"),
    (["--fq1", "x/a.fq", "--fq2", "y/a.fq"], "same base name"),
]


@pytest.mark.parametrize("flags,message", REJECTED)
def test_rejected_combinations(flags, message):
    r = run_cli(["stats", "--print-params"] + flags, check=False)
    assert r.returncode != 0 and message in r.stdout, (r.returncode, r.stdout[:400])


def test_missing_mate_file_rejected(tmp_path):
    fq = tmp_path / "a_1.fq"
    fq.write_bytes(b"@r\nA\n+\nI\n")
    r = run_cli(["stats", "--fq1", fq, "--fq2", tmp_path / "none.fq", "-o", tmp_path], check=False)
    assert r.returncode != 0 and "Input file name not found" in r.stdout


def test_help_lists_paired_flags():
    r = run_cli(["filter", "--help"], check=False)
    for flag in ("--fq1", "--fastq2", "--interleaved"):
        assert flag in r.stdout
