"""`stats --adapters` without a GPU: the argument checks of
hpgq_adapt_open, hpgq_adapt_find against bytes.find, hpgq_adapt_add, the default
set, the adapter-file parser and the flag rules through the CLI, the report
writer's bytes against tests/adapt_ref.py, and the same host code under ASan +
UBSan in a stand-alone program (tests/sanitize/adapt_main.c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hpgfastq as H
import adapt_ref
import hostile_lib as HL
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOOD = b"AGATCGGAAGAG"
BAD_PROBES = [b"ACGTACG", b"A" * 33, b"", b"ACGTACGa", b"ACGTNCGT", b"ACGTACG\xc1", b"ACGT ACGT"]


def _open(probes, rows=10):
    arr = (C.c_char_p * max(len(probes), 1))(*probes)
    h = C.c_void_p()
    rc = H.lib.hpgq_adapt_open(C.byref(h), 0, arr, len(probes), rows, None)
    if h.value:
        H.lib.hpgq_adapt_close(h)
    return rc


def test_open_argument_checks():
    """All rejected with HPGQ_E_INVALID before any device call (there is no device here)."""
    assert _open([]) == -1 and _open([GOOD] * 33) == -1
    assert _open([GOOD], rows=0) == -1 and _open([GOOD], rows=-5) == -1
    for bad in BAD_PROBES:
        assert _open([bad]) == -1, bad
        assert _open([GOOD, bad, GOOD]) == -1, bad
    h = C.c_void_p()
    assert H.lib.hpgq_adapt_open(C.byref(h), 0, None, 1, 10, None) == -1
    assert H.lib.hpgq_adapt_open(None, 0, None, 1, 10, None) == -1
    # a set that follows the rules gets as far as the device (0 with one, HPGQ_E_NO_DEVICE without)
    assert _open([GOOD, b"A" * 8, b"ACGT" * 8, GOOD]) in (0, -5)
    assert _open([GOOD] * 32) in (0, -5)
    for f in ("sync", "reset"):
        assert getattr(H.lib, "hpgq_adapt_" + f)(None) == -1
    assert H.lib.hpgq_adapt_reserve_length(None, 5) == -1
    assert H.lib.hpgq_adapt_count_device(None, None, None) == -1
    assert H.lib.hpgq_adapt_read(None, None, 0, None) == -1
    assert H.lib.hpgq_adapt_debug_set_max_workgroups(None, 1) == -1
    H.lib.hpgq_adapt_close(None)


def test_find_against_bytes_find():
    rng = np.random.default_rng(51)
    probes = adapt_ref.DEFAULT_PROBES + [b"ACGTACGT", b"ACGT" * 8, b"A" * 8]
    hits = 0
    for i in range(400):
        n = int(rng.integers(0, 200))
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])
        p = probes[i % len(probes)]
        if i % 3 == 0 and n >= len(p):
            at = int(rng.integers(0, n - len(p) + 1))
            s = s[:at] + p + s[at + len(p):]
        if i % 5 == 0 and n:                               # one hostile byte somewhere
            at = int(rng.integers(0, n))
            s = s[:at] + bytes([int(rng.integers(0, 256))]) + s[at + 1:]
        for q in probes:
            assert H.adapt_find(s, q) == s.find(q), (s, q)
        hits += s.find(p) >= 0
    assert hits > 80
    reads, _ = HL.atlas((1, 2, 49, 50, 51, 150))            # every byte value at every place
    blob = bytes(reads.seq)
    for q in probes + [b"CGTACGTACGTA"]:
        for i in range(0, reads.n, 7):
            s = blob[int(reads.idx[i]):int(reads.idx[i + 1])]
            assert H.adapt_find(s, q) == s.find(q)
    assert H.adapt_find(b"", GOOD) == -1 and H.adapt_find(GOOD[:-1], GOOD) == -1 and H.adapt_find(GOOD, GOOD) == 0
    assert H.adapt_find(b"A" * 40, b"A" * 12) == 0
    for bad in BAD_PROBES:
        assert H.lib.hpgq_adapt_find(GOOD, len(GOOD), bad) == -2, bad
    assert H.lib.hpgq_adapt_find(GOOD, len(GOOD), None) == -2
    with pytest.raises(H.HpgqError):
        H.adapt_find(GOOD, b"acgtacgt")


def test_add():
    rng = np.random.default_rng(52)
    dst = rng.integers(0, 1 << 62, size=(5, 40), dtype=np.uint64)
    src = rng.integers(0, 1 << 62, size=(5, 17), dtype=np.uint64)
    want = dst.copy()
    want[:, :17] += src
    got = H.adapt_add(dst.copy(), src)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(H.adapt_add(dst.copy(), np.zeros((5, 0), np.uint64)), dst)
    same = H.adapt_add(dst.copy(), dst)
    np.testing.assert_array_equal(same, dst * np.uint64(2))
    with pytest.raises(H.HpgqError) as e:
        H.adapt_add(src.copy(), dst)
    assert e.value.code == H.E_INVALID
    one = np.zeros(4, np.uint64).ctypes.data_as(C.c_void_p)
    assert H.lib.hpgq_adapt_add(one, 2, one, 2, 33) == -1
    assert H.lib.hpgq_adapt_add(one, -1, one, 0, 1) == -1
    assert H.lib.hpgq_adapt_add(None, 2, one, 2, 1) == -1
    assert H.lib.hpgq_adapt_add(None, 0, None, 0, 1) == 0


def test_default_set():
    assert H.adapt_defaults() == adapt_ref.DEFAULTS
    assert [p for _, p in H.adapt_defaults()] == [b"AGATCGGAAGAG", b"TGGAATTCTCGG", b"GATCGTCGGACT", b"CTGTCTCTTATA",
                                                  b"A" * 12, b"G" * 12]
    assert H.lib.hpgq_adapt_default(99, None, None) == 6 and H.lib.hpgq_adapt_default(0, None, None) == 6


# -- the flag rules and the adapter file, through the CLI (all end before any device call) ------

# (file bytes, what the error line says after <path>:<line>: , the line) -- None: accepted
NAME64 = b"n" * 64
FILES = {
    "plain": (b"one\tAGATCGGAAGAG\ntwo\t\tACGTACGT\n", None, 0),
    "crlf_comments_blank": (b"# adapters\r\n\r\none\tAGATCGGAAGAG\r\n\n#x\tACGT\ntwo\t" + b"ACGT" * 8 + b"\r\n", None, 0),
    "tab_in_name": (b"a\tb \t\tAGATCGGAAGAG\n", None, 0),
    "name64_no_newline": (NAME64 + b"\tAGATCGGAAGAG", None, 0),
    "thirty_two": (b"".join(b"p%d\tAGATCGGAAGAG\n" % i for i in range(32)), None, 0),
    "thirty_three": (b"".join(b"p%d\tAGATCGGAAGAG\n" % i for i in range(33)), "more than 32", 33),
    "empty": (b"", "no adapter", 0),
    "only_comments": (b"# a\n\n# b\n", "no adapter", 3),
    "no_tab": (b"one\tAGATCGGAAGAG\nAGATCGGAAGAG\n", "expected a name", 2),
    "spaces_not_tabs": (b"one AGATCGGAAGAG\n", "expected a name", 1),
    "empty_name": (b"\tAGATCGGAAGAG\n", "name is empty", 1),
    "name65": (NAME64 + b"n\tAGATCGGAAGAG\n", "longer than 64", 1),
    "short_seq": (b"one\tACGTACG\n", "sequence must be", 1),
    "long_seq": (b"one\t" + b"A" * 33 + b"\n", "sequence must be", 1),
    "lower_case": (b"ok\tAGATCGGAAGAG\none\tagatcggaagag\n", "sequence must be", 2),
    "with_N": (b"one\tAGATCNGAAGAG\n", "sequence must be", 1),
    "trailing_tab": (b"one\tAGATCGGAAGAG\t\n", "sequence must be", 1),
    "trailing_space": (b"one\tAGATCGGAAGAG \n", "sequence must be", 1),
}
WANT_SETS = {
    "plain": [(b"one", b"AGATCGGAAGAG"), (b"two", b"ACGTACGT")],
    "crlf_comments_blank": [(b"one", b"AGATCGGAAGAG"), (b"two", b"ACGT" * 8)],
    "tab_in_name": [(b"a\tb ", b"AGATCGGAAGAG")],
    "name64_no_newline": [(NAME64, b"AGATCGGAAGAG")],
    "thirty_two": [(b"p%d" % i, b"AGATCGGAAGAG") for i in range(32)],
}


@pytest.mark.parametrize("name", sorted(FILES))
def test_adapter_file_through_the_cli(tmp_path, name):
    data, what, line = FILES[name]
    path = tmp_path / "adapters.txt"
    path.write_bytes(data)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["stats", "-f", tmp_path / "in.fq", "-o", out, "--print-params", "--adapters", "--adapter-file", path],
                check=False)
    if what is None:
        assert r.returncode == 0 and r.stderr == "", r.stderr
        return
    assert r.returncode == 1 and r.stdout == "" and list(out.iterdir()) == []
    lines = r.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith(f"hpg-fastq: --adapter-file: {path}:{line}: "), r.stderr
    assert what in lines[0]


def test_missing_adapter_file(tmp_path):
    r = run_cli(["stats", "-f", tmp_path / "in.fq", "--print-params", "--adapters", "--adapter-file",
                 tmp_path / "none.txt"], check=False)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.splitlines() == [f"hpg-fastq: --adapter-file: {tmp_path / 'none.txt'}:0: cannot open the file"]


INPUTS = {"se": lambda f: ["-f", f], "pair": lambda f: ["--fq1", f, "--fq2", f + "2"],
          "interleaved": lambda f: ["-f", f, "--interleaved"]}


@pytest.mark.parametrize("inputs", sorted(INPUTS))
def test_option_parses_on_stats_and_changes_no_parameter(tmp_path, inputs):
    files = INPUTS[inputs](str(tmp_path / "in.fq"))
    flags = files + ["--read-quality-range", "20,", "--lmax", "150"]
    (tmp_path / "a.txt").write_bytes(FILES["plain"][0])
    got = print_params("stats", *flags, "--adapters", "--adapter-file", str(tmp_path / "a.txt"), "--adapters-out",
                       str(tmp_path / "dump"))
    assert got == print_params("stats", *flags) == print_params("stats", *flags, "--adapters")
    assert not (tmp_path / "dump").exists()


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]),
                                       ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
def test_option_rejected_on_filter_and_edit(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in (["--adapters"], ["--adapter-file", "x"], ["--adapters-out", "x"]):
        r = run_cli([cmd, "-f", fq, "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        assert r.stderr == f"hpg-fastq: --adapters is an option of the stats command, not of {cmd}\n"
        assert r.stdout == "" and list(out.iterdir()) == []


@pytest.mark.parametrize("extra", [["--adapter-file", "x"], ["--adapters-out", "x"]])
def test_value_flags_need_the_flag(tmp_path, extra):
    r = run_cli(["stats", "-f", tmp_path / "in.fq", "--print-params", *extra], check=False)
    assert r.returncode != 0 and "Error: --adapter-file and --adapters-out need --adapters" in r.stdout


def test_help_shows_the_flags():
    r = run_cli(["stats", "--help"], check=False)
    for flag in ("--adapters ", "--adapter-file=<file>", "--adapters-out=<file>"):
        assert flag in r.stdout, flag
    r = run_cli(["filter", "--help"], check=False)
    assert "--adapter" not in r.stdout


# -- the report writer, the parser and the host entry points under ASan + UBSan ------------------

BIG = (1 << 63) - 5
NAMES32 = [b"probe %d" % i for i in range(32)]
# (base, names, first rows, reads, with_any)
RENDER = [
    ("zero_reads.fq", [n for n, _ in adapt_ref.DEFAULTS], [[0] * 5] * 6, 0, 0),
    ("npos0.fq", [n for n, _ in adapt_ref.DEFAULTS], [[]] * 6, 7, 0),
    ("nothing.fq", [n for n, _ in adapt_ref.DEFAULTS], [[]] * 6, 0, 0),
    ("thirty_two.fq", NAMES32, [[(a * 7 + p * 3) % 11 for p in range(40)] for a in range(32)], 1000, 640),
    ("big.fq", [b"a", b"tab\tin name", b"c d"], [[BIG, 3, 1], [0, BIG, 0], [1, 2, 3]], BIG + 9, BIG + 4),
    ("thirds.fq", [b"x"], [[1, 0, 1, 0, 0, 1]], 3, 3),
    ("one_position.fq", [b"x", b"y"], [[2], [0]], 7, 2),
]


def _want_render(case):
    base, names, rows, reads, with_any = RENDER[case]
    npos = len(rows[0])
    return adapt_ref.render(rows, dict(reads=reads, with_any=with_any, npos=npos), names)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """csrc/hpgq_adapt_post.cpp and host/hpgq_report_adapt.c with their own main
    (nothing loaded into Python), built with ASan + UBSan and run once."""
    tmp = tmp_path_factory.mktemp("adapt_san")
    exe, obj = tmp / "adapt_main", tmp / "adapt_post.o"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hpg-fastq_amd", "host")]
    for cmd in (["g++", *san, "-std=c++17", *inc, "-c", os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_adapt_post.cpp"),
                 "-o", str(obj)],
                ["gcc", *san, "-std=gnu11", "-Wall", *inc, os.path.join(HERE, "sanitize", "adapt_main.c"),
                 os.path.join(ROOT, "hpg-fastq_amd", "host", "hpgq_report_adapt.c"), str(obj), "-o", str(exe),
                 "-lstdc++"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    lines = []
    rng = np.random.default_rng(53)
    probes = adapt_ref.DEFAULT_PROBES + [b"ACGTACGT", b"ACGT" * 8]
    for i in range(60):
        n = int(rng.integers(0, 80))
        s = bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) if i % 2 else bytes(
            np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])
        p = probes[i % len(probes)]
        if i % 3 == 0 and n >= len(p):
            s = s[:n - len(p)] + p                           # ending in the probe: the last window
        lines.append(f"F {s.hex() or '-'} {p.decode()} {s.find(p)}\n")
    lines += [f"F {GOOD.hex()} ACGTACG -2\n", f"F {GOOD.hex()} {'A' * 33} -2\n", f"F - {GOOD.decode()} -1\n",
              f"F {GOOD.hex()} AGATCGGAAGAg -2\n"]
    files = sorted(FILES)
    for name in files:
        (tmp / (name + ".txt")).write_bytes(FILES[name][0])
        lines.append(f"P {tmp / (name + '.txt')}\n")
    for base, names, rows, reads, with_any in RENDER:
        words = [base, reads, with_any, len(names), len(rows[0])] + [n.hex() for n in names] + [x for r in rows for x in r]
        lines.append("R " + " ".join(map(str, words)) + "\n")
    (tmp / "cases.txt").write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp / "cases.txt"), str(tmp)], capture_output=True, text=True, timeout=300, env=env)
    return r, len(lines), tmp, files


def test_host_code_under_asan_ubsan(sanitized):
    r, ncases, _, _ = sanitized
    assert r.returncode == 0 and f"adapt_main: ok {ncases} cases" in r.stdout, r.stdout + r.stderr


def test_parsed_sets(sanitized):
    """What the parser made of every file of FILES: the names and probes in order, or the refusal."""
    r, _, _, files = sanitized
    assert r.returncode == 0, r.stdout + r.stderr
    sets = [ln.split(" ") for ln in r.stdout.splitlines() if ln.startswith("set ")]
    assert len(sets) == len(files)
    for name, words in zip(files, sets):
        if FILES[name][1] is not None:
            assert words[1:] == ["-1", "0"], name
            continue
        got = [(bytes.fromhex(w.split(":")[0]), w.split(":")[1].encode()) for w in words[3:]]
        assert words[1] == "0" and int(words[2]) == len(got) and got == WANT_SETS[name], name
    errors = [ln for ln in r.stderr.splitlines() if ln.startswith("hpg-fastq: --adapter-file: ")]
    assert len(errors) == sum(1 for n in files if FILES[n][1] is not None)


@pytest.mark.parametrize("case", range(len(RENDER)))
def test_rendered_file_bytes(sanitized, case):
    """host/hpgq_report_adapt.c's file against adapt_ref.render: zero reads, npos 0,
    32 probes, counts near 2^63."""
    r, _, tmp, _ = sanitized
    assert r.returncode == 0, r.stdout + r.stderr
    want = _want_render(case)
    assert (tmp / (RENDER[case][0] + ".adapter.content.data")).read_bytes() == want
    assert want.count(b"\n") == 3 + len(RENDER[case][2][0])


def test_reference_by_hand():
    """tests/adapt_ref.py itself on a few reads worked out by hand."""
    seqs = [b"xxAGATCGGAAGAGyyAGATCGGAAGAG", b"AAAAAAAAAAAAAAA", b"AGATCGGAAGA", b"", b"aaaaaaaaaaaa", b"GGGGGGGGGGGGAAAAAAAAAAAA"]
    idx = np.cumsum([0] + [len(s) for s in seqs])
    first, info = adapt_ref.table(np.frombuffer(b"".join(seqs), np.uint8), idx, adapt_ref.DEFAULT_PROBES)
    assert info == dict(reads=6, with_any=3, nprobes=6, npos=28)
    want = np.zeros((6, 28), np.uint64)
    want[0, 2] = 1
    want[4, 0] = 1
    want[4, 12] = 1
    want[5, 0] = 1
    np.testing.assert_array_equal(first, want)
    first, info = adapt_ref.table(np.frombuffer(b"".join(seqs), np.uint8), idx, adapt_ref.DEFAULT_PROBES, [0, 1, 2, 1, 0, 0])
    assert info == dict(reads=2, with_any=1, nprobes=6, npos=15) and int(first.sum()) == first[4, 0] == 1
    text = adapt_ref.render([[1, 0, 1]], dict(reads=3, with_any=2, npos=3), [b"x"])
    assert text == b"# Reads\tWith adapter\t% with adapter\n3\t2\t66.67\n# Position\tx\n1\t33.3333\n2\t33.3333\n3\t66.6667\n"
    assert adapt_ref.render([[]], dict(reads=0, with_any=0, npos=0), [b"x"]) == (
        b"# Reads\tWith adapter\t% with adapter\n0\t0\t0.00\n# Position\tx\n")
