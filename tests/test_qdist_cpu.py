"""`stats --quality-dist` without a GPU: the host-only half of
the C-ABI (hpgq_qdist_quantiles, hpgq_qdist_add) against tests/qdist_ref.py
and hand-derived answers, the option rules, the argument checks of
hpgq_qdist_open, and the same host code under ASan + UBSan in a stand-alone
program (tests/sanitize/qdist_main.c)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hpgfastq as H
import qdist_ref
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KAT = json.load(open(os.path.join(HERE, "golden", "qdist_kat.json")))["cases"]


def _row(counts):
    r = np.zeros(256, dtype=np.uint64)
    for b, c in counts.items():
        r[int(b)] = c
    return r


def _check(hist, phred):
    got = H.qdist_quantiles(hist, phred)
    assert got.shape == (hist.shape[0], 8) and got.dtype == np.int64
    want = qdist_ref.quantiles(hist, phred)
    for p in range(hist.shape[0]):
        g = [int(got[p, 0]) % (1 << 64)] + [int(x) for x in got[p, 1:]]   # (count: u64 in an int64 column)
        assert g == want[p], (p, g, want[p])


def _random_table(rng, npos, dense):
    if dense:
        h = rng.integers(0, 1 << 40, size=(npos, 256), dtype=np.uint64)
    else:
        h = np.zeros((npos, 256), dtype=np.uint64)
        for p in range(npos):
            k = int(rng.integers(0, 6))   # 0: an empty row
            cols = rng.integers(0, 256, size=k)
            h[p, cols] = rng.integers(1, 1000, size=k, dtype=np.uint64)
    return h


@pytest.mark.parametrize("phred", [33, 64])
@pytest.mark.parametrize("npos,dense", [(1, False), (1, True), (7, False), (150, True), (300, False), (300, True)])
def test_quantiles_random_tables(npos, dense, phred):
    rng = np.random.default_rng(1000 * npos + phred + dense)
    _check(_random_table(rng, npos, dense), phred)


@pytest.mark.parametrize("phred", [33, 64])
def test_quantiles_rank_arithmetic_and_signed_order(phred):
    """One cell of 2^63 (9 * c overflows u64), row sums near 2^64, c = 0 and
    c = 1, and all mass on 0x80 or 0xFF (the signed order's two ends)."""
    h = np.zeros((9, 256), dtype=np.uint64)
    h[0, 40] = 1 << 63
    h[1, 40] = 1 << 63
    h[1, 0x90] = (1 << 63) - 1            # c = 2^64 - 1, most of it on a negative byte
    h[2, 200] = (1 << 63) + 12345
    h[2, 10] = 3
    # row 3: c = 0
    h[4, 0x21] = 1                        # c = 1
    h[5, 0x80] = 7                        # all on the smallest signed byte
    h[6, 0xFF] = 7                        # all on -1
    h[7, 0x80] = 1
    h[7, 0x7F] = 1                        # the two ends of the order
    h[8, :] = (1 << 56) - 1               # every byte, c = 2^64 - 256
    _check(h, phred)
    got = H.qdist_quantiles(h, phred)
    assert list(got[3]) == [0] * 8
    assert list(got[5][1:]) == [-128 - phred] * 7 and list(got[6][1:]) == [-1 - phred] * 7
    assert got[7][1] == -128 - phred and got[7][7] == 127 - phred


@pytest.mark.parametrize("case", range(len(KAT)))
def test_quantiles_known_answers(case):
    k = KAT[case]
    h = _row(k["counts"]).reshape(1, 256)
    assert [int(x) for x in H.qdist_quantiles(h, k["phred"])[0]] == k["want"], k["why"]
    assert qdist_ref.quantile_row(h[0], k["phred"]) == k["want"], k["why"]


def test_kat_file_has_a_negative_byte_case():
    assert len(KAT) >= 5 and any(int(b) >= 128 for k in KAT for b in k["counts"])


def test_qdist_add():
    rng = np.random.default_rng(5)
    dst = rng.integers(0, 1 << 62, size=(9, 256), dtype=np.uint64)
    src = rng.integers(0, 1 << 62, size=(4, 256), dtype=np.uint64)
    want = dst.copy()
    want[:4] += src
    out = H.qdist_add(dst, src)
    assert out is dst
    np.testing.assert_array_equal(dst, want)           # the first rows added, the rest untouched
    np.testing.assert_array_equal(want, qdist_ref.add([want - 0, np.zeros((2, 256), np.uint64)]))
    with pytest.raises(H.HpgqError) as e:              # npos_src > npos_dst
        H.qdist_add(src, dst)
    assert e.value.code == -1
    np.testing.assert_array_equal(H.qdist_add(dst, np.zeros((0, 256), np.uint64)), want)
    assert H.lib.hpgq_qdist_add(None, 3, None, 2) == -1
    assert H.lib.hpgq_qdist_quantiles(None, 2, 33, None) == -1


def test_reference_table_by_hand():
    """tests/qdist_ref.py itself on three reads worked out by hand."""
    qual = np.frombuffer(b"xxIJ!5\xff", dtype=np.uint8)   # two bytes before the first read
    idx = np.array([2, 4, 4, 7], dtype=np.int32)          # "IJ", "", "!5\xff"
    t = qdist_ref.table(qual, idx)
    assert t.shape == (3, 256) and int(t.sum()) == 5
    assert t[0, ord("I")] == 1 and t[0, ord("!")] == 1 and t[1, ord("J")] == 1 and t[1, ord("5")] == 1
    assert t[2, 255] == 1
    t = qdist_ref.table(qual, idx, np.array([1, 1, 0], np.uint8))
    assert t.shape == (2, 256) and int(t.sum()) == 2
    assert qdist_ref.table(qual, idx, np.zeros(3, np.uint8)).shape == (0, 256)
    assert qdist_ref.render(t, 33) == qdist_ref.HEADER + b"1\t1\t40\t40\t40\t40\t40\t40\t40\n" \
        b"2\t1\t41\t41\t41\t41\t41\t41\t41\n"


def test_open_argument_checks():
    h = C.c_void_p()
    for rows, base in ((0, 33), (-1, 33), (150, 193), (150, -1)):
        assert H.lib.hpgq_qdist_open(C.byref(h), 0, rows, base, None) == -1, (rows, base)
    assert H.lib.hpgq_qdist_open(None, 0, 150, 33, None) == -1
    for fn in (H.lib.hpgq_qdist_sync, H.lib.hpgq_qdist_reset):
        assert fn(None) == -1
    assert H.lib.hpgq_qdist_reserve_length(None, 10) == -1
    assert H.lib.hpgq_qdist_debug_set_max_workgroups(None, 2) == -1
    assert H.lib.hpgq_qdist_count_device(None, None, None) == -1
    assert H.lib.hpgq_qdist_read(None, None, 0, None) == -1
    H.lib.hpgq_qdist_close(None)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device path")
def test_open_fails_loudly_without_device():
    for base in (0, 33, 192):
        with pytest.raises(H.HpgqError) as e:
            H.QualityDist(150, base=base)
        assert e.value.code == -5


INPUTS = {"se": lambda f: ["-f", f], "pair": lambda f: ["--fq1", f, "--fq2", f + "2"],
          "interleaved": lambda f: ["-f", f, "--interleaved"]}


@pytest.mark.parametrize("inputs", sorted(INPUTS))
def test_option_parses_on_stats_and_changes_no_parameter(tmp_path, inputs):
    files = INPUTS[inputs](str(tmp_path / "in.fq"))
    flags = files + ["--read-quality-range", "20,", "--lmax", "150", "--quality-encoding", "phred64"]
    assert print_params("stats", *flags, "--quality-dist") == print_params("stats", *flags)
    assert print_params("stats", *flags, "--quality-dist", "--quality-dist-out", str(tmp_path / "q.bin")) == \
        print_params("stats", *flags)


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]),
                                       ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
def test_option_rejected_on_filter_and_edit(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    for extra in (["--quality-dist"], ["--quality-dist-out", str(tmp_path / "q.bin")]):
        r = run_cli([cmd, "-f", fq, "-o", out, *flags, *extra], check=False)
        assert r.returncode == 1
        assert len(r.stderr.strip().splitlines()) == 1 and "--quality-dist" in r.stderr
        assert r.stdout == "" and list(out.iterdir()) == [] and not (tmp_path / "q.bin").exists()


def test_help_shows_the_flags():
    r = run_cli(["stats", "--help"], check=False)
    assert "--quality-dist " in r.stdout and "--quality-dist-out=<file>" in r.stdout
    r = run_cli(["filter", "--help"], check=False)
    assert "--quality-dist" not in r.stdout


def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/hpgq_qdist_post.cpp with its own main (nothing loaded into Python):
    the known answers, the 2^63 cell and full-range rows, and hpgq_qdist_add."""
    exe = tmp_path / "qdist_main"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "include")]
    obj = tmp_path / "qdist_post.o"
    for cmd in (["g++", *san, "-std=c++17", *inc, "-c", os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_qdist_post.cpp"),
                 "-o", str(obj)],
                ["gcc", *san, "-std=gnu11", "-Wall", *inc, os.path.join(HERE, "sanitize", "qdist_main.c"), str(obj),
                 "-o", str(exe), "-lstdc++"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    cases = [(k["phred"], {int(b): c for b, c in k["counts"].items()}) for k in KAT]
    big = 1 << 63
    cases += [(33, {40: big}), (64, {40: big, 0x90: big - 1}), (33, {200: big + 12345, 10: 3}),
              (33, {b: (1 << 56) - 1 for b in range(256)}), (33, {0x80: 1, 0x7F: 1})]
    lines = []
    for phred, counts in cases:
        want = qdist_ref.quantile_row(_row(counts), phred)
        cells = " ".join(f"{b} {c}" for b, c in counts.items())
        lines.append(f"{phred} {len(counts)} {cells} {' '.join(map(str, want))}\n")
    (tmp_path / "cases.txt").write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"qdist_main: ok {len(cases)} cases" in r.stdout, r.stdout + r.stderr
