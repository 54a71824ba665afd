"""`edit --merge-overlap` without a GPU: hpgq_ovl_merge against
tests/ovl_merge_ref.py on the edge list, on random pairs and on planted
disagreements, hand-checked cases for each of the three ranges, the -2 and 0
returns, the property that merging a corrected pair gives the bytes of merging
the pair itself, the flag rules through the CLI, and the host function under
ASan + UBSan in a stand-alone program (tests/sanitize/ovl_merge_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hpgfastq as H
import ovl_ref as R
import ovl_fix_ref as X
import ovl_merge_ref as G
from cli_lib import run_cli, print_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

THRESHOLDS = [(33, 30, 14), (33, 1, 0), (33, 93, 92), (64, 30, 14), (33, 20, 19)]


def _qual(rng, n, hostile):
    if hostile:
        return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
    return bytes(rng.integers(33, 75, size=n, dtype=np.uint8))


def _with_quals(pairs, seed, hostile=False):
    rng = np.random.default_rng(seed)
    return [(a, _qual(rng, len(a), hostile), b, _qual(rng, len(b), hostile)) for a, b in pairs]


def _planted():
    return X.position_pairs() + X.byte_pairs() + X.threshold_pairs(33, 30, 14) + X.several_pairs(30, 5) + G.tie_pairs()


def _check(p, F):
    want = G.merge(*p, F)
    assert H.ovl_merge(*p, F) == want, (p, F)
    return want


def test_merge_against_reference_edges_and_random():
    merged = resolved = 0
    for mo, M in ((8, 0), (30, 5)):
        pairs = [(a, b) for a, b in R.edge_pairs(mo, M) if len(a) <= 512 and len(b) <= 512]
        for hostile in (False, True):
            for p in _with_quals(pairs, 51 + mo, hostile):
                F = R.find(p[0], p[2], mo, M)
                want = _check(p, F)
                merged += F > 0
                resolved += sum(want[2])
    for hostile in (False, True):
        for p in _with_quals(R.random_pairs(800, 52), 53, hostile):
            F = R.find(p[0], p[2], 30, 5)
            want = _check(p, F)
            merged += F > 0
            resolved += sum(want[2])
    assert merged > 1000 and resolved > 500


def test_merge_planted_disagreements():
    both = [0, 0]
    for p in _planted():
        F = R.find(p[0], p[2], 30, 5)
        assert F > 0
        m, qm, res = _check(p, F)
        both = [a + b for a, b in zip(both, res)]
    assert min(both) > 300


def test_ties_and_losers_by_hand():
    """tie_pairs' first rows, worked out: who wins and with which quality byte."""
    pairs = G.tie_pairs()
    for i, (wq, lq) in enumerate(((60, 60), (61, 60), (0, 0), (255, 255), (255, 254), (1, 0), (128, 127))):
        for winner, p in ((1, pairs[i]), (2, pairs[17 + i])):
            off = 7 + (i if winner == 1 else 17 + i)
            m, qm, res = G.merge(*p, 70)
            assert H.ovl_merge(*p, 70) == (m, qm, res)
            j = 69 - off
            if winner == 1 or wq == lq:            # mate 1's base stays: the planted winner, or the tie
                assert m[off] == p[0][off] and qm[off] == p[1][off] and res == [1, 0]
            else:
                assert m[off] == R.COMP[p[2][j]] and qm[off] == wq and res == [0, 1]


def test_three_ranges_by_hand():
    """The reference itself, and the library, on pairs worked out by hand."""
    for f in (G.merge, H.ovl_merge):
        # F > n1, n2: mate 1's head, 8 facing positions, the reverse complement of mate 2's head
        s1, q1 = b"ACGTACGTAA", b"0123456789"
        s2, q2 = b"GGTTACGTAC", b"abcdefghij"          # rc(s2) = GTACGTAACC: F = 12, lo = 2, hi = 10
        assert R.find(s1, s2, 8, 0) == 12
        assert f(s1, q1, s2, q2, 12) == (b"ACGTACGTAACC", b"01jihgfedcba", [0, 0])
        # a read-through: F < n1, n2, every position faces; one disagreement each way and a tie
        s1, q1 = b"ACGTACGTACGG", b"IIIIIIIIIIII"
        s2, q2 = b"GTACGTACGTTT", b"5555J5555I55"      # rc(s2[:10]) = ACGTACGTAC
        assert R.find(s1, s2, 8, 0) == 10
        assert f(s1, q1, s2, q2, 10) == (b"ACGTACGTAC", b"IIIIIJIIII", [0, 0])
        bad1 = b"ACGTAGGTAC"                            # p = 5: G against rc = C
        assert f(bad1 + b"GG", q1, s2, q2, 10) == (b"ACGTACGTAC", b"IIIIIJIIII", [0, 1])      # Q2 = J > I
        assert f(bad1 + b"GG", q1, s2, b"5555I5555I55", 10) == (b"ACGTAGGTAC", b"IIIIIIIIII", [1, 0])   # a tie
        assert f(bad1 + b"GG", q1, s2, b"5555H5555I55", 10) == (b"ACGTAGGTAC", b"IIIIIIIIII", [1, 0])
        # N in mate 1 loses to a base at any quality; N against N keeps mate 1's
        assert f(b"ACGTANGTACGG", q1, s2, b"555505555I55", 10) == (b"ACGTACGTAC", b"IIIII0IIII", [0, 1])
        assert f(b"ACGTANGTACGG", q1, b"GTACNTACGTTT", q2, 10) == (b"ACGTANGTAC", b"IIIIIIIIII", [1, 0])
        # F = n1 = n2 with a non-base outside the facing range of a longer F: rc(N) = N, rc(a) = a
        s1, q1 = b"ACGTACGTAAGG", b"0123456789AB"
        s2, q2 = b"NaCCTTACGTAC", b"abcdefghijkl"      # rc tail: ...GGtN -> "GTACGTAAGG" + "aN"
        assert R.find(s1, s2, 8, 0) == 14              # lo = 2, hi = 12
        assert f(s1, q1, s2, q2, 14) == (b"ACGTACGTAAGGaN", b"01lkjihgfedcba", [0, 0])


def test_returns():
    s, q = b"ACGTACGTACGT", b"IIIIIIIIIIII"
    out = C.create_string_buffer(64)
    res = (C.c_uint32 * 2)(9, 9)
    f = H.lib.hpgq_ovl_merge
    for F in (0, -1, -5):
        out.raw = b"\xA5" * 64
        assert f(s, q, 12, s, q, 12, F, out, out, res) == 0 and out.raw == b"\xA5" * 64 and list(res) == [0, 0]
        assert H.ovl_merge(s, q, s, q, F) == (b"", b"", [0, 0])
    assert f(None, None, 0, None, None, 0, 0, None, None, None) == 0
    # a NULL with bytes
    for args in ((None, q, 12, s, q, 12), (s, None, 12, s, q, 12), (s, q, 12, None, q, 12), (s, q, 12, s, None, 12)):
        assert f(*args, 12, out, out, res) == -2
    assert f(s, q, 12, s, q, 12, 12, None, out, res) == -2 and f(s, q, 12, s, q, 12, 12, out, None, res) == -2
    # an F that §2.13 cannot return for these lengths: fewer than 8 facing bytes, a mate of 513 bases
    assert f(s, q, 12, s, q, 12, 7, out, out, res) == -2 and f(s, q, 12, s, q, 12, 17, out, out, res) == -2
    assert f(s, q, 12, s, q, 12, 8, out, out, res) == 8 and f(s, q, 12, s, q, 12, 16, out, out, res) == 16
    long = b"A" * 513
    assert f(long, long, 513, s, q, 12, 12, out, out, res) == -2 and f(s, q, 12, long, long, 513, 12, out, out, res) == -2
    assert f(long, long, 513, s, q, 12, 0, out, out, res) == 0
    with pytest.raises(H.HpgqError):
        H.ovl_merge(s, q, s, q, 7)
    with pytest.raises(ValueError):
        H.ovl_merge(s, q[:5], s, q, 12)
    # the longest: two mates of 512 at F = 1016
    rng = np.random.default_rng(7)
    a, b = R.pair_of(rng, 512, 512, 1016)
    qa, qb = _qual(rng, 512, True), _qual(rng, 512, True)
    assert H.ovl_merge(a, qa, b, qb, 1016) == G.merge(a, qa, b, qb, 1016)
    with pytest.raises(H.HpgqError):
        H.ovl_merge(a, qa, b, qb, 1017)


def _hostile_pairs(n, seed):
    """Pairs from a fragment with hostile bytes and disagreements strewn over both mates, quality bytes 0 .. 255."""
    rng = np.random.default_rng(seed)
    out = []
    hostile = np.frombuffer(b"NnacgtACGT\x00\xff\x20", np.uint8)
    for i in range(n):
        n1, n2 = int(rng.integers(30, 120)), int(rng.integers(30, 120))
        F = int(rng.integers(30, n1 + n2 - 29))
        s1, s2 = (bytearray(x) for x in R.pair_of(rng, n1, n2, F))
        for s in (s1, s2):
            for _ in range(int(rng.integers(0, 4))):
                s[int(rng.integers(0, len(s)))] = int(hostile[rng.integers(0, len(hostile))])
        if i % 3 == 0:
            q1, q2 = _qual(rng, n1, True), _qual(rng, n2, True)
        else:                                           # qualities round the thresholds, so that corrections fire
            q1 = bytes(rng.choice([33, 34, 47, 48, 53, 63, 73, 126, 64, 65, 78, 94], size=n1).astype(np.uint8))
            q2 = bytes(rng.choice([33, 34, 47, 48, 53, 63, 73, 126, 64, 65, 78, 94], size=n2).astype(np.uint8))
        out.append((bytes(s1), q1, bytes(s2), q2))
    return out


def test_merging_a_corrected_pair_changes_nothing():
    """§2.15: the merge reads the inputs.  merge(correct(pair)) == merge(pair) for every threshold set."""
    pairs = _hostile_pairs(1500, 61) + _planted()
    changed = merged = 0
    for p in pairs:
        F = R.find(p[0], p[2], 30, 12)
        if F <= 0:
            continue
        merged += 1
        want = G.merge(*p, F)
        for th in THRESHOLDS:
            c = X.correct(*p, F, *th)
            changed += sum(c[4])
            got = G.merge(*c[:4], F)
            assert got[:2] == want[:2], (p, F, th)
            assert H.ovl_merge(*c[:4], F)[:2] == want[:2]
    assert merged > 1000 and changed > 2000


def test_compacted_reference_by_hand():
    """ovl_merge_ref.Merged and render on three pairs: a self-check of the
    reference (the GPU and CLI tests compare the product with both), which
    needs no product code."""
    import oracle_lib as O
    rng = np.random.default_rng(3)
    a = R.pair_of(rng, 40, 40, 35)
    b = (R.acgt(rng, 20), R.acgt(rng, 25))
    c = R.pair_of(rng, 50, 60, 100)

    def reads(seqs):
        idx = np.zeros(len(seqs) + 1, np.int32)
        idx[1:] = np.cumsum([len(s) for s in seqs])
        flat = np.frombuffer(b"".join(seqs), np.uint8)
        return O.Reads(flat, np.full(len(flat), 73, np.uint8), idx)

    w = G.Merged(reads([a[0], b[0], c[0]]), reads([a[1], b[1], c[1]]), 8, 0)
    assert w.insert.tolist() == [35, 0, 100]
    assert w.merged.idx.tolist() == [0, 35, 135] and w.out[0].idx.tolist() == [0, 20] and w.out[1].idx.tolist() == [0, 25]
    assert bytes(w.out[0].seq) == b[0] and bytes(w.out[1].seq) == b[1]
    assert bytes(w.merged.seq[:35]) == a[0][:35] and bytes(w.merged.seq[35:85]) == c[0]
    assert bytes(w.merged.seq[85:]) == R.revcomp(c[1])[10:]
    assert w.merge == dict(merged_pairs=2, merged_bases=135, resolved=[0, 0])
    assert w.hist[[0, 35, 100]].tolist() == [1, 1, 1]
    assert G.render(w.info, w.merge) == (b"# Pairs\tOverlapping\tMerged\t% merged\tMerged bases\tResolved by mate 1\tResolved by mate 2\n"
                                         b"3\t2\t2\t66.67\t135\t0\t0\n")
    z = dict(pairs=0, overlapping=0)
    assert G.render(z, G.info_of([], [0, 0])).endswith(b"\n0\t0\t0\t0.00\t0\t0\t0\n")


def test_null_handle_and_arguments():
    b = H.Batch()
    assert H.lib.hpgq_ovl_merge_device(None, C.byref(b), C.byref(b), C.byref(b), C.byref(b), C.byref(b)) == -1
    assert H.lib.hpgq_ovl_read_merge(None, None) == -1
    # the ctx on a caller's stream: a NULL stream is refused before any device call
    h = C.c_void_p()
    assert H.lib.hpgq_open_on_stream(C.byref(h), 0, C.byref(H.stats_params(lmax=100)), None) == -1 and not h.value


# -- the flag rules, through the CLI (all end before any device call) ----------------------------

EDIT = ["--left-length", "5", "--left-quality-range", "20,"]


@pytest.mark.parametrize("cmd,flags", [("filter", ["--read-quality-range", "20,"]), ("stats", [])])
def test_flag_rejected_on_stats_and_filter(tmp_path, cmd, flags):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r/1\nACGT\n+\nIIII\n@r/2\nACGT\n+\nIIII\n")
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli([cmd, "-f", fq, "--interleaved", "-o", out, *flags, "--merge-overlap"], check=False)
    assert r.returncode == 1
    assert r.stderr == f"hpg-fastq: --merge-overlap is an option of the edit command, not of {cmd}\n"
    assert r.stdout == "" and list(out.iterdir()) == []


def test_flag_needs_clip_overlap(tmp_path):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, "--merge-overlap"], check=False)
    assert r.returncode == 1 and "\nError: --merge-overlap needs --clip-overlap\n" in r.stdout and "Usage:" in r.stdout


def test_flag_excludes_the_correction(tmp_path):
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "--print-params", *EDIT, "--clip-overlap", "--merge-overlap",
                 "--correct-overlap"], check=False)
    assert r.returncode == 1
    assert ("\nError: --merge-overlap makes --correct-overlap void: a merged read is the same with and without it\n"
            in r.stdout)


def test_flag_parses_on_edit_and_changes_no_parameter(tmp_path):
    flags = ["-f", str(tmp_path / "in.fq"), "--interleaved", *EDIT, "--read-quality-range", "20,", "--lmax", "150"]
    plain = print_params("edit", *flags, "--clip-overlap")
    assert print_params("edit", *flags, "--clip-overlap", "--merge-overlap") == plain
    assert print_params("edit", *flags, "--clip-overlap", "--merge-overlap", "--insert-size", "--clip-adapters") == plain
    help_ = run_cli(["edit", "--help"], check=False).stdout
    assert "--merge-overlap " in help_
    for cmd in ("stats", "filter"):
        assert "--merge-overlap" not in run_cli([cmd, "--help"], check=False).stdout


# -- the host function under ASan + UBSan ----------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/hpgq_ovl_post.cpp with its own main, the outputs heap blocks of
    exactly F bytes: nothing loaded into Python."""
    exe = tmp_path / "ovl_merge_main"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    r = subprocess.run(["g++", *san, "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(HERE, "sanitize", "ovl_merge_main.cpp"),
                        os.path.join(ROOT, "hpg-fastq_amd", "csrc", "hpgq_ovl_post.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    hexed = lambda b: b.hex() or "-"    # noqa: E731
    lines = []
    rng = np.random.default_rng(71)
    cases = _with_quals(R.edge_pairs(8, 0, 6), 72, True) + _with_quals(R.random_pairs(400, 73), 74, True) + _planted()
    a, b = R.pair_of(rng, 512, 512, 1016)
    cases.append((a, _qual(rng, 512, True), b, _qual(rng, 512, True)))
    for p in cases:
        if len(p[0]) > 20000:
            continue
        F = R.find(p[0], p[2], 8, 0)
        if F == -1:                                     # a skipped pair: F <= 0 returns 0, an F > 0 is refused
            lines.append(f"{hexed(p[0])} {hexed(p[1])} {hexed(p[2])} {hexed(p[3])} -1 0 - - 0 0")
            lines.append(f"{hexed(p[0])} {hexed(p[1])} {hexed(p[2])} {hexed(p[3])} 40 -2 - - 0 0")
            continue
        m, qm, res = G.merge(*p, F)
        lines.append(f"{hexed(p[0])} {hexed(p[1])} {hexed(p[2])} {hexed(p[3])} {F} {max(F, 0)} {hexed(m)} {hexed(qm)} {res[0]} {res[1]}")
    # an F with fewer than 8 facing bytes
    lines.append(f"{hexed(b'ACGTACGTAC')} {hexed(b'IIIIIIIIII')} {hexed(b'GTACGTACGT')} {hexed(b'IIIIIIIIII')} 13 -2 - - 0 0")
    assert sum(" -2 " in x for x in lines) >= 3 and len(lines) > 1500
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"ovl_merge_main: ok {len(lines)} cases" in r.stdout, r.stdout + r.stderr
