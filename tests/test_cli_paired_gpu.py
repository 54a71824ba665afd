"""Paired-end input through the C host CLI on the GPU: --fq1/--fq2 and
--interleaved for stats | filter | edit, against the oracle with paired = 1 on
the same mates (counters, every report file, all four output files), and the
pairing errors.  The mates differ in length and in bytes per record, so the
chunk cuts of the two files fall at different records."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import cli_lib

pytestmark = pytest.mark.gpu


def run_cli(args, **kw):
    """One GPU unless the test says otherwise: the page-locked chunk buffers
    (two texts per chunk) are sized per worker."""
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


STREAM_LINE = "writer: one stream writer thread"
FILTER = ["--read-quality-range", "20,", "--read-length-range", "50,"]
EDIT = ["--left-length", 10, "--left-quality-range", "20,", "--right-length", 30, "--right-quality-range", "20,",
        "--read-length-range", "60,"]


def _mates(n, seed):
    """Independent seeds; mate 2 alone is truncated (30 %), so the mates' lengths differ."""
    return O.synth(n, seed=seed, L=150), O.synth(n, seed=seed + 100, L=150, trunc_pct=30)


def _write_pair(tmp_path, r1, r2, crlf=False, fat=2, names=("in_1.fq", "in_2.fq")):
    """The mate files; the `fat` mate repeats its header on the '+' line (about
    1.3 x the bytes per record).  Returns the paths and the records."""
    rec1 = PL.records(r1, PL.mate_headers(r1.n, 1), crlf=crlf, plus_header=fat == 1)
    rec2 = PL.records(r2, PL.mate_headers(r2.n, 2), crlf=crlf, plus_header=fat == 2)
    f1, f2 = tmp_path / names[0], tmp_path / names[1]
    f1.write_bytes(b"".join(rec1))
    f2.write_bytes(b"".join(rec2))
    return str(f1), str(f2), rec1, rec2


def _trimmed(rec, t):
    """An edit output record: header and '+' line as read, sequence and quality trimmed."""
    h, s, plus, q = rec.split(b"\n")[:4]
    ts, te = int(t) & 0xFFFF, int(t) >> 16
    return h + b"\n" + s[ts:len(s) - te] + b"\n" + plus + b"\n" + q[ts:len(q) - te] + b"\n"


def _expected_files(cmd, p, r1, r2, rec1, rec2):
    """The four output files, assembled from the oracle's mask and both halves of its trims."""
    mask, trim, _ = O.run(p, r1, r2)
    n = r1.n
    out = {}
    for m, recs in enumerate((rec1, rec2)):
        if cmd == "edit":
            recs = [_trimmed(r, trim[m * n + i]) for i, r in enumerate(recs)]
        ok = "edit" if cmd == "edit" else "passed"
        out[f"{ok}_{m + 1}.fq"] = b"".join(r for r, k in zip(recs, mask) if k)
        out[f"failed_{m + 1}.fq"] = b"".join(r for r, k in zip(recs, mask) if not k)
    return out


def _check_files(d, want):
    for name, data in want.items():
        assert (d / name).read_bytes() == data, name
    for m in (1, 2):   # pair i is in the _1 file of a class iff it is in its _2 file
        for cls in [n[:-5] for n in want if n.endswith("_1.fq")]:
            assert (d / f"{cls}_1.fq").read_bytes().count(b"\n") == (d / f"{cls}_{m}.fq").read_bytes().count(b"\n")


@pytest.fixture(scope="module")
def stats_mates():
    r1, r2 = _mates(20000, 51)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    _, _, want = O.run(p, r1, r2)
    return r1, r2, want


@pytest.mark.parametrize("fat", [2, 1])
@pytest.mark.parametrize("chunk_mb", [1, 256])
def test_cli_paired_stats(tmp_path, stats_mates, chunk_mb, fat):
    from oracle import report_ref
    r1, r2, want = stats_mates
    f1, f2, _, _ = _write_pair(tmp_path, r1, r2, fat=fat)
    out = tmp_path / "out"
    out.mkdir()
    ctr = tmp_path / "ctr.bin"
    r = run_cli(["stats", "--fq1", f1, "--fq2", f2, "-o", out, *FILTER, "--lmax", 150, "--chunk-mb", chunk_mb,
                 "--counters-out", ctr])
    assert "Throughput: 20000 pairs" in r.stdout and "in_2.fq" in r.stdout   # the results block
    got = np.fromfile(ctr, np.uint64)
    np.testing.assert_array_equal(got, want)   # mate 1's set, then mate 2's
    n = H.counters_len(150)
    names = set()
    for m, base in enumerate(("in_1.fq", "in_2.fq")):
        exp = report_ref.report_files(got[m * n:(m + 1) * n], 150, 33, base,
                                      {"filter_on": True, "read_quality_range": "20,", "read_length_range": "50,"})
        for suffix, data in exp.items():
            assert (out / f"{base}.{suffix}").read_bytes() == data, (base, suffix)
            names.add(f"{base}.{suffix}")
    assert {p.name for p in out.iterdir()} == names


@pytest.mark.parametrize("crlf", [False, True])
def test_cli_paired_filter_outputs(tmp_path, crlf):
    r1, r2 = _mates(15000, 52)
    f1, f2, rec1, rec2 = _write_pair(tmp_path, r1, r2, crlf=crlf)
    r = run_cli(["filter", "--fq1", f1, "--fq2", f2, "-o", tmp_path, *FILTER, "--max-N", 1, "--chunk-mb", 1, "--quiet"],
                env={"HPGQ_TRACE": "1"})
    assert STREAM_LINE in r.stderr, r.stderr[-2000:]
    p = PL.paired(H.filter_params(lmax=1024, read_quality_range="20,", read_length_range="50,", max_N=1))
    want = _expected_files("filter", p, r1, r2, rec1, rec2)
    assert 0 < len(want["failed_1.fq"]) and 0 < len(want["passed_1.fq"])
    _check_files(tmp_path, want)


def test_cli_paired_edit_outputs(tmp_path):
    r1, r2 = _mates(12000, 53)
    f1, f2, rec1, rec2 = _write_pair(tmp_path, r1, r2)
    r = run_cli(["edit", "--fq1", f1, "--fq2", f2, "-o", tmp_path, *EDIT, "--chunk-mb", 1, "--quiet"],
                env={"HPGQ_TRACE": "1"})
    assert STREAM_LINE in r.stderr, r.stderr[-2000:]
    p = PL.paired(H.edit_params(lmax=1024, left_length=10, left_quality_range="20,", right_length=30,
                                right_quality_range="20,", read_length_range="60,"))
    _check_files(tmp_path, _expected_files("edit", p, r1, r2, rec1, rec2))


@pytest.mark.parametrize("cmd", ["stats", "filter", "edit"])
def test_cli_interleaved_equals_two_files(tmp_path, cmd):
    """The same mates as one interleaved file: counters and outputs identical to the two-file run."""
    r1, r2 = _mates(12000, 54)
    f1, f2, rec1, rec2 = _write_pair(tmp_path, r1, r2)
    fi = tmp_path / "inter.fq"
    fi.write_bytes(PL.interleave(rec1, rec2))
    flags = {"stats": FILTER + ["--lmax", 150], "filter": FILTER, "edit": EDIT}[cmd]
    dirs = []
    for form, inputs in (("two", ["--fq1", f1, "--fq2", f2]), ("inter", ["--interleaved", "-f", fi])):
        d = tmp_path / form
        d.mkdir()
        run_cli([cmd, *inputs, "-o", d, *flags, "--chunk-mb", 1, "--counters-out", tmp_path / f"{form}.bin", "--quiet"])
        dirs.append(d)
    two, inter = dirs
    np.testing.assert_array_equal(np.fromfile(tmp_path / "two.bin", np.uint64),
                                  np.fromfile(tmp_path / "inter.bin", np.uint64))
    if cmd == "stats":
        p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
        _, _, want = O.run(p, r1, r2)
        np.testing.assert_array_equal(np.fromfile(tmp_path / "inter.bin", np.uint64), want)
        # the report sets are named <base>_1 / <base>_2 and hold what the two-file run's hold
        for m in (1, 2):
            for f in sorted(two.glob(f"in_{m}.fq.*")):
                a = f.read_bytes().replace(f"in_{m}.fq".encode(), b"NAME")
                b = (inter / f.name.replace(f"in_{m}.fq", f"inter.fq_{m}")).read_bytes()
                assert a == b.replace(f"inter.fq_{m}".encode(), b"NAME"), f.name
        assert len(list(inter.iterdir())) == len(list(two.iterdir())) == 14
    else:
        names = sorted(p.name for p in two.iterdir())
        assert names == sorted(p.name for p in inter.iterdir()) and len(names) == 4
        for n in names:
            assert (two / n).read_bytes() == (inter / n).read_bytes(), n
        p = (PL.paired(H.filter_params(lmax=1024, read_quality_range="20,", read_length_range="50,"))
             if cmd == "filter" else
             PL.paired(H.edit_params(lmax=1024, left_length=10, left_quality_range="20,", right_length=30,
                                     right_quality_range="20,", read_length_range="60,")))
        _check_files(inter, _expected_files(cmd, p, r1, r2, rec1, rec2))


@pytest.mark.parametrize("cmd", ["stats", "filter", "edit"])
def test_cli_paired_workers_merge(tmp_path, cmd):
    """--gpus 1 --gpu-workers 3 gives the counters and files of one worker."""
    r1, r2 = _mates(30000, 55)
    f1, f2, _, _ = _write_pair(tmp_path, r1, r2)
    flags = {"stats": FILTER + ["--lmax", 150], "filter": FILTER, "edit": EDIT}[cmd]
    dirs = []
    for workers in (1, 3):
        d = tmp_path / f"w{workers}"
        d.mkdir()
        run_cli([cmd, "--fq1", f1, "--fq2", f2, "-o", d, *flags, "--chunk-mb", 1, "--gpus", 1, "--gpu-workers", workers,
                 "--counters-out", d / "ctr.bin", "--quiet"])
        dirs.append(d)
    a, b = dirs
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    if cmd == "stats":
        p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
        _, _, want = O.run(p, r1, r2)
        np.testing.assert_array_equal(np.fromfile(b / "ctr.bin", np.uint64), want)


def test_cli_paired_long_mate(tmp_path):
    """A 70,000-base mate 2 beside a 100-base mate 1 merges at full length: the
    long-read tail with two counter sets."""
    rng = np.random.default_rng(56)

    def read(L):
        return (rng.choice(np.frombuffer(b"ACGTN", np.uint8), L).tobytes(),
                (33 + rng.integers(2, 41, L)).astype(np.uint8).tobytes())
    l1 = [150] * 40 + [100] + [150] * 40
    l2 = [120] * 40 + [70000] + [120] * 40
    r1, r2 = O.Reads.from_pairs([read(L) for L in l1]), O.Reads.from_pairs([read(L) for L in l2])
    f1, f2, _, _ = _write_pair(tmp_path, r1, r2)
    ctr = tmp_path / "ctr.bin"
    out = tmp_path / "out"
    out.mkdir()
    run_cli(["stats", "--fq1", f1, "--fq2", f2, "-o", out, "--lmax", 150, "--counters-out", ctr, "--quiet"])
    _, _, want = O.run(PL.paired(H.stats_params(lmax=70000)), r1, r2)
    np.testing.assert_array_equal(np.fromfile(ctr, np.uint64), want)
    # mate 2's report comes from mate 2's set: (80 x 120 + 70,000) / 81 bases per read
    assert "(120, 982.72, 70000)" in (out / "in_2.fq.summary.txt").read_text()
    assert "(100, 149.38, 150)" in (out / "in_1.fq.summary.txt").read_text()


# ---- edges and pairing errors ---------------------------------------------------
def test_cli_paired_empty_files(tmp_path):
    f1, f2 = tmp_path / "e_1.fq", tmp_path / "e_2.fq"
    f1.write_bytes(b"")
    f2.write_bytes(b"")
    ctr = tmp_path / "ctr.bin"
    run_cli(["filter", "--fq1", f1, "--fq2", f2, "-o", tmp_path, "--max-N", 1, "--counters-out", ctr, "--quiet"])
    for n in ("passed_1.fq", "passed_2.fq", "failed_1.fq", "failed_2.fq"):
        assert (tmp_path / n).read_bytes() == b""
    got = np.fromfile(ctr, np.uint64)
    assert got.size == 2 * H.counters_len(1024) and not got.any()


@pytest.mark.parametrize("longer", [1, 2])
@pytest.mark.parametrize("chunk_mb", [1, 256])
def test_cli_one_file_has_records_left(tmp_path, longer, chunk_mb):
    """F2 one record short / one record long: exit status 1, and the line names
    the file that has records left and the number of the pair without a mate."""
    r1, r2 = _mates(9000, 57)
    f1, f2, rec1, rec2 = _write_pair(tmp_path, r1, r2)
    short = (tmp_path / "in_2.fq", rec2) if longer == 1 else (tmp_path / "in_1.fq", rec1)
    short[0].write_bytes(b"".join(short[1][:-1]))
    r = run_cli(["stats", "--fq1", f1, "--fq2", f2, "-o", tmp_path, "--chunk-mb", chunk_mb, "--quiet"], check=False)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    line = [ln for ln in r.stderr.splitlines() if "pairing error" in ln]
    assert len(line) == 1, r.stderr[-2000:]
    assert f"pair 8999: {f1 if longer == 1 else f2} has records left" in line[0], line
    assert "mate pairs out of step (-10)" in r.stderr


def test_cli_interleaved_odd_record_count(tmp_path):
    r1, r2 = _mates(500, 58)
    _, _, rec1, rec2 = _write_pair(tmp_path, r1, r2)
    fi = tmp_path / "odd.fq"
    fi.write_bytes(PL.interleave(rec1, rec2) + rec1[0])
    r = run_cli(["stats", "--interleaved", "-f", fi, "-o", tmp_path, "--quiet"], check=False)
    assert r.returncode == 1 and "pair 500:" in r.stderr and "odd number of records" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("form", ["two", "inter"])
def test_cli_swapped_record_in_third_chunk(tmp_path, form):
    """Two records of mate 2 swapped inside the third 1 MB chunk: exit status 1
    with the first bad pair's number over the whole input and both names."""
    r1, r2 = _mates(20000, 59)
    _, _, rec1, rec2 = _write_pair(tmp_path, r1, r2, fat=0)
    # the pair at 2.5 MB of the larger text: inside the third chunk of either form
    size = np.cumsum([len(a) + (len(b) if form == "inter" else 0) for a, b in zip(rec1, rec2)])
    k = int(np.searchsorted(size, 2.5 * 2**20))
    assert 100 < k < 19000
    rec2[k], rec2[k + 1] = rec2[k + 1], rec2[k]
    if form == "two":
        (tmp_path / "in_2.fq").write_bytes(b"".join(rec2))
        inputs = ["--fq1", tmp_path / "in_1.fq", "--fq2", tmp_path / "in_2.fq"]
    else:
        (tmp_path / "inter.fq").write_bytes(PL.interleave(rec1, rec2))
        inputs = ["--interleaved", "-f", tmp_path / "inter.fq"]
    r = run_cli(["filter", *inputs, "-o", tmp_path, "--max-N", 1, "--chunk-mb", 1, "--gpu-workers", 2, "--quiet"],
                check=False)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    line = [ln for ln in r.stderr.splitlines() if "pairing error" in ln]
    assert len(line) == 1, r.stderr[-2000:]
    assert f"pair {k}: mate names differ: 'r{k}/1' and 'r{k + 1}/2'" in line[0], line
