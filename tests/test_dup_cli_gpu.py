"""`hpg-fastq stats --duplication` end to end on the GPU: the table
(--duplication-out) and <base>.duplication.data against tests/dup_ref.py over
the reads (pairs) the oracle passes; workers merge through export / import;
paired input; an empty input; nothing changes without the flag; the flag on
filter."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import dup_ref
import cli_lib
from fastq_io import to_fastq

pytestmark = pytest.mark.gpu

DISPLAY_LINE = "\tDuplication levels   : exact, per sequence (--duplication)\n"
FILTER = ["--read-quality-range", "20,"]
SUFFIX = "duplication.data"


def run_cli(args, **kw):
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


def _with_duplicates(reads, rng, hot=300):
    """A third of the reads replaced by copies of the first `hot` ones, a few of
    those many times over, so that several levels are populated."""
    pairs = reads.pairs()
    for i in rng.integers(hot, len(pairs), size=len(pairs) // 3):
        pairs[int(i)] = pairs[int(min(rng.integers(0, hot), rng.integers(0, hot), rng.integers(0, hot)))]
    return O.Reads.from_pairs(pairs)


def _check_dump(got, want):
    wk, wc = dup_ref.arrays(want)
    np.testing.assert_array_equal(got[0], wk)
    np.testing.assert_array_equal(got[1], wc)


@pytest.fixture(scope="module")
def single():
    reads = _with_duplicates(O.synth(30000, seed=71, L=150, trunc_pct=10), np.random.default_rng(71))
    text, _ = to_fastq(reads)
    want = {}
    for filt in (False, True):
        mask = O.run(H.stats_params(lmax=150, read_quality_range="20,"), reads)[0] if filt else None
        want[filt] = dup_ref.table_of(reads, mask)
    lv = dup_ref.levels_of_table(want[False])
    assert lv["reads"] == 30000 and lv["max_count"] >= 50 and sum(1 for x in lv["distinct_at"] if x) >= 8
    assert sum(want[True].values()) < 30000
    return reads, text, want


@pytest.mark.parametrize("workers", [1, 2])
@pytest.mark.parametrize("filt", [False, True])
def test_single_end(tmp_path, single, filt, workers):
    """1 MB parse units; with two workers, worker 1's table is exported and
    imported into worker 0's."""
    reads, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["stats", "-f", fq, "--lmax", 150, "-o", out, "--chunk-mb", 1, "--gpu-workers", workers,
                 "--duplication", "--duplication-out", tmp_path / "d.bin"] + (FILTER if filt else []))
    (got,) = dup_ref.parse_dump((tmp_path / "d.bin").read_bytes())
    _check_dump(got, want[filt])
    assert (out / f"in.fq.{SUFFIX}").read_bytes() == dup_ref.render(dup_ref.levels_of_table(want[filt]))
    assert DISPLAY_LINE in r.stdout


@pytest.mark.parametrize("filt", [False, True])
def test_nothing_else_changes(tmp_path, single, filt):
    """Without the flag: no duplication file, no line that mentions it; with
    it: the other files byte for byte, and stdout but for the display line."""
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    plain, dup = tmp_path / "plain", tmp_path / "dup"
    plain.mkdir()
    dup.mkdir()
    common = ["stats", "-f", fq, "--lmax", 150] + (FILTER if filt else [])
    r0 = run_cli(common + ["-o", plain, "--duplication-out", tmp_path / "d.bin"])
    assert not (tmp_path / "d.bin").exists()
    names = sorted(p.name for p in plain.iterdir())
    assert names and not any("duplication" in n for n in names)
    assert "uplication" not in r0.stdout and "uplication" not in r0.stderr
    r1 = run_cli(common + ["-o", dup, "--duplication"])
    assert sorted(p.name for p in dup.iterdir()) == sorted(names + [f"in.fq.{SUFFIX}"])
    for n in names:
        assert (plain / n).read_bytes() == (dup / n).read_bytes(), n
    assert _stable(r1.stdout).replace(DISPLAY_LINE, "").replace(str(dup), str(plain)) == _stable(r0.stdout)
    assert r1.stderr == r0.stderr


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, layout):
    rng = np.random.default_rng(72)
    r1 = _with_duplicates(O.synth(12000, seed=73, L=150), rng)
    r2 = _with_duplicates(O.synth(12000, seed=173, L=150, trunc_pct=30), rng)
    rec1 = PL.records(r1, PL.mate_headers(r1.n, 1))
    rec2 = PL.records(r2, PL.mate_headers(r2.n, 2), plus_header=True)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    mask = O.run(p, r1, r2)[0]
    assert 0 < int(mask.sum()) < r1.n
    want = [dup_ref.table_of(r1, mask), dup_ref.table_of(r2, mask)]
    if layout == "two_files":
        (tmp_path / "in_1.fq").write_bytes(b"".join(rec1))
        (tmp_path / "in_2.fq").write_bytes(b"".join(rec2))
        inputs, bases = ["--fq1", tmp_path / "in_1.fq", "--fq2", tmp_path / "in_2.fq"], ("in_1.fq", "in_2.fq")
    else:
        (tmp_path / "in.fq").write_bytes(PL.interleave(rec1, rec2))
        inputs, bases = ["-f", tmp_path / "in.fq", "--interleaved"], ("in.fq_1", "in.fq_2")
    out = tmp_path / "out"
    out.mkdir()
    run_cli(["stats", *inputs, "-o", out, "--lmax", 150, *FILTER, "--read-length-range", "50,", "--chunk-mb", 1,
             "--gpu-workers", 2, "--duplication", "--duplication-out", tmp_path / "d.bin", "--quiet"])
    got = dup_ref.parse_dump((tmp_path / "d.bin").read_bytes(), mates=2)
    for m in range(2):
        _check_dump(got[m], want[m])
        assert (out / f"{bases[m]}.{SUFFIX}").read_bytes() == dup_ref.render(dup_ref.levels_of_table(want[m])), bases[m]


def test_no_records(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"")
    r = run_cli(["stats", "-f", fq, "-o", tmp_path, "--duplication", "--duplication-out", tmp_path / "d.bin",
                 "--quiet"])
    assert r.returncode == 0
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes() == dup_ref.render(dup_ref.levels([]))
    assert (tmp_path / "d.bin").read_bytes() == bytes(8)


def test_filter_rejects_the_flag(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["filter", "-f", fq, "-o", out, *FILTER, "--duplication"], check=False)
    assert r.returncode == 1 and r.stdout == ""
    assert len(r.stderr.strip().splitlines()) == 1 and "--duplication" in r.stderr
    assert list(out.iterdir()) == []
