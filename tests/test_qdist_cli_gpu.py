"""`hpg-fastq stats --quality-dist` end to end on the GPU: the table
(--quality-dist-out) and <base>.quality.dist.per.nt.data against
tests/qdist_ref.py over the reads (pairs) the oracle passes; nothing else
changes; workers merge; long reads are reserved per unit; paired input; an
empty input; the flag on filter."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import qdist_ref
import cli_lib
from fastq_io import to_fastq

pytestmark = pytest.mark.gpu

DISPLAY_LINE = "\tQuality distribution : per read position (--quality-dist)\n"
FILTER = ["--read-quality-range", "20,"]
SUFFIX = "quality.dist.per.nt.data"


def run_cli(args, **kw):
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


@pytest.fixture(scope="module")
def single():
    reads = O.synth(20000, seed=31, L=150, trunc_pct=10)
    text, _ = to_fastq(reads)
    want = {}
    for filt in (False, True):
        mask = O.run(H.stats_params(lmax=150, read_quality_range="20,"), reads)[0] if filt else None
        want[filt] = qdist_ref.table_of(reads, mask)
    assert want[True].sum() < want[False].sum()
    return reads, text, want


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("filt", [False, True])
def test_single_end(tmp_path, single, filt, split):
    """split: 1 MB parse units on two workers, whose tables hpgq_qdist_add merges."""
    reads, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    plain, dist = tmp_path / "plain", tmp_path / "dist"
    plain.mkdir()
    dist.mkdir()
    common = ["stats", "-f", fq, "--lmax", 150] + (FILTER if filt else []) + \
        (["--chunk-mb", 1, "--gpu-workers", 2] if split else [])
    r0 = run_cli(common + ["-o", plain])
    r1 = run_cli(common + ["-o", dist, "--quality-dist", "--quality-dist-out", tmp_path / "q.bin"])
    (got,) = qdist_ref.parse_dump((tmp_path / "q.bin").read_bytes())
    np.testing.assert_array_equal(got, want[filt])
    assert (dist / f"in.fq.{SUFFIX}").read_bytes() == qdist_ref.render(want[filt], 33)
    # nothing else changes: the other files, and stdout but for the display line
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in dist.iterdir()) == sorted(names + [f"in.fq.{SUFFIX}"])
    for n in names:
        assert (plain / n).read_bytes() == (dist / n).read_bytes(), n
    assert DISPLAY_LINE in r1.stdout and DISPLAY_LINE not in r0.stdout
    assert _stable(r1.stdout).replace(DISPLAY_LINE, "").replace(str(dist), str(plain)) == _stable(r0.stdout)
    assert r1.stderr == r0.stderr


def test_without_the_flag_nothing_is_written(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    run_cli(["stats", "-f", fq, "-o", out, "--lmax", 150, "--quality-dist-out", tmp_path / "q.bin", "--quiet"])
    assert not (tmp_path / "q.bin").exists() and not (out / f"in.fq.{SUFFIX}").exists()


def test_long_reads_are_reserved_per_unit(tmp_path):
    """150 bp reads mixed with reads of 1 .. 5,000 bases at --lmax 150, in 1 MB
    units on two workers: every unit reserves its longest record, nothing clips."""
    rng = np.random.default_rng(32)
    lens = np.where(rng.random(6000) < 0.9, 150, rng.integers(1, 5001, size=6000))
    lens[4321] = 5000
    idx = np.zeros(len(lens) + 1, np.int32)
    idx[1:] = np.cumsum(lens)
    qual = rng.integers(33, 74, size=int(idx[-1]), dtype=np.uint8)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(idx[-1]))]
    reads = O.Reads(seq, qual, idx)
    fq = tmp_path / "in.fq"
    fq.write_bytes(to_fastq(reads)[0])
    mask = O.run(H.stats_params(lmax=150, read_length_range="100,"), reads)[0]
    want = qdist_ref.table_of(reads, mask)
    assert want.shape[0] == 5000
    run_cli(["stats", "-f", fq, "-o", tmp_path, "--lmax", 150, "--read-length-range", "100,", "--chunk-mb", 1,
             "--gpu-workers", 2, "--quality-dist", "--quality-dist-out", tmp_path / "q.bin", "--quiet"])
    (got,) = qdist_ref.parse_dump((tmp_path / "q.bin").read_bytes())
    np.testing.assert_array_equal(got, want)
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes() == qdist_ref.render(want, 33)


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, layout):
    r1 = O.synth(12000, seed=33, L=150)
    r2 = O.synth(12000, seed=133, L=150, trunc_pct=30)
    rec1 = PL.records(r1, PL.mate_headers(r1.n, 1))
    rec2 = PL.records(r2, PL.mate_headers(r2.n, 2), plus_header=True)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    mask = O.run(p, r1, r2)[0]
    assert 0 < int(mask.sum()) < r1.n
    want = [qdist_ref.table_of(r1, mask), qdist_ref.table_of(r2, mask)]
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
             "--quality-dist", "--quality-dist-out", tmp_path / "q.bin", "--quiet"])
    got = qdist_ref.parse_dump((tmp_path / "q.bin").read_bytes(), mates=2)
    for m in range(2):
        np.testing.assert_array_equal(got[m], want[m], err_msg=f"mate {m + 1}")
        assert (out / f"{bases[m]}.{SUFFIX}").read_bytes() == qdist_ref.render(want[m], 33), bases[m]


def test_no_records(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"")
    r = run_cli(["stats", "-f", fq, "-o", tmp_path, "--quality-dist", "--quality-dist-out", tmp_path / "q.bin",
                 "--quiet"])
    assert r.returncode == 0
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes() == qdist_ref.HEADER
    assert (tmp_path / "q.bin").read_bytes() == bytes(8)


def test_filter_rejects_the_flag(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["filter", "-f", fq, "-o", out, *FILTER, "--quality-dist"], check=False)
    assert r.returncode == 1 and r.stdout == ""
    assert len(r.stderr.strip().splitlines()) == 1 and "--quality-dist" in r.stderr
    assert list(out.iterdir()) == []
