"""`hpg-fastq stats --overrepresented` end to end on the GPU:
<base>.overrepresented.data against tests/overrep_ref.py over the reads (pairs)
the oracle passes; every worker's tables keep at ceil(K / workers) and the
bytes come from whichever kept them; paired input; an empty input and a K above
every count; with and without --duplication; nothing changes without the flag;
the flag on filter."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import dup_ref
import overrep_ref
import cli_lib
from fastq_io import to_fastq

pytestmark = pytest.mark.gpu

FILTER = ["--read-quality-range", "20,"]
SUFFIX = "overrepresented.data"
FLAGS = ["--overrepresented", "--overrepresented-min-count", 8, "--overrepresented-top", 50]
DISPLAY_LINE = "\tOverrepresented      : top 50 with count >= 8 (--overrepresented)\n"


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


def _listed(seqs, n=50, k=8):
    """The reference's list; asserts that it is a test of something: at least 10
    sequences qualify and one tie in count falls inside the list."""
    entries, total = overrep_ref.select(seqs, n, k)
    assert total >= 10
    assert any(a[1] == b[1] for a, b in zip(entries, entries[1:]))
    return entries


@pytest.fixture(scope="module")
def single():
    reads = _with_duplicates(O.synth(30000, seed=71, L=150, trunc_pct=10), np.random.default_rng(71))
    text, _ = to_fastq(reads)
    want = {}
    for filt in (False, True):
        mask = O.run(H.stats_params(lmax=150, read_quality_range="20,"), reads)[0] if filt else None
        seqs = dup_ref.sequences(reads.seq, reads.idx, mask)
        want[filt] = overrep_ref.render(_listed(seqs), len(seqs))
    assert want[False] != want[True]
    return reads, text, want


@pytest.mark.parametrize("workers", [1, 2])
@pytest.mark.parametrize("filt", [False, True])
def test_single_end(tmp_path, single, filt, workers):
    """1 MB parse units; with two workers each table keeps at 4 and the list is
    taken from the merged counts."""
    _, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["stats", "-f", fq, "--lmax", 150, "-o", out, "--chunk-mb", 1, "--gpu-workers", workers, *FLAGS] +
                (FILTER if filt else []))
    assert (out / f"in.fq.{SUFFIX}").read_bytes() == want[filt]
    assert DISPLAY_LINE in r.stdout
    assert not (out / "in.fq.duplication.data").exists()


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
    want = []
    for r in (r1, r2):
        seqs = dup_ref.sequences(r.seq, r.idx, mask)
        want.append(overrep_ref.render(_listed(seqs), len(seqs)))
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
             "--gpu-workers", 2, *FLAGS, "--quiet"])
    for m in range(2):
        assert (out / f"{bases[m]}.{SUFFIX}").read_bytes() == want[m], bases[m]


def test_no_records_and_no_qualifying_sequence(tmp_path, single):
    fq = tmp_path / "empty.fq"
    fq.write_bytes(b"")
    r = run_cli(["stats", "-f", fq, "-o", tmp_path, "--overrepresented", "--quiet"])
    assert r.returncode == 0
    assert (tmp_path / f"empty.fq.{SUFFIX}").read_bytes() == overrep_ref.HEADER
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    run_cli(["stats", "-f", fq, "-o", tmp_path, "--lmax", 150, "--overrepresented", "--overrepresented-min-count", 100000,
             "--quiet"])
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes() == overrep_ref.HEADER


def test_with_and_without_duplication(tmp_path, single):
    _, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    dirs = {}
    for name, flags in (("dup", ["--duplication"]), ("both", ["--duplication", *FLAGS]), ("over", FLAGS)):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        run_cli(["stats", "-f", fq, "--lmax", 150, "-o", dirs[name], "--quiet", *flags])
    assert not (dirs["over"] / "in.fq.duplication.data").exists()
    assert not (dirs["dup"] / f"in.fq.{SUFFIX}").exists()
    assert (dirs["both"] / "in.fq.duplication.data").read_bytes() == (dirs["dup"] / "in.fq.duplication.data").read_bytes()
    assert (dirs["both"] / f"in.fq.{SUFFIX}").read_bytes() == want[False]
    assert (dirs["over"] / f"in.fq.{SUFFIX}").read_bytes() == want[False]


@pytest.mark.parametrize("filt", [False, True])
def test_nothing_else_changes(tmp_path, single, filt):
    """Without the flag: no such file, no line that mentions it; with it: the
    other files byte for byte, and stdout but for the display line."""
    _, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    plain, over = tmp_path / "plain", tmp_path / "over"
    plain.mkdir()
    over.mkdir()
    common = ["stats", "-f", fq, "--lmax", 150] + (FILTER if filt else [])
    r0 = run_cli(common + ["-o", plain])
    names = sorted(p.name for p in plain.iterdir())
    assert names and not any("overrepresented" in n for n in names)
    assert "verrepresented" not in r0.stdout and "verrepresented" not in r0.stderr
    r1 = run_cli(common + ["-o", over, *FLAGS])
    assert sorted(p.name for p in over.iterdir()) == sorted(names + [f"in.fq.{SUFFIX}"])
    for n in names:
        assert (plain / n).read_bytes() == (over / n).read_bytes(), n
    assert (over / f"in.fq.{SUFFIX}").read_bytes() == want[filt]
    assert _stable(r1.stdout).replace(DISPLAY_LINE, "").replace(str(over), str(plain)) == _stable(r0.stdout)
    assert r1.stderr == r0.stderr


def test_arena_too_small_is_one_line(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["stats", "-f", fq, "--lmax", 150, "-o", out, "--quiet", *FLAGS, "--overrepresented-bytes", 1000],
                check=False)
    assert r.returncode == 1
    assert r.stderr.strip().splitlines() == [
        "hpg-fastq: --overrepresented: the sequences that reached the minimum count need more than 1000 bytes; "
        "raise --overrepresented-min-count or --overrepresented-bytes"]


def test_filter_rejects_the_flag(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli(["filter", "-f", fq, "-o", out, *FILTER, "--overrepresented"], check=False)
    assert r.returncode == 1 and r.stdout == ""
    assert len(r.stderr.strip().splitlines()) == 1 and "--overrepresented" in r.stderr
    assert list(out.iterdir()) == []
