"""`hpg-fastq stats --adapters` end to end on the GPU: the dump (--adapters-out)
and <base>.adapter.content.data against tests/adapt_ref.py over the reads
(pairs) the oracle passes; --adapter-file; paired input; workers merge; a long
record is reserved; nothing else changes; the flag on filter / edit."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import adapt_ref
import cli_lib
from fastq_io import to_fastq

pytestmark = pytest.mark.gpu

FILTER = ["--read-quality-range", "20,"]
SUFFIX = "adapter.content.data"
NAMES = [n for n, _ in adapt_ref.DEFAULTS]
OWN = [(b"universal", b"AGATCGGAAGAG"), (b"long one", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTC"), (b"tab\tname", b"CTGTCTCT"),
       (b"again", b"AGATCGGAAGAG")]
OWN_FILE = b"# name<TAB>sequence\r\n" + b"".join(n + b"\t\t" + p + b"\r\n" for n, p in OWN) + b"\n"


def display_line(n):
    return f"\tAdapter content      : {n} probes, first occurrence per read (--adapters)\n"


def run_cli(args, **kw):
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


def planted(n, seed, probes, **kw):
    """Synthetic reads, about a third of them with a probe (some with two) somewhere, the end included."""
    reads = O.synth(n, seed=seed, L=150, **kw)
    rng = np.random.default_rng(seed)
    seq = reads.seq.copy()
    for i in range(n):
        a, b = int(reads.idx[i]), int(reads.idx[i + 1])
        for p in ([probes[i % len(probes)]] if i % 3 == 0 else []) + ([probes[(i // 7) % len(probes)]] if i % 7 == 0 else []):
            if b - a >= len(p):
                at = b - len(p) if i % 5 == 0 else a + int(rng.integers(0, b - a - len(p) + 1))
                seq[at:at + len(p)] = np.frombuffer(p, np.uint8)
    return O.Reads(seq, reads.qual, reads.idx)


def check(dump, mates, want, out, bases, names):
    got = adapt_ref.parse_dump(dump.read_bytes(), mates=mates)
    for m in range(mates):
        np.testing.assert_array_equal(got[m][0], want[m][0], err_msg=f"mate {m + 1}")
        assert got[m][1] == want[m][1]
        assert (out / f"{bases[m]}.{SUFFIX}").read_bytes() == adapt_ref.render(*want[m], names), bases[m]


@pytest.fixture(scope="module")
def single():
    reads = planted(6000, 41, adapt_ref.DEFAULT_PROBES + [OWN[1][1]], trunc_pct=10)
    text, _ = to_fastq(reads)
    mask = O.run(H.stats_params(lmax=150, read_quality_range="20,"), reads)[0]
    want = {(filt, own): adapt_ref.table_of(reads, [p for _, p in OWN] if own else adapt_ref.DEFAULT_PROBES,
                                            mask if filt else None) for filt in (False, True) for own in (False, True)}
    assert 0 < want[True, False][1]["reads"] == int(mask.sum()) < reads.n
    assert want[False, False][1]["with_any"] > 1500 and (want[False, True][0][1] != 0).any()
    return reads, text, want


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("filt", [False, True])
def test_single_end(tmp_path, single, filt, split):
    """split: 1 MB parse units on two workers, whose tables hpgq_adapt_add merges."""
    reads, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    plain, ad = tmp_path / "plain", tmp_path / "ad"
    plain.mkdir()
    ad.mkdir()
    common = ["stats", "-f", fq, "--lmax", 150] + (FILTER if filt else []) + \
        (["--chunk-mb", 1, "--gpu-workers", 2] if split else [])
    r0 = run_cli(common + ["-o", plain, "--counters-out", tmp_path / "c.bin"])
    r1 = run_cli(common + ["-o", ad, "--adapters", "--adapters-out", tmp_path / "a.bin"])
    check(tmp_path / "a.bin", 1, [want[filt, False]], ad, ["in.fq"], NAMES)
    # the reads / failed split is the engine's own
    ctr = np.frombuffer((tmp_path / "c.bin").read_bytes(), np.uint64)
    info = want[filt, False][1]
    assert int(ctr[H.S_NUM_STATS]) == info["reads"]
    if filt:
        assert int(ctr[H.S_NUM_PASSED]) == info["reads"] and int(ctr[H.S_NUM_FAILED]) == reads.n - info["reads"]
    # nothing else changes: the other files, and stdout but for the display line
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in ad.iterdir()) == sorted(names + [f"in.fq.{SUFFIX}"])
    for n in names:
        assert (plain / n).read_bytes() == (ad / n).read_bytes(), n
    line = display_line(6)
    assert line in r1.stdout and "Adapter content" not in r0.stdout
    assert _stable(r1.stdout).replace(line, "").replace(str(ad), str(plain)) == _stable(r0.stdout)
    assert r1.stderr == r0.stderr


@pytest.mark.parametrize("filt", [False, True])
def test_adapter_file(tmp_path, single, filt):
    reads, text, want = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    (tmp_path / "own.txt").write_bytes(OWN_FILE)
    r = run_cli(["stats", "-f", fq, "-o", tmp_path, "--lmax", 150, *(FILTER if filt else []), "--adapters",
                 "--adapter-file", tmp_path / "own.txt", "--adapters-out", tmp_path / "a.bin"])
    assert display_line(4) in r.stdout
    check(tmp_path / "a.bin", 1, [want[filt, True]], tmp_path, ["in.fq"], [n for n, _ in OWN])
    np.testing.assert_array_equal(want[filt, True][0][0], want[filt, True][0][3])   # identical probes, identical rows


def test_without_the_flag_nothing_is_written(tmp_path, single):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    run_cli(["stats", "-f", fq, "-o", out, "--lmax", 150, "--quiet"])
    assert not (out / f"in.fq.{SUFFIX}").exists()


def test_a_long_record_is_reserved(tmp_path):
    """150 bp reads and one record of 3,000 bases at --lmax 150, with probes past
    every tile and step edge of it: the unit reserves its longest record."""
    reads = planted(3000, 42, adapt_ref.DEFAULT_PROBES)
    pairs = reads.pairs()
    rng = np.random.default_rng(43)
    long_seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=3000)].copy()
    for p, at in zip(adapt_ref.DEFAULT_PROBES, (2988, 250, 700, 1500, 245, 2200)):
        long_seq[at:at + 12] = np.frombuffer(p, np.uint8)
    pairs.insert(1777, (long_seq, np.full(3000, ord("I"), np.uint8)))
    reads = O.Reads.from_pairs(pairs)
    fq = tmp_path / "in.fq"
    fq.write_bytes(to_fastq(reads)[0])
    want = adapt_ref.table_of(reads, adapt_ref.DEFAULT_PROBES)
    assert want[1]["npos"] == 3000 and want[0][0, 2988] == 1 and int(want[0][:, 256:].sum()) >= 4
    run_cli(["stats", "-f", fq, "-o", tmp_path, "--lmax", 150, "--adapters", "--adapters-out", tmp_path / "a.bin",
             "--quiet"])
    check(tmp_path / "a.bin", 1, [want], tmp_path, ["in.fq"], NAMES)


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, layout):
    r1 = planted(5000, 44, adapt_ref.DEFAULT_PROBES)
    r2 = planted(5000, 144, adapt_ref.DEFAULT_PROBES[::-1], trunc_pct=30)
    rec1 = PL.records(r1, PL.mate_headers(r1.n, 1))
    rec2 = PL.records(r2, PL.mate_headers(r2.n, 2), plus_header=True)
    p = PL.paired(H.stats_params(lmax=150, read_quality_range="20,", read_length_range="50,"))
    mask = O.run(p, r1, r2)[0]
    assert 0 < int(mask.sum()) < r1.n
    want = [adapt_ref.table_of(r1, adapt_ref.DEFAULT_PROBES, mask), adapt_ref.table_of(r2, adapt_ref.DEFAULT_PROBES, mask)]
    assert want[0][1]["reads"] == want[1][1]["reads"] == int(mask.sum())
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
             "--adapters", "--adapters-out", tmp_path / "a.bin", "--quiet"])
    check(tmp_path / "a.bin", 2, want, out, bases, NAMES)


def test_no_records(tmp_path):
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"")
    r = run_cli(["stats", "-f", fq, "-o", tmp_path, "--adapters", "--adapters-out", tmp_path / "a.bin", "--quiet"])
    assert r.returncode == 0
    empty = (np.zeros((6, 0), np.uint64), dict(reads=0, with_any=0, nprobes=6, npos=0))
    check(tmp_path / "a.bin", 1, [empty], tmp_path, ["in.fq"], NAMES)
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes().count(b"\n") == 3


@pytest.mark.parametrize("cmd,flags", [("filter", FILTER), ("edit", ["--left-length", "5", "--left-quality-range", "20,"])])
def test_filter_and_edit_reject_the_flag(tmp_path, single, cmd, flags):
    _, text, _ = single
    fq = tmp_path / "in.fq"
    fq.write_bytes(text)
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli([cmd, "-f", fq, "-o", out, *flags, "--adapters"], check=False)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"hpg-fastq: --adapters is an option of the stats command, not of {cmd}\n"
    assert list(out.iterdir()) == []
