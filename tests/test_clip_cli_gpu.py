"""`hpg-fastq edit --clip-adapters` end to end on the GPU.

Metamorphic: for an input X and the text X' that tests/clip_ref.py cuts from it
in Python, `edit --clip-adapters ...` on X writes the same output files, byte for
byte, as plain `edit` with the same trim and filter flags on X'.  Single-end
input goes through the mapped writer, paired input through the stream writer.
<base>.adapter.clip.data against clip_ref.render, the stdout lines, and no new
file and no changed byte without the flag.

X' holds empty records (reads cut at 0), which plain `edit` takes; only the last
record of a parse unit must not be empty (paired-end input, (d)),
so the last read of every X keeps bases and X' goes through as one unit, while X
is cut into units of 1 MB."""
import numpy as np
import pytest

import oracle_lib as O
import pairs_lib as PL
import clip_ref
import cli_lib
from adapt_ref import DEFAULTS, DEFAULT_PROBES as DEF

pytestmark = pytest.mark.gpu

EDIT = ["--left-length", 10, "--left-quality-range", "20,", "--right-length", 30, "--right-quality-range", "20,",
        "--read-quality-range", "20,", "--read-length-range", "60,"]
SUFFIX = "adapter.clip.data"
NAMES = [n for n, _ in DEFAULTS]
OWN = [(b"universal", b"AGATCGGAAGAG"), (b"long one", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTC"), (b"tab\tname", b"CTGTCTCT"),
       (b"again", b"AGATCGGAAGAG")]
OWN_FILE = b"# name<TAB>sequence\r\n" + b"".join(n + b"\t\t" + p + b"\r\n" for n, p in OWN) + b"\n"
# name -> (the flags, the probes, their names, min_overlap)
FORMS = {
    "default": (["--clip-adapters"], DEF, NAMES, 8),
    "file": (["--clip-adapters", "--clip-adapter-file", "own.txt"], [p for _, p in OWN], [n for n, _ in OWN], 8),
    "overlap3": (["--clip-adapters", "--clip-min-overlap=3"], DEF, NAMES, 3),
}


def run_cli(args, **kw):
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


def planted(n, seed, **kw):
    """Synthetic reads; about a third holds a probe somewhere, the very start
    included, every ninth ends inside one; the last read has none."""
    reads = O.synth(n, seed=seed, L=150, **kw)
    rng = np.random.default_rng(seed)
    probes = DEF + [OWN[1][1], OWN[2][1]]
    seq = reads.seq.copy()
    for i in range(n - 1):
        a, b = int(reads.idx[i]), int(reads.idx[i + 1])
        p = np.frombuffer(probes[i % len(probes)], np.uint8)
        if i % 3 == 0 and b - a >= len(p):
            at = a if i % 15 == 0 else a + int(rng.integers(0, b - a - len(p) + 1))
            seq[at:at + len(p)] = p
        if i % 9 == 4 and b - a >= len(p):
            m = int(rng.integers(1, len(p)))
            seq[b - m:b] = p[:m]
    seq[int(reads.idx[n - 1]):] = ord("N")
    return O.Reads(seq, reads.qual, reads.idx)


def _records(reads, headers, plus_header=False):
    return [(h, *reads.read(i), plus_header) for i, h in enumerate(headers)]


def _text(records):
    return [h + b"\n" + s + b"\n" + (b"+" + h[1:] if ph else b"+") + b"\n" + q + b"\n" for h, s, q, ph in records]


def _clipped(records, probes, mo):
    cut, info = clip_ref.clip_records([(h, s, q) for h, s, q, _ in records], probes, mo)
    return [(h, s, q, rec[3]) for (h, s, q), rec in zip(cut, records)], info


def _outputs(d):
    return {p.name: p.read_bytes() for p in d.iterdir() if p.name.endswith(".fq")}


def _same_outputs(got_dir, want_dir, names):
    got, want = _outputs(got_dir), _outputs(want_dir)
    assert sorted(got) == sorted(want) == sorted(names)
    for n in names:
        assert got[n] == want[n], n
        assert want[n].count(b"\n") > 400, n                             # (both classes hold records)


def _display_line(n, mo):
    return f"\tAdapter clipping     : {n} probes, min overlap {mo} (--clip-adapters)\n"


@pytest.fixture(scope="module")
def single():
    reads = planted(4000, 71, trunc_pct=10)
    return _records(reads, [f"@r{i} extra:{i % 7}".encode() for i in range(reads.n)])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_single_end(tmp_path, single, form):
    flags, probes, names, mo = FORMS[form]
    (tmp_path / "own.txt").write_bytes(OWN_FILE)
    flags = [str(tmp_path / f) if f == "own.txt" else f for f in flags]
    cut, info = _clipped(single, probes, mo)
    assert 400 < info["clipped"] < 3000 and any(len(r[1]) == 0 for r in cut) and len(cut[-1][1]) > 0
    (tmp_path / "x.fq").write_bytes(b"".join(_text(single)))
    (tmp_path / "cut.fq").write_bytes(b"".join(_text(cut)))
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    # 1 MB parse units on two workers: their scalars are added
    r1 = run_cli(["edit", "-f", tmp_path / "x.fq", "-o", a, *EDIT, *flags, "--chunk-mb", 1, "--gpu-workers", 2])
    r0 = run_cli(["edit", "-f", tmp_path / "cut.fq", "-o", b, *EDIT, "--gpu-workers", 2])
    _same_outputs(a, b, ["edit.fq", "failed.fq"])
    assert "mapped files" in r1.stdout
    assert (a / f"x.fq.{SUFFIX}").read_bytes() == clip_ref.render(info, names)
    assert sorted(p.name for p in a.iterdir()) == ["edit.fq", "failed.fq", f"x.fq.{SUFFIX}"]
    assert sorted(p.name for p in b.iterdir()) == ["edit.fq", "failed.fq"]
    # stdout: the display line and the clipped reads, nothing else
    line, res = _display_line(len(probes), mo), f"Num. clipped reads : {info['clipped']}\n"
    assert line in r1.stdout and res in r1.stdout and "clipp" not in r0.stdout
    assert r1.stdout.index("Num. edited reads :") < r1.stdout.index(res) < r1.stdout.index("Output file")
    same = _stable(r1.stdout).replace(line, "").replace(res, "").replace(str(a), str(b)).replace("x.fq", "cut.fq")
    same = same.replace(": 1 MB of FastQ text", ": 256 MB of FastQ text")
    assert same == _stable(r0.stdout)
    assert r1.stderr == r0.stderr


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, layout):
    """Each mate is cut on its own; mate 2 repeats its header on the '+' line."""
    r1, r2 = planted(3000, 72), planted(3000, 172, trunc_pct=30)
    rec = [_records(r1, PL.mate_headers(r1.n, 1)), _records(r2, PL.mate_headers(r2.n, 2), plus_header=True)]
    cut, info = zip(*[_clipped(r, DEF, 5) for r in rec])
    assert info[0]["clipped"] != info[1]["clipped"] and min(i["clipped"] for i in info) > 600
    dirs = {}
    for name, mates in (("x", rec), ("cut", cut)):
        t1, t2 = _text(mates[0]), _text(mates[1])
        if layout == "two_files":
            (tmp_path / f"{name}_1.fq").write_bytes(b"".join(t1))
            (tmp_path / f"{name}_2.fq").write_bytes(b"".join(t2))
            inputs = ["--fq1", tmp_path / f"{name}_1.fq", "--fq2", tmp_path / f"{name}_2.fq"]
        else:
            (tmp_path / f"{name}.fq").write_bytes(PL.interleave(t1, t2))
            inputs = ["-f", tmp_path / f"{name}.fq", "--interleaved"]
        dirs[name] = tmp_path / ("out_" + name)
        dirs[name].mkdir()
        extra = ["--clip-adapters", "--clip-min-overlap", 5, "--chunk-mb", 1] if name == "x" else []
        r = run_cli(["edit", *inputs, "-o", dirs[name], *EDIT, *extra])
        assert "one stream writer thread" in r.stdout
        if name == "x":
            assert _display_line(6, 5) in r.stdout
            res = f"Num. clipped reads : {info[0]['clipped']} (mate 1)\n"
            assert r.stdout.index("Num. edited reads :") < r.stdout.index(res) < r.stdout.index("Num. passed pairs")
        else:
            assert "clipp" not in r.stdout
    _same_outputs(dirs["x"], dirs["cut"], ["edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq"])
    bases = ("x_1.fq", "x_2.fq") if layout == "two_files" else ("x.fq_1", "x.fq_2")
    for m in range(2):
        assert (dirs["x"] / f"{bases[m]}.{SUFFIX}").read_bytes() == clip_ref.render(info[m], NAMES), bases[m]
    assert not [p for p in dirs["cut"].iterdir() if p.name.endswith(SUFFIX)]


def test_no_records(tmp_path):
    (tmp_path / "in.fq").write_bytes(b"")
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "-o", tmp_path, *EDIT, "--clip-adapters"])
    assert "Num. clipped reads : 0\n" in r.stdout
    zero = dict(reads=0, clipped=0, bases_removed=0, by_probe=[0] * 6)
    assert (tmp_path / f"in.fq.{SUFFIX}").read_bytes() == clip_ref.render(zero, NAMES)
