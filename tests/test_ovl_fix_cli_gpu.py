"""`hpg-fastq edit --clip-overlap --correct-overlap --insert-size` end to end on
the GPU.

Metamorphic, as tests/test_ovl_cli_gpu.py: for a paired input X and the texts X'
that tests/ovl_fix_ref.py cuts and corrects from it in Python, the flags on X
write the same output files, byte for byte, as plain `edit` with the same trim
and filter flags on X' -- so the trim and the filter saw the corrected bytes.
Two-file and interleaved input; <mate 1's base>.overlap.correct.data and
.insert.size.data against the reference's renderers; the stdout lines; and with
--clip-overlap alone no new file and no new stdout line."""
import numpy as np
import pytest

import pairs_lib as PL
import ovl_ref as R
import ovl_fix_ref as X
import cli_lib

pytestmark = pytest.mark.gpu

EDIT = ["--left-length", 10, "--left-quality-range", "20,", "--right-length", 30, "--right-quality-range", "20,",
        "--read-quality-range", "20,", "--read-length-range", "60,"]
FIX, INS, CLIP = "overlap.correct.data", "insert.size.data", "overlap.clip.data"
FQ = ["edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq"]


def run_cli(args, **kw):
    return cli_lib.run_cli(list(args) + ["--gpus", 1, "--gpu-workers", 2], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


@pytest.fixture(scope="module")
def case():
    """200 pairs of (header, seq, qual, plus_header) per mate: random pairs whose
    quality depends on read and position, and in every fourth overlapping pair a
    disagreement of a high against a low quality; the last pair keeps its bases."""
    n = 200
    heads = (PL.mate_headers(n, 1), PL.mate_headers(n, 2))
    rec = ([], [])
    for i, (s1, s2) in enumerate(R.random_pairs(n, 41, L=(70, 151))):
        q1 = bytes(33 + (7 * j + 3 * i) % 41 for j in range(len(s1)))
        q2 = bytes(33 + (5 * j + 11 * i) % 41 for j in range(len(s2)))
        F = R.find(s1, s2, 30, 5)
        if F > 0 and i % 4 == 1:
            ov = min(len(s1), F) - max(0, F - len(s2))
            s1, q1, s2, q2 = X.plant((s1, q1, s2, q2), F, ov // 2, 1 + i // 4 % 2, 33 + 38, 33 + 4)
        rec[0].append((heads[0][i], s1, q1, False))
        rec[1].append((heads[1][i], s2, q2, True))
    fixed, info, fix, hist = X.fix_records(rec[0], rec[1])
    # by the reference: pairs are cut, bases corrected in both mates, several insert sizes, pairs without an overlap
    assert info["clipped"] > 30 and min(fix["corrected_bases"]) >= 10 and np.count_nonzero(hist[1:]) > 30 and hist[0] > 30
    assert fixed[0] != R.cut_records(rec[0], rec[1])[0][0] and len(fixed[0][-1][1]) > 0 and len(fixed[1][-1][1]) > 0
    return rec, fixed, info, fix, hist


def _text(records):
    return [h + b"\n" + s + b"\n" + (b"+" + h[1:] if ph else b"+") + b"\n" + q + b"\n" for h, s, q, ph in records]


def _inputs(tmp_path, name, mates, layout):
    t1, t2 = _text(mates[0]), _text(mates[1])
    if layout == "two_files":
        (tmp_path / f"{name}_1.fq").write_bytes(b"".join(t1))
        (tmp_path / f"{name}_2.fq").write_bytes(b"".join(t2))
        return ["--fq1", tmp_path / f"{name}_1.fq", "--fq2", tmp_path / f"{name}_2.fq"]
    (tmp_path / f"{name}.fq").write_bytes(PL.interleave(t1, t2))
    return ["-f", tmp_path / f"{name}.fq", "--interleaved"]


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, case, layout):
    rec, fixed, info, fix, hist = case
    dirs, out = {}, {}
    for name, mates, flags in (("x", rec, ["--clip-overlap", "--correct-overlap", "--insert-size"]), ("ref", fixed, []),
                               ("clip", rec, ["--clip-overlap"])):
        dirs[name] = tmp_path / ("out_" + name)
        dirs[name].mkdir()
        out[name] = run_cli(["edit", *_inputs(tmp_path, "x" if name == "clip" else name, mates, layout), "-o", dirs[name],
                             *EDIT, *flags])
    files = {k: {p.name: p.read_bytes() for p in d.iterdir()} for k, d in dirs.items()}
    base = "x_1.fq" if layout == "two_files" else "x.fq_1"
    assert sorted(files["ref"]) == FQ
    for name in FQ:
        assert files["x"][name] == files["ref"][name], name
    assert files["x"]["edit_1.fq"].count(b"\n") > 40 and files["x"]["failed_1.fq"].count(b"\n") > 40          # (both classes hold records)
    assert files["x"]["edit_1.fq"] != files["clip"]["edit_1.fq"] or files["x"]["edit_2.fq"] != files["clip"]["edit_2.fq"]
    assert files["x"][f"{base}.{FIX}"] == X.render_correct(info, fix)
    assert files["x"][f"{base}.{INS}"] == X.render_inserts(info, hist)
    assert files["x"][f"{base}.{CLIP}"] == R.render(info) == files["clip"][f"{base}.{CLIP}"]
    assert sorted(files["x"]) == sorted(FQ + [f"{base}.{s}" for s in (FIX, INS, CLIP)])
    # --clip-overlap alone: neither new file, no new stdout line
    assert sorted(files["clip"]) == sorted(FQ + [f"{base}.{CLIP}"])
    so, plain = out["x"].stdout, out["clip"].stdout
    assert "orrect" not in plain and "nsert" not in plain
    lines = ["\tOverlap correction   : high quality 30, low quality 14 (--correct-overlap)\n",
             "\tInsert sizes         : counted (--insert-size)\n",
             f"Num. overlap-corrected pairs : {fix['corrected_pairs']}\n"]
    assert all(x in so for x in lines)
    assert so.index("\tOverlap clipping ") < so.index(lines[0]) < so.index(lines[1])
    assert so.index("Num. overlap-clipped pairs :") < so.index(lines[2]) < so.index("Num. passed pairs")
    same = _stable(so)
    for x in lines:
        same = same.replace(x, "")
    # the rest of stdout is --clip-overlap's own, but for the passed and edited pairs and the directory
    drop = ("Num. edited reads", "Num. passed pairs", "Num. failed pairs")
    keep = lambda text: [x for x in text.replace(str(dirs["x"]), "D").replace(str(dirs["clip"]), "D").splitlines()   # noqa: E731
                         if not x.startswith(drop)]
    assert keep(same) == keep(_stable(plain))
    assert out["x"].stderr == out["clip"].stderr


def test_values_and_phred64(tmp_path, case):
    """Own thresholds, and phred from --quality-encoding: the same bytes moved up by 31."""
    rec = case[0]
    up = lambda q: bytes(x + 31 for x in q)   # noqa: E731
    rec64 = tuple([(h, s, up(q), ph) for h, s, q, ph in mate] for mate in rec)
    fixed, info, fix, hist = X.fix_records(rec64[0], rec64[1], 30, 5, 64, 25, 9)
    assert min(fix["corrected_bases"]) >= 10
    flags = ["--quality-encoding", "phred64"]
    out = {}
    for name, mates, extra in (("x", rec64, ["--clip-overlap", "--correct-overlap", "--correct-overlap-high=25",
                                              "--correct-overlap-low", 9]), ("ref", fixed, [])):
        d = tmp_path / ("out_" + name)
        d.mkdir()
        out[name] = run_cli(["edit", *_inputs(tmp_path, name, mates, "interleaved"), "-o", d, *EDIT, *flags, *extra])
    got, want = tmp_path / "out_x", tmp_path / "out_ref"
    for name in FQ:
        assert (got / name).read_bytes() == (want / name).read_bytes(), name
    assert (got / f"x.fq_1.{FIX}").read_bytes() == X.render_correct(info, fix)
    assert not (got / f"x.fq_1.{INS}").exists()
    so = out["x"].stdout
    assert "\tOverlap correction   : high quality 25, low quality 9 (--correct-overlap)\n" in so and "Insert sizes" not in so
    assert f"Num. overlap-corrected pairs : {fix['corrected_pairs']}\n" in so


def test_no_records(tmp_path):
    (tmp_path / "in.fq").write_bytes(b"")
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "-o", tmp_path, *EDIT, "--clip-overlap", "--correct-overlap",
                 "--insert-size"])
    assert "Num. overlap-corrected pairs : 0\n" in r.stdout
    zero = dict(pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0])
    none = dict(corrected_pairs=0, corrected_bases=[0, 0])
    assert (tmp_path / f"in.fq_1.{FIX}").read_bytes() == X.render_correct(zero, none)
    assert (tmp_path / f"in.fq_1.{INS}").read_bytes() == X.render_inserts(zero, np.zeros(X.BINS, np.uint64))
