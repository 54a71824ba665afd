"""`hpg-fastq edit --clip-overlap` end to end on the GPU.

Metamorphic, as tests/test_clip_cli_gpu.py: for a paired input X and the texts X'
that tests/ovl_ref.py (and, with --clip-adapters, tests/clip_ref.py after it)
cuts from it in Python, `edit --clip-overlap ...` on X writes the same output
files, byte for byte, as plain `edit` with the same trim and filter flags on X'.
Two-file and interleaved input, with and without --clip-adapters, default and
own value flags.  <mate 1's base>.overlap.clip.data against ovl_ref.render, the
stdout lines, and no new file and no new stdout byte without the flag.

X' may hold empty records once the probes have cut too (plain `edit` takes them);
only the last record of a parse unit must not be empty, so the last pair of X
keeps bases and X' goes through as one unit, while X is cut into units of 1 MB."""
import numpy as np
import pytest

import pairs_lib as PL
import clip_ref
import ovl_ref as R
import cli_lib
from adapt_ref import DEFAULTS, DEFAULT_PROBES as DEF

pytestmark = pytest.mark.gpu

EDIT = ["--left-length", 10, "--left-quality-range", "20,", "--right-length", 30, "--right-quality-range", "20,",
        "--read-quality-range", "20,", "--read-length-range", "60,"]
SUFFIX = "overlap.clip.data"
CLIP_SUFFIX = "adapter.clip.data"
NAMES = [n for n, _ in DEFAULTS]
# name -> (the flags, min_overlap, M, the probes' min_overlap or None)
FORMS = {
    "default": (["--clip-overlap"], 30, 5, None),
    "values": (["--clip-overlap", "--clip-overlap-min=20", "--clip-overlap-mismatches", 2], 20, 2, None),
    "with_adapters": (["--clip-overlap", "--clip-adapters", "--clip-min-overlap", 5], 30, 5, 5),
}


def run_cli(args, **kw):
    args = list(args)
    return cli_lib.run_cli(args if "--gpus" in args else args + ["--gpus", 1], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


def _quality(i, n, rng):
    """Qualities of read i: a level per read (so that the filter passes some and fails others), low ends in some."""
    q = 8 + (i * 7) % 30 + (np.arange(n) * 5 + i) % 9
    if i % 4 == 1:
        q[:4] = 3
        q[max(n - 6, 0):] = 3
    return bytes((33 + np.clip(q, 0, 41)).astype(np.uint8))


@pytest.fixture(scope="module")
def pairs():
    """3000 pairs of [(header, seq, qual, plus_header)] per mate: a read-through
    ends in an adapter in both mates, some other reads hold a probe or end inside
    one; the last pair has neither."""
    n = 3000
    rng = np.random.default_rng(95)
    rec = ([], [])
    heads = (PL.mate_headers(n, 1), PL.mate_headers(n, 2))
    for i in range(n):
        n1, n2 = int(rng.integers(70, 151)), int(rng.integers(70, 151))
        if i % 3 != 2 and i != n - 1:
            F = int(rng.integers(25, n1 + n2))
            s1, s2 = R.pair_of(rng, n1, n2, F, tail1=DEF[0] + R.acgt(rng, 150), tail2=DEF[1] + R.acgt(rng, 150))
            for _ in range(int(rng.integers(0, 7)) if i % 4 == 0 else 0):
                s1 = R.flip(s1, int(rng.integers(0, n1)))
        else:
            s1, s2 = R.acgt(rng, n1), R.acgt(rng, n2)
            if i % 5 == 0 and i != n - 1:                               # a probe inside mate 1, mate 2 ends inside one
                at = int(rng.integers(0, n1 - 12))
                s1 = s1[:at] + DEF[i % len(DEF)] + s1[at + 12:]
                s2 = s2[:n2 - 7] + DEF[2][:7]
        rec[0].append((heads[0][i], s1, _quality(2 * i, n1, rng), False))
        rec[1].append((heads[1][i], s2, _quality(2 * i + 1, n2, rng), True))   # mate 2 repeats its header on the '+' line
    return rec


def _text(records):
    return [h + b"\n" + s + b"\n" + (b"+" + h[1:] if ph else b"+") + b"\n" + q + b"\n" for h, s, q, ph in records]


def _cut(pairs, mo, M, probe_mo):
    """The reference's texts: by overlap first, by the probes second; the scalars of both."""
    cut, info = R.cut_records(pairs[0], pairs[1], mo, M)
    clip_info = None
    if probe_mo is not None:
        both = [clip_ref.clip_records([(h, s, q) for h, s, q, _ in recs], DEF, probe_mo) for recs in cut]
        cut = [[(h, s, q, old[3]) for (h, s, q), old in zip(c, recs)] for (c, _), recs in zip(both, cut)]
        clip_info = [i for _, i in both]
    return cut, info, clip_info


def _outputs(d):
    return {p.name: p.read_bytes() for p in d.iterdir() if p.name.endswith(".fq")}


def _same_outputs(got_dir, want_dir, names):
    got, want = _outputs(got_dir), _outputs(want_dir)
    assert sorted(got) == sorted(want) == sorted(names)
    for n in names:
        assert got[n] == want[n], n
        assert want[n].count(b"\n") > 400, n                             # (both classes hold records)


def _display_line(mo, M):
    return f"\tOverlap clipping     : min overlap {mo}, max mismatches {M} (--clip-overlap)\n"


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, pairs, layout, form):
    flags, mo, M, probe_mo = FORMS[form]
    cut, info, clip_info = _cut(pairs, mo, M, probe_mo)
    assert info["overlapping"] > 900 and 500 < info["clipped"] < 2500 and min(info["bases_removed"]) > 5000
    assert all(len(r[-1][1]) > 0 for r in cut)
    if clip_info:                                                        # the probes still find work in what the overlap kept
        assert min(i["clipped"] for i in clip_info) > 50
    dirs, out = {}, {}
    for name, mates in (("x", pairs), ("cut", cut)):
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
        # X in parse units of 1 MB on two workers: their scalars are added
        extra = [*flags, "--chunk-mb", 1, "--gpu-workers", 2] if name == "x" else ["--gpu-workers", 2]
        out[name] = run_cli(["edit", *inputs, "-o", dirs[name], *EDIT, *extra])
    _same_outputs(dirs["x"], dirs["cut"], ["edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq"])
    bases = ("x_1.fq", "x_2.fq") if layout == "two_files" else ("x.fq_1", "x.fq_2")
    assert (dirs["x"] / f"{bases[0]}.{SUFFIX}").read_bytes() == R.render(info)
    want_files = {"edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq", f"{bases[0]}.{SUFFIX}"}
    if clip_info:
        for m in range(2):
            assert (dirs["x"] / f"{bases[m]}.{CLIP_SUFFIX}").read_bytes() == clip_ref.render(clip_info[m], NAMES), bases[m]
            want_files.add(f"{bases[m]}.{CLIP_SUFFIX}")
    assert {p.name for p in dirs["x"].iterdir()} == want_files
    # without the flag: no new file, no new stdout byte
    assert sorted(p.name for p in dirs["cut"].iterdir()) == ["edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq"]
    assert "verlap" not in out["cut"].stdout and "clipp" not in out["cut"].stdout
    # stdout: the display line and the clipped pairs, nothing else
    so = out["x"].stdout
    line, res = _display_line(mo, M), f"Num. overlap-clipped pairs : {info['clipped']}\n"
    assert line in so and res in so
    assert so.index("Num. edited reads :") < so.index(res) < so.index("Num. passed pairs")
    same = _stable(so).replace(line, "").replace(res, "")
    if clip_info:
        clip_line = f"\tAdapter clipping     : 6 probes, min overlap {probe_mo} (--clip-adapters)\n"
        clip_res = f"Num. clipped reads : {clip_info[0]['clipped']} (mate 1)\n"
        assert so.index(line) < so.index(clip_line) and so.index(res) < so.index(clip_res)
        same = same.replace(clip_line, "").replace(clip_res, "")
    same = same.replace(str(dirs["x"]), str(dirs["cut"])).replace("x_1.fq", "cut_1.fq").replace("x_2.fq", "cut_2.fq")
    same = same.replace("x.fq", "cut.fq").replace(": 1 MB of FastQ text", ": 256 MB of FastQ text")
    assert same == _stable(out["cut"].stdout)
    assert out["x"].stderr == out["cut"].stderr


def test_no_records(tmp_path):
    (tmp_path / "in.fq").write_bytes(b"")
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "-o", tmp_path, *EDIT, "--clip-overlap"])
    assert "Num. overlap-clipped pairs : 0\n" in r.stdout
    zero = dict(pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0])
    assert (tmp_path / f"in.fq_1.{SUFFIX}").read_bytes() == R.render(zero)
