"""`hpg-fastq edit --clip-overlap --merge-overlap` end to end on the GPU
(DESIGN.md §2.15).

Metamorphic against the existing commands on texts that tests/ovl_merge_ref.py
builds in Python from a paired input X: edit_1/2.fq and failed_1/2.fq are byte
for byte what plain paired `edit` (no --clip-overlap) writes for the records of
the pairs that do not merge, and edit_merged.fq / failed_merged.fq what plain
single-end `edit` writes as edit.fq / failed.fq for the reference's merged
records -- so the trims and the filter saw the merged bytes.  Two-file and
interleaved input; once with --clip-adapters and --insert-size; once with
--chunk-mb 1 --gpu-workers 2; the .overlap.merge.data, .overlap.clip.data and
.insert.size.data files against the reference's renderers; the stdout lines; an
input of no records; one where every pair merges; and without the flag no new
file and no new stdout byte."""
import numpy as np
import pytest

import pairs_lib as PL
import ovl_ref as R
import ovl_fix_ref as X
import ovl_merge_ref as G
import cli_lib

pytestmark = pytest.mark.gpu

EDIT = ["--left-length", 10, "--left-quality-range", "20,", "--right-length", 30, "--right-quality-range", "20,",
        "--read-quality-range", "20,", "--read-length-range", "60,"]
MERGE, INS, CLIP = "overlap.merge.data", "insert.size.data", "overlap.clip.data"
FQ = ["edit_1.fq", "edit_2.fq", "failed_1.fq", "failed_2.fq"]
MFQ = ["edit_merged.fq", "failed_merged.fq"]
FLAGS = ["--clip-overlap", "--merge-overlap"]


def run_cli(args, **kw):
    return cli_lib.run_cli(list(args) + ["--gpus", 1, "--gpu-workers", 2], **kw)


def _stable(stdout):
    """stdout without the one line that holds the run's wall time."""
    return "".join(x for x in stdout.splitlines(True) if not x.startswith("Throughput:"))


def _records(pairs):
    heads = (PL.mate_headers(len(pairs), 1), PL.mate_headers(len(pairs), 2))
    rec = ([], [])
    for i, (s1, q1, s2, q2) in enumerate(pairs):
        rec[0].append((heads[0][i], s1, q1, False))
        rec[1].append((heads[1][i], s2, q2, True))
    return rec


@pytest.fixture(scope="module")
def case():
    """About 300 pairs of (header, seq, qual, plus_header) per mate: random pairs
    whose quality depends on read and position, a disagreement in every fourth
    overlapping pair, either mate winning, and three skipped pairs (a mate of 513
    bases) among them."""
    rng = np.random.default_rng(43)
    pairs = []
    for i, (s1, s2) in enumerate(R.random_pairs(297, 42, L=(70, 151))):
        q1 = bytes(33 + (7 * j + 3 * i) % 41 for j in range(len(s1)))
        q2 = bytes(33 + (5 * j + 11 * i) % 41 for j in range(len(s2)))
        F = R.find(s1, s2, 30, 5)
        if F > 0 and i % 4 == 1:
            ov = min(len(s1), F) - max(0, F - len(s2))
            s1, q1, s2, q2 = X.plant((s1, q1, s2, q2), F, ov // 2, 1 + i // 4 % 2, 33 + 38, 33 + 4)
        pairs.append((s1, q1, s2, q2))
        if i % 100 == 50:
            a, b = R.pair_of(rng, 513, 120, 100)
            pairs.append((a, bytes(33 + (3 * j) % 41 for j in range(513)), b, bytes(33 + (5 * j) % 41 for j in range(120))))
    rec = _records(pairs)
    want = G.merge_records(rec[0], rec[1])
    out1, out2, merged, info, minfo, hist = want
    assert len(rec[0]) == 300 and info["skipped"] == 3 and len(merged) > 100 and len(out1) > 80 and min(minfo["resolved"]) >= 5
    return rec, want


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


def _run(tmp_path, name, args):
    d = tmp_path / ("out_" + name)
    d.mkdir()
    r = run_cli(["edit", *args, "-o", d, *EDIT])
    return r, {p.name: p.read_bytes() for p in d.iterdir()}, d


def _references(tmp_path, want, layout, pair_flags=()):
    """Plain paired `edit` on the unmerged pairs' records, plain single-end `edit` on the merged records."""
    out1, out2, merged = want[:3]
    _, pairs, _ = _run(tmp_path, "ref_pairs", [*_inputs(tmp_path, "ref", (out1, out2), layout), *pair_flags])
    (tmp_path / "merged.fq").write_bytes(b"".join(_text(merged)))
    _, single, _ = _run(tmp_path, "ref_merged", ["-f", tmp_path / "merged.fq"])
    return pairs, single


def _same_reads(files, pairs, single):
    for name in FQ:
        assert files[name] == pairs[name], name
    assert files["edit_merged.fq"] == single["edit.fq"] and files["failed_merged.fq"] == single["failed.fq"]
    for name in ("edit_1.fq", "failed_1.fq", "edit_merged.fq", "failed_merged.fq"):   # (every class holds records)
        assert files[name].count(b"\n") >= 40, name


@pytest.mark.parametrize("layout", ["two_files", "interleaved"])
def test_paired(tmp_path, case, layout):
    rec, want = case
    info, minfo = want[3], want[4]
    out, files, d = _run(tmp_path, "x", [*_inputs(tmp_path, "x", rec, layout), *FLAGS])
    plain, clip_files, dclip = _run(tmp_path, "clip", [*_inputs(tmp_path, "x", rec, layout), "--clip-overlap"])
    pairs, single = _references(tmp_path, want, layout)
    base = "x_1.fq" if layout == "two_files" else "x.fq_1"
    _same_reads(files, pairs, single)
    assert files[f"{base}.{MERGE}"] == G.render(info, minfo)
    assert files[f"{base}.{CLIP}"] == R.render(info) == clip_files[f"{base}.{CLIP}"]
    assert sorted(files) == sorted(FQ + MFQ + [f"{base}.{s}" for s in (MERGE, CLIP)])
    # without the flag: no new file, no new stdout byte
    assert sorted(clip_files) == sorted(FQ + [f"{base}.{CLIP}"])
    assert "erge" not in plain.stdout
    so = out.stdout
    recs = lambda blob: blob.count(b"\n") // 4   # noqa: E731
    lines = ["\tOverlap merging      : pairs with an overlap become one read (--merge-overlap)\n",
             f"Num. merged pairs : {minfo['merged_pairs']} ({d}/edit_merged.fq)\n",
             f"\tNum. passed merged reads : {recs(single['edit.fq'])}\n",
             f"\tNum. failed merged reads : {recs(single['failed.fq'])}\n"]
    assert all(x in so for x in lines), so
    assert so.index("\tOverlap clipping ") < so.index(lines[0])
    assert so.index("Num. overlap-clipped pairs :") < so.index(lines[1]) < so.index(lines[2]) < so.index(lines[3]) < so.index("Num. passed pairs")
    # the existing pair lines count the pairs that did not merge
    assert f"Num. passed pairs : {recs(pairs['edit_1.fq'])} " in so
    assert f"Num. failed pairs : {recs(pairs['failed_1.fq'])} " in so
    same = _stable(so)
    for x in lines:
        same = same.replace(x, "")
    drop = ("Num. edited reads", "Num. passed pairs", "Num. failed pairs")
    keep = lambda text, dd: [x for x in text.replace(str(dd), "D").splitlines() if not x.startswith(drop)]   # noqa: E731
    assert keep(same, d) == keep(_stable(plain.stdout), dclip)
    assert out.stderr == plain.stderr


def test_with_adapter_clip_and_insert_sizes(tmp_path, case):
    """--clip-adapters cuts the unmerged pairs only; --insert-size counts in the merge call's find pass."""
    rec, want = case
    info, minfo, hist = want[3:]
    out, files, d = _run(tmp_path, "x", [*_inputs(tmp_path, "x", rec, "two_files"), *FLAGS, "--clip-adapters", "--insert-size"])
    pairs, single = _references(tmp_path, want, "two_files", ["--clip-adapters"])
    _same_reads(files, pairs, single)
    assert files[f"x_1.fq.{MERGE}"] == G.render(info, minfo)
    assert files[f"x_1.fq.{INS}"] == X.render_inserts(info, hist)
    assert files[f"x_1.fq.{CLIP}"] == R.render(info)
    assert files["x_1.fq.adapter.clip.data"] == pairs["ref_1.fq.adapter.clip.data"]
    assert files["x_2.fq.adapter.clip.data"] == pairs["ref_2.fq.adapter.clip.data"]


def test_small_chunks_two_workers(tmp_path, case):
    rec, want = case
    out, files, d = _run(tmp_path, "x", [*_inputs(tmp_path, "x", rec, "interleaved"), *FLAGS, "--chunk-mb", 1, "--gpu-workers", 2])
    pairs, single = _references(tmp_path, want, "interleaved")
    _same_reads(files, pairs, single)
    assert files[f"x.fq_1.{MERGE}"] == G.render(want[3], want[4])


def test_no_records(tmp_path):
    (tmp_path / "in.fq").write_bytes(b"")
    r = run_cli(["edit", "-f", tmp_path / "in.fq", "--interleaved", "-o", tmp_path, *EDIT, *FLAGS])
    assert f"Num. merged pairs : 0 ({tmp_path}/edit_merged.fq)\n" in r.stdout
    assert "\tNum. passed merged reads : 0\n" in r.stdout and "\tNum. failed merged reads : 0\n" in r.stdout
    zero = dict(pairs=0, skipped=0, overlapping=0, clipped=0, bases_removed=[0, 0])
    assert (tmp_path / f"in.fq_1.{MERGE}").read_bytes() == G.render(zero, G.info_of([], [0, 0]))
    for name in FQ + MFQ:
        assert (tmp_path / name).read_bytes() == b"", name


def test_every_pair_merges(tmp_path):
    rng = np.random.default_rng(44)
    pairs = []
    for i in range(40):
        n1, n2 = 90 + i % 30, 100 + i % 23
        pairs.append(X.clean(rng, n1, n2, 110 + i, i, phred=33, high=35, low=25))
    rec = _records(pairs)
    want = G.merge_records(rec[0], rec[1])
    assert len(want[2]) == 40 and want[0] == []
    out, files, d = _run(tmp_path, "x", [*_inputs(tmp_path, "x", rec, "two_files"), *FLAGS])
    (tmp_path / "merged.fq").write_bytes(b"".join(_text(want[2])))
    _, single, _ = _run(tmp_path, "ref_merged", ["-f", tmp_path / "merged.fq"])
    assert files["edit_merged.fq"] == single["edit.fq"] and files["failed_merged.fq"] == single["failed.fq"]
    assert files["edit_merged.fq"].count(b"\n") + files["failed_merged.fq"].count(b"\n") == 160
    for name in FQ:
        assert files[name] == b"", name
    assert files[f"x_1.fq.{MERGE}"] == G.render(want[3], want[4])
    assert "Num. merged pairs : 40 " in out.stdout and "Num. passed pairs : 0 " in out.stdout
