"""`hpg-fastq stats` with several add-on flags at once, and `hpg-fastq edit
--clip-adapters` under drawn trim and filter flags, against the references (GPU;
the cases: tests/combined_lib.py, held to their coverage by
tests/test_combined_cases_cpu.py).

A stats case spells its drawn engine parameters as flags, as
tests/test_cli_fuzz_gpu.py does, adds the flags and dumps of two to six add-ons
(--kmers, --cg, --quality-dist, --duplication, --overrepresented, --adapters
with the default probes or an --adapter-file), --lmax 64 / 150 / 252 or the
default, 1 MB or 256 MB parse units on one or two workers, and single-end,
two-file or interleaved input.  Every dump is compared with its reference over
the reads (pairs) the oracle passes, every add-on's report file byte for byte
with the reference's render, the counter set with the oracle's at the longest
counted read.

An edit case runs the clip form and the drawn flags in 1 MB units.  The expected
edit*.fq and failed*.fq are assembled here from clip_ref's kept reads and the
oracle's mask and trims over them; <base>.adapter.clip.data from
clip_ref.render.

Measured on an MI355X: the slowest case 1.8 s (stats case 2: two mate files,
four add-ons, two workers), most under 1 s, which includes building the case
and its references; the 36 cases of the file 31 s in all.

That the cases fail when the code is wrong was checked with planted faults in
the worker's chunk step, none of them kept: mate 2's adapter count given mate 1's
batch (stats case 2 fails on mate 2's adapter table), the duplication count
given no mask under a filter (case 2, the duplication keys), the quality
table's reservation dropped (case 3: the run ends with "read longer than the
reserved rows"), and in the library the clip kernel's tail compare skipped (edit
case 2, edit_1.fq)."""
import numpy as np
import pytest

import hpgfastq as H
import adapt_ref
import clip_ref
import dup_ref
import overrep_ref
import qdist_ref
import cli_lib
import combined_lib as CL
from test_cli_fuzz_gpu import _flags

pytestmark = pytest.mark.gpu


def run_cli(args, **kw):
    return cli_lib.run_cli(list(args) + ["--gpus", 1], **kw)


def _addon_flags(c, d):
    """The add-ons' flags with their dumps in directory d."""
    out = []
    if c.has("kmers"):
        out += ["--kmers", "--kmers-out", d / "k.bin"]
    if c.has("cg"):
        out += ["--cg", "--k", c.k, "--cg-out", d / "cg.bin"] + (["--cg-batch-size", CL.CG_BATCH] if c.chunk_mb == 1 else [])
    if c.has("qdist"):
        out += ["--quality-dist", "--quality-dist-out", d / "q.bin"]
    if c.has("dup"):
        out += ["--duplication", "--duplication-out", d / "d.bin"]
    if c.has("overrep"):
        out += ["--overrepresented", "--overrepresented-min-count", c.min_count, "--overrepresented-top", c.top_n]
    if c.has("adapt"):
        out += ["--adapters", "--adapters-out", d / "a.bin"]
        if c.own:
            (d / "own.txt").write_bytes(CL.OWN_FILE)
            out += ["--adapter-file", d / "own.txt"]
    return out


@pytest.mark.parametrize("case", range(CL.N_CLI))
def test_stats_with_addons(tmp_path, case):
    c = CL.cli_case(case)
    p, nm, info = c.p, c.nm, CL.summary(c)
    inputs, bases, ends = CL.write_inputs(c, tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    args = ["stats", *inputs, "-o", out, *_flags(c.o), *_addon_flags(c, tmp_path), "--counters-out", tmp_path / "c.bin",
            "--chunk-mb", c.chunk_mb, "--gpu-workers", c.workers, "--quiet"]
    if c.cli_lmax is not None:
        args += ["--lmax", c.cli_lmax]
    info = f"{info} {[str(a) for a in args]}"
    run_cli(args)

    # the engine's counter set, in the layout of the longest counted read
    got = np.fromfile(tmp_path / "c.bin", np.uint64)
    L = max(p.lmax, c.longest_counted)
    assert got.size == H.counters_len(L) * nm, (info, got.size, L)
    np.testing.assert_array_equal(got, c.counters_at(L), err_msg=info + ": counters")

    if c.has("kmers"):
        got = np.fromfile(tmp_path / "k.bin", np.uint64)
        npos = got.size // 1024
        assert got.size == 1024 * npos and max(p.lmax, c.longest_counted) <= npos + 4 <= max(p.lmax, c.longest), (info, got.size)
        np.testing.assert_array_equal(got.reshape(1024, npos), c.kmers(npos + 4), err_msg=info + ": kmers")
    if c.has("cg"):
        got = np.fromfile(tmp_path / "cg.bin", np.uint32)
        groups = CL.cg_groups(ends, CL.CG_BATCH) if c.chunk_mb == 1 else [(0, c.mates[0].n)]
        assert c.chunk_mb != 1 or len(groups) > 3
        ts, tq, wc = c.cgr(groups)
        dim2 = 1 << (2 * c.k)
        np.testing.assert_array_equal(got[:dim2], ts, err_msg=info + ": chaos-game table")
        np.testing.assert_array_equal(got[dim2:2 * dim2], tq, err_msg=info + ": chaos-game quality table")
        assert got.size == 2 * dim2 + 1 and int(got[-1]) == int(wc[0]), info
    if c.has("qdist"):
        got = qdist_ref.parse_dump((tmp_path / "q.bin").read_bytes(), mates=nm)
        for m in range(nm):
            np.testing.assert_array_equal(got[m], c.qdist[m], err_msg=f"{info}: quality table, mate {m + 1}")
            assert (out / f"{bases[m]}.quality.dist.per.nt.data").read_bytes() == qdist_ref.render(c.qdist[m], p.phred), (info, m)
    if c.has("dup"):
        got = dup_ref.parse_dump((tmp_path / "d.bin").read_bytes(), mates=nm)
        for m in range(nm):
            wk, wc = dup_ref.arrays(c.dup[m])
            np.testing.assert_array_equal(got[m][0], wk, err_msg=f"{info}: duplication keys, mate {m + 1}")
            np.testing.assert_array_equal(got[m][1], wc, err_msg=f"{info}: duplication counts, mate {m + 1}")
            assert (out / f"{bases[m]}.duplication.data").read_bytes() == dup_ref.render(dup_ref.levels_of_table(c.dup[m])), (info, m)
    if c.has("overrep"):
        for m in range(nm):
            want = overrep_ref.render(c.overrep[m][0], len(c.seqs[m]))
            assert (out / f"{bases[m]}.overrepresented.data").read_bytes() == want, (info, m)
    if c.has("adapt"):
        got = adapt_ref.parse_dump((tmp_path / "a.bin").read_bytes(), mates=nm)
        for m in range(nm):
            np.testing.assert_array_equal(got[m][0], c.adapt[m][0], err_msg=f"{info}: adapter table, mate {m + 1}")
            assert got[m][1] == c.adapt[m][1], (info, m)
            assert (out / f"{bases[m]}.adapter.content.data").read_bytes() == adapt_ref.render(*c.adapt[m], c.names), (info, m)
    # and no add-on that was not asked for left a file
    suffixes = {"qdist": "quality.dist.per.nt.data", "dup": "duplication.data", "overrep": "overrepresented.data",
                "adapt": "adapter.content.data", "kmers": "kmers.txt"}
    names = [f.name for f in out.iterdir()]
    for a, suffix in suffixes.items():
        assert any(x.endswith(suffix) for x in names) == c.has(a), (info, a, names)


def _expected_edit_files(c):
    """name -> bytes of edit*.fq and failed*.fq: every mate's kept reads, trimmed, with the header
    and '+' lines as read, split by the oracle's mask."""
    n = c.mates[0].n
    files = {}
    for m in range(c.nm):
        lines = CL.mate_records(c.mates[m], c.layout, m)
        recs = []
        for i, (h, plus) in enumerate(lines):
            s, q = c.kept[m].read(i)
            t = int(c.trim[m * n + i])
            ts, te = t & 0xFFFF, t >> 16
            recs.append(h + b"\n" + s[ts:len(s) - te] + b"\n" + plus + b"\n" + q[ts:len(q) - te] + b"\n")
        tag = f"_{m + 1}" if c.nm == 2 else ""
        files[f"edit{tag}.fq"] = b"".join(r for r, k in zip(recs, c.mask) if k)
        if c.filter:
            files[f"failed{tag}.fq"] = b"".join(r for r, k in zip(recs, c.mask) if not k)
    return files


@pytest.mark.parametrize("case", range(CL.N_CLI_EDIT))
def test_edit_with_clipping(tmp_path, case):
    c = CL.cli_edit_case(case)
    info = CL.summary(c)
    inputs, bases, _ = CL.write_inputs(c, tmp_path)
    (tmp_path / "own.txt").write_bytes(CL.OWN_FILE)
    clip_flags = [str(tmp_path / f) if f == "own.txt" else f for f in CL.FORMS[c.form][0]]
    out = tmp_path / "out"
    out.mkdir()
    args = ["edit", *inputs, "-o", out, *_flags(c.o), *clip_flags, "--chunk-mb", 1, "--gpu-workers", c.workers, "--quiet"]
    info = f"{info} {[str(a) for a in args]}"
    run_cli(args)
    want = _expected_edit_files(c)
    for m in range(c.nm):
        want[f"{bases[m]}.adapter.clip.data"] = clip_ref.render(c.cut[m].info, c.names)
    assert sorted(f.name for f in out.iterdir()) == sorted(want), info
    for name, data in want.items():
        got = (out / name).read_bytes()
        if got != data:
            at = next((k for k, (a, b) in enumerate(zip(got, data)) if a != b), min(len(got), len(data)))
            raise AssertionError(f"{info}: {name} differs at byte {at} of {len(data)} (got {len(got)}): "
                                 f"{got[max(at - 60, 0):at + 60]!r} vs {data[max(at - 60, 0):at + 60]!r}")
