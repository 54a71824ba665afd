"""The engine kernels' LDS layout (hpg-fastq_amd/csrc/hpgq_engine_lds.h), checked
on the CPU: the header both the kernels and the host take every LDS offset
and the launch's byte count from is compiled by a plain host compiler
(tests/lds_layout/, UBSan) and prints, per kernel instance and lmax, bytes()
and every region.

(a) bytes() equals the byte count the host computed by hand before the layout
    header existed (seg_lds / catch_all_lds of commit 547bfb6, restated here
    independently): it decides the workgroups per CU and with them every grid.
(b) every region lies inside [0, bytes());
(c) no two regions that are live at the same time overlap; the two documented
    reuses (pos_fix's wave totals in the segmented kernels' mask table and in
    the catch-all's compaction scratch, both after the unit loop) lie inside
    the region they reuse;
(d) 16 B alignment for the read tables, DMA rows, ST buffers and the mask
    table, 8 B for sc, the deferral word and the mean-quality slots;
(e) bytes() <= 160 KiB (the LDS of a CU).
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

LMAX = [1, 2, 155, 156, 157, 160, 161, 251, 252, 253, 1023, 1024]
GEO = {0: dict(block=54, pos=160, nw=2), 1: dict(block=48, pos=156, nw=4), 2: dict(block=60, pos=252, nw=4)}
X_NOOR, X_LR, X_ST = 1, 2, 4
WAVES, FX_WORDS, ST_WORDS, SCALARS, MEANQ_BINS, GC_BINS, COLD_BYTES = 4, 64, 2 * (64 * 4 + 8), 8, 256, 101, 136
ALIGN = {"tab": 16, "dma_row": 16, "stbuf": 16, "mtab": 16, "sc": 8, "dword": 8, "fxs": 8}
REUSES = {"seg": {"pos_fix_wtot": "mtab"}, "catch_all": {"pos_fix_wtot": "scratch"}}


def parent_seg_lds(nm, geo, xm, edit, follow, lmax):
    """seg_lds() of the parent commit (hpgq_engine.hip), with plan_chain's arguments."""
    pos, block = GEO[geo]["pos"], GEO[geo]["block"]
    lp = min(lmax, pos)
    hlen = lp + 1 + MEANQ_BINS + GC_BINS
    mate_words = 6 * lp + ((hlen + 1) & ~1) + 2 * SCALARS
    lists = 1 + (1 if xm & X_NOOR else 0) + (1 if xm & X_LR else 0)
    tdma = edit and not follow and nm == 2 and xm == 0
    dma_words = nm * 3 * block * 4 if tdma else 0
    st_words = ST_WORDS if xm & X_ST else 0
    return (nm * mate_words * 4 + 16 + 17 * 16 + (pos + 1) * 4
            + WAVES * (nm * (2 * 256 + 64 * lists + FX_WORDS) + 64 + 4 + dma_words + st_words) * 4)


def parent_catch_all_lds(nm, lmax):
    """catch_all_lds() of the parent commit."""
    hlen = lmax + 1 + MEANQ_BINS + GC_BINS
    hist_words = (nm * hlen + 1) & ~1
    return (nm * 6 * lmax + hist_words) * 4 + nm * SCALARS * 8 + COLD_BYTES + WAVES * 64 * 4


def expected_instances():
    seg = [(g, nm, xm, e, 0) for g in (0, 1, 2) for nm in (1, 2) for e in (0, 1) for xm in (0, X_NOOR, X_LR, X_NOOR | X_LR)]
    seg.append((1, 1, X_ST, 1, 0))
    seg += [(2, nm, xm, e, 1) for nm in (1, 2) for e in (0, 1) for xm in (0, X_NOOR, X_LR, X_NOOR | X_LR)]
    return {("seg",) + s for s in seg} | {("catch_all", nm) for nm in (1, 2)}


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """[(instance key, lmax, bytes, [(name, begin, end, align, reuses)])]"""
    out = tmp_path_factory.mktemp("lds_layout")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "lds_layout"), f"OUT={out}"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(out / "lds_layout_main")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "I":
            kv = {k: int(v) for k, v in (x.split("=") for x in f[2:])}
            key = (("seg", kv["geo"], kv["nm"], kv["xm"], kv["edit"], kv["follow"]) if f[1] == "seg"
                   else ("catch_all", kv["nm"]))
            if f[1] == "seg":
                assert (kv["block"], kv["pos"]) == (GEO[kv["geo"]]["block"], GEO[kv["geo"]]["pos"]), line
            rows.append((key, kv["lmax"], kv["bytes"], []))
        else:
            assert f[0] == "R" and rows, line
            rows[-1][3].append((f[1], int(f[2]), int(f[3]), int(f[4]), f[5]))
    return rows


def test_every_instance_and_lmax_is_printed(layouts):
    assert {r[0] for r in layouts} == expected_instances()
    assert len(layouts) == len(expected_instances()) * len(LMAX) == 67 * 12
    for key in expected_instances():
        assert [r[1] for r in layouts if r[0] == key] == LMAX, key


def test_bytes_equal_the_parents_formulas(layouts):
    """(a), (e)"""
    for key, lmax, nbytes, _ in layouts:
        want = parent_seg_lds(key[2], key[1], key[3], key[4], key[5], lmax) if key[0] == "seg" \
            else parent_catch_all_lds(key[1], lmax)
        assert nbytes == want, (key, lmax, nbytes, want)
        assert nbytes <= 160 * 1024, (key, lmax, nbytes)


def test_regions_fit_do_not_overlap_and_are_aligned(layouts):
    """(b), (c), (d)"""
    for key, lmax, nbytes, regions in layouts:
        what = (key, lmax)
        names = {r[0] for r in regions}
        assert len(names) == len(regions), what
        live, reuse = [], []
        for name, begin, end, align, reuses in regions:
            kind = re.match(r"\w+", name).group(0)
            assert 0 <= begin < end <= nbytes, (what, name, begin, end, nbytes)                   # (b)
            assert align >= ALIGN.get(kind, 4) and begin % align == 0, (what, name, begin, align)   # (d)
            if reuses == "-":
                assert kind not in REUSES[key[0]], (what, name)
                live.append((begin, end, name))
            else:   # a documented reuse: inside the region it takes over
                assert REUSES[key[0]].get(kind) == re.match(r"\w+", reuses).group(0) and reuses in names, (what, name)
                reuse.append((begin, end, name, reuses))
        live.sort()
        for (b0, e0, n0), (b1, e1, n1) in zip(live, live[1:]):                                      # (c)
            assert e0 <= b1, (what, n0, (b0, e0), n1, (b1, e1))
        assert len(reuse) == 1, what
        for begin, end, name, reuses in reuse:
            host = next(r for r in regions if r[0] == reuses)
            assert host[1] <= begin and end <= host[2], (what, name, reuses)
        # the regions the kernels of every variant must have
        kinds = {re.match(r"\w+", n).group(0) for n in names}
        if key[0] == "seg":
            _, geo, nm, xm, edit, follow = key
            tdma = bool(edit and not follow and nm == 2 and xm == 0)
            want = {"pos_acc", "other", "hist", "sc", "tab", "ends", "fxs", "scratch", "dword", "mtab", "rtab",
                    "pos_fix_wtot"} | ({"ends2"} if xm & X_NOOR else set()) | ({"ends3"} if xm & X_LR else set()) \
                | ({"stbuf"} if xm & X_ST else set()) | ({"dma_row"} if tdma else set())
            assert kinds == want, (what, kinds ^ want)
            assert sum(n.startswith("tab[") for n in names) == 2 * nm * WAVES, what
            assert sum(n.startswith("dma_row[") for n in names) == (3 * nm * WAVES if tdma else 0), what
            mask = next(r for r in regions if r[0].startswith("mtab["))
            nw = GEO[geo]["nw"]
            assert mask[2] - mask[1] == (4 * nw + 1) * nw * 4, what
        else:
            assert kinds == {"pos_acc", "hist", "sc", "cold", "scratch", "pos_fix_wtot"}, what
            assert sum(n.startswith("scratch[") for n in names) == WAVES, what
