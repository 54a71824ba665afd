"""The case table of the combined tests (a helper, not collected; host only).

Every per-feature suite runs its feature alone.  The cases here run the stats
add-ons together on one stream and one mask, and `edit --clip-adapters` under
drawn trim and filter flags, at two layers:

  lib_case(i)       0 .. N_LIB - 1       the add-on handles on the engine's stream (C-ABI)
  lib_clip_case(i)  0 .. N_LIB_CLIP - 1  hpgq_clip in front of an edit engine (C-ABI)
  cli_case(i)       0 .. N_CLI - 1       `hpg-fastq stats` with the add-on flags
  cli_edit_case(i)  0 .. N_CLI_EDIT - 1  `hpg-fastq edit --clip-adapters`

What a case fixes by its number (so that tests/test_combined_cases_cpu.py can
hold the table to its coverage conditions): whether a filter is on, the input
layout, how many add-ons it draws.  Everything else is a seeded draw: the engine
parameters are test_fuzz_gpu._params', redrawn until the subcommand and the
filter are the case's and, with a filter, between 5 % and 95 % of the reads
(pairs) pass.  On top of the reads, so that no add-on's output is trivial:
a probe of the case's set in a third of the reads (some at position 0, some
ending on the last byte, every ninth read ending inside a probe), and
whole-read (whole-pair) copies of a handful of counted reads, at least three of
which reach the case's overrepresented min-count.

Expected values come from the references the per-feature suites use
(oracle_lib, qdist_ref, dup_ref, overrep_ref, adapt_ref, clip_ref), every add-on
over the reads (pairs) whose oracle mask is 1 with a filter, over all without."""
import functools

import numpy as np

import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
import adapt_ref
import clip_ref
import dup_ref
import overrep_ref
import qdist_ref
from fastq_io import to_fastq
from test_fuzz_gpu import _params, _reads, ROUTES
from test_adapt_cli_gpu import OWN, OWN_FILE  # noqa: F401  (OWN_FILE: the CLI tests write it)
from test_clip_cli_gpu import FORMS

N_LIB, N_LIB_CLIP, N_CLI, N_CLI_EDIT = 48, 8, 24, 12
ADDONS = ("kmers", "cg", "qdist", "dup", "overrep", "adapt")
PAIRED_ADDONS = ("qdist", "dup", "overrep", "adapt")     # (the CLI refuses --kmers and --cg on pairs)
DEF = adapt_ref.DEFAULT_PROBES
DEF_NAMES = [n for n, _ in adapt_ref.DEFAULTS]
OWN_PROBES, OWN_NAMES = [p for _, p in OWN], [n for n, _ in OWN]
LAYOUTS = ("single", "two_files", "interleaved")
CLI_LMAX = (64, 150, 252, None)                          # None: the CLI's default, 1024
CG_BATCH = 300_000                                       # --cg-batch-size of the cases in 1 MB units
ATTEMPTS = 400


def sub(reads, lo, hi):
    """Reads lo .. hi - 1 as a batch of their own (offsets from 0)."""
    a, b = int(reads.idx[lo]), int(reads.idx[hi])
    return O.Reads(reads.seq[a:b].copy(), reads.qual[a:b].copy(), (reads.idx[lo:hi + 1] - reads.idx[lo]).astype(np.int32))


def lengths(reads):
    return np.diff(reads.idx.astype(np.int64))


def plant_probes(reads, probes, rng):
    """A probe in every third read that has room for it: at position 0 (i = 0 mod 15), ending on the
    last byte (i = 6 mod 15), else anywhere; every ninth read (i = 4 mod 9) ends in a probe's
    first 1 .. K - 1 bases.  The qualities stay."""
    seq = reads.seq.copy()
    for i in range(reads.n):
        a, b = int(reads.idx[i]), int(reads.idx[i + 1])
        p = np.frombuffer(probes[i % len(probes)], np.uint8)
        if i % 3 == 0 and b - a >= len(p):
            at = a if i % 15 == 0 else b - len(p) if i % 15 == 6 else a + int(rng.integers(0, b - a - len(p) + 1))
            seq[at:at + len(p)] = p
        if i % 9 == 4 and b > a:
            m = int(rng.integers(1, min(len(p), b - a + 1)))
            seq[b - m:b] = p[:m]
    return O.Reads(seq, reads.qual, reads.idx)


def plant_copies(mates, rng, mask, min_count):
    """Whole-read copies (of both mates of a pair): seven counted reads of 20 bases or more are
    written over other reads, so that they occur min_count + 9, + 4, + 0, + 0, 3, 2 and 2 times."""
    n = mates[0].n
    counts = [min_count + 9, min_count + 4, min_count, min_count, 3, 2, 2]
    ok = np.ones(n, bool) if mask is None else np.asarray(mask) == 1
    for r in mates:
        ok &= lengths(r) >= 20
    cand = np.nonzero(ok)[0]
    if len(cand) < len(counts) or n < 2 * sum(counts):
        return mates
    src = rng.choice(cand, size=len(counts), replace=False)
    rest = np.setdiff1d(np.arange(n), src)
    dst = rng.choice(rest, size=sum(counts) - len(counts), replace=False)
    pairs = [r.pairs() for r in mates]
    at = 0
    for s, c in zip(src, counts):
        for d in dst[at:at + c - 1]:
            for pr in pairs:
                pr[int(d)] = pr[int(s)]
        at += c - 1
    return [O.Reads.from_pairs(pr) for pr in pairs]


def _draw_params(rng, want_cmd, want_filter):
    """test_fuzz_gpu._params until the subcommand is an edit one or not, and the filter on or off."""
    for _ in range(ATTEMPTS):
        p, cmd, o = _params(rng)
        kind = "edit" if cmd.startswith("edit") else cmd
        if kind == want_cmd and (want_filter is None or bool(p.filter_on) == want_filter):
            return p, cmd, o
    raise AssertionError("no parameter draw of the wanted kind")


def _subset(rng, size, paired):
    pool = PAIRED_ADDONS if paired else ADDONS
    return tuple(sorted(rng.choice(len(pool), size=min(size, len(pool)), replace=False).tolist())), pool


def _mixed(mask):
    share = float(np.mean(np.asarray(mask) == 1))
    return 0.05 <= share <= 0.95


class StatsCase:
    """One stats case of either layer.  p: the engine's parameters (lmax: the case's); mates: one or
    two O.Reads; mask / counters: the oracle's at p.lmax; counted: the mask with a filter, else None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.nm = len(self.mates)
        self.mask, _, self.counters = O.run(self.p, *self.mates)
        self.filter = bool(self.p.filter_on)
        self.counted = self.mask if self.filter else None
        keep = np.ones(self.mates[0].n, bool) if self.counted is None else self.counted == 1
        self.longest_counted = max([int(lengths(r)[keep].max()) if keep.any() else 0 for r in self.mates])
        self.longest = max(int(lengths(r).max()) for r in self.mates)

    def has(self, name):
        return name in self.addons

    def counters_at(self, lmax):
        """The oracle's counter set in the layout of lmax (no read is long there)."""
        px = H.Params.from_buffer_copy(self.p)
        px.lmax = lmax
        c = O.run(px, *self.mates)[2]
        assert int(c[H.S_LONG_READS]) == 0
        return c

    def kmers(self, lmax):
        return O.kmers(self.mates[0], lmax, None if self.counted is None else np.asarray(self.counted, np.uint8))

    @functools.cached_property
    def qdist(self):
        return [qdist_ref.table_of(r, self.counted) for r in self.mates]

    @functools.cached_property
    def adapt(self):
        return [adapt_ref.table_of(r, self.probes, self.counted) for r in self.mates]

    @functools.cached_property
    def seqs(self):
        return [dup_ref.sequences(r.seq, r.idx, self.counted) for r in self.mates]

    @functools.cached_property
    def dup(self):
        return [dup_ref.table(s) for s in self.seqs]

    @functools.cached_property
    def overrep(self):
        """Per mate ([(key, count, bytes)] the list, how many qualify)."""
        return [overrep_ref.select(s, self.top_n, self.min_count) for s in self.seqs]

    def cgr(self, groups):
        """The oracle's tables after one fill call per group of read numbers."""
        dim2 = 1 << (2 * self.k)
        tables = (np.zeros(dim2, np.uint32), np.zeros(dim2, np.uint32), np.zeros(1, np.uint32))
        r = self.mates[0]
        for lo, hi in groups:
            if hi > lo:
                O.cgr(self.k, sub(r, lo, hi), self.p.phred, None if self.counted is None else self.counted[lo:hi].copy(),
                      H.CGR_ONLY_VALID_READS if self.filter else H.CGR_ALL_READS, tables)
        return tables

    def nontrivial(self):
        """The add-ons this case draws whose output would be trivial (none, the CPU test asserts)."""
        bad = []
        if self.has("adapt") and not all(info["with_any"] > 0 for _, info in self.adapt):
            bad.append("adapt")
        if self.has("dup") and not all(sum(1 for x in dup_ref.levels_of_table(t)["distinct_at"] if x) >= 2 for t in self.dup):
            bad.append("dup")
        if self.has("overrep") and not all(len(entries) > 0 for entries, _ in self.overrep):
            bad.append("overrep")
        return bad


def _stats_case(seed, i, layer, want_filter, paired, size, make_reads, extra):
    """The first attempt whose parameters and reads are the case's kind."""
    for attempt in range(ATTEMPTS):
        rng = np.random.default_rng([seed, i, attempt])
        p, _, o = _draw_params(rng, "stats", want_filter)
        kw = extra(rng, p, o)
        p = kw.pop("p", p)
        p.paired = int(paired)
        nm = 2 if paired else 1
        picks, pool = _subset(rng, size, paired)
        addons = tuple(pool[k] for k in picks)
        probes, names = (OWN_PROBES, OWN_NAMES) if rng.random() < 0.4 else (DEF, DEF_NAMES)
        min_count, top_n = int(rng.choice([3, 5, 8])), int(rng.choice([5, 20, 50]))
        mates = [plant_probes(make_reads(rng, p, kw, m), probes + [OWN_PROBES[1]], rng) for m in range(nm)]
        mask = O.run(p, *mates)[0]
        mates = plant_copies(mates, rng, mask if p.filter_on else None, min_count)
        c = StatsCase(layer=layer, number=i, attempt=attempt, p=p, o=o, addons=addons, probes=probes, names=names,
                      own=probes is OWN_PROBES, min_count=min_count, top_n=top_n, k=int(rng.choice([4, 5, 6])),
                      mates=mates, **kw)
        if (not c.filter or _mixed(c.mask)) and not c.nontrivial():
            return c
    raise AssertionError(f"{layer} case {i}: no draw in {ATTEMPTS} attempts")


# -- the library layer --------------------------------------------------------------------------

def _three(n, i):
    """small | large | small.  The small ones differ by nine reads: a caching allocator that got the
    first one's mask buffer back too early would hand the same block to the third."""
    n1 = 40 + (i * 13) % 150
    n3 = n1 - 9
    return [(0, n1), (n1, n - n3), (n - n3, n)]


@functools.lru_cache(maxsize=4)
def lib_case(i):
    """filter: off on every third case; paired: every fourth; 2 + i % 5 add-ons."""
    def reads(rng, p, kw, m):
        return _reads(rng, kw["n"], p.lmax, p.phred, p.lmax + 120)

    def extra(rng, p, o):
        return dict(n=int(rng.integers(600, 2500)))

    c = _stats_case(7100, i, "lib", i % 3 != 0, i % 4 == 3, 2 + i % 5, reads, extra)
    c.route = ROUTES[i % len(ROUTES)]
    c.sync_each = (i // 2) % 2 == 0
    c.batches = _three(c.n, i)
    return c


@functools.lru_cache(maxsize=4)
def lib_clip_case(i):
    """hpgq_clip in front of an edit / edit_stats engine: paired on the odd cases, the clip forms in turn."""
    form = sorted(FORMS)[i % 3]
    _, probes, names, mo = FORMS[form]
    paired = i % 2 == 1
    for attempt in range(ATTEMPTS):
        rng = np.random.default_rng([7200, i, attempt])
        p, cmd, o = _draw_params(rng, "edit", None)
        p.paired = int(paired)
        n = int(rng.integers(600, 2500))
        mates = [plant_probes(_reads(rng, n, p.lmax, p.phred, p.lmax + 120), DEF + OWN_PROBES[1:3], rng)
                 for _ in range(2 if paired else 1)]
        c = ClipCase(layer="lib", number=i, attempt=attempt, p=p, cmd=cmd, o=o, form=form, probes=probes, names=names,
                     min_overlap=mo, mates=mates, n=n)
        if c.ok():
            c.route = ROUTES[(i + 2) % len(ROUTES)]
            c.batches = _three(n, i)
            return c
    raise AssertionError(f"lib clip case {i}: no draw in {ATTEMPTS} attempts")


class ClipCase:
    """One clip case of either layer.  cut: clip_ref.Clipped per mate; kept: their kept reads;
    mask / trim / counters: the oracle's over the kept reads."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.nm = len(self.mates)
        self.cut = [clip_ref.Clipped(r, self.probes, self.min_overlap) for r in self.mates]
        self.kept = [O.Reads(c.seq, c.qual, c.idx) for c in self.cut]
        self.mask, self.trim, self.counters = O.run(self.p, *self.kept)
        self.filter = bool(self.p.filter_on)

    def counters_at(self, lmax):
        px = H.Params.from_buffer_copy(self.p)
        px.lmax = lmax
        c = O.run(px, *self.kept)[2]
        assert int(c[H.S_LONG_READS]) == 0
        return c

    def ok(self):
        n = self.mates[0].n
        return all(0 < c.info["clipped"] < n for c in self.cut) and (not self.filter or _mixed(self.mask))

    def nothing_then_too_short(self):
        """A read with bases, clipped to nothing, that then fails the length filter."""
        if not self.filter or self.p.min_read_length < 1:
            return False
        return any(bool(((c.pos == 0) & (lengths(r) > 0) & (self.mask == 0)).any()) for c, r in zip(self.cut, self.mates))

    def clipped_then_trimmed_both_sides(self):
        n = self.mates[0].n
        for m, (c, r) in enumerate(zip(self.cut, self.mates)):
            t = self.trim[m * n:(m + 1) * n]
            if bool(((c.pos < lengths(r)) & ((t & 0xFFFF) > 0) & ((t >> 16) > 0)).any()):
                return True
        return False


# -- the CLI layer ------------------------------------------------------------------------------

def _synth(rng, kw, phred, m):
    return O.synth(kw["n"], seed=int(rng.integers(1, 1 << 30)), L=kw["L"], trunc_pct=25, n_per_1024=8, phred=phred, mate=m)


def _cli_extra(rng, lmax, o, edit=False):
    L = int(rng.choice([60, 150, 250]))
    kw = dict(L=L, n=int(rng.integers(2_300_000, 3_400_000)) // (2 * L + 30), cli_lmax=lmax,
              workers=int(rng.integers(1, 3)))
    make = H.edit_params if edit else H.stats_params
    kw["p"] = make(lmax=lmax or 1024, **o)
    return kw


def mate_records(reads, layout, m):
    """[(header line, plus line)] of mate m's records as the case's files spell them."""
    if layout == "single":
        return [(f"@r{i} extra:{i % 7}".encode(), b"+") for i in range(reads.n)]
    return [(h, b"+" + h[1:] if m == 1 else b"+") for h in PL.mate_headers(reads.n, m + 1)]


def write_inputs(c, d):
    """The case's FASTQ file(s) in directory d -> (the CLI's input flags, the report base names,
    the record end offsets of a single-end text)."""
    ends = None
    if c.layout == "single":
        text, ends = to_fastq(c.mates[0])
        (d / "in.fq").write_bytes(text)
        return ["-f", d / "in.fq"], ("in.fq",), ends
    recs = [PL.records(r, PL.mate_headers(r.n, m + 1), plus_header=m == 1) for m, r in enumerate(c.mates)]
    if c.layout == "two_files":
        (d / "in_1.fq").write_bytes(b"".join(recs[0]))
        (d / "in_2.fq").write_bytes(b"".join(recs[1]))
        return ["--fq1", d / "in_1.fq", "--fq2", d / "in_2.fq"], ("in_1.fq", "in_2.fq"), ends
    (d / "in.fq").write_bytes(PL.interleave(*recs))
    return ["-f", d / "in.fq", "--interleaved"], ("in.fq_1", "in.fq_2"), ends


def cg_groups(ends, batch):
    """[lo, hi) read numbers per chaos-game call: the records ending in ((j - 1) B, j B] (hpgq_reader.c)."""
    call = (np.asarray(ends, np.int64) - 1) // batch
    cuts = [0] + (np.nonzero(np.diff(call))[0] + 1).tolist() + [len(ends)]
    return list(zip(cuts[:-1], cuts[1:]))


@functools.lru_cache(maxsize=4)
def cli_case(i):
    """filter: off on every third case; layout: single, single, two files, interleaved in turn;
    2 + i % 5 add-ons; --lmax 64, 150, 252 or the default by (i // 2) % 4."""
    layout = ("single", "single", "two_files", "interleaved")[i % 4]
    lmax = CLI_LMAX[(i // 2) % 4]

    def reads(rng, p, kw, m):
        return _synth(rng, kw, p.phred, m)

    c = _stats_case(7300, i, "cli", i % 3 != 0, layout != "single", 2 + i % 5, reads,
                    lambda rng, p, o: _cli_extra(rng, lmax, o))
    c.layout = layout
    c.chunk_mb = (1, 1, 256)[i % 3] if i % 5 else 256
    return c


@functools.lru_cache(maxsize=4)
def cli_edit_case(i):
    """layout i % 3; the clip form by (i + i // 3) % 3; 1 MB units on 1 + i % 2 workers; every
    fourth case (i = 2 mod 4) has both edit windows and a clipped read that both of them trim."""
    layout = LAYOUTS[i % 3]
    form = sorted(FORMS)[(i + i // 3) % 3]
    _, probes, names, mo = FORMS[form]
    both = i % 4 == 2
    for attempt in range(ATTEMPTS):
        rng = np.random.default_rng([7400, i, attempt])
        _, _, o = _draw_params(rng, "edit", None)
        if both and not ("left_length" in o and "right_length" in o):
            continue
        kw = _cli_extra(rng, None, o, edit=True)
        p = kw.pop("p")
        p.paired = int(layout != "single")
        mates = [plant_probes(_synth(rng, kw, p.phred, m), DEF + OWN_PROBES[1:3], rng) for m in range(1 + p.paired)]
        kw["workers"] = 1 + i % 2
        c = ClipCase(layer="cli", number=i, attempt=attempt, p=p, o=o, form=form, probes=probes, names=names,
                     min_overlap=mo, mates=mates, layout=layout, **kw)
        if c.ok() and (not both or c.clipped_then_trimmed_both_sides()):
            return c
    raise AssertionError(f"cli edit case {i}: no draw in {ATTEMPTS} attempts")


def summary(c):
    """One line that names a case in an assertion message."""
    what = ",".join(c.addons) if hasattr(c, "addons") else c.form
    return (f"{c.layer} case {c.number} (attempt {c.attempt}): {what} nm={c.nm} lmax={c.p.lmax} phred={c.p.phred} "
            f"n={c.mates[0].n} {c.o}")
