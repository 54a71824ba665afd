#!/usr/bin/env python3
"""End-to-end rates of paired-end `hpg-fastq stats`, and what the
pipeline's paired refactor costs single-end input.

Two synthetic mate files (tools/fqgen.c, --reads records each, seeds 2 and 3,
150 bp, the same names in both) are written to --dir.

  (a) single-end `stats` and `filter` (stored through the mapped writer) on mate
      1's file, end to end, this tree's CLI against --parent-cli (a build of the
      parent commit) on one box: one warm-up round, then --reps alternating runs
      each; medians and the min-max spread.
  (b) paired `stats` on both files and on an interleaved file of half as many
      pairs, against --parent-cli in the same way: pairs/s and FASTQ GB/s next
      to (a)'s GB/s.
  (c) with --trace: a rocprofv3 kernel trace (a run of its own, not timed) of a
      two-file and of an interleaved paired run over --trace-pairs pairs; the
      time of pair_check_kernel and of the de-interleaving (the two extra scans'
      share is inside the scan kernels; split_copy_kernel against copy_kernel)
      as shares of the parse kernels' time.

Times are the CLI's own clock (reader start to counters merged), parsed from its
"Throughput" line.  Writes one JSON file; fails without a GPU
(the CLI has no CPU path).

    python tools/pe_rate.py profiles/pe_rate.json [--reads 10000000] [--reps 5] \
        [--parent-cli PATH] [--trace] [--dir /dev/shm]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hpg-fastq_amd", "hpg-fastq")
PARSE_KERNELS = ("nl_count_kernel", "nl_write_kernel", "record_kernel", "copy_kernel", "split_copy_kernel",
                 "pair_check_kernel", "scan", "Scan", "lookback")


FILTER = ["--read-quality-range", "20,", "--read-length-range", "50,"]


def run_cli(cli, command, inputs, outd, threads):
    """One `stats` or `filter` run: (seconds, GB of FASTQ, reads or pairs) from the CLI's Throughput line."""
    shutil.rmtree(outd, ignore_errors=True)
    os.makedirs(outd)
    r = subprocess.run([cli, command, *inputs, *(FILTER if command == "filter" else []), "-o", outd, "--gpus", "1",
                        "--gpu", "0", "--lmax", "150", "--num-threads", str(threads)],
                       capture_output=True, text=True, timeout=600)
    m = re.search(r"Throughput: (\d+) \w+, ([0-9.]+) GB of FastQ in ([0-9.]+) s", r.stdout)
    if r.returncode or not m:
        sys.exit(f"pe_rate: {cli} {inputs} -> {r.returncode}\n{r.stdout[-400:]}\n{r.stderr[-400:]}")
    return float(m.group(3)), float(m.group(2)), int(m.group(1))


def summary(runs):
    s = [x[0] for x in runs]
    med = statistics.median(s)
    gb, n = runs[0][1], runs[0][2]
    return {"seconds_runs": s, "seconds_median": round(med, 4), "seconds_min": min(s), "seconds_max": max(s),
            "fastq_GB": gb, "records": n, "GB_per_s": round(gb / med, 3), "M_per_s": round(n / med / 1e6, 3)}


def compare(label, command, inputs, outd, a):
    """`command` on `inputs`, end to end: this tree's CLI and, with --parent-cli, the parent's on one box,
    one warm-up round, then --reps alternating runs each; medians and the min-max spread.  The tree's
    median is within the parent's spread when it is no further above the parent's median than that."""
    clis = [("this_tree", CLI)] + ([("parent", a.parent_cli)] if a.parent_cli else [])
    runs = {name: [] for name, _ in clis}
    for rep in range(a.reps + 1):          # round 0: warm-up, not counted
        for name, cli in clis:
            t = run_cli(cli, command, inputs, outd, a.threads)
            if rep:
                runs[name].append(t)
            print(label, name, rep, t[0], flush=True)
    res = {name: summary(v) for name, v in runs.items()}
    if a.parent_cli:
        p, t = res["parent"], res["this_tree"]
        res["parent_spread_s"] = round(p["seconds_max"] - p["seconds_min"], 4)
        res["median_difference_s"] = round(t["seconds_median"] - p["seconds_median"], 4)
        res["within_parent_spread"] = t["seconds_median"] - p["seconds_median"] <= p["seconds_max"] - p["seconds_min"]
    return res


def interleave(f1, f2, out, pairs):
    """The first `pairs` records of f1 and f2, alternating, into `out`."""
    with open(f1, "rb") as a, open(f2, "rb") as b, open(out, "wb") as o:
        for _ in range(pairs):
            o.writelines([a.readline(), a.readline(), a.readline(), a.readline(),
                          b.readline(), b.readline(), b.readline(), b.readline()])


def first_records(path, n):
    """The first n four-line records of a FASTQ file, as a list of bytes."""
    out, lines = [], []
    with open(path, "rb") as f:
        for ln in f:
            lines.append(ln)
            if len(lines) == 4:
                out.append(b"".join(lines))
                lines = []
                if len(out) == n:
                    break
    return out


def kernel_trace(inputs, outd, tdir, threads):
    """Kernel totals (us) of one paired run under rocprofv3 --kernel-trace --stats."""
    shutil.rmtree(outd, ignore_errors=True)
    os.makedirs(outd)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "run", "--output-format", "csv",
                        "--", CLI, "stats", *inputs, "-o", outd, "--gpus", "1", "--gpu", "0", "--lmax", "150",
                        "--num-threads", str(threads), "--quiet"], capture_output=True, text=True, timeout=600)
    files = glob.glob(os.path.join(tdir, "**", "run_kernel_stats.csv"), recursive=True)
    if r.returncode or not files:
        return {"error": (r.stderr or r.stdout)[-300:]}
    us = {}
    for row in csv.DictReader(open(files[0])):
        us[row["Name"]] = us.get(row["Name"], 0.0) + float(row["TotalDurationNs"]) / 1e3
    parse = sum(v for k, v in us.items() if any(p in k for p in PARSE_KERNELS))
    pick = lambda name: sum(v for k, v in us.items() if name in k)   # noqa: E731
    res = {"kernel_us": {k: round(v, 1) for k, v in sorted(us.items(), key=lambda kv: -kv[1])},
           "parse_kernels_us": round(parse, 1)}
    if parse > 0:
        res["pair_check_share_of_parse"] = round(pick("pair_check_kernel") / parse, 4)
        res["split_copy_share_of_parse"] = round(pick("split_copy_kernel") / parse, 4)
        res["scans_share_of_parse"] = round(sum(v for k, v in us.items()
                                                if any(p in k for p in ("scan", "Scan", "lookback"))) / parse, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_json")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-pairs", type=int, default=1_000_000)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    # (no GPU: the first CLI run ends with "no HIP device" and so does this tool)
    tmp = tempfile.mkdtemp(prefix="hpgq_pe_")
    tag = f"hpgq_pe_{os.getpid()}"
    f1, f2, fi = (os.path.join(a.dir, f"{tag}_{m}.fq") for m in (1, 2, "i"))
    outd = os.path.join(a.dir, f"{tag}_out")
    small = [os.path.join(a.dir, f"{tag}_s{m}.fq") for m in (1, 2, "i")]
    res = {"tool": "pe_rate", "reads_per_file": a.reads, "reps": a.reps, "threads": a.threads,
           "clock": "the CLI's own (reader start to merged counters)"}
    try:
        gen = os.path.join(tmp, "fqgen")
        subprocess.run(["gcc", "-O2", "-fopenmp", os.path.join(ROOT, "tools", "fqgen.c"), "-o", gen], check=True,
                       timeout=120)
        for f, seed in ((f1, 2), (f2, 3)):
            subprocess.run([gen, f, str(a.reads), "150", str(seed)], check=True, timeout=600,
                           env=dict(os.environ, OMP_NUM_THREADS=str(a.threads)))
        # (a) single-end `stats` and `filter` (the mapped writer), (b) paired `stats` from two files and
        # from one interleaved file of half as many pairs: this tree against the parent build, alternating
        res["single_end"] = compare("single", "stats", ["-f", f1], outd, a)
        res["single_end_filter"] = compare("filter", "filter", ["-f", f1], outd, a)
        res["paired"] = compare("paired", "stats", ["--fq1", f1, "--fq2", f2], outd, a)
        interleave(f1, f2, fi, a.reads // 2)
        res["interleaved"] = compare("interleaved", "stats", ["--interleaved", "-f", fi], outd, a)
        for k in ("paired", "interleaved"):
            t = res[k]["this_tree"]
            t["pairs_per_s"] = round(t["records"] / t["seconds_median"])
        # (c) kernel trace, a run of its own
        if a.trace:
            r1, r2 = first_records(f1, a.trace_pairs), first_records(f2, a.trace_pairs)
            open(small[0], "wb").write(b"".join(r1))
            open(small[1], "wb").write(b"".join(r2))
            with open(small[2], "wb") as f:
                for x, y in zip(r1, r2):
                    f.write(x)
                    f.write(y)
            res["trace_pairs"] = len(r1)
            res["trace_two_files"] = kernel_trace(["--fq1", small[0], "--fq2", small[1]], outd,
                                                  os.path.join(tmp, "t2"), a.threads)
            res["trace_interleaved"] = kernel_trace(["--interleaved", "-f", small[2]], outd,
                                                    os.path.join(tmp, "ti"), a.threads)
    finally:
        for f in [f1, f2, fi] + small:
            if os.path.exists(f):
                os.remove(f)
        shutil.rmtree(outd, ignore_errors=True)
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out_json)), exist_ok=True)
    json.dump(res, open(a.out_json, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
