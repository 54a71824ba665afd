#!/usr/bin/env python3
"""Rate of hpgq_adapt_count_device next to
hpgq_qdist_count_device and hpgq_kmers_count_device on the same device batch.

Shapes: 10 M x 150 bp and 8.59 M x 250 bp reads of one length, each with the
default 6 probes and with 32 probes (the default ones and 26 random ones of 8
.. 32 bases), in three fillings planted on the device with torch:
  none     random A C G T, nothing planted;
  planted  20 % of the reads carry the Illumina Universal probe at a start drawn
           from U[30, L - 12], followed by A to the read's end;
  all_g    every read all G: every start is a candidate until PolyG is found at 0.
Every call is timed between two HIP events on the stream it runs on, after
--warmup calls, without a mask.  Prints one JSON line per shape, probe set and
filling: us per launch and (L + 5) * reads / time as a fraction of 8 TB/s.  Not
a test; fails without a GPU.

    python tools/adapt_rate.py [--reads 10000000] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpg-fastq_amd"))

HBM_PEAK = 8.0e12   # bytes / s
UNIVERSAL = b"AGATCGGAAGAG"


def timed(torch, stream, call, warmup, steps):
    for _ in range(warmup):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    stream.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]   # us


def summary(us, nbytes, reads):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1), "bytes": nbytes,
            "fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4), "reads_per_us": round(reads / med, 1)}


def fill(torch, seq, n, L, filling, gen):
    """The n x L bases of `seq` for one filling -> the reads that carry the planted probe."""
    if filling == "all_g":
        seq[:n * L] = ord("G")
        return 0
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, n * L, step):
        m = min(step, n * L - lo)
        seq[lo:lo + m] = lut.index_select(0, torch.randint(0, 4, (m,), dtype=torch.int32, device="cuda", generator=gen))
    if filling == "none":
        return 0
    sel = torch.nonzero(torch.rand(n, device="cuda", generator=gen) < 0.2).flatten()
    start = torch.randint(30, L - 12 + 1, (sel.numel(),), device="cuda", generator=gen)
    probe = torch.tensor(list(UNIVERSAL), dtype=torch.uint8, device="cuda")
    view = seq[:n * L].view(n, L)
    step = 1 << 20
    for lo in range(0, sel.numel(), step):
        rows_i = sel[lo:lo + step]
        rel = torch.arange(L, device="cuda")[None, :] - start[lo:lo + step, None]
        rows = view[rows_i]
        rows = torch.where(rel >= 12, torch.full_like(rows, ord("A")), rows)
        rows = torch.where((rel >= 0) & (rel < 12), probe[rel.clamp(0, 11)], rows)
        view[rows_i] = rows
    return int(sel.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adapt_rate: no GPU (rates are measured on the device or not at all)")
    import numpy as np
    import hpgfastq as H

    props = torch.cuda.get_device_properties(0)
    box = {"device": torch.cuda.get_device_name(0), "cus": props.multi_processor_count, "host": os.uname().nodename}
    rng = np.random.default_rng(7)
    defaults = [p for _, p in H.adapt_defaults()]
    sets = {"default6": defaults,
            "probes32": defaults + [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(k))])
                                    for k in rng.integers(8, 33, size=26)]}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    calls = a.warmup + a.steps
    for name, L in (("150bp", 150), ("250bp", 250)):
        n = min(a.reads, (2 ** 31 - 1024) // L)   # data_indices are int32: < 2 GiB of bases per batch
        total = n * L
        idx = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * L).to(torch.int32)
        seq = torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")
        qual = torch.full((total + H.DEVICE_SLACK,), ord("I"), dtype=torch.uint8, device="cuda")
        batch = H.engine.device_batch(n, seq.data_ptr(), qual.data_ptr(), idx.data_ptr())
        nbytes = total + 5 * n
        for filling in ("none", "planted", "all_g"):
            carriers = fill(torch, seq, n, L, filling, gen)
            torch.cuda.synchronize()
            yard = {}
            with H.QualityDist(L, base=33, stream=sp) as q:
                yard["qdist_all_reads"] = summary(timed(torch, stream, lambda: q.count_device(batch, None), a.warmup, a.steps),
                                                  nbytes, n)
                q.sync()
            km = H.Kmers(L, stream=sp)
            yard["kmers_all_reads"] = summary(timed(torch, stream, lambda: km.count_device(batch, None), a.warmup, a.steps),
                                              nbytes, n)
            km.sync()
            km.close()
            for set_name, probes in sets.items():
                with H.AdapterContent(probes, rows=L, stream=sp) as ad:
                    us = timed(torch, stream, lambda: ad.count_device(batch, None), a.warmup, a.steps)
                    first, info = ad.table()
                assert info["reads"] == n * calls and info["npos"] == L, info
                if filling == "all_g":
                    assert int(first[5, 0]) == n * calls == info["with_any"] == int(first.sum()), info
                if filling == "planted":
                    assert int(first[0, 30:].sum()) >= carriers * calls and info["with_any"] >= carriers * calls, info
                res = {"tool": "adapt_rate", "shape": name, "reads": n, "read_length": L, "rows": L, "bases": total,
                       "probe_set": set_name, "probes": len(probes), "longest_probe": max(len(p) for p in probes),
                       "filling": filling, "planted_reads": carriers, "with_any_per_call": info["with_any"] // calls,
                       "steps": a.steps, "warmup": a.warmup, **box, "adapt_all_reads": summary(us, nbytes, n), **yard}
                print(json.dumps(res), flush=True)
        del seq, qual, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
