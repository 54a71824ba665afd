#!/usr/bin/env python3
"""Rate of hpgq_qdist_count_device next to the engine's C2
kernels and hpgq_kmers_count_device on the same device batch.

Reads are generated on the device (hpgq_synth_device).  Shapes: 150 bp and 250
bp reads with as many rows as the reads are long, and the 150 bp reads with
1024 rows (the CLI's default --lmax).  Every call is timed between two HIP
events on the stream it runs on, after --warmup calls; with the engine's pass
mask of the C2 filter (what `stats --quality-dist --read-quality-range 20,`
runs) and without a mask.  Prints one JSON line per shape: us per launch and
(L + 5) * reads / time as a fraction of 8 TB/s.  Not a test; fails without a
GPU.

    python tools/qdist_rate.py [--reads 10000000] [--steps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpg-fastq_amd"))

HBM_PEAK = 8.0e12   # bytes / s


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


def summary(us, nbytes):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "bytes": nbytes, "fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("qdist_rate: no GPU (rates are measured on the device or not at all)")
    import numpy as np
    import hpgfastq as H

    props = torch.cuda.get_device_properties(0)
    box = {"device": torch.cuda.get_device_name(0), "cus": props.multi_processor_count,
           "pci_bus": "%04x:%02x:%02x.0" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0),
                                            getattr(props, "pci_device_id", 0)),
           "host": os.uname().nodename}
    for name, L, rows in (("150bp", 150, 150), ("250bp", 250, 250), ("150bp_rows1024", 150, 1024)):
        n = min(a.reads, (2 ** 31 - 1024) // L)   # data_indices are int32: < 2 GiB of bases per batch
        s = H.Synth(7, L, 5, 5, 1, 33, 0)
        idx_h = np.zeros(n + 1, np.int32)
        H.check(H.lib.hpgq_synth_indices_host(C.byref(s), 0, n, idx_h.ctypes.data), "indices")
        total = int(idx_h[-1])
        idx = torch.from_numpy(idx_h).cuda()
        seq = torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")
        qual = torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")
        mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
        p = H.stats_params(lmax=rows, read_quality_range="20,", read_length_range="50,")
        with H.Engine(p) as e:
            stream = torch.cuda.ExternalStream(e.stream)
            H.check(H.lib.hpgq_synth_device(C.byref(s), 0, n, seq.data_ptr(), qual.data_ptr(), idx.data_ptr(),
                                            e.stream), "synth")
            e.sync()
            batch = H.engine.device_batch(n, seq.data_ptr(), qual.data_ptr(), idx.data_ptr())
            res = {"tool": "qdist_rate", "shape": name, "reads": n, "read_length": L, "rows": rows, "bases": total,
                   "steps": a.steps, "warmup": a.warmup, **box}
            us = timed(torch, stream, lambda: e.run_device(batch, None, mask.data_ptr(), None), a.warmup, a.steps)
            e.sync()
            res["engine_c2"] = summary(us, 2 * total + 5 * n)
            res["engine_c2"]["kernels"] = e.kernel_chain
            passed = int(mask.sum())
            res["passed_reads"] = passed
            km = H.Kmers(rows, stream=e.stream)
            us = timed(torch, stream, lambda: km.count_device(batch, mask.data_ptr()), a.warmup, a.steps)
            km.sync()
            km.close()
            res["kmers_masked"] = summary(us, total + 5 * n)
            for label, mp in (("qdist_masked", mask.data_ptr()), ("qdist_all_reads", None)):
                with H.QualityDist(rows, base=33, stream=e.stream) as q:
                    us = timed(torch, stream, lambda: q.count_device(batch, mp), a.warmup, a.steps)
                    q.sync()
                    h = q.hist()
                calls = a.warmup + a.steps
                counted = total if mp is None else int(
                    (torch.diff(idx.to(torch.int64)) * (mask == 1)).sum())
                assert int(h.sum()) == counted * calls, (int(h.sum()), counted, calls)
                res[label] = summary(us, total + 5 * n)
                res[label]["counted_bases_per_call"] = counted
        print(json.dumps(res), flush=True)
        del seq, qual, idx, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
