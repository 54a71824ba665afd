#!/usr/bin/env python3
"""Rate of hpgq_dup_count_device next to the engine's C2
kernels, hpgq_kmers_count_device and hpgq_qdist_count_device on the same device
batch.

Reads are generated on the device (hpgq_synth_device, every read at full
length) and then rewritten on the device into three forms: all distinct; about
30 % of the reads copies of other reads; one sequence holding 10 % of the
reads.  Every call is timed between two HIP events on the stream it runs on,
after --warmup calls.  hpgq_dup_count_device is timed twice: into an emptied
table of its final size (every distinct sequence claims a slot) and again onto
the filled table (every key is found, adds only); the fingerprint and the insert
kernel separately (hpgq_dup_debug_set_timing) and the call as a whole.  Prints
one JSON line per form and writes them all to --out (profiles/dup_rate.json).
Bytes: fingerprint L + 5 + 8 per read, insert 8 + a 64-byte line per read.  Not
a test; fails without a GPU.

--keep adds the keep leg: per form and for thresholds 2 and
100, a table in keeping mode (hpgq_dup_keep_sequences) counted into when
emptied (the representatives are copied again) and onto itself filled (lookups
only): keep_kernel's time by its own events beside the fingerprint's and the
insert's of the same call, the representatives held and the arena bytes they
take (16 + the length rounded up to 16 each).  Lookup bytes: 8 + a 64-byte line
per read.  --only-dup leaves out the engine, k-mer and quality-distribution
calls and the masked leg.  With --keep the default --out is
profiles/overrep_rate.json.

    python tools/dup_rate.py [--reads 10000000] [--steps 10] [--warmup 3] [--out FILE] [--keep] [--only-dup]
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
L = 150


def timed(torch, stream, call, warmup, steps, before=None, after=None):
    out, extra = [], []
    for k in range(warmup + steps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        stream.synchronize()
        if k >= warmup:
            out.append(a.elapsed_time(b) * 1e3)   # us
            if after:
                extra.append(after())
    return out, extra


def summary(us, nbytes):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "bytes": nbytes, "fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", action="store_true", help="add the keep leg (thresholds 2 and 100)")
    ap.add_argument("--only-dup", action="store_true", help="time hpgq_dup_count_device only")
    ap.add_argument("--arena", type=int, default=1 << 31, help="--keep: arena bytes of the table")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "overrep_rate.json" if a.keep else "dup_rate.json")
    import torch
    if not torch.cuda.is_available():
        sys.exit("dup_rate: no GPU (rates are measured on the device or not at all)")
    import numpy as np
    import hpgfastq as H

    props = torch.cuda.get_device_properties(0)
    box = {"device": torch.cuda.get_device_name(0), "cus": props.multi_processor_count, "host": os.uname().nodename}
    n = min(a.reads, (2 ** 31 - 1024) // L)
    s = H.Synth(7, L, 0, 5, 1, 33, 0)   # trunc_pct 0: every read has L bases
    idx_h = np.zeros(n + 1, np.int32)
    H.check(H.lib.hpgq_synth_indices_host(C.byref(s), 0, n, idx_h.ctypes.data), "indices")
    total = int(idx_h[-1])
    assert total == n * L
    idx = torch.from_numpy(idx_h).cuda()
    seq0 = torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")
    qual = torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    p = H.stats_params(lmax=L, read_quality_range="20,", read_length_range="50,")
    results = []
    with H.Engine(p) as e:
        stream = torch.cuda.ExternalStream(e.stream)
        H.check(H.lib.hpgq_synth_device(C.byref(s), 0, n, seq0.data_ptr(), qual.data_ptr(), idx.data_ptr(), e.stream),
                "synth")
        e.sync()
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for form in ("all_distinct", "30pct_duplicates", "one_sequence_10pct"):
            seq = seq0.clone()
            rows, src = seq[:total].view(n, L), seq0[:total].view(n, L)
            if form == "30pct_duplicates":      # 30 % of the reads become copies of reads of the other 70 %
                perm = torch.randperm(n, device="cuda", generator=g)
                k = (3 * n) // 10
                rows[perm[:k]] = src[perm[k + torch.randint(0, n - k, (k,), device="cuda", generator=g)]]
            elif form == "one_sequence_10pct":
                perm = torch.randperm(n, device="cuda", generator=g)
                rows[perm[:n // 10]] = src[0]
            torch.cuda.synchronize()
            batch = H.engine.device_batch(n, seq.data_ptr(), qual.data_ptr(), idx.data_ptr())
            res = {"tool": "dup_rate", "form": form, "reads": n, "read_length": L, "bases": total,
                   "steps": a.steps, "warmup": a.warmup, **box}
            if not a.only_dup:
                us, _ = timed(torch, stream, lambda: e.run_device(batch, None, mask.data_ptr(), None), a.warmup, a.steps)
                res["engine_c2"] = summary(us, 2 * total + 5 * n)
                res["engine_c2"]["kernels"] = e.kernel_chain
                km = H.Kmers(L, stream=e.stream)
                us, _ = timed(torch, stream, lambda: km.count_device(batch, None), a.warmup, a.steps)
                km.close()
                res["kmers_all_reads"] = summary(us, total + 4 * n)
                with H.QualityDist(L, base=33, stream=e.stream) as q:
                    us, _ = timed(torch, stream, lambda: q.count_device(batch, None), a.warmup, a.steps)
                res["qdist_all_reads"] = summary(us, total + 4 * n)
            with H.Duplication(log2_slots=20, log2_max_slots=30, stream=e.stream) as d:
                d.count_device(batch, None)      # grows the table to its final size
                d.sync()
                lv = d.levels()
                assert lv["reads"] == n
                res.update(distinct=lv["distinct"], max_count=lv["max_count"], log2_slots=d.info()[0],
                           table_bytes=16 << d.info()[0])
                d.set_timing(True)
                fp_bytes, ins_bytes = total + 13 * n, 72 * n
                for label, before in (("dup_into_empty_table", d.reset), ("dup_onto_filled_table", None)):
                    us, parts = timed(torch, stream, lambda: d.count_device(batch, None), a.warmup, a.steps,
                                      before=before, after=d.last_times)
                    res[label] = summary(us, fp_bytes + ins_bytes)
                    res[label]["fingerprint_kernel"] = summary([x[0] for x in parts], fp_bytes)
                    res[label]["insert_kernel"] = summary([x[1] for x in parts], ins_bytes)
                if not a.only_dup:   # masked, as `stats --duplication --read-quality-range 20,` runs it
                    d.reset()
                    us, parts = timed(torch, stream, lambda: d.count_device(batch, mask.data_ptr()), a.warmup, a.steps,
                                      before=d.reset, after=d.last_times)
                    passed = int(mask.sum())
                    res["dup_masked_into_empty_table"] = summary(us, passed * (L + 72) + 13 * n)
                    res["dup_masked_into_empty_table"]["passed_reads"] = passed
                    assert d.levels()["reads"] == passed
            for threshold in (2, 100) if a.keep else ():
                with H.Duplication(log2_slots=20, log2_max_slots=30, stream=e.stream) as d:
                    d.keep_sequences(threshold, a.arena)
                    d.count_device(batch, None)      # grows the table to its final size
                    d.sync()
                    d.set_timing(True)
                    leg = {"arena_bytes": a.arena}
                    for label, before in (("into_empty_table", d.reset), ("onto_filled_table", None)):
                        us, parts = timed(torch, stream, lambda: d.count_device(batch, None), a.warmup, a.steps,
                                          before=before, after=lambda: d.last_times() + (d.last_keep_time(),))
                        d.sync()                     # (raises if a representative did not fit)
                        held = d.kept()
                        leg[label] = summary(us, fp_bytes + ins_bytes + 72 * n)
                        leg[label]["fingerprint_kernel"] = summary([x[0] for x in parts], fp_bytes)
                        leg[label]["insert_kernel"] = summary([x[1] for x in parts], ins_bytes)
                        leg[label]["keep_kernel"] = summary([x[2] for x in parts], 72 * n)
                        leg[label].update(kept_sequences=held[0], kept_bytes=held[1],
                                          arena_bytes_used=16 * held[0] + (L + 15) // 16 * 16 * held[0])
                    assert d.levels()["reads"] == n * (a.warmup + a.steps + 1)
                    res["keep_at_%d" % threshold] = leg
            print(json.dumps(res), flush=True)
            results.append(res)
            del seq, rows
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
