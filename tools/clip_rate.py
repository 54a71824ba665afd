#!/usr/bin/env python3
"""Rate of hpgq_clip_find_device and hpgq_clip_device next to
hpgq_adapt_count_device on the same device batch and a device-to-device
hipMemcpyAsync of the same sequence + quality bytes.

Shapes, probe sets and fillings are tools/adapt_rate.py's: 10 M x 150 bp and
8.59 M x 250 bp reads of one length; the default 6 probes and 32 probes; random
A C G T with nothing planted, 20 % of the reads carrying the Illumina Universal
probe followed by A to the read's end, and every read all G (cut at 0).  Every
call is timed between two HIP events on the stream it runs on, after --warmup
calls, in one session.  Prints one JSON line per shape, probe set and filling: us
per launch (median, min, max) of the find pass (with and without the winners'
byte per read), of find + scan + copy, of the adapter-content kernel and of the
memcpy; find_vs_adapt is the ratio of the medians.  Not a test; fails without a
GPU.

    python tools/clip_rate.py [--reads 10000000] [--steps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpg-fastq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adapt_rate import timed, summary, fill   # noqa: E402

HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_rate: no GPU (rates are measured on the device or not at all)")
    import numpy as np
    import hpgfastq as H

    hip = C.CDLL("libamdhip64.so")   # (the runtime torch has loaded)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
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
        seq_out, qual_out = torch.empty_like(seq), torch.empty_like(qual)
        idx_out = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        pos = torch.empty(n, dtype=torch.int32, device="cuda")
        who = torch.empty(n, dtype=torch.uint8, device="cuda")
        batch = H.engine.device_batch(n, seq.data_ptr(), qual.data_ptr(), idx.data_ptr())

        def memcpy():
            for dst, src in ((seq_out, seq), (qual_out, qual)):
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), total, HIP_MEMCPY_DEVICE_TO_DEVICE, sp)
                assert rc == 0, rc

        for filling in ("none", "planted", "all_g"):
            carriers = fill(torch, seq, n, L, filling, gen)
            torch.cuda.synchronize()
            copy_us = timed(torch, stream, memcpy, a.warmup, a.steps)
            for set_name, probes in sets.items():
                with H.AdapterContent(probes, rows=L, stream=sp) as ad:
                    adapt_us = timed(torch, stream, lambda: ad.count_device(batch, None), a.warmup, a.steps)
                    ad.sync()
                with H.AdapterClip(probes, 8, stream=sp) as cl:
                    find_us = timed(torch, stream, lambda: cl.find(batch, pos.data_ptr(), who.data_ptr()), a.warmup, a.steps)
                    bare_us = timed(torch, stream, lambda: cl.find(batch, pos.data_ptr(), None), a.warmup, a.steps)
                    clip_us = timed(torch, stream, lambda: cl.clip_device(batch, seq_out.data_ptr(), qual_out.data_ptr(),
                                                                          idx_out.data_ptr(), pos.data_ptr(), who.data_ptr()),
                                    a.warmup, a.steps)
                    info = cl.info()
                kept = int(idx_out[-1].item())
                assert info["reads"] == 3 * n * calls and kept == total - info["bases_removed"] // (3 * calls), info
                if filling == "all_g":
                    assert kept == 0 and info["by_probe"][5] == info["clipped"] == info["reads"], info
                if filling == "planted":
                    assert info["clipped"] >= 3 * calls * carriers, info
                f, ad_ = summary(find_us, total + 9 * n, n), summary(adapt_us, total + 5 * n, n)
                res = {"tool": "clip_rate", "shape": name, "reads": n, "read_length": L, "bases": total,
                       "probe_set": set_name, "probes": len(probes), "longest_probe": max(len(p) for p in probes),
                       "min_overlap": 8, "filling": filling, "planted_reads": carriers,
                       "clipped_per_call": info["clipped"] // (3 * calls), "kept_bytes": kept, "steps": a.steps,
                       "warmup": a.warmup, **box,
                       "clip_find": f, "clip_find_no_probe_out": summary(bare_us, total + 8 * n, n), "adapt_count": ad_,
                       "find_vs_adapt": round(f["us_median"] / ad_["us_median"], 3),
                       # find + scan + copy: reads L + 4, writes 9 bytes per read, then moves the kept bytes twice
                       "clip_device": summary(clip_us, total + 13 * n + 4 * kept + 8 * n, n),
                       "memcpy_d2d_seq_qual": summary(copy_us, 4 * total, n)}
                print(json.dumps(res), flush=True)
        del seq, qual, idx, seq_out, qual_out, idx_out, pos, who
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
