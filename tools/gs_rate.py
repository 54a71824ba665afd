#!/usr/bin/env python3
"""Rate of hpgq_gs_add_device next to hpgq_cgr_fill_device.

A device-resident synthetic FASTA (60-column lines, uniform ACGT, N at 1/1024)
is added --warmup + --steps times at k = 7 and k = 10, each call between two
HIP events on the stream it runs on; the chaos-game accumulator then takes the
same bases cut into 250-base reads (bench config C5's shape) at k = 7, timed
the same way, and k = 7 is timed once more after it to show the spread.
--e2e-gb G also times the `signature` command on a G GB file written to
--e2e-dir.  Prints one JSON line; fails without a GPU.

    python tools/gs_rate.py [--mb 256] [--steps 20] [--warmup 5] [--e2e-gb 1]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpg-fastq_amd"))


def pci_device_id(torch):
    p = torch.cuda.get_device_properties(0)
    bus = "%04x:%02x:%02x.0" % (getattr(p, "pci_domain_id", 0), getattr(p, "pci_bus_id", 0),
                                getattr(p, "pci_device_id", 0))
    try:
        return bus, open(f"/sys/bus/pci/devices/{bus}/device").read().strip()
    except OSError:
        return bus, None


def synth_fasta(torch, nbytes, seed):
    """(text u8 [~nbytes], bases u8 [rows * 60]) on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rows = max(nbytes // 61, 1)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    bases = lut[torch.randint(0, 4, (rows * 60,), generator=g, device="cuda")]
    bases[torch.randint(0, 1024, (rows * 60,), generator=g, device="cuda") == 0] = ord("N")
    lines = torch.empty((rows, 61), dtype=torch.uint8, device="cuda")
    lines[:, :60] = bases.view(rows, 60)
    lines[:, 60] = 10
    header = torch.tensor(list(b">chr1 synthetic\n"), dtype=torch.uint8, device="cuda")
    return torch.cat([header, lines.view(-1)]).contiguous(), bases


def timed(torch, stream, call, warmup, steps):
    """ms per call: events on the stream the calls run on."""
    for _ in range(warmup):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    stream.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def stats(ms, nbytes, nbases):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "text_GB_per_s": round(nbytes / med / 1e6, 2), "ns_per_kbase": round(med * 1e6 / nbases * 1e3, 3),
            "Gbases_per_s": round(nbases / med / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e-gb", type=float, default=0.0)
    ap.add_argument("--e2e-dir", default="/dev/shm")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gs_rate: no GPU (rates are measured on the device or not at all)")
    import numpy as np
    import hpgfastq as H

    text, bases = synth_fasta(torch, a.mb << 20, 1)
    nbytes, nbases = text.numel(), int((bases != ord("N")).sum())
    bus, dev_id = pci_device_id(torch)
    res = {"tool": "gs_rate", "device": torch.cuda.get_device_name(0), "pci_bus": bus, "pci_device_id": dev_id,
           "text_bytes": nbytes, "bases": nbases, "steps": a.steps, "warmup": a.warmup}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def gs_run(k):
        with H.Signature(k, stream=stream.cuda_stream) as sig:
            ms = timed(torch, stream, lambda: sig.add(text), a.warmup, a.steps)
            info = sig.info()
        calls = a.warmup + a.steps
        assert info["bases"] == nbases * calls and info["sequences"] == calls, info
        return stats(ms, nbytes, nbases)

    res["gs_k7"] = gs_run(7)

    # the same bases as 250-base reads through the chaos-game accumulator (C5's shape)
    nreads = bases.numel() // 250
    seq = torch.cat([bases[:nreads * 250], torch.zeros(H.DEVICE_SLACK, dtype=torch.uint8, device="cuda")])
    qual = torch.full_like(seq, 73)
    idx = (torch.arange(nreads + 1, device="cuda", dtype=torch.int64) * 250).to(torch.int32)
    torch.cuda.synchronize()
    cg = H.ChaosGame(7)
    cstream = torch.cuda.ExternalStream(cg.stream)
    batch = H.engine.device_batch(nreads, seq.data_ptr(), qual.data_ptr(), idx.data_ptr())
    ms = timed(torch, cstream, lambda: cg.fill_device(batch), a.warmup, a.steps)
    cg.sync()
    res["cgr_fill_k7_250"] = stats(ms, 2 * nreads * 250 + 4 * nreads, int((bases[:nreads * 250] != ord("N")).sum()))
    res["cgr_fill_k7_250"]["exact_redo"] = cg.last_exact()
    cg.close()

    res["gs_k10"] = gs_run(10)
    res["gs_k7_again"] = gs_run(7)
    res["gs_k7_over_cgr_per_base"] = round(res["gs_k7"]["ns_per_kbase"] / res["cgr_fill_k7_250"]["ns_per_kbase"], 3)

    if a.e2e_gb > 0:
        path = os.path.join(a.e2e_dir, "gs_rate_ref.fa")
        host = text.cpu().numpy()
        reps = max(-(-int(a.e2e_gb * 1e9) // host.size), 1)   # whole copies: at least --e2e-gb
        try:
            with open(path, "wb") as f:
                for _ in range(reps):
                    f.write(host.tobytes())
            out = path + ".fg"
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(ROOT, "hpg-fastq_amd", "hpg-fastq"), "signature", "-f", path,
                                    "--k", "7", "--gs-filename", out], capture_output=True, text=True, timeout=300)
                runs.append(round(time.perf_counter() - t0, 3))
                assert r.returncode == 0, r.stdout + r.stderr
            inside = [ln for ln in r.stdout.splitlines() if ln.startswith("Throughput")]
            t, w = H.cgr_load_gs(out, 7)
            assert int(np.asarray(t, dtype=np.uint64).sum()) == w
            res["cli_e2e"] = {"file_bytes": reps * host.size, "wall_s_runs": runs, "last_run": inside[0] if inside else None,
                              "words": w}
        finally:
            for p in (path, path + ".fg"):
                if os.path.exists(p):
                    os.remove(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
