#!/usr/bin/env python3
"""Rate of hpgq_ovl_find_device and hpgq_ovl_batch_device next
to hpgq_clip_find_device on both mates of the same device batches, in one
session.

Shapes: 10 M x 150 bp and 8.59 M x 250 bp pairs of one length.  Fillings: random
A C G T mates that have nothing to do with each other ("none"); every pair from a
fragment of L + 1 .. 2 L - 30 bases, so the mates overlap and nothing is cut
("overlap"); 20 % of the pairs from a fragment of 30 .. L - 1 bases, both mates
going on with random bases behind it ("readthrough").  Every call is timed
between two HIP events on the stream it runs on, after --warmup calls.  Prints
one JSON line per shape and filling: us per call (median, min, max) of the
overlap find, of find + scan + copy of both mates, and of the two adapter find
passes (default probes, min overlap 8) together; ovl_vs_two_finds is the ratio of
the medians.  Everything also goes to --out (default profiles/ovl_rate.json).  Not a
test; fails without a GPU.

--correct and --inserts switch on the handle's overlap correction (phred 33,
thresholds 30 / 14) and its insert-size histogram for the
ovl_batch timing; the filling "short" (only with --fillings) makes every pair
from a fragment of 30 .. L - 1 bases and flips 1 % of mate 1's bases.  The
qualities run through 33 .. 73 along the batch, so facing bases differ in
quality.  --shapes / --fillings pick some of them, --only-batch times
hpgq_ovl_batch_device alone: for A/B runs of one call, each variant a process of
its own (HPGQ_LIB_PATH loads another build of the library).  --merge times
hpgq_ovl_merge_device alone in the same way: find, plan, the
copies of the unmerged pairs, the compaction and the merged reads.
--append-key KEY keeps what --out holds and appends the run's rows under KEY:
profiles/ovl_rate.json's "merge" is four such runs, parent and merge in turn.

    python tools/ovl_rate.py [--pairs 10000000] [--steps 20] [--warmup 5] [--out profiles/ovl_rate.json]
                             [--correct] [--inserts] [--shapes 150bp,250bp] [--fillings none,overlap,readthrough,short]
                             [--only-batch | --merge] [--append-key merge]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpg-fastq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adapt_rate import timed, summary   # noqa: E402


def fill_pairs(torch, seq1, seq2, n, L, filling, gen):
    """The n x L bases of both mates for one filling -> the pairs made from a fragment."""
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    comp = torch.tensor([3, 2, 1, 0], dtype=torch.int64, device="cuda")          # index of the complement in ACGT
    v1, v2 = seq1[:n * L].view(n, L), seq2[:n * L].view(n, L)
    made = 0
    step = 1 << 20
    col = torch.arange(L, device="cuda")[None, :]
    for lo in range(0, n, step):
        m = min(step, n - lo)
        frag = torch.randint(0, 4, (m, 2 * L), dtype=torch.int64, device="cuda", generator=gen)
        other = torch.randint(0, 4, (m, L), dtype=torch.int64, device="cuda", generator=gen)
        a, b = frag[:, :L], other
        if filling != "none":
            if filling == "overlap":
                F = torch.randint(L + 1, 2 * L - 30 + 1, (m, 1), device="cuda", generator=gen)
                on = torch.ones((m, 1), dtype=torch.bool, device="cuda")
            elif filling == "short":
                F = torch.randint(30, L, (m, 1), device="cuda", generator=gen)
                on = torch.ones((m, 1), dtype=torch.bool, device="cuda")
            else:
                F = torch.randint(30, L, (m, 1), device="cuda", generator=gen)
                on = torch.rand((m, 1), device="cuda", generator=gen) < 0.2
            # mate 2 base j is the complement of fragment base F - 1 - j; behind the fragment both mates are random
            src = (F - 1 - col).clamp(0, 2 * L - 1)
            rc = comp[frag.gather(1, src)]
            b = torch.where(on & (col < F), rc, other)
            a = torch.where(on & (col >= F), other.flip(1), a)
            if filling == "short":   # 1 % of mate 1's bases become another base
                a = torch.where(torch.rand((m, L), device="cuda", generator=gen) < 0.01, (a + 1) % 4, a)
            made += int(on.sum().item())
        v1[lo:lo + m] = lut[a]
        v2[lo:lo + m] = lut[b]
    return made


def write_profile(path, rows, steps, warmup, key=None):
    what = (f"tools/ovl_rate.py --steps {steps} --warmup {warmup} on one MI355X, one session: hpgq_ovl_find_device (min overlap "
            "30, max mismatches 5), hpgq_ovl_batch_device (find + scan + copy of both mates) and hpgq_clip_find_device on "
            "both mates of the same device batches (default probes, min overlap 8, no winners' byte); HIP events on the "
            "stream, us per call.  Fillings: none = unrelated random mates; overlap = every pair from a fragment of "
            "L+1 .. 2L-30 bases (found, nothing cut); readthrough = 20 % of the pairs from a fragment of 30 .. L-1 bases, "
            "random bases behind it in both mates.  Rows with ovl_merge: hpgq_ovl_merge_device alone (--merge; find, "
            "plan, the unmerged pairs' copies, the compaction and the merged reads), the pairs capped so that both mates' "
            "bytes together stay below 2 GiB.")
    if key:   # an A/B run's rows behind those already under `key` of the file; everything else in it stays
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[key] = {"what": what, "results": doc.get(key, {}).get("results", []) + rows}
    else:
        doc = {"what": what, "results": rows}
    with open(path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ovl_rate.json"))
    ap.add_argument("--correct", action="store_true", help="ovl_batch with the overlap correction on (33, 30, 14)")
    ap.add_argument("--inserts", action="store_true", help="ovl_batch with the insert sizes counted")
    ap.add_argument("--shapes", default="150bp,250bp")
    ap.add_argument("--fillings", default="none,overlap,readthrough")
    ap.add_argument("--only-batch", action="store_true", help="time hpgq_ovl_batch_device alone")
    ap.add_argument("--merge", action="store_true", help="time hpgq_ovl_merge_device alone")
    ap.add_argument("--append-key", default=None,
                    help="keep --out's contents and append this run's rows under this top-level key (the runs of an A/B)")
    a = ap.parse_args()
    if a.merge and a.only_batch:
        sys.exit("ovl_rate: --merge and --only-batch time one call each, in processes of their own")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ovl_rate: no GPU (rates are measured on the device or not at all)")
    import hpgfastq as H

    props = torch.cuda.get_device_properties(0)
    box = {"device": torch.cuda.get_device_name(0), "cus": props.multi_processor_count, "host": os.uname().nodename}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    calls = a.warmup + a.steps
    rows = []
    for name, L in (("150bp", 150), ("250bp", 250)):
        if name not in a.shapes.split(","):
            continue
        n = min(a.pairs, (2 ** 31 - 1024) // L)   # data_indices are int32: < 2 GiB of bases per batch
        if a.merge:                               # (the merged offsets too: both mates together)
            n = min(n, (2 ** 31 - 1024) // (2 * L))
        total = n * L
        idx = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * L).to(torch.int32)
        seq = [torch.zeros(total + H.DEVICE_SLACK, dtype=torch.uint8, device="cuda") for _ in range(2)]
        qual = (33 + torch.arange(total + H.DEVICE_SLACK, dtype=torch.int64, device="cuda") * 7 % 41).to(torch.uint8)
        ins = torch.empty(n, dtype=torch.int32, device="cuda")
        pos = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        b = [H.engine.device_batch(n, s.data_ptr(), qual.data_ptr(), idx.data_ptr()) for s in seq]
        for filling in a.fillings.split(","):
            made = fill_pairs(torch, seq[0], seq[1], n, L, filling, gen)
            torch.cuda.synchronize()
            if a.merge:
                with H.OverlapClip(30, 5, stream=sp) as ov:
                    if a.inserts:
                        ov.count_inserts(True)
                    merge_us = timed(torch, stream, lambda: ov.merge_batch(b[0], b[1]), a.warmup, a.steps)
                    info, merged = ov.info(), ov.merge_info()
                per = {k: (v // calls if isinstance(v, int) else [x // calls for x in v]) for k, v in {**info, **merged}.items()
                       if k not in ("min_overlap", "max_mismatches")}
                assert per["pairs"] == n and per["merged_pairs"] == per["overlapping"], (info, merged)
                if filling in ("overlap", "short"):
                    assert per["merged_pairs"] > n - n // 100, merged
                # find; the plan's arrays and three sums; the unmerged pairs' bytes once each way; both mates of
                # the merged pairs in, the merged reads out
                unmerged = 2 * L * (n - per["merged_pairs"])
                moved = 2 * total + 24 * n + 56 * n + 4 * unmerged + 4 * L * per["merged_pairs"] + 2 * per["merged_bases"]
                res = {"tool": "ovl_rate", "shape": name, "pairs": n, "read_length": L, "filling": filling, "inserts": a.inserts,
                       "lib": os.path.basename(os.path.dirname(H.LIB_PATH)) + "/" + os.path.basename(H.LIB_PATH),
                       "per_call": per, "steps": a.steps, "warmup": a.warmup, **box, "ovl_merge": summary(merge_us, moved, n)}
                print(json.dumps(res), flush=True)
                rows.append(res)
                continue
            if a.only_batch:
                with H.OverlapClip(30, 5, stream=sp) as ov:
                    if a.correct:
                        ov.set_correct((33, 30, 14))
                    if a.inserts:
                        ov.count_inserts(True)
                    cut_us = timed(torch, stream, lambda: ov.clip_batch(b[0], b[1]), a.warmup, a.steps)
                    info = ov.info()
                    fixed = ov.correct_info() if a.correct else None
                    counted = int(ov.inserts().sum()) if a.inserts else None
                per = {k: (v // calls if isinstance(v, int) else [x // calls for x in v]) for k, v in info.items()
                       if k not in ("min_overlap", "max_mismatches")}
                assert per["pairs"] == n and (counted is None or counted == n * calls), (info, counted)
                if filling == "short":
                    assert per["overlapping"] > n - n // 100 and per["clipped"] == per["overlapping"], info
                    assert fixed is None or min(fixed["corrected_bases"]) > 0, fixed
                kept = total * 2 - sum(per["bases_removed"])
                res = {"tool": "ovl_rate", "shape": name, "pairs": n, "read_length": L, "filling": filling, "correct": a.correct,
                       "inserts": a.inserts, "lib": os.path.basename(os.path.dirname(H.LIB_PATH)) + "/" + os.path.basename(H.LIB_PATH),
                       "per_call": per, "steps": a.steps, "warmup": a.warmup, **box,
                       "corrected_per_call": None if fixed is None else
                       {"pairs": fixed["corrected_pairs"] // calls, "bases": [x // calls for x in fixed["corrected_bases"]]},
                       "ovl_batch": summary(cut_us, 2 * total + 24 * n + 4 * kept + 16 * n, n)}
                print(json.dumps(res), flush=True)
                rows.append(res)
                continue
            with H.AdapterClip(None, 8, stream=sp) as cl:
                def two_finds():
                    cl.find(b[0], pos[0].data_ptr(), None)
                    cl.find(b[1], pos[1].data_ptr(), None)
                clip_us = timed(torch, stream, two_finds, a.warmup, a.steps)
                cl.sync()
            with H.OverlapClip(30, 5, stream=sp) as ov:
                find_us = timed(torch, stream, lambda: ov.find(b[0], b[1], ins.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr()),
                                a.warmup, a.steps)
                info = ov.info()
                ov.reset()
                if a.correct:
                    ov.set_correct((33, 30, 14))
                if a.inserts:
                    ov.count_inserts(True)
                cut_us = timed(torch, stream, lambda: ov.clip_batch(b[0], b[1]), a.warmup, a.steps)
                ov.sync()
            per = {k: (v // calls if isinstance(v, int) else [x // calls for x in v]) for k, v in info.items()
                   if k not in ("min_overlap", "max_mismatches")}
            assert per["pairs"] == n and per["skipped"] == 0, info
            if filling == "none":
                assert per["overlapping"] < n // 1000, info
            if filling == "overlap":
                assert per["overlapping"] == n and per["clipped"] == 0, info
            if filling == "readthrough":
                assert per["clipped"] >= made, info
            kept = total * 2 - sum(per["bases_removed"])
            f, c = summary(find_us, 2 * total + 20 * n, n), summary(clip_us, 2 * total + 16 * n, n)
            res = {"tool": "ovl_rate", "shape": name, "pairs": n, "read_length": L, "bases": 2 * total, "min_overlap": 30,
                   "max_mismatches": 5, "filling": filling, "correct": a.correct, "inserts": a.inserts, "fragment_pairs": made, "per_call": per, "steps": a.steps,
                   "warmup": a.warmup, **box,
                   # find: both mates' bases and offsets in, 12 bytes per pair out
                   "ovl_find": f,
                   # find + two scans + two copies: the kept bytes of sequence and quality move once each way
                   "ovl_batch": summary(cut_us, 2 * total + 24 * n + 4 * kept + 16 * n, n),
                   "clip_find_both_mates": c,
                   "ovl_vs_two_finds": round(f["us_median"] / c["us_median"], 3)}
            print(json.dumps(res), flush=True)
            rows.append(res)
        del seq, qual, idx, ins, pos
        torch.cuda.empty_cache()
    write_profile(a.out, rows, a.steps, a.warmup, a.append_key)


if __name__ == "__main__":
    main()
