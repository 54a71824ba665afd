"""The stats add-ons together on the engine's stream, and hpgq_clip in front of an
edit engine, against the references (GPU; the cases: tests/combined_lib.py, held
to their coverage by tests/test_combined_cases_cpu.py).

A stats case opens every handle it draws on the engine's stream, as the CLI's
worker does: hpgq_kmers, hpgq_qdist / hpgq_adapt / hpgq_dup per mate (keeping
sequences for the overrepresented list), and hpgq_cgr, which fills after the
sync.  The reads go up in three batches, small | large | small, each through
hostile_lib.device_batch (garbage before the reads and in the slack, pointers off
their alignment); per batch every handle reserves the longest read, the engine
writes its mask into a poisoned hostile_lib.Guarded buffer and every add-on
counts with that same pointer, nothing synchronised in between.  Half the cases
synchronise once per batch, the others only after the last one, with every
device buffer alive until then.  Mask and guard bands, counters (dense and full
length), k-mers (dense and every start), quality table, adapter table, the
duplication table, its levels, the top list and its kept bytes, the chaos-game
tables: all equal to the references, and the inputs are as they were uploaded.

A clip case cuts every batch with hpgq_clip_batch_device (both mates of a pair)
and hands the kept reads, in the handle's own buffers, to an edit or edit_stats
engine on a forced route: kept bytes and offsets, mask, trims, counters and the
clip scalars against clip_ref and the oracle over clip_ref's kept reads.

Measured on an MI355X: the slowest case 0.35 s (stats case 0, the first to touch
the device), every other one under 0.2 s; the 56 cases of the file 5.7 s in all.

That the cases fail when the code is wrong was checked with planted faults, none
of them kept: with hpgq_clip's tail compare (overlaps under 8 bases) skipped,
clip case 2 fails on a trim; with a mask buffer of a late-sync case given back
to the allocator and reused before the final sync, stats case 2 fails on that
mask."""
import contextlib

import numpy as np
import pytest

import hpgfastq as H
import pairs_lib as PL
import dup_ref
import overrep_ref
import hostile_lib as HL
import combined_lib as CL

pytestmark = pytest.mark.gpu

POISON = 0xA5
SHIFTS = [(s, q) for s in range(4) for q in range(4) if s != q]


def _upload(c, k, lo, hi):
    """Batch k of the case: every mate's reads lo .. hi - 1 on the device."""
    s, q = SHIFTS[(c.number * 3 + k) % len(SHIFTS)]
    lead = (0, 5, 1, 13, 2, 3)[(c.number + k) % 6]
    subs = [CL.sub(r, lo, hi) for r in c.mates]
    ts = [HL.device_batch(b, lead=lead + m, seq_shift=(s + m) % 4, qual_shift=q) for m, b in enumerate(subs)]
    return subs, ts, max(int(CL.lengths(b).max()) for b in subs)


def _same_counters(e, c, info):
    got = e.counters()
    if not np.array_equal(got, c.counters):
        bad = np.nonzero(got != c.counters)[0]
        raise AssertionError(f"{info}: counters differ at {bad[:10]} gpu={got[bad[:10]]} oracle={c.counters[bad[:10]]}")
    ext, lmax_ext = e.counters_ext()
    np.testing.assert_array_equal(ext, c.counters_at(lmax_ext), err_msg=info + ": full-length counters")


@pytest.mark.parametrize("case", range(CL.N_LIB))
def test_stats_addons_on_one_stream(case):
    c = CL.lib_case(case)
    p, nm, info = c.p, c.nm, CL.summary(c)
    with contextlib.ExitStack() as stack:
        e = stack.enter_context(H.Engine(p, route=c.route))
        km = stack.enter_context(H.Kmers(p.lmax, stream=e.stream)) if c.has("kmers") else None
        qd = [stack.enter_context(H.QualityDist(p.lmax, base=p.phred, stream=e.stream)) for _ in range(nm)] if c.has("qdist") else []
        ad = [stack.enter_context(H.AdapterContent(c.probes, rows=p.lmax, stream=e.stream)) for _ in range(nm)] \
            if c.has("adapt") else []
        dp = [stack.enter_context(H.Duplication(log2_slots=10, stream=e.stream)) for _ in range(nm)] \
            if c.has("dup") or c.has("overrep") else []
        if c.has("overrep"):
            for d in dp:
                d.keep_sequences(c.min_count)
        cg = stack.enter_context(H.ChaosGame(c.k, base_quality=p.phred)) if c.has("cg") else None
        alive = []                                   # (lo, hi, uploads, the guarded mask) of the batches not yet checked

        def settle():
            """After a sync: the chaos-game fills of the batches launched since the last one, then
            their masks, bands and inputs."""
            for lo, hi, ts, g in alive:
                if cg:
                    cg.fill_device(ts[0].batch, g.ptr if c.filter else None,
                                   H.CGR_ONLY_VALID_READS if c.filter else H.CGR_ALL_READS)
                    cg.sync()
                np.testing.assert_array_equal(g.check(), c.mask[lo:hi], err_msg=f"{info}: mask of reads {lo} .. {hi}")
                for t in ts:
                    HL.inputs_unchanged(t)
            alive.clear()

        for k, (lo, hi) in enumerate(c.batches):
            _, ts, longest = _upload(c, k, lo, hi)
            g = HL.Guarded(hi - lo, (case + k) % 4, POISON)
            for h in [e] + ([km] if km else []) + qd + ad:     # the CLI's order: every reservation, the engine, the add-ons
                h.reserve_length(longest)
            e.run_device(ts[0].batch, ts[1].batch if nm == 2 else None, g.ptr, None)
            mask_ptr = g.ptr if c.filter else None               # (paired: the pair mask for both mates)
            if km:
                km.count_device(ts[0].batch, mask_ptr)
            for handles in (qd, ad, dp):
                for m, h in enumerate(handles):
                    h.count_device(ts[m].batch, mask_ptr)
            alive.append((lo, hi, ts, g))
            if c.sync_each:
                e.sync()
                settle()
        e.sync()
        settle()

        _same_counters(e, c, info)
        if km:
            np.testing.assert_array_equal(km.by_pos(), c.kmers(p.lmax), err_msg=info + ": kmers")
            ext = km.by_pos_ext()
            # every start of every counted read: as wide as the longest counted read at least, the longest read at most
            assert max(p.lmax, c.longest_counted) <= ext.shape[1] + 4 <= max(p.lmax, c.longest), (info, ext.shape)
            np.testing.assert_array_equal(ext, c.kmers(ext.shape[1] + 4), err_msg=info + ": kmers, every start")
        for m in range(nm):
            if qd:
                np.testing.assert_array_equal(qd[m].hist(), c.qdist[m], err_msg=f"{info}: quality table, mate {m + 1}")
            if ad:
                first, scalars = ad[m].table()
                np.testing.assert_array_equal(first, c.adapt[m][0], err_msg=f"{info}: adapter table, mate {m + 1}")
                assert scalars == c.adapt[m][1], (info, m)
            if dp:
                keys, counts = dp[m].export()
                wk, wc = dup_ref.arrays(c.dup[m])
                np.testing.assert_array_equal(keys, wk, err_msg=f"{info}: duplication keys, mate {m + 1}")
                np.testing.assert_array_equal(counts, wc, err_msg=f"{info}: duplication counts, mate {m + 1}")
                assert dp[m].levels() == dup_ref.levels_of_table(c.dup[m]), (info, m)
            if c.has("overrep"):
                entries, total = c.overrep[m]
                assert dp[m].count_at_least(c.min_count) == total, (info, m)
                keys, counts = dp[m].top(c.top_n, c.min_count)
                assert [(int(a), int(b)) for a, b in zip(keys, counts)] == [(a, b) for a, b, _ in entries], (info, m)
                for key, _, s in entries:
                    assert dp[m].sequence(key) == s, (info, m, key)
                assert dp[m].kept() == overrep_ref.kept(c.seqs[m], c.min_count), (info, m)
        if cg:
            ts_, tq_, wc_ = c.cgr(c.batches)
            got_s, got_q, got_w = cg.tables()
            np.testing.assert_array_equal(got_s.reshape(-1), ts_, err_msg=info + ": chaos-game table")
            np.testing.assert_array_equal(got_q.reshape(-1), tq_, err_msg=info + ": chaos-game quality table")
            assert got_w == int(wc_[0]), info


@pytest.mark.parametrize("case", range(CL.N_LIB_CLIP))
def test_clip_then_edit_engine(case):
    c = CL.lib_clip_case(case)
    p, nm, n, info = c.p, c.nm, c.n, CL.summary(c)
    with contextlib.ExitStack() as stack:
        e = stack.enter_context(H.Engine(p, route=c.route))
        cl = [stack.enter_context(H.AdapterClip(c.probes, c.min_overlap, stream=e.stream)) for _ in range(nm)]
        for k, (lo, hi) in enumerate(c.batches):
            _, ts, longest = _upload(c, k, lo, hi)
            nb = hi - lo
            g_mask, g_trim = HL.Guarded(nb, (case + k) % 4, POISON), HL.Guarded(4 * nb * nm, 4, POISON)
            out = [cl[m].clip_batch(ts[m].batch) for m in range(nm)]     # (valid until the handle's next batch)
            e.reserve_length(longest)
            e.run_device(out[0], out[1] if nm == 2 else None, g_mask.ptr, g_trim.ptr)
            e.sync()
            np.testing.assert_array_equal(g_mask.check(), c.mask[lo:hi], err_msg=f"{info}: mask of reads {lo} .. {hi}")
            trim = g_trim.check().view(np.uint32)
            for m in range(nm):
                assert out[m].num_reads == nb and out[m].seq != ts[m].batch.seq
                if p.edit_on:
                    np.testing.assert_array_equal(trim[m * nb:(m + 1) * nb], c.trim[m * n + lo:m * n + hi],
                                                  err_msg=f"{info}: trims of reads {lo} .. {hi}, mate {m + 1}")
                seq, qual, idx = PL.fetch(e, out[m])
                want = CL.sub(c.kept[m], lo, hi)
                np.testing.assert_array_equal(idx, want.idx, err_msg=f"{info}: kept offsets, mate {m + 1}")
                assert seq == want.seq.tobytes() and qual == want.qual.tobytes(), (info, "kept bytes", m, lo, hi)
                HL.inputs_unchanged(ts[m])
        _same_counters(e, c, info)
        for m in range(nm):
            assert cl[m].info() == c.cut[m].info, (info, m)
