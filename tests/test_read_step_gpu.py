"""The edges that csrc/hpgq_reads.h owns, for the three counters that read a
step's reads through it: hpgq_qdist, hpgq_adapt and hpgq_dup (gfx950) against
tests/qdist_ref.py, adapt_ref.py and dup_ref.py, every count exact.

Per counter: read counts around a wave step (R reads) and a workgroup step (G
reads), each with one workgroup and with as many as the library takes, with and
without a mask that drops the first and the last read, with the byte pointer at
each alignment mod 4.  Every batch has no lead and exactly HPGQ_DEVICE_SLACK
garbage bytes after the last read's last byte (hostile_lib.device_batch), so
the tail loads land in the slack and the first dword-aligned load starts before
the pointer.

Elsewhere, and not repeated here: thousands of reads of every length up to past
a tile at every alignment (test_qdist_gpu.py::test_edge_lengths_and_alignments,
::test_unaligned_quality_pointer, test_adapt_gpu.py::
test_every_start_every_alignment, test_dup_gpu.py::test_fingerprints_per_read),
hostile bytes around the reads (test_hostile_*_gpu.py) and tables at capacity
(test_capacity_gpu.py)."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import adapt_ref
import dup_ref
import hostile_lib as HL
import qdist_ref

pytestmark = pytest.mark.gpu

PROBES = adapt_ref.DEFAULT_PROBES
K = 12                                  # their length
LENGTHS = [0, 1, 3, 4, 5, K, 300]       # 300: past the 256 positions that stay on chip, two passes of a dup segment
ROWS = 300


def _reads(n):
    """n reads whose lengths cycle through LENGTHS (from n on, so the counts
    differ in what comes first), the last one not empty.  Qualities: all 256
    values.  Sequences: A C G T, a probe planted in the reads long enough --
    across position 256, after it, and ending on the read's last byte."""
    rng = np.random.default_rng(1000 + n)
    lens = [LENGTHS[(i + n) % len(LENGTHS)] for i in range(n)]
    if lens[-1] == 0:
        lens[-1] = 300
    seqs = []
    for i, ln in enumerate(lens):
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=ln)].tobytes())
        p = PROBES[i % len(PROBES)]
        if ln == K and i % 2 == 0:
            s[:] = p
        elif ln > K:
            at = (250, 280, ln - K)[i % 3]
            s[at:at + K] = p
        seqs.append(bytes(s))
    idx = np.zeros(n + 1, dtype=np.int32)
    idx[1:] = np.cumsum(lens)
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    qual = rng.integers(0, 256, size=len(seq), dtype=np.uint8)
    return O.Reads(seq, qual, idx)


def _check_qdist(h, want):
    np.testing.assert_array_equal(h.hist(), want)


def _check_adapt(h, want):
    first, info = h.table()
    np.testing.assert_array_equal(first, want[0])
    assert info == want[1]


def _check_dup(h, want):
    keys, counts = h.export()
    wk, wc = dup_ref.arrays(want)
    np.testing.assert_array_equal(keys, wk)
    np.testing.assert_array_equal(counts, wc)


# R, G: reads per wave step and per workgroup step -- kR and kGroup of
# csrc/hpgq_qdist.hip and csrc/hpgq_adapt.hip, kSegs and kGroup of csrc/hpgq_dup.hip.
# shift: which pointer of the batch the counter reads.
COUNTERS = {
    "qdist": dict(R=16, G=128, shift="qual_shift", open=lambda: H.QualityDist(ROWS, base=33),
                  want=lambda r, m: qdist_ref.table_of(r, m), check=_check_qdist),
    "adapt": dict(R=16, G=128, shift="seq_shift", open=lambda: H.AdapterContent(PROBES, rows=ROWS),
                  want=lambda r, m: adapt_ref.table_of(r, PROBES, m), check=_check_adapt),
    "dup": dict(R=6, G=48, shift="seq_shift", open=lambda: H.Duplication(log2_slots=10),
                want=lambda r, m: dup_ref.table_of(r, m), check=_check_dup),
}
CASES = [(name, which, d) for name in COUNTERS for which in "RG" for d in (-1, 0, 1)]


@pytest.mark.parametrize("name,which,d", CASES, ids=[f"{c}-{w}{d:+d}" for c, w, d in CASES])
def test_read_counts_around_a_step(name, which, d):
    c = COUNTERS[name]
    n = c[which] + d
    reads = _reads(n)
    assert {0, 1, 3, 4, 5, 300} <= set(np.diff(reads.idx).tolist()) or n < len(LENGTHS)
    assert int(np.diff(reads.idx)[-1]) > 0 and int(np.diff(reads.idx).max()) == 300
    drop = np.ones(n, np.uint8)
    drop[0] = drop[-1] = 0
    with c["open"]() as h:
        for mask in (None, drop):
            want = c["want"](reads, mask)       # once per mask: alignment and grid do not change it
            for shift in range(4):
                t = HL.device_batch(reads, **{c["shift"]: shift}, mask=mask)
                for max_wg in (1, 0):
                    h.reset()
                    h.set_max_workgroups(max_wg)
                    h.count_device(t.batch, t.mask_ptr)
                    h.sync()
                    try:
                        c["check"](h, want)
                    except AssertionError as e:
                        raise AssertionError(f"{name} n={n} mask={mask is not None} pointer%4={shift} "
                                             f"max_wg={max_wg}: {e}") from None
                HL.inputs_unchanged(t)
