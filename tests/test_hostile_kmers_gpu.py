"""hpgq_kmers_* on hostile bytes (tests/hostile_lib.py), exactly against the
oracle's 5-mer counts.

  * every byte value at each of a lane's 20 window bytes, in both half-tile
    lanes, at every residue of the read's offset: the bytes whose exactness
    test leaves codes4's sign-replicating v_perm selectors (I K O \\ 0x00 0x02
    0x05 0x06 0x08 \\n \\r) among them; with lmax 40 (every tile works), lmax
    300 (the maxlen prepass) and lmax 20 (the same bytes in the long-read
    pass's scalar classifier);
  * lead and slack that are bases (ACGT...): no 5-mer crosses a read's end
    or the batch's;
  * pass-mask bytes 0, 1, 2, 0x80, 0xFF in each byte lane of the prepass's
    packed mask dword, in the one-by-one tail (n = 1, 2, 3 mod 4) and on reads
    longer than lmax: only the value 1 counts."""
import functools

import numpy as np
import pytest

import hostile_lib as HL
import hpgfastq as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

BASES = b"ACGTACGT"


def _count(lmax, reads, mask=None, lead=0):
    """-> (by_pos, by_pos_ext) of one device batch inside base-valued lead and slack."""
    t = HL.device_batch(reads, lead=lead, lead_fill=BASES, slack_fill=BASES, mask=mask)
    assert bytes(t.host["seq"][-H.DEVICE_SLACK:]) == BASES
    km = H.Kmers(lmax)
    try:
        km.count_device(t.batch, t.mask_ptr)
        km.sync()
        got = km.by_pos(), km.by_pos_ext()
    finally:
        km.close()
    HL.inputs_unchanged(t)
    return got


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} cells differ, first (id, start) {bad[:6].tolist()}: "
                           f"gpu {[int(got[tuple(b)]) for b in bad[:6]]} oracle {[int(want[tuple(b)]) for b in bad[:6]]}")


@functools.lru_cache(maxsize=None)
def _window_want(lmax):
    w = O.kmers(HL.kmer_window_reads(), lmax)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("lead", [4, 5, 6, 7])
@pytest.mark.parametrize("lmax", [40, 300, 20])
def test_window_atlas(lmax, lead):
    reads = HL.kmer_window_reads()
    dense, ext = _count(lmax, reads, lead=lead)
    _same(dense, _window_want(lmax), f"lmax {lmax} lead {lead}")
    _same(ext, _window_want(max(lmax, 40)), f"lmax {lmax} lead {lead}, every start")
    if lmax == 20:     # starts 16 .. 35 are the long-read pass's: the planted bytes reach it
        assert int(_window_want(40)[:, 16:].sum()) > 0 and int(dense.sum()) < int(ext.sum())


@functools.lru_cache(maxsize=None)
def _ending_in_acgt():
    """500 reads of 5 .. 60 bases, nothing but bases, each ending in ACGT (as
    does the batch): a 5-mer that crossed an end would be a valid one."""
    rng = np.random.default_rng(5)
    ln = rng.integers(5, 61, 500)
    ln[-1] = 60
    pat = np.frombuffer(b"ACGT", np.uint8)
    pairs = [(pat[(np.arange(L) - L) % 4].tobytes(), b"I" * int(L)) for L in ln]
    assert all(s.endswith(b"ACGT") for s, _ in pairs)
    return O.Reads.from_pairs(pairs)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("lmax", [20, 64, 300])
def test_no_kmer_crosses_the_end(lmax, lead):
    reads = _ending_in_acgt()
    dense, ext = _count(lmax, reads, lead=lead)
    _same(dense, O.kmers(reads, lmax), f"lmax {lmax} lead {lead}")
    _same(ext, O.kmers(reads, max(lmax, 60)), f"lmax {lmax} lead {lead}, every start")
    assert not ext[:, 56:].any()      # no start past the longest read's last


MASK_VALUES = (0, 1, 2, 0x80, 0xFF)


def _mask_reads(tail, long_len):
    """20 + tail reads; read i has mask byte MASK_VALUES[(i // 4 + i % 4) % 5]:
    every value in every byte lane of a packed mask dword.  The reads that count
    are the long ones (long_len + i bases, the others 50): a prepass that took
    another lane's byte would find a shorter longest read.  The `tail` reads
    past the last whole dword count and are the longest of all."""
    n = 20 + tail
    i = np.arange(n)
    mask = np.array(MASK_VALUES, np.uint8)[(i // 4 + i % 4) % 5]
    mask[20:] = 1
    ln = np.where(mask == 1, long_len + i, 50)
    ln[20:] += 40
    rng = np.random.default_rng(tail)
    pairs = [(rng.choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes(), b"I" * int(L)) for L in ln]
    for lane in range(4):
        assert set(mask[:20][lane::4].tolist()) == set(MASK_VALUES)
    return O.Reads.from_pairs(pairs), mask


@pytest.mark.parametrize("tail", [1, 2, 3])
@pytest.mark.parametrize("lmax,long_len", [(300, 200), (300, 400), (20, 200)])
def test_only_mask_value_one_counts(lmax, long_len, tail):
    reads, mask = _mask_reads(tail, long_len)
    longest = int(np.diff(reads.idx)[mask == 1].max())
    dense, ext = _count(lmax, reads, mask=mask, lead=tail)
    _same(dense, O.kmers(reads, lmax, mask), f"lmax {lmax} long {long_len} tail {tail}")
    _same(ext, O.kmers(reads, max(lmax, longest), mask), f"lmax {lmax} long {long_len} tail {tail}, every start")
    # and the same counts from a batch of the counted reads alone
    only = O.Reads.from_pairs([reads.read(i) for i in np.nonzero(mask == 1)[0]])
    _same(ext, O.kmers(only, max(lmax, longest)), "the counted reads alone")
