"""The pass-first kernels' per-read filter bounds: the
unit prologue packs a read's length test and both quality products into two
16-bit bounds in its record (filter_bounds, hpgq_engine_kernel.h) and the steps
and the unit epilogue decide by lo16 <= S <= hi16.  Masks and every counter bit
for bit against the CPU oracle, 3,000-read batches, on each geometry (route
hex, tri, wide; lmax = the geometry's longest read, so its kernel takes every
read):

  * lengths 1, 2, 49, 50, 51 (the length range is "50,"), 149, 150, 156, and
    157, 160 (tri, wide), 200, 251, 252 (wide);
  * every read's quality sum sits exactly at the lower bound lo_r n, one below
    it, at the upper bound hi_r n or one above it (an open end: the other
    bound's pair again), spread unevenly over the read's bytes;
  * quality ranges "20,", "20,30", ",30"; two that nothing passes ("60," with
    Q <= 41, and "300,", whose product lo_r n leaves 16 bits) and one that
    everything passes ("0,400": the upper product is clamped to 16 bits);
  * Phred offsets 33 and 64; also with max_N / max_out_of_quality (the N /
    out-of-range variants of the kernels), reads holding 0 .. 3 N;
  * no filter at all (stats alone);
  * a byte that is none of A, C, G, T, N in a passing read and in a failing
    one (the steps' rare path).
"""
import functools

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

N_READS = 3000
LENGTHS = {
    "hex": (1, 2, 49, 50, 51, 149, 150, 156),
    "tri": (1, 2, 49, 50, 51, 149, 150, 156, 157, 160),
    "wide": (1, 2, 49, 50, 51, 149, 150, 156, 157, 160, 200, 251, 252),
}
# filter range -> the range whose bounds the reads' sums are built on
RANGES = {"20,": "20,", "20,30": "20,30", ",30": ",30", "60,": "20,30", "300,": "20,30", "0,400": "20,30"}
NONE_PASS, ALL_PASS = ("60,", "300,"), ("0,400",)
NOOR = dict(max_N=2, max_out_of_quality=20)


def _bounds(text):
    lo, _, hi = text.partition(",")
    return (int(lo) if lo else None), (int(hi) if hi else None)


@functools.lru_cache(maxsize=None)
def _reads(route, built_on, phred):
    """Read i: length LENGTHS[i % k]; its quality sum at one of the four edges."""
    lens = LENGTHS[route]
    lo, hi = _bounds(built_on)
    i = np.arange(N_READS)
    ln = np.array(lens, np.int64)[i % len(lens)]
    idx = np.zeros(N_READS + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    nb = int(idx[-1])
    # (mean bound, offset of the sum from bound x n): lo - 1, lo, hi, hi + 1
    edges = [(lo if lo is not None else hi, -1 if lo is not None else 0), (lo if lo is not None else hi, 0),
             (hi if hi is not None else lo, 0), (hi if hi is not None else lo, 1 if hi is not None else 0)]
    which = (i // len(lens) + i // 7) % 4
    mean = np.array([e[0] for e in edges])[which]
    delta = np.array([e[1] for e in edges])[which]
    start = idx[:-1].astype(np.int64)
    j = np.arange(nb) - np.repeat(start, ln)          # position in the read
    n_of = np.repeat(ln, ln)
    r_of = np.repeat(i, ln)
    qual = np.repeat(phred + mean, ln)
    # a zero-sum wiggle over the first 0 .. 39 byte pairs (2k, 2k + 1) of a read,
    # amplitude 1 .. 3: as many bytes leave the quality range (max_out_of_quality)
    w = 1 + r_of % 3
    paired = j < np.minimum(n_of & ~1, 2 * ((r_of // 3) % 40))
    qual = qual + np.where(paired, np.where(j % 2 == 0, w, -w), 0)
    # the edge's +-1 on one byte of the read
    at = start + (i * 7) % ln
    qual[at] += delta
    # bases: ACGT in turn, 0 .. 3 N per read where it is long enough
    seq = np.frombuffer(b"ACGT", np.uint8)[(j + r_of) % 4].copy()
    n_n = np.repeat((i // 5) % 4, ln)
    seq[(j % 11 == 3) & (j // 11 < n_n)] = ord("N")
    return O.Reads(np.ascontiguousarray(seq), qual.astype(np.uint8), idx)


def _flags(rng, phred, noor):
    f = dict(read_quality_range=rng, read_length_range="50,", quality_encoding=f"phred{phred}")
    if noor:
        f.update(NOOR)
    return f


def _same(e, reads, want, what):
    mask, _ = e.process(reads.seq, reads.qual, reads.idx)
    m_o, c_o = want
    np.testing.assert_array_equal(mask, m_o, err_msg=what)
    ctr = e.counters()
    if not np.array_equal(ctr, c_o):
        bad = np.nonzero(ctr != c_o)[0]
        raise AssertionError(f"{what}: counters differ at {bad[:10]} gpu={ctr[bad[:10]]} oracle={c_o[bad[:10]]}")


def _oracle(p, reads):
    mask, _, ctr = O.run(p, reads)
    return mask, ctr


def _expect_kernel(e, route, noor):
    assert "engine_tri" in e.kernel_name and route in e.kernel_name, e.kernel_chain
    assert ("noor" in e.kernel_name) == noor, e.kernel_chain


@pytest.mark.parametrize("noor", [False, True])
@pytest.mark.parametrize("phred", [33, 64])
@pytest.mark.parametrize("rng", list(RANGES))
@pytest.mark.parametrize("route", list(LENGTHS))
def test_sums_at_the_bounds(route, rng, phred, noor):
    reads = _reads(route, RANGES[rng], phred)
    p = H.stats_params(lmax=max(LENGTHS[route]), **_flags(rng, phred, noor))
    want = _oracle(p, reads)
    npass = int(want[0].sum())
    print(f"{route} {rng} phred{phred} noor={noor}: oracle passes {npass} of {N_READS}")
    if rng in NONE_PASS:
        assert npass == 0
    elif rng in ALL_PASS and not noor:
        assert npass == int((np.diff(reads.idx) >= 50).sum())   # (the length range alone fails reads)
    else:
        assert 0 < npass < N_READS
    with H.Engine(p, route=route) as e:
        _expect_kernel(e, route, noor)
        _same(e, reads, want, f"{route} {rng} phred{phred} noor={noor}")


def test_edges_are_hit():
    """The batches hold reads whose mean sits exactly on each bound and one off it."""
    reads = _reads("wide", "20,30", 33)
    ln = np.diff(reads.idx).astype(np.int64)
    sums = np.add.reduceat(reads.qual.astype(np.int64), reads.idx[:-1].astype(np.int64)) - 33 * ln
    for n in LENGTHS["wide"]:
        got = set(sums[ln == n].tolist())
        assert {20 * n - 1, 20 * n, 30 * n, 30 * n + 1} <= got, (n, sorted(got))


@pytest.mark.parametrize("route", list(LENGTHS))
def test_no_filter(route):
    reads = _reads(route, "20,30", 33)
    p = H.stats_params(lmax=max(LENGTHS[route]))
    assert not p.filter_on
    want = _oracle(p, reads)
    assert int(want[0].sum()) == N_READS
    with H.Engine(p, route=route) as e:
        _expect_kernel(e, route, False)
        _same(e, reads, want, f"{route} no filter")


@pytest.mark.parametrize("noor", [False, True])
@pytest.mark.parametrize("route", list(LENGTHS))
def test_other_bytes_in_passing_and_failing_reads(route, noor):
    base = _reads(route, "20,30", 33)
    p = H.stats_params(lmax=max(LENGTHS[route]), **_flags("20,30", 33, noor))
    m0, _ = _oracle(p, base)
    ln = np.diff(base.idx)
    seq = base.seq.copy()
    hit = []
    for passing in (1, 0):
        # several reads of each kind, lengths 50 .. the geometry's longest, bytes in different lanes
        cand = np.nonzero((m0 == passing) & (ln >= 50))[0]
        assert len(cand) >= 8
        for k, r in enumerate(cand[:: max(len(cand) // 8, 1)][:8]):
            pos = (k * 37) % int(ln[r])
            seq[base.idx[r] + pos] = (ord("a"), ord("R"), ord("n"), 0x2E)[k % 4]
            hit.append((int(r), passing))
    reads = O.Reads(seq, base.qual, base.idx)
    want = _oracle(p, reads)
    for r, passing in hit:   # a base's letter does not move a read across the quality filter
        assert want[0][r] == passing or noor, r
    with H.Engine(p, route=route) as e:
        _expect_kernel(e, route, noor)
        _same(e, reads, want, f"{route} other bytes noor={noor}")
