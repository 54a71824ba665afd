"""The pass-first kernels' group-boundary lines: in
C2's kernels the last step of every group of steps is loaded with the plain
cache policy and the others non-temporal (its N / out-of-range variant keeps
every step non-temporal), so the line a group shares with the next one -- this
unit's next group, or the next unit's first -- stays in L2.  A cache policy
cannot change a counter; what these tests guard is the address logic at every
edge of the group / unit structure (where each step's reads come from, what a
padding step, a deferred read and a short last unit load): masks and counters
bit for bit against the CPU oracle (as tests/test_engine_gpu.py's assert_same).

  * routes: the default chain (hex first) and wide / tri forced first, with
    C2's filter at lmax 150 and 1024; hex also with max_N / max_out_of_quality
    (the N / out-of-range variant of the kernel);
  * read counts around the group (12 reads for hex), the unit (48) and the
    persistent grid (48 * 4096 + 5: more than one unit for every wave and a
    short last unit);
  * read lengths: 150; 128 and 64 (every group ends on a line boundary); and
    an explicit mix over 0 .. 156 plus longer reads, which are deferred and sit
    on the first read of groups and units of every geometry, with zero-length
    reads beside them and one unit deferred as a whole (at lmax 150 the
    deferred reads go to the catch-all as a follow-up stage, in more units than
    its grid has waves);
  * the device path with the buffers' base pointers 1, 2 and 3 bytes off a
    dword (the descriptor's base rounding), exactly data + HPGQ_DEVICE_SLACK
    bytes allocated, three batches accumulated into one context, a reset
    between repeats.
"""
import functools

import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

COUNTS = (1, 11, 12, 13, 47, 48, 49, 96, 97, 48 * 4096 + 5)
PATTERNS = ("fixed150", "fixed128", "fixed64", "mixed")
FLAGS = {
    "c2": dict(read_quality_range="20,", read_length_range="50,"),
    "noor": dict(read_quality_range="20,", read_length_range="50,", max_N=2, max_out_of_quality=20),
}
# (route, flags, lmax)
CONFIGS = [(r, "c2", lmax) for r in ("auto", "wide", "tri") for lmax in (150, 1024)] + [("auto", "noor", 150)]


def _lengths(pattern, n):
    """Read lengths, built explicitly (no random draw)."""
    if pattern.startswith("fixed"):
        return np.full(n, int(pattern[5:]), np.int64)
    i = np.arange(n, dtype=np.int64)
    ln = (i * 37) % 157   # 0 .. 156, every value
    # the last read of a hex group / the first of one: zero length
    ln[(i % 12 == 11) & ((i // 12) % 3 == 1)] = 0
    ln[(i % 12 == 0) & ((i // 12) % 5 == 4)] = 0
    # deferred reads (longer than lmax 150: 151 .. 156; longer than the hex and
    # tri geometries at any lmax: 157 .. 256, the longest past wide's 252 too)
    # on the first read of a group and of a unit: hex 12 / 48, wide 8 / 60, tri 9 / 54
    for grp, unit, a, b in ((12, 48, 5, 2), (8, 60, 7, 3), (9, 54, 7, 5)):
        first = ((i % grp == 0) & ((i // grp) % a == b)) | ((i % unit == 0) & ((i // unit) % 2 == 1))
        ln[first] = np.where((i // grp) % 2 == 0, 151 + i % 6, 157 + (i * 7) % 100)[first]
    ln[(i >= 3 * 48) & (i < 4 * 48)] = 200   # hex unit 3: deferred as a whole
    return ln


@functools.lru_cache(maxsize=None)
def _reads(pattern, n):
    ln = _lengths(pattern, n)
    idx = np.zeros(n + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    nb = int(idx[-1])
    rng = np.random.default_rng(7)
    seq = np.frombuffer(b"ACGT" * 15 + b"ACGN", np.uint8)[rng.integers(0, 64, nb)]   # ~2 N per 150 bases
    # a level per read around the filter's Phred 20, so both outcomes occur
    i = np.arange(n)
    level = np.repeat(33 + 12 + (i * 7 + i // 48) % 20, ln)
    qual = (level + rng.integers(0, 9, nb)).astype(np.uint8)
    return O.Reads(np.ascontiguousarray(seq), qual, idx)


@functools.lru_cache(maxsize=None)
def _oracle(pattern, n, flags, lmax):
    """The reference result, computed once and shared (read-only)."""
    mask, _, ctr = O.run(H.stats_params(lmax=lmax, **FLAGS[flags]), _reads(pattern, n))
    mask.setflags(write=False)
    ctr.setflags(write=False)
    return mask, ctr


def _check(mask, ctr, pattern, n, flags, lmax, what):
    m_o, c_o = _oracle(pattern, n, flags, lmax)
    np.testing.assert_array_equal(mask, m_o, err_msg=what)
    if not np.array_equal(ctr, c_o):
        bad = np.nonzero(ctr != c_o)[0]
        raise AssertionError(f"{what}: counters differ at {bad[:10]} gpu={ctr[bad[:10]]} oracle={c_o[bad[:10]]}")


def _expect_kernel(e, route, flags):
    geo = {"auto": "hex", "wide": "wide", "tri": "tri"}[route]
    assert "engine_tri" in e.kernel_name and geo in e.kernel_name, e.kernel_chain
    assert ("noor" in e.kernel_name) == (flags == "noor"), e.kernel_chain


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("route,flags,lmax", CONFIGS)
def test_counts_and_lengths(route, flags, lmax, pattern):
    p = H.stats_params(lmax=lmax, **FLAGS[flags])
    with H.Engine(p, route=route) as e:
        _expect_kernel(e, route, flags)
        for n in COUNTS:
            r = _reads(pattern, n)
            e.reset()
            mask, _ = e.process(r.seq, r.qual, r.idx)
            _check(mask, e.counters(), pattern, n, flags, lmax, f"{n} reads")
    both = _oracle(pattern, COUNTS[-1], flags, lmax)[0]
    assert 0 < int(both.sum()) < COUNTS[-1]   # the filter passes some reads and fails some


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("route,flags,lmax", CONFIGS)
def test_device_path_unaligned_bases(route, flags, lmax, shift):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    pattern, n = "mixed", 48 * 40 + 13
    r = _reads(pattern, n)
    nb = int(r.idx[-1])
    # seq shifted by `shift`, quality by another residue; exactly data + slack bytes from there
    sh_q = shift % 3 + 1
    seq = torch.zeros(shift + nb + H.DEVICE_SLACK, dtype=torch.uint8, device=dev)
    qual = torch.zeros(sh_q + nb + H.DEVICE_SLACK, dtype=torch.uint8, device=dev)
    seq[shift:shift + nb] = torch.from_numpy(r.seq).to(dev)
    qual[sh_q:sh_q + nb] = torch.from_numpy(r.qual).to(dev)
    assert seq.data_ptr() % 4 == 0 and qual.data_ptr() % 4 == 0
    idx = torch.from_numpy(r.idx).to(dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cuts = [0, 48 * 13 + 1, 48 * 13 + 12, n]   # three batches: their first reads start anywhere in a line
    m_o, c_o = _oracle(pattern, n, flags, lmax)
    p = H.stats_params(lmax=lmax, **FLAGS[flags])
    with H.Engine(p, route=route) as e:
        _expect_kernel(e, route, flags)
        for rep in range(2):
            e.reset()
            mask.zero_()
            torch.cuda.synchronize()
            for lo, hi in zip(cuts, cuts[1:]):
                b = H.engine.device_batch(hi - lo, seq.data_ptr() + shift, qual.data_ptr() + sh_q,
                                          idx.data_ptr() + 4 * lo)
                e.run_device(b, None, mask.data_ptr() + lo, None)
                e.sync()
            _check(mask.cpu().numpy(), e.counters(), pattern, n, flags, lmax, f"repeat {rep}")
