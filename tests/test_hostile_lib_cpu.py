"""The atlas of tests/hostile_lib.py holds what it promises, checked with the
references alone, and the references agree with each other on it: the CPU
oracle against oracle/pyref.py for the engine's counters and for the 5-mers,
gs_ref.loop against gs_ref.fast and against the rule as hpgq_gs.hip states it."""
import functools
import os
import sys

import numpy as np
import pytest

import gs_ref
import hostile_lib as HL
import hpgfastq as H
import oracle_lib as O

sys.path.insert(0, os.path.join(O.ROOT, "oracle"))
import pyref  # noqa: E402

SETS = sorted(HL.ATLAS_SETS)       # every atlas, at the lmax, the GPU tests run
LENGTHS, _, LMAX = HL.ATLAS_SETS["hex"]


@functools.lru_cache(maxsize=None)
def _atlas(name="hex"):
    lengths, units, _ = HL.ATLAS_SETS[name]
    return HL.atlas(lengths, deferred_units=units)


@functools.lru_cache(maxsize=None)
def _run(config, name="hex"):
    reads, _ = _atlas(name)
    return O.run(HL.params(config, HL.ATLAS_SETS[name][2]), reads, HL.reverse(reads) if config == "paired" else None)


@pytest.mark.parametrize("name", SETS)
def test_size_and_shape(name):
    reads, planted = _atlas(name)
    lengths, units, _ = HL.ATLAS_SETS[name]
    assert 4000 <= reads.n - 48 * units <= 4300 and reads.n % 64 == 1 and all(reads.n % s for s in (3, 4, 6))
    ln = np.diff(reads.idx)
    assert ln[0] == 0 and ln[-1] == 0 and set(lengths) <= set(ln.tolist()) and (ln == 0).sum() >= 5
    # the table says what the reads hold
    at = reads.idx[planted[:, 0]] + planted[:, 1]
    np.testing.assert_array_equal(reads.seq[at], planted[:, 2])
    assert (planted[:, 1] < ln[planted[:, 0]]).all()


@pytest.mark.parametrize("name", SETS)
def test_every_value_at_every_residue_first_and_last(name):
    reads, planted = _atlas(name)
    ln = np.diff(reads.idx)
    r, pos, v = planted.T
    assert len(set(zip(v.tolist(), (pos % 4).tolist()))) == 1024
    assert set(v[pos == 0].tolist()) == set(range(256))
    assert set(v[pos == ln[r] - 1].tolist()) == set(range(256))
    # ... and at every residue of the absolute offset, which is what a kernel's dword loads see
    assert len(set(zip(v.tolist(), ((reads.idx[r] + pos) % 4).tolist()))) == 1024
    # dense: a read of nothing but v, and v in seven bytes in a row
    for val in range(256):
        rows = planted[v == val]
        per_read = np.bincount(rows[:, 0], minlength=reads.n)
        assert (per_read[ln > 0] == ln[ln > 0]).any(), val
        assert (per_read == 7).any(), val


@pytest.mark.parametrize("config", ["c2", "noor", "edit", "paired"])
@pytest.mark.parametrize("name", SETS)
def test_every_value_in_a_passing_and_in_a_failing_read(name, config):
    reads, planted = _atlas(name)
    mask = _run(config, name)[0]
    assert 0 < int(mask.sum()) < reads.n
    passed = mask[planted[:, 0]] == 1
    failed = ~passed
    if config == "paired":       # read r is mate 1 of pair r and mate 2 of pair n - 1 - r
        as_mate2 = mask[reads.n - 1 - planted[:, 0]] == 1
        passed, failed = passed | as_mate2, failed | ~as_mate2
    assert set(planted[passed, 2].tolist()) == set(range(256))
    assert set(planted[failed, 2].tolist()) == set(range(256))


@pytest.mark.parametrize("name", SETS)
def test_a_pair_couples_a_passing_read_with_a_failing_one(name):
    reads, _ = _atlas(name)
    single = _run("edit", name)[0]
    pair = _run("paired", name)[0]
    np.testing.assert_array_equal(pair, single & single[::-1])
    assert int((single != single[::-1]).sum()) > reads.n // 8     # pairs of a passing and a failing read
    assert int(pair.sum()) >= 256                                 # and pairs that pass: one per byte value at least


@pytest.mark.parametrize("name", SETS)
def test_every_value_inside_and_outside_a_trimmed_window(name):
    reads, planted = _atlas(name)
    trim = _run("edit", name)[1].astype(np.int64)
    ts, te = trim & 0xFFFF, trim >> 16
    ln = np.diff(reads.idx)
    r, pos, v = planted.T
    cut = (pos < ts[r]) | (pos >= ln[r] - te[r])
    assert set(v[cut].tolist()) == set(range(256))
    assert set(v[~cut].tolist()) == set(range(256))
    assert (trim == 0).any() and (ts > 0).any() and (te > 0).any()


def test_reverse_is_the_reads_in_reverse_order():
    reads, _ = _atlas()
    rev = HL.reverse(reads)
    assert rev.n == reads.n and rev.pairs() == reads.pairs()[::-1]


def _one(reads, i):
    return O.Reads.from_pairs([reads.read(i)])


@pytest.mark.parametrize("name", SETS)
def test_look_alikes_are_not_n_c_or_g(name):
    reads, _ = _atlas(name)
    mask = _run("noor", name)[0]
    LMAX = HL.ATLAS_SETS[name][2]
    o = pyref.layout(LMAX)
    for i in reads.marks["n_like"]:
        s, _q = reads.read(i)
        assert s.count(b"N") == HL.MAX_N and mask[i] == 1, (i, s)
        extra = O.Reads.from_pairs([(s[:20] + b"N" + s[21:], _q)])      # one real N more: over max_N
        assert O.run(HL.params("noor", LMAX), extra)[0][0] == 0
    p = HL.params("stats", LMAX)
    twin = O.run(p, _one(reads, reads.marks["gc_twin"]))[2][o["hist_gc"]:o["hist_gc"] + 101]
    assert twin[0] == 1
    for i in reads.marks["gc_like"]:
        got = O.run(p, _one(reads, i))[2][o["hist_gc"]:o["hist_gc"] + 101]
        np.testing.assert_array_equal(got, twin)
        s, q = reads.read(i)
        real = O.run(p, O.Reads.from_pairs([(s[:7] + b"C" + s[8:], q)]))[2][o["hist_gc"]:o["hist_gc"] + 101]
        assert real[0] == 0      # a real C moves the read out of the bin: the length tells them apart


@pytest.mark.parametrize("config", ["stats", "noor", "edit"])
def test_oracle_equals_pyref_on_the_atlas(config):
    """Two independent restatements of the byte rules: every counter, so the
    A/C/G/T/N rows, hist_gc and the N filter among them."""
    reads, _ = _atlas()
    p = HL.params(config, LMAX)
    pd = pyref.default_params(**{f: getattr(p, f) for f in pyref.default_params() if hasattr(p, f)})
    assert pd["lmax"] == LMAX and pd["edit_on"] == p.edit_on and pd["max_N"] == p.max_N
    m_p, t_p, c_p = pyref.run(pd, reads.pairs())
    m_o, t_o, c_o = _run(config)
    np.testing.assert_array_equal(np.array(m_p, np.uint8), m_o)
    np.testing.assert_array_equal(np.array(t_p, np.uint32), t_o)
    np.testing.assert_array_equal(np.array(c_p, np.uint64), c_o)


def _pyref_kmers(reads, lmax):
    out = np.zeros((1024, max(lmax - 4, 0)), np.uint64)
    for (kid, p), c in pyref.kmers(reads.pairs(), lmax).items():
        out[kid, p] = c
    return out


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("lmax", [20, 40, 300])
def test_oracle_kmers_equal_pyref(lmax, half):
    """(the window reads of byte values 0..127 and 128..255: pyref is slow)"""
    reads = HL.kmer_window_reads()
    n = reads.n // 2         # (every read has 40 bases)
    part = O.Reads(reads.seq[half * n * 40:(half + 1) * n * 40].copy(), reads.qual[:n * 40].copy(),
                   (np.arange(n + 1) * 40).astype(np.int32))
    np.testing.assert_array_equal(O.kmers(part, lmax), _pyref_kmers(part, lmax))


@functools.lru_cache(maxsize=None)
def _small_atlas():
    return HL.atlas((1, 2, 49, 50, 51))[0]


def test_oracle_kmers_equal_pyref_on_the_atlas():
    reads = _small_atlas()
    np.testing.assert_array_equal(O.kmers(reads, 51), _pyref_kmers(reads, 51))


def test_oracle_cgr_equals_pyref_on_the_atlas():
    reads = _small_atlas()
    for k in (4, 8):
        ts, tq, wc = O.cgr(k, reads)
        ps, pq, pw = pyref.cgr_fill(k, 33, reads.pairs())
        assert int(wc[0]) == pw
        np.testing.assert_array_equal(ts, np.array(ps, np.uint32))
        np.testing.assert_array_equal(tq, np.array(pq, np.uint32))


def test_gs_ref_reads_the_bytes_as_the_kernel_header_says():
    """hpgq_gs.hip: headers ('>' .. '\\n') are dropped and break the word, N/n
    breaks the word, A/C/G/T in either case are bases, every other byte is
    skipped without breaking the word."""
    k = 4
    for v in range(256):
        text = b"ACGTACG" + bytes([v]) + b"TACGTAC\n"
        table, info = gs_ref.loop(text, k)
        t2, i2 = gs_ref.fast(text, k)
        np.testing.assert_array_equal(table, t2)
        assert info == i2
        if v == ord(">"):
            want = dict(words=4, bases=7, ns=0, sequences=1)      # TACGTAC is header text
        elif v in b"Nn":
            want = dict(words=8, bases=14, ns=1, sequences=0)
        elif v in b"ACGTacgt":
            want = dict(words=12, bases=15, ns=0, sequences=0)
        else:   # '\n' among them
            want = dict(words=11, bases=14, ns=0, sequences=0)
            joined = gs_ref.loop(b"ACGTACGTACGTAC\n", k)
            np.testing.assert_array_equal(table, joined[0])
        assert info == want, (v, info)
    text = HL.gs_atlas_text()
    a, b = gs_ref.loop(text, 3), gs_ref.fast(text, 3)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1] and a[1]["sequences"] == 2 and a[1]["ns"] == 2
