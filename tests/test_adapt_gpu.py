"""`stats --adapters` on the GPU: hpgq_adapt_* (gfx950) against
tests/adapt_ref.py, cell for cell and scalar for scalar (DESIGN.md §2.11,
§4.13).  Counts of first occurrences below P = 256 stay on chip; a step covers
244 starts (probes of up to 13 bases) or 224 (longer ones).  Every batch goes up
through hostile_lib.device_batch: ACGT garbage before the reads and in the
slack."""
import numpy as np
import pytest

import hpgfastq as H
import oracle_lib as O
import adapt_ref
import hostile_lib as HL

pytestmark = pytest.mark.gpu

P = 256
DEF = adapt_ref.DEFAULT_PROBES
K = 12


def _reads(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    idx = np.zeros(len(seqs) + 1, dtype=np.int32)
    idx[1:] = np.cumsum(lens)
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    return O.Reads(seq, np.full(len(seq), ord("I"), np.uint8), idx)


def _count(ad, reads, mask=None, lead=0, seq_shift=0, keep=None):
    t = HL.device_batch(reads, lead=lead, seq_shift=seq_shift, mask=mask)
    if keep is not None:
        keep.append(t)
    ad.count_device(t.batch, t.mask_ptr)
    if keep is None:
        ad.sync()
    return t


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1] == want[1]


def _plant(s, at, p):
    s = bytearray(s)
    s[at:at + len(p)] = p
    return bytes(s)


def _acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


# -- 1. every start, every alignment ------------------------------------------------------------

@pytest.fixture(scope="module")
def every_start():
    seqs = []
    L = P + 40
    for p in DEF:
        assert len(p) == K
        seqs.append(p)                                                   # L = K
        seqs += [_plant(b"N" * L, s, p) for s in range(L - K + 1)]       # every start of L = P + 40
        for cut in range(1, K):                                          # cut pairs: none counts
            seqs += [b"N" * 20 + p[:cut], p[cut:] + b"N" * 20]
        for v in range(256):                                             # near misses
            if v != p[v % K]:
                seqs.append(b"N" * 5 + _plant(p, v % K, bytes([v])) + b"N" * 5)
    reads = _reads(seqs)
    want = adapt_ref.table_of(reads, DEF)
    # the recipe means what it says: every start 0 .. P + 40 - K of every probe is hit, nothing else
    assert want[0].shape == (len(DEF), L)
    assert (want[0][:, :L - K + 1] != 0).all() and (want[0][:, L - K + 1:] == 0).all()
    assert int(want[0].sum()) == len(DEF) * (L - K + 2) == want[1]["with_any"]
    return reads, want


@pytest.mark.parametrize("seq_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("lead", [0, 1, 2, 3, 13])
def test_every_start_every_alignment(every_start, lead, seq_shift):
    reads, want = every_start
    with H.AdapterContent(rows=P + 40) as ad:
        t = _count(ad, reads, lead=lead, seq_shift=seq_shift)
        _same(ad.table(), want)
        HL.inputs_unchanged(t)


# -- 2. short reads -----------------------------------------------------------------------------

def test_short_reads():
    rng = np.random.default_rng(31)
    seqs = []
    for i in range(500):
        n = int(rng.integers(0, K + 3))
        s = _acgt(rng, n)
        if i % 7 == 0:
            s = (DEF[i % len(DEF)] + _acgt(rng, 2))[:max(n, K)]          # the probe itself, or with a tail
        if i % 11 == 0 and n >= K:
            s = _acgt(rng, n - K) + DEF[i % len(DEF)]                    # ending in the probe
        seqs.append(s)
    assert {len(s) for s in seqs} == set(range(K + 3))
    reads = _reads(seqs)
    want = adapt_ref.table_of(reads, DEF)
    assert want[1]["with_any"] > 50
    with H.AdapterContent(rows=K + 2) as ad:
        _count(ad, reads, lead=3)
        _same(ad.table(), want)


# -- 3. probe sets ------------------------------------------------------------------------------

def _set32():
    rng = np.random.default_rng(32)
    ps = list(DEF)
    share = _acgt(rng, 8)
    ps += [share + b"ACCA", share + b"ACCT" + _acgt(rng, 9)]             # the same first 8 bases, differing later
    long_ = _acgt(rng, 32)
    ps += [long_, long_[:19], long_[:8]]                                 # lengths 32 and 8; proper prefixes
    ps += [ps[1], ps[7]]                                                 # identical probes
    while len(ps) < 32:
        ps.append(_acgt(rng, int(rng.integers(8, 33))))
    assert len(ps) == 32 and {8, 32} <= {len(p) for p in ps}
    return ps


def _planted_batch(probes, n=20000, L=150, seed=33):
    rng = np.random.default_rng(seed)
    codes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, L))]
    seqs = []
    for i in range(n):
        s = bytes(codes[i])
        kind = i % 10 if rng.random() < 0.3 else -1
        p = probes[i % len(probes)]
        q = probes[(i * 7 + 1) % len(probes)]
        if kind in (0, 1, 2, 3, 4):
            s = _plant(s, int(rng.integers(0, L - len(p) + 1)), p)
        elif kind == 5:                                                  # the same probe twice
            s = _plant(_plant(s, int(rng.integers(0, 50)), p), int(rng.integers(90, L - len(p) + 1)), p)
        elif kind in (6, 7):                                             # two different probes
            s = _plant(_plant(s, int(rng.integers(0, 50)), p), int(rng.integers(90, L - len(q) + 1)), q)
        elif kind == 8:                                                  # 40 A: PolyA at the run's start
            s = _plant(s, int(rng.integers(1, L - 40)), b"C" + b"A" * 39)
        elif kind == 9:                                                  # the probe at the read's very end
            s = _plant(s, L - len(p), p)
        seqs.append(s)
    return _reads(seqs)


@pytest.fixture(scope="module")
def set_cases():
    out = {}
    for name, probes in (("one", [DEF[0]]), ("32", _set32())):
        reads = _planted_batch(probes if name == "32" else DEF)
        want = adapt_ref.table_of(reads, probes)
        assert want[1]["with_any"] > (2000 if name == "32" else 300)
        out[name] = (probes, reads, want)
    return out


@pytest.mark.parametrize("name", ["one", "32"])
def test_probe_sets(set_cases, name):
    probes, reads, want = set_cases[name]
    with H.AdapterContent(probes, rows=150) as ad:
        _count(ad, reads, lead=1, seq_shift=1)
        _same(ad.table(), want)


# -- 4. hot cell --------------------------------------------------------------------------------

def test_hot_cell():
    one = _plant(b"ACGT" * 38, 100, DEF[0])[:150]
    reads = _reads([one] * 70000)
    want = np.zeros((len(DEF), 150), np.uint64)
    want[0, 100] = 70000
    np.testing.assert_array_equal(adapt_ref.table_of(_reads([one]), DEF)[0] * np.uint64(70000), want)
    with H.AdapterContent(rows=150) as ad:
        _count(ad, reads)
        first, info = ad.table()
    np.testing.assert_array_equal(first, want)
    assert info == dict(reads=70000, with_any=70000, nprobes=len(DEF), npos=150)


# -- 5. mask, batches, reset --------------------------------------------------------------------

def test_mask_batches_and_reset():
    rng = np.random.default_rng(35)
    batches = [_planted_batch(DEF, n=2000, L=int(L), seed=350 + k) for k, L in enumerate((150, 120, 160))]
    masks = [(rng.random(2000) < 0.6).astype(np.uint8) for _ in range(3)]
    masks[1][:] = 0                                      # one batch all masked out
    masks[2][7] = 2                                      # (only mask == 1 counts)
    want = adapt_ref.add([adapt_ref.table_of(b, DEF, m) for b, m in zip(batches, masks)])
    assert want[1]["npos"] == 160 and 0 < want[1]["with_any"] < want[1]["reads"] < 4000
    keep = []
    with H.AdapterContent(rows=160) as ad:
        for b, m in zip(batches, masks):
            _count(ad, b, m, lead=13, keep=keep)
        ad.count_device(H.engine.device_batch(0, 0, 0, 0), None)         # an empty batch
        _count(ad, _reads([]), np.zeros(0, np.uint8), keep=keep)         # a batch of 0 reads
        ad.sync()
        _same(ad.table(), want)
        ad.reset()
        first, info = ad.table()
        assert first.shape == (len(DEF), 0) and info == dict(reads=0, with_any=0, nprobes=len(DEF), npos=0)
        _count(ad, batches[0], masks[0])
        _same(ad.table(), adapt_ref.table_of(batches[0], DEF, masks[0]))
    for t in keep:
        HL.inputs_unchanged(t)


# -- 6. long reads and rows ---------------------------------------------------------------------

def _long_batch(probes, seed):
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(300):
        L = int(rng.integers(500, 1501))
        s = _acgt(rng, L)
        p = probes[i % len(probes)]
        if i % 3 == 0:                                                   # past P only
            s = _plant(s, int(rng.integers(P, L - len(p) + 1)), p)
        elif i % 3 == 1:                                                 # past P, and again later
            a = int(rng.integers(P, L - 2 * len(p)))
            s = _plant(_plant(s, a, p), int(rng.integers(a + 1, L - len(p) + 1)), p)
        seqs.append(s)
    for p in probes:                                                     # straddling the tile, and each step's edge
        for edge in (P, 224, 244, 448, 488):
            seqs += [_plant(b"N" * 600, s, p) for s in range(edge - len(p) + 1, edge + 1)]
    return _reads(seqs)


@pytest.mark.parametrize("name", ["default", "32"])
def test_long_reads(name):
    probes = DEF if name == "default" else _set32()
    reads = _long_batch(probes, 36)
    want = adapt_ref.table_of(reads, probes)
    assert int(want[0][:, P:].sum()) > 300 and int(want[0][:, P - 40:P].sum()) > 0
    with H.AdapterContent(probes, rows=1500) as ad:
        _count(ad, reads, lead=2, seq_shift=3)
        _same(ad.table(), want)


def test_growth_keeps_counts():
    short = _planted_batch(DEF, n=3000, seed=37)
    long_ = _long_batch(DEF, 38)
    m = np.ones(long_.n, np.uint8)
    longest = int(np.argmax(np.diff(long_.idx)))
    m[longest] = 0                                                       # the longest read is masked out
    want = adapt_ref.add([adapt_ref.table_of(short, DEF), adapt_ref.table_of(long_, DEF, m)])
    keep = []
    with H.AdapterContent(rows=150) as ad:
        _count(ad, short, keep=keep)
        ad.reserve_length(int(np.diff(long_.idx)[m == 1].max()))
        ad.reserve_length(10)                                            # never shrinks
        _count(ad, long_, m, lead=1, keep=keep)
        ad.sync()
        _same(ad.table(), want)


def test_too_long_is_an_error_until_reset():
    reads = _reads([_plant(b"C" * 40, 3, DEF[0]), _plant(b"C" * 101, 80, DEF[1]), _plant(b"C" * 100, 88, DEF[2])])
    m = np.array([1, 0, 1], np.uint8)
    with H.AdapterContent(rows=100) as ad:
        _count(ad, reads, m)                             # the read of 101 masked out: no error
        _same(ad.table(), adapt_ref.table_of(reads, DEF, m))
        t = _count(ad, reads, keep=[])
        for call in (ad.sync, ad.table, ad.sync):
            with pytest.raises(H.HpgqError) as e:
                call()
            assert e.value.code == H.E_READ_TOO_LONG
        del t
        ad.reset()
        fits = _reads([_plant(b"C" * 100, 88, DEF[2]), b"", _plant(b"G" * 99, 0, DEF[3])])
        _count(ad, fits)
        _same(ad.table(), adapt_ref.table_of(fits, DEF))


# -- 7. few workgroups --------------------------------------------------------------------------

@pytest.mark.parametrize("max_wg", [1, 2, 3])
def test_few_workgroups(set_cases, max_wg):
    probes, reads, want = set_cases["32"]
    with H.AdapterContent(probes, rows=150) as ad:
        ad.set_max_workgroups(max_wg)
        _count(ad, reads, lead=1)
        _same(ad.table(), want)


# -- 8. hostile atlas ---------------------------------------------------------------------------

def test_hostile_atlas():
    reads, planted = HL.atlas(HL.AUTO_LENGTHS)
    assert len(planted) > 2000
    probes = DEF + [b"CGTACGTACGTA"]                     # from the atlas' own ACGT base pattern
    want = adapt_ref.table_of(reads, probes)
    assert int(want[0][-1].sum()) > 500 and want[1]["npos"] == max(HL.AUTO_LENGTHS)
    with H.AdapterContent(probes, rows=max(HL.AUTO_LENGTHS)) as ad:
        t = _count(ad, reads, lead=13, seq_shift=2)
        _same(ad.table(), want)
        HL.inputs_unchanged(t)
