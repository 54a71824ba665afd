"""hpgq_gs_* (gfx950) against the rule of tests/gs_ref.py, exactly: the table
and all four counts, for every text length around the kernels' granules, for
what a tile may hold, for texts cut anywhere between calls, for workgroups
that run several tiles, and against the chaos-game accumulator where the two
rules agree."""
import functools
import os
import random

import numpy as np
import pytest

import gs_ref
import hpgfastq as H

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = [1, 2, 5, 7, 8, 12]


@functools.lru_cache(maxsize=None)
def _sig(k):
    return H.Signature(k)


@functools.lru_cache(maxsize=64)
def _ref(text, k):
    table, info = (gs_ref.loop if len(text) <= 300 else gs_ref.fast)(text, k)
    table.setflags(write=False)
    return table, info


def _to_dev(data):
    import torch
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _check(k, text, pieces=None, max_wg=0, what=""):
    """pieces: host bytes or device tensors that concatenate to text."""
    sig = _sig(k)
    sig.set_max_workgroups(max_wg)
    sig.reset()
    for p in ([text] if pieces is None else pieces):
        sig.add(p)
    table, info = sig.table(), sig.info()
    sig.set_max_workgroups(0)
    rt, ri = _ref(bytes(text), k)
    assert info == ri, (what, k, len(text))
    np.testing.assert_array_equal(table, rt, err_msg=f"{what} k={k} n={len(text)}")
    assert int(table.sum(dtype=np.uint64)) == info["words"]


@pytest.mark.parametrize("k", KS)
def test_known_answer(k):
    text = open(os.path.join(GOLD, "gs_kat.fa"), "rb").read()
    _check(k, text, what="kat host")
    _check(k, text, [_to_dev(text)], what="kat device")


@functools.lru_cache(maxsize=None)
def _length_master():
    # one record: 5-byte header, line width 7, 1 % N
    t = gs_ref.fasta_np(11, (1 << 20) + 4096, width=7, n_frac=0.01, header=b">r01\n")
    assert len(t) > (1 << 20) + 1 and t[:5] == b">r01\n" and t[12:13] == b"\n"
    return t


@pytest.mark.parametrize("k", [3, 7])
def test_every_text_length(k):
    """Every length 0..130 and 2^p - 1, 2^p, 2^p + 1 for p = 5..20: each
    power-of-two granule of the kernels (16 B load, 64 B lane, 16 KB pack tile,
    16 KB count group, ...) is crossed by one byte on either side."""
    master = _length_master()
    dev = _to_dev(master)
    lengths = list(range(0, 131))
    for p in range(5, 21):
        lengths += [(1 << p) - 1, 1 << p, (1 << p) + 1]
    for n in lengths:
        _check(k, master[:n], [dev[:n]], what="length device")
        if n <= 130 or n in (4095, 4096, 4097, 16383, 16384, 16385):
            _check(k, master[:n], what="length host")
    # the same lengths from an unaligned start (the kernel loads aligned 16 B)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 65536):
        for a in (1, 7, 15):
            _check(k, master[a:a + n], [dev[a:a + n]], what=f"length device +{a}")


def _tile_texts():
    rng = random.Random(3)
    acgt = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    t = {}
    t["only class 4"] = b"\n" * 65536
    t["100 KB header"] = b">" + b"h" * 100000 + b"\n" + acgt(10)
    t["200 KB of N"] = b">s\n" + acgt(20) + b"N" * 200000 + acgt(20) + b"\n"
    t["line width 1"] = b">w\n" + b"".join(bytes([c]) + b"\n" for c in acgt(150000))
    t["crlf"] = gs_ref.fasta(rng, 3, 100, 3000, 60, crlf=True)
    t["no final newline"] = gs_ref.fasta(rng, 2, 100, 3000, 61).rstrip(b"\n")
    t["header last"] = gs_ref.fasta(rng, 2, 100, 3000, 60) + b">tail header ACGT"
    t["short records"] = b"".join(b">s%d\n" % i + acgt(i % 13) + b"\n" for i in range(400))
    t["gt in header"] = b">a>b>c ACGT>\n" + acgt(50) + b"\n>d>\n" + acgt(50)
    t["ACGTN header"] = b">ACGTNacgtn NNNN ACGT\n" + acgt(100) + b"\n>TTTTTTTTTTTTTTTT\n" + acgt(30)
    t["lower and iupac"] = gs_ref.fasta_np(5, 200000, lower=0.30, iupac=0.05, rec_bases=50000)
    t["100 KB of A"] = b">a\n" + b"A" * 100000 + b"\n"
    t["no header"] = acgt(5000)
    return t


_TILE = _tile_texts()


@pytest.mark.parametrize("name", sorted(_TILE))
@pytest.mark.parametrize("k", KS)
def test_what_a_tile_may_hold(k, name):
    _check(k, _TILE[name], what=name)


@pytest.mark.parametrize("k", KS)
def test_kth_base_is_the_last_byte(k):
    rng = random.Random(k)
    s = bytes(rng.choice(b"ACGT") for _ in range(k))
    for text in (b">r\n" + s, b">r\n" + s[:-1], b">r\nAC\n" * 3 + b">q\n" + s[:k // 2] + b"\n" + s[k // 2:]):
        _check(k, text, what="k-th base last")
        _check(k, text, [_to_dev(text)], what="k-th base last, device")


@functools.lru_cache(maxsize=None)
def _mib():
    return gs_ref.fasta_np(21, 1 << 20, width=60, n_frac=0.002, lower=0.1, rec_bases=300000,
                           header=b">chr ACGT len=300000\n")[:1 << 20]


@pytest.mark.parametrize("max_wg", [1, 2])
@pytest.mark.parametrize("k", [7, 8])
def test_several_tiles_per_workgroup(k, max_wg):
    """1 MiB = 64 pack tiles and 64 count groups on one or two workgroups."""
    text = _mib()
    _check(k, text, [_to_dev(text)], max_wg=max_wg, what=f"max_wg {max_wg}")


def _everything():
    rng = random.Random(9)
    acgt = lambda n: bytes(rng.choice(b"ACGTacgt") for _ in range(n))   # noqa: E731
    t = (acgt(30) + b"\n>h1 ACGTN>x\n" + acgt(61) + b"\r\n" + acgt(5) + b"NNnN" + acgt(40) + b"RYK\n" +
         b">h2\n" + acgt(2) + b"\n>h3\n\n" + acgt(300) + b"\n" + b"N" * 50 + acgt(7) + b" \t" + acgt(9) + b"\n")
    while len(t) < 3000:
        t += b">r%d\n" % len(t) + acgt(rng.randint(0, 200)) + b"\n"
    return t[:3000] + b">end"


def test_two_pieces_cut_at_every_byte():
    k = 3
    text = _everything()
    dev = _to_dev(text)
    for c in range(len(text) + 1):
        if c % 2:
            pieces = [dev[:c], dev[c:]]          # (the second piece starts at any alignment)
        else:
            pieces = [text[:c], text[c:]]
        _check(k, text, pieces, what=f"cut at {c}")


def test_one_byte_per_call():
    k = 3
    text = _everything()[:400]
    dev = _to_dev(text)
    _check(k, text, [text[i:i + 1] for i in range(len(text))], what="bytes, host")
    _check(k, text, [dev[i:i + 1] for i in range(len(text))], what="bytes, device")


def test_seven_random_pieces_host_and_device_mixed():
    k = 3
    text = _mib()
    dev = _to_dev(text)
    rng = random.Random(4)
    for trial in range(3):
        cuts = [0] + sorted(rng.randrange(len(text) + 1) for _ in range(6)) + [len(text)]
        pieces = []
        for i in range(7):
            a, b = cuts[i], cuts[i + 1]
            pieces.append(dev[a:b] if (i + trial) % 2 else text[a:b])
        _check(k, text, pieces, what=f"7 pieces {cuts}")


def test_host_text_larger_than_a_staging_slot():
    """hpgq_gs_add_host cuts at its 8 MB slots; 20 MB takes three."""
    k = 7
    text = gs_ref.fasta_np(8, 20 << 20, n_frac=0.001, rec_bases=5000000)
    _check(k, text, what="20 MB host")


def test_reset_between_two_texts():
    k = 3
    a = b">a\nACGTTGCA\nAC"          # ends inside a word
    b = b">b header without end"     # ends inside a header
    c = b"GT\nACGT\n"
    sig = _sig(k)
    for first in (a, b):
        sig.reset()
        sig.add(first)
        sig.info()
        _check(k, c, what="after reset")   # neither the open word nor the open header survives
    # and without the reset both do
    _check(k, a + c, [a, c], what="carried word")
    _check(k, b + c, [b, c], what="carried header")


@pytest.mark.parametrize("k", [5, 7])
def test_equals_chaos_game_fill_on_run_free_text(k):
    """On an uppercase, N-sprinkled FASTA without long runs the table is the
    table_seq of H.ChaosGame(k).fill_device over its records as reads, one
    call per record (the double state restarts with every call)."""
    import torch
    text = gs_ref.fasta_np(31 + k, 40000, width=60, n_frac=0.01, rec_bases=7000, header=b">rec\n")
    recs = gs_ref.records(text)
    assert len(recs) >= 5
    seq = np.frombuffer(b"".join(recs), dtype=np.uint8)
    idx = np.concatenate(([0], np.cumsum([len(r) for r in recs]))).astype(np.int32)
    pad = np.zeros(H.DEVICE_SLACK, np.uint8)
    d_seq = torch.from_numpy(np.concatenate([seq, pad])).cuda()
    d_qual = torch.from_numpy(np.concatenate([np.full(seq.size, 73, np.uint8), pad])).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    cg = H.ChaosGame(k)
    for i in range(len(recs)):
        cg.fill_device(H.engine.device_batch(1, d_seq.data_ptr(), d_qual.data_ptr(),
                                             d_idx.data_ptr() + 4 * i))
        cg.sync()
    ts, _, wc = cg.tables()
    cg.close()
    sig = _sig(k)
    sig.reset()
    sig.add(text)
    np.testing.assert_array_equal(sig.table(), ts)
    assert sig.info()["words"] == wc
    _check(k, text, what="cgr text")
