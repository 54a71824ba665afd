"""The chaos game, the genomic signature and the FASTQ parser on hostile bytes
(tests/hostile_lib.py), each exactly against its reference.

  cgr     the atlas (every byte value at every residue, whole reads of it,
          four in a dword) at k = 4 (stream pass and its gate) and k = 8
          (exact kernels), both hpgq_cgr_set_path values, inside a lead and a
          slack that would count; then reads of nothing but A/C/G/T/N inside
          the same garbage, whichever path the gate picks;
  gs      ACGTACG v TACGTAC for every byte value v, whole, cut in two at every
          byte from 3 before to 3 after each v, and laid out so that each v is
          the last / the first byte of a 16-byte load and of a 16 KB tile;
  parser  records whose sequence and quality lines hold every byte value but
          '\\n', lines that start with '@', '+' and '>', LF and CRLF, one text
          and interleaved mates: the device batch is the input reads byte for
          byte, the record offsets are the reference splitter's."""
import functools

import numpy as np
import pytest

import gs_ref
import hostile_lib as HL
import hpgfastq as H
import oracle_lib as O
import pairs_lib as PL
from fastq_io import split_records

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# cgr
# ---------------------------------------------------------------------------

CGR_LENGTHS = (1, 2, 49, 50, 51, 150, 157)


@functools.lru_cache(maxsize=None)
def _cgr_atlas():
    return HL.atlas(CGR_LENGTHS)[0]


@functools.lru_cache(maxsize=None)
def _cgr_want(which, k):
    reads = _cgr_atlas() if which == "atlas" else _plain_reads()
    ts, tq, wc = O.cgr(k, reads)
    return ts, tq, int(wc[0])


@functools.lru_cache(maxsize=None)
def _plain_reads():
    return O.synth(3000, seed=31, L=150, n_per_1024=8)


def _cgr(k, reads, path, lead):
    t = HL.device_batch(reads, lead=lead)
    cg = H.ChaosGame(k, 33, path=path)
    try:
        cg.fill_device(t.batch)
        cg.sync()
        exact = cg.last_exact()
        ts, tq, wc = cg.tables()
    finally:
        cg.close()
    HL.inputs_unchanged(t)
    return ts.reshape(-1), tq.reshape(-1), wc, exact


@pytest.mark.parametrize("lead", [0, 5, 16384 - 6, 16384 + 3])
@pytest.mark.parametrize("path", [H.CGR_PATH_AUTO, H.CGR_PATH_EXACT])
@pytest.mark.parametrize("k", [4, 8])
def test_cgr_atlas(k, path, lead):
    ts, tq, wc, exact = _cgr(k, _cgr_atlas(), path, lead)
    os_, oq, ow = _cgr_want("atlas", k)
    assert wc == ow
    np.testing.assert_array_equal(ts, os_)
    np.testing.assert_array_equal(tq, oq)
    assert exact == 1      # bytes other than A/C/G/T/N: the exact simulation, whatever the path asked for


@pytest.mark.parametrize("lead", [0, 5, 16384 - 6, 16384 + 3])
@pytest.mark.parametrize("k", [4, 8])
def test_cgr_plain_reads_inside_garbage(k, lead):
    """(the path is the gate's business: garbage outside the reads may send it to the exact kernels)"""
    ts, tq, wc, _ = _cgr(k, _plain_reads(), H.CGR_PATH_AUTO, lead)
    os_, oq, ow = _cgr_want("plain", k)
    assert wc == ow
    np.testing.assert_array_equal(ts, os_)
    np.testing.assert_array_equal(tq, oq)


# ---------------------------------------------------------------------------
# gs
# ---------------------------------------------------------------------------

GS_KS = (3, 7, 8)
LINE = 16
GS_GARBAGE = b"ACGTNacgt>\nTTTT\n"      # around the device text: counts if read


@functools.lru_cache(maxsize=None)
def _gs_text(layout):
    """atlas: '>h\\n' + a 16-byte line per v (v at 10 mod 16); last16 / first16:
    the header sized so that v is byte 15 / byte 0 of a 16-byte granule;
    last_tile / first_tile: 1,023 filler lines before each, so that v is the
    last / the first byte of a 16 KB tile."""
    lines = [b"ACGTACG" + bytes([v]) + b"TACGTAC\n" for v in range(256)]
    if layout == "atlas":
        return HL.gs_atlas_text()
    header = b">" + b"h" * (6 if layout.startswith("last") else 7) + b"\n"
    fill = b"ACGTTGCAGATCCTA\n" * 1023 if layout.endswith("tile") else b""
    text = header + b"".join(fill + ln for ln in lines)
    at = len(header) + (len(fill) + LINE) * np.arange(256) + len(fill) + 7      # where each v lies
    gran = 16384 if layout.endswith("tile") else 16
    np.testing.assert_array_equal(np.frombuffer(text, np.uint8)[at], np.arange(256))
    assert (at % gran == (gran - 1 if layout.startswith("last") else 0)).all()
    return text


@functools.lru_cache(maxsize=None)
def _gs_ref(layout, k):
    table, info = gs_ref.fast(_gs_text(layout), k)
    table.setflags(write=False)
    return table, info


GS_LAYOUTS = ("atlas", "last16", "first16", "last_tile", "first_tile")


def _gs_buffer(layout):
    return (GS_GARBAGE * 1024)[:16384] + _gs_text(layout) + GS_GARBAGE * 4


@pytest.fixture(scope="module")
def gs():
    """The signature contexts and the device texts (each between garbage, its
    start 16 KB aligned), closed and freed when the module is done."""
    import torch
    sigs = {k: H.Signature(k) for k in GS_KS}
    bufs = {}
    for layout in GS_LAYOUTS:
        bufs[layout] = torch.frombuffer(bytearray(_gs_buffer(layout)), dtype=torch.uint8).cuda()
        assert bufs[layout].data_ptr() % 16 == 0
    torch.cuda.synchronize()
    yield sigs, bufs
    for sig in sigs.values():
        sig.close()
    bufs.clear()


def _gs_dev(gs, layout):
    buf = gs[1][layout]
    return buf, buf[16384:16384 + len(_gs_text(layout))]


def _gs_check(gs, k, layout, pieces, what):
    sig = gs[0][k]
    sig.reset()
    for p in pieces:
        sig.add(p)
    table, info = sig.table(), sig.info()
    rt, ri = _gs_ref(layout, k)
    assert info == ri, (what, k, info, ri)
    np.testing.assert_array_equal(table, rt, err_msg=f"{what} k={k}")


@pytest.mark.parametrize("layout", GS_LAYOUTS)
@pytest.mark.parametrize("k", GS_KS)
def test_gs_every_byte_value(gs, k, layout):
    text = _gs_text(layout)
    loop = gs_ref.loop(text, k) if len(text) < 10000 else None
    if loop:    # the specification itself on the small layouts
        np.testing.assert_array_equal(loop[0], _gs_ref(layout, k)[0])
        assert loop[1] == _gs_ref(layout, k)[1]
    buf, dev = _gs_dev(gs, layout)
    _gs_check(gs, k, layout, [dev], f"{layout} device")
    _gs_check(gs, k, layout, [text], f"{layout} host")
    np.testing.assert_array_equal(buf.cpu().numpy(), np.frombuffer(_gs_buffer(layout), np.uint8))


@pytest.mark.parametrize("off", range(-3, 4))
@pytest.mark.parametrize("k", GS_KS)
def test_gs_cut_around_every_planted_byte(gs, k, off):
    """Two calls, cut `off` bytes from each planted v (before it: off <= 0):
    device pieces for even v (the second starts at any alignment), host for odd."""
    text = _gs_text("atlas")
    _, dev = _gs_dev(gs, "atlas")
    for v in range(256):
        c = 3 + LINE * v + 7 + off
        pieces = [dev[:c], dev[c:]] if v % 2 == 0 else [text[:c], text[c:]]
        _gs_check(gs, k, "atlas", pieces, f"v {v:#04x} cut at {c}")


# ---------------------------------------------------------------------------
# parser
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hostile_records():
    """2,000 reads of 0 .. 300 bytes, every value but '\\n' in sequence and
    quality, no line ending in '\\r'; lines starting with '@' '+' '>'."""
    rng = np.random.default_rng(77)
    values = np.array([v for v in range(256) if v != 10], np.uint8)
    pairs = []
    for i in range(2000):
        L = int(rng.integers(0, 301)) if i % 50 else (0, 1, 300, 299)[i // 50 % 4]
        if i == 1999:
            L = 300         # (a text ending in an empty line is trimmed there)
        s, q = values[rng.integers(0, 255, L)], values[rng.integers(0, 255, L)]
        if L:
            s[0] = (ord("@"), ord("+"), ord(">"), s[0])[i % 4]
            q[0] = (q[0], ord("@"), ord("+"))[i % 3]
            for a in (s, q):
                if a[-1] == 13:
                    a[-1] = 0
        pairs.append((s.tobytes(), q.tobytes()))
    reads = O.Reads.from_pairs(pairs)
    assert set(reads.seq.tolist()) == set(values.tolist()) == set(reads.qual.tolist())
    return reads


@pytest.fixture(scope="module")
def gpu():
    with H.Engine(H.stats_params(lmax=300)) as e:
        with H.Parser(stream=e.stream) as ps:
            yield e, ps


def _same_batch(e, batch, reads, what):
    seq, qual, idx = PL.fetch(e, batch)
    assert batch.num_reads == reads.n, what
    np.testing.assert_array_equal(idx, reads.idx, err_msg=f"{what}: data_indices")
    for name, got, want in (("seq", seq, reads.seq), ("quality", qual, reads.qual)):
        got = np.frombuffer(got, np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} {name} bytes differ, first at {bad[:8]}: {got[bad[:8]]} for {want[bad[:8]]}"


def _same_records(ps, text, what):
    recs = ps.records()
    ref = np.array(split_records(text), np.uint32)
    for col, name in enumerate(("start", "seq", "plus", "qual")):
        np.testing.assert_array_equal(recs[name], ref[:, col], err_msg=f"{what}: {name} offsets")


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("plus_header", [False, True])
@pytest.mark.parametrize("crlf", [False, True])
def test_parser_keeps_every_byte(gpu, crlf, plus_header, cap):
    e, ps = gpu
    reads = _hostile_records()
    headers = [b"@r%d x:%d" % (i, i % 7) for i in range(reads.n)]
    text = b"".join(PL.records(reads, headers, crlf=crlf, plus_header=plus_header))
    ps.set_max_workgroups(cap)
    what = f"crlf {crlf} plus {plus_header} cap {cap}"
    _same_batch(e, ps.parse(text), reads, what)
    assert ps.max_length == 300
    _same_records(ps, text, what)
    ps.set_max_workgroups(0)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("crlf", [False, True])
def test_parser_interleaved_keeps_every_byte(gpu, crlf, cap):
    e, ps = gpu
    reads = _hostile_records()
    n = reads.n // 2
    mates = [O.Reads.from_pairs(reads.pairs()[m::2]) for m in (0, 1)]
    recs = [PL.records(mates[m], PL.mate_headers(n, m + 1), crlf=crlf, plus_header=bool(m)) for m in (0, 1)]
    text = PL.interleave(*recs)
    ps.set_max_workgroups(cap)
    b1, b2 = ps.parse_interleaved(text)
    what = f"interleaved crlf {crlf} cap {cap}"
    _same_batch(e, b1, mates[0], what + " mate 1")
    _same_batch(e, b2, mates[1], what + " mate 2")
    _same_records(ps, text, what)
    assert ps.pair_check() == -1
    ps.set_max_workgroups(0)
