"""Helpers for the paired-end tests: the mate-name rule restated in Python
(include/hpgq.h) and writers for mate files whose header lines
the tests choose themselves."""
import re

import numpy as np

import hpgfastq as H


def mate_name(header):
    """The header line's bytes after '@' up to the first space, tab, CR or LF."""
    assert header.startswith(b"@")
    return re.match(rb"[^ \t\r\n]*", header[1:]).group(0)


def in_step(h1, h2):
    """"/1" on mate 1 together with "/2" on mate 2 is dropped from both (no other
    suffix pair); then the names must be the same bytes (two empty names are)."""
    a, b = mate_name(h1), mate_name(h2)
    if a.endswith(b"/1") and b.endswith(b"/2"):
        a, b = a[:-2], b[:-2]
    return a == b


def first_bad(headers1, headers2):
    """-1, or the lowest pair out of step, or min(n1, n2) when only the counts differ."""
    n = min(len(headers1), len(headers2))
    for i in range(n):
        if not in_step(headers1[i], headers2[i]):
            return i
    return -1 if len(headers1) == len(headers2) else n


def records(reads, headers, crlf=False, plus_header=False):
    """One FASTQ record (bytes) per read; headers[i] is the whole header line
    without its line end, starting with '@'."""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(reads.n):
        s, q = reads.read(i)
        plus = b"+" + headers[i][1:] if plus_header else b"+"
        out.append(headers[i] + nl + s + nl + plus + nl + q + nl)
    return out


def mate_headers(n, mate, first=0):
    return [f"@r{first + i}/{mate} c".encode() for i in range(n)]


def interleave(recs1, recs2):
    assert len(recs1) == len(recs2)
    return b"".join(a + b for a, b in zip(recs1, recs2))


def paired(p):
    """A copy of the params for mate pairs."""
    q = H.Params.from_buffer_copy(p)
    q.paired = 1
    return q


def fetch(engine, batch):
    """A parser's device batch -> (seq bytes, quality bytes, data_indices) on the
    host; the parser runs on the engine's stream, whose copies follow its kernels."""
    import ctypes as C
    n = int(batch.num_reads)
    if n == 0:
        return b"", b"", np.zeros(1, np.int32)
    idx = np.zeros(n + 1, np.int32)
    H.check(H.lib.hpgq_copy_to_host(engine._h, idx.ctypes.data_as(C.c_void_p), batch.data_indices, idx.nbytes),
            "hpgq_copy_to_host")
    engine.sync()
    end = int(idx[-1])
    seq, qual = np.zeros(max(end, 1), np.uint8), np.zeros(max(end, 1), np.uint8)
    if end:
        H.check(H.lib.hpgq_copy_to_host(engine._h, seq.ctypes.data_as(C.c_void_p), batch.seq, end), "seq")
        H.check(H.lib.hpgq_copy_to_host(engine._h, qual.ctypes.data_as(C.c_void_p), batch.quality, end), "qual")
        engine.sync()
    return seq[:end].tobytes(), qual[:end].tobytes(), idx
