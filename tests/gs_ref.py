"""The genomic-signature rule (include/hpgq.h hpgq_gs_*), twice:
`loop` is the specification, one byte at a time; `fast` is the same rule in
numpy for megabyte texts.  tests/test_gs_cpu.py checks one against the other;
the GPU tests compare the device with them exactly.

Both return (table, info): table is uint32 [dim, dim] indexed [co_x][co_y],
info is {'words', 'bases', 'ns', 'sequences'}.
"""
import numpy as np

DX = {65: 1, 67: 0, 71: 0, 84: 1}
DY = {65: 0, 67: 0, 71: 1, 84: 1}
FOLD = {97: 65, 99: 67, 103: 71, 116: 84, 110: 78}


def loop(text, k):
    dim = 1 << k
    table = [0] * (dim * dim)
    words = bases = ns = seqs = 0
    hist = []
    in_hdr = False
    for b in bytes(text):
        if in_hdr:
            if b == 10:
                in_hdr = False
            continue
        if b == 62:              # '>' outside a header: a header starts, the word ends
            in_hdr = True
            hist = []
            seqs += 1
            continue
        b = FOLD.get(b, b)
        if b == 78:              # N / n: the word ends
            hist = []
            ns += 1
            continue
        if b not in DX:          # class 4: skipped, the word goes on
            continue
        bases += 1
        hist.append(b)
        hist = hist[-k:]
        if len(hist) == k:       # hist[0] is the oldest base: bit 0
            cx = sum(DX[c] << i for i, c in enumerate(hist))
            cy = sum(DY[c] << i for i, c in enumerate(hist))
            table[cx * dim + cy] = (table[cx * dim + cy] + 1) & 0xFFFFFFFF
            words += 1
    return (np.array(table, dtype=np.uint32).reshape(dim, dim),
            {"words": words, "bases": bases, "ns": ns, "sequences": seqs})


_CODE = np.full(256, 5, dtype=np.uint8)      # 0..3 = dx | dy << 1, 4 = N, 5 = skipped
for _c, _v in ((65, 1), (67, 0), (71, 2), (84, 3), (78, 4)):
    _CODE[_c] = _v
    _CODE[_c + 32] = _v


def fast(text, k):
    dim = 1 << k
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    n = b.size
    info = {"words": 0, "bases": 0, "ns": 0, "sequences": 0}
    table = np.zeros(dim * dim, dtype=np.uint64)
    if n == 0:
        return table.astype(np.uint32).reshape(dim, dim), info
    gt = b == 62
    nl = b == 10
    # inside a header <=> the last '>' or '\n' before the byte is a '>'
    last = np.maximum.accumulate(np.where(gt | nl, np.arange(1, n + 1), 0))
    prev = np.concatenate(([0], last[:-1]))
    hdr = np.where(prev > 0, gt[np.maximum(prev, 1) - 1], False)
    code = _CODE[b]
    out = ~hdr
    info["sequences"] = int(np.count_nonzero(gt & out))
    info["ns"] = int(np.count_nonzero((code == 4) & out))
    info["bases"] = int(np.count_nonzero((code < 4) & out))
    keep = out & ((code <= 4) | gt)
    s = np.where(gt, 4, code)[keep].astype(np.int64)      # 4: the word ends here
    m = s.size
    if m >= k:
        isb = (s < 4).astype(np.int64)
        c = np.concatenate(([0], np.cumsum(isb)))
        valid = (c[k:] - c[:-k]) == k                      # window [j, j + k) is all bases
        cx = np.zeros(m - k + 1, dtype=np.int64)
        cy = np.zeros(m - k + 1, dtype=np.int64)
        for i in range(k):                                 # window's i-th oldest base: bit i
            w = s[i:m - k + 1 + i]
            cx |= (w & 1) << i
            cy |= ((w >> 1) & 1) << i
        cells = (cx * dim + cy)[valid]
        info["words"] = int(cells.size)
        table = np.bincount(cells, minlength=dim * dim).astype(np.uint64)
    return (table & 0xFFFFFFFF).astype(np.uint32).reshape(dim, dim), info


def records(text):
    """The records of a FASTA as reads for oracle/pyref.py cgr_fill: headers
    dropped, case folded, every byte but A/C/G/T/N removed."""
    recs = []
    cur = None
    in_hdr = False
    for b in bytes(text):
        if in_hdr:
            if b == 10:
                in_hdr = False
            continue
        if b == 62:
            in_hdr = True
            if cur is not None:
                recs.append(bytes(cur))
            cur = bytearray()
            continue
        b = FOLD.get(b, b)
        if b in DX or b == 78:
            if cur is None:
                cur = bytearray()
            cur.append(b)
    if cur is not None:
        recs.append(bytes(cur))
    return recs


def fasta(rng, nrec, lo, hi, width, crlf=False, lower=0.3, n_frac=0.01, iupac=0.01,
          header=b">chr%d ACGT>x len"):
    """A random multi-record FASTA (rng: random.Random)."""
    out = bytearray()
    eol = b"\r\n" if crlf else b"\n"
    for r in range(nrec):
        out += (header % r if b"%d" in header else header) + eol
        n = rng.randint(lo, hi)
        s = bytearray()
        for _ in range(n):
            u = rng.random()
            if u < n_frac:
                s.append(rng.choice(b"Nn"))
            elif u < n_frac + iupac:
                s.append(rng.choice(b"RYKMSWrykm"))
            elif u < n_frac + iupac + lower:
                s.append(rng.choice(b"acgt"))
            else:
                s.append(rng.choice(b"ACGT"))
        for i in range(0, n, width):
            out += s[i:i + width] + eol
    return bytes(out)


def fasta_np(seed, nbytes, width=60, n_frac=0.01, lower=0.0, iupac=0.0, header=b">r\n",
             rec_bases=0):
    """A large random FASTA built with numpy: about nbytes bytes, records of
    rec_bases bases (0: one record)."""
    g = np.random.default_rng(seed)
    nb = max(int(nbytes * width / (width + 1)), 1)
    u = g.random(nb)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[g.integers(0, 4, nb)].copy()
    low = u < lower
    s[low] += 32
    s[(u >= lower) & (u < lower + n_frac)] = 78
    iu = (u >= lower + n_frac) & (u < lower + n_frac + iupac)
    s[iu] = np.frombuffer(b"RYKMSWrykm", dtype=np.uint8)[g.integers(0, 10, int(iu.sum()))]
    out = bytearray()
    step = rec_bases or nb
    for a in range(0, nb, step):
        rec = s[a:a + step]
        out += header
        full = rec.size // width * width
        lines = np.empty((full // width, width + 1), dtype=np.uint8)
        lines[:, :width] = rec[:full].reshape(-1, width)
        lines[:, width] = 10
        out += lines.tobytes()
        if rec.size > full:
            out += rec[full:].tobytes() + b"\n"
    return bytes(out)
