"""Hostile inputs and guarded outputs for the GPU tests (a helper, not collected).

  atlas(lengths)          reads that hold every byte value 0..255 at every
                          place a kernel treats differently, and the table of
                          what was planted where
  device_batch(reads)     torch buffers whose surroundings count if touched
  Guarded(n, align, poison)  an output buffer inside memory the test owns:
                          a skipped store leaves poison, a stray one breaks a band
  inputs_unchanged(t)     the uploaded bytes are still what was uploaded

The atlas (`atlas`), over the read lengths it is given:
  * the base pattern is ACGT in turn with 0..3 N (tests/test_filter_bounds_gpu.py);
  * every byte v at a position = r (mod 4), for every r: 1024 plantings;
  * every v at position 0 of one read and at position len - 1 of another;
  * dense: a read made only of v, and a read with seven v in a row (a whole
    aligned dword holds v four times wherever the read starts);
  * exactly MAX_N N plus one byte whose low bits are N's (N_LIKE); all-A reads
    with one byte whose low bits are C's or G's (GC_LIKE), and their plain twin.
Each planting is made twice, in consecutive reads, one with qualities 25..40
and one with qualities 5..15 (every third planting the low ones first), so the
C2 filter "20," passes the one (when it is long enough) and fails the other,
and the pairs (i, n - 1 - i) couple a passing read with a failing one, two
passing ones and two failing ones.  Every fourth planting, and every
planting at a read's first base, has low-quality ends (5 and 8 bases
of Q 3), which the edit windows TRIMS cut off.  Filler reads, every third of
them empty, sit in the middle so that n = 1 (mod 64) and n is no multiple of
3; the first and the last read are empty.
`deferred_units` puts units of 48 reads into the middle, starting at a multiple
of 48, whose reads of 157..300 bases a first stage hands on (one at position
0; three at 1, B/2, B-1; a whole unit), each holding two planted bytes."""
import numpy as np

import hpgfastq as H
import oracle_lib as O
from test_filter_bounds_gpu import LENGTHS

# the atlases the engine tests run: name -> (read lengths, deferred units, lmax).  "auto" and
# "chain" hold the same reads: at lmax 150 a hex first stage hands every longer read straight to
# the catch-all, at lmax 1024 the wide follow-up stage takes those up to 252 bases in between.
AUTO_LENGTHS = (1, 2, 49, 50, 51, 149, 150, 151, 200, 300, 1100)
ATLAS_SETS = {"hex": (LENGTHS["hex"], 0, 156), "tri": (LENGTHS["tri"], 0, 160), "wide": (LENGTHS["wide"], 0, 252),
              "auto": (AUTO_LENGTHS, 8, 150), "chain": (AUTO_LENGTHS, 8, 1024)}

MAX_N = 2
C2 = dict(read_quality_range="20,", read_length_range="50,")
NOOR = dict(max_N=MAX_N, max_out_of_quality=20)
TRIMS = dict(left_length=10, left_quality_range="20,", right_length=30, right_quality_range="20,")
N_LIKE = (0x6E, 0x46, 0x06, 0x0E, 0xCE)            # n F and three more with byte & 7 == 6
GC_LIKE = (0x63, 0x67, 0x4B, 0x4F, 0xC3, 0xC7)     # c g K O and two with bit 7 set
SEQ_GARBAGE = b"GCGTACGT"
QUAL_GARBAGE = 0x7F
CONFIGS = ("stats", "c2", "noor", "edit", "paired")


def params(config, lmax):
    """The five option sets every engine route is run with."""
    if config == "stats":
        return H.stats_params(lmax=lmax)
    if config == "c2":
        return H.stats_params(lmax=lmax, **C2)
    if config == "noor":
        return H.stats_params(lmax=lmax, **C2, **NOOR)
    p = H.edit_params(lmax=lmax, stats=True, **TRIMS, **C2)
    if config == "paired":
        p.paired = 1
    else:
        assert config == "edit"
    return p


class _Spec:
    def __init__(self, L, hi, ends=False, n_n=0, plants=(), fill=None):
        self.L, self.hi, self.ends, self.n_n, self.plants, self.fill = L, hi, ends, n_n, list(plants), fill


def _build(specs):
    n = len(specs)
    ln = np.array([s.L for s in specs], np.int64)
    idx = np.zeros(n + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    start = idx[:-1].astype(np.int64)
    per = lambda values, t=np.int32: np.repeat(np.asarray(values, t), ln)    # noqa: E731  (a read's value at each byte)
    i = per(np.arange(n))
    j = np.arange(int(idx[-1]), dtype=np.int32) - per(start)
    L = per(ln)
    seq = np.frombuffer(b"ACGT", np.uint8)[(j + i) & 3]
    n_n = per([s.n_n for s in specs])
    seq[(j < 11 * n_n) & (j % 11 == 3)] = ord("N")
    for r, s in enumerate(specs):
        if s.fill is not None:
            seq[start[r]:start[r] + s.L] = s.fill
    planted = np.array([(r, pos, v) for r, s in enumerate(specs) for pos, v in s.plants], np.int64).reshape(-1, 3)
    seq[start[planted[:, 0]] + planted[:, 1]] = planted[:, 2]
    qual = np.where(per([s.hi for s in specs], bool), 33 + 25 + (j * 7 + i) % 16, 33 + 5 + (j * 5 + i) % 11).astype(np.uint8)
    low = per([s.ends for s in specs], bool) & ((j < np.minimum(5, L // 3)) | (j >= L - np.minimum(8, L // 4)))
    qual[low] = 33 + 3
    return O.Reads(seq, qual, idx), planted


def _deferred_units(units, B=48):
    specs = []
    for i in range(units * B):
        u, pos = divmod(i, B)
        cls = u % 4
        L = 0 if (i * 5) % 23 == 3 else 20 + (i * 11) % 41
        if cls == 1 and pos == 0:
            L = 200
        elif cls == 2 and pos in (1, B // 2, B - 1):
            L = {1: 157, B // 2: 252, B - 1: 253}[pos]
        elif cls == 3:
            L = 157 + (i * 29) % 144          # 157 .. 300: the wide stage's and the catch-all's
        plants = []
        if L > 150:
            plants = [((i * 53) % L, (i * 37 + 11) % 256), (L - 1 - i % 5, (i * 91 + 128) % 256)]
            if plants[0][0] == plants[1][0]:
                del plants[1]
        specs.append(_Spec(L, i % 2 == 0, ends=i % 5 == 2, n_n=(i // 5) % 4, plants=plants))
    return specs


class _Lengths:
    """Hands out read lengths from a pool in turn."""

    def __init__(self):
        self.turn = 0

    def next(self, pool, least=1):
        while True:
            L = pool[self.turn % len(pool)]
            self.turn += 1
            if L >= least:
                return L


def _plantings(lengths, dense):
    """What is planted: a list of _Spec arguments plus 'lo_first' (which of
    the planting's two copies comes first), and the planting numbers of the
    look-alikes."""
    long_ = tuple(L for L in lengths if L >= 50)
    assert long_ and min(lengths) >= 1
    take = _Lengths()
    out = []

    def residue(v, r, **kw):
        # r = 0: long enough for "50," and at most one N of its own, so its high-quality copy passes
        L = take.next(long_) if r == 0 else take.next(lengths, r + 1)
        pos = r + 4 * ((v * 13 + r) % ((L - r + 3) // 4))
        out.append(dict(L=L, ends=r == 3, n_n=v % 2 if r == 0 else (4 * v + r) // 5 % 4, plants=[(pos, v)], **kw))

    # the first 256 plantings and the last 256 are each other's pair partners (planting c meets
    # planting P - 1 - c): v at residue 0 with the high qualities first, v at the last base with
    # the low ones first, both long and untrimmed, so every v sits in a pair that passes
    for v in range(256):
        residue(v, 0, lo_first=False)
    for v in range(256):
        for r in (1, 2, 3):
            residue(v, r)
    # v at a read's first base, seven in a row and (below) at its last base: between them in a
    # read of each of the three longest lengths, so every later stage of a chain meets every v
    def longest(v, turn):
        return long_[-1 - (v + turn) % min(3, len(long_))]

    for v in range(256):
        out.append(dict(L=longest(v, 0), ends=True, n_n=v % 2, plants=[(0, v)]))
    if dense:
        for v in range(256):
            L = take.next(lengths)
            out.append(dict(L=L, ends=v % 4 == 3, fill=v, plants=[(p, v) for p in range(L)]))
        for v in range(256):
            L = longest(v, 1)
            first = (v * 5) % (L - 7)
            out.append(dict(L=L, ends=v % 4 == 3, n_n=v % 4, plants=[(first + k, v) for k in range(7)]))
    marks = {"n_like": [], "gc_like": []}
    L0 = min(long_)
    for v in N_LIKE:        # N at 3 and 14: exactly MAX_N of them
        marks["n_like"].append(len(out))
        out.append(dict(L=L0, n_n=MAX_N, plants=[(20, v)]))
    for v in GC_LIKE:
        marks["gc_like"].append(len(out))
        out.append(dict(L=L0, fill=ord("A"), plants=[(7, v)]))
    marks["gc_twin"] = len(out)
    out.append(dict(L=L0, fill=ord("A")))
    for v in range(255, -1, -1):
        L = longest(v, 2)
        out.append(dict(L=L, n_n=v % 2, plants=[(L - 1, v)], lo_first=True))
    # (every third of the others the low qualities first: pairs of two passing and of two failing reads)
    for number, kw in enumerate(out):
        kw.setdefault("lo_first", number % 3 == 0)
    return out, marks


def _layout(plantings, lengths, deferred_units, B=48):
    """The batch's reads in order:
        empty | first half of the copies | filler, deferred units, filler | second half | empty
    Copy k of the 2P copies meets copy 2P - 1 - k in a pair (i, n - 1 - i) whatever
    the middle holds.  The filler before the units starts them at a multiple of
    B; the filler after them makes n = 1 (mod 64) and no multiple of 3.
    -> (specs, read number of copy k)."""
    copies = []
    for kw in plantings:
        kw = dict(kw)
        for hi in ((False, True) if kw.pop("lo_first") else (True, False)):
            copies.append(_Spec(hi=hi, **kw))
    half = len(copies) // 2
    before = -(1 + half) % B
    fixed = 2 + len(copies) + before + deferred_units * B
    after = (1 - fixed) % 64
    while (fixed + after) % 3 == 0 or before + after < 3:
        after += 64
    filler = [_Spec(0 if k % 3 == 0 else lengths[k % len(lengths)], k % 2 == 0, n_n=k % 4) for k in range(before + after)]
    middle = filler[:before] + _deferred_units(deferred_units, B) + filler[before:]
    specs = [_Spec(0, True)] + copies[:half] + middle + copies[half:] + [_Spec(0, False)]
    assert (1 + half + before) % B == 0 and len(specs) % 64 == 1 and len(specs) % 3

    def read_of(k):
        return 1 + k + (len(middle) if k >= half else 0)

    return specs, read_of


def atlas(lengths, *, dense=True, deferred_units=0):
    """-> (O.Reads, int64 [k, 3] rows (read, position, byte) of what was planted).
    reads.marks: {'n_like': reads, 'gc_like': reads, 'gc_twin': read} (the
    high-quality copies)."""
    lengths = tuple(lengths)
    plantings, marks = _plantings(lengths, dense)
    specs, read_of = _layout(plantings, lengths, deferred_units)

    def hi_read(number):      # the read that holds planting `number` with high qualities
        return read_of(2 * number + (1 if plantings[number]["lo_first"] else 0))

    reads, planted = _build(specs)
    reads.marks = {"n_like": [hi_read(c) for c in marks["n_like"]], "gc_like": [hi_read(c) for c in marks["gc_like"]],
                   "gc_twin": hi_read(marks["gc_twin"])}
    for arr in (reads.seq, reads.qual, reads.idx, planted):
        arr.setflags(write=False)
    return reads, planted


def kmer_window_reads():
    """Reads of 40 bases ACGT... with v at position p, all 256 v x p in 0..35:
    both half-tile lanes of the 5-mer kernel and each of a lane's 20 window bytes."""
    base = np.frombuffer(b"ACGT" * 10, np.uint8)
    seq = np.tile(base, 256 * 36).reshape(256, 36, 40).copy()
    for p in range(36):
        seq[:, p, p] = np.arange(256)
    idx = (np.arange(256 * 36 + 1) * 40).astype(np.int32)
    seq = seq.reshape(-1)
    return O.Reads(seq, np.full(seq.size, ord("I"), np.uint8), idx)


def gs_atlas_text():
    """'>h' and, for every byte value v, the line ACGTACG v TACGTAC."""
    return b">h\n" + b"".join(b"ACGTACG" + bytes([v]) + b"TACGTAC\n" for v in range(256))


def reverse(reads):
    """The same reads in reverse order (mate 2 of the paired runs)."""
    ln = np.diff(reads.idx)[::-1]
    idx = np.zeros(reads.n + 1, np.int32)
    idx[1:] = np.cumsum(ln)
    src = np.repeat(reads.idx[:-1][::-1].astype(np.int64) - idx[:-1], ln) + np.arange(int(idx[-1]))
    return O.Reads(np.ascontiguousarray(reads.seq[src]), np.ascontiguousarray(reads.qual[src]), idx)


def _garbage(n, fill, kind, phase=0):
    if isinstance(fill, (bytes, bytearray)):
        pat = np.frombuffer(bytes(fill), np.uint8) if kind == "seq" else np.full(1, QUAL_GARBAGE, np.uint8)
    elif fill == "zero":
        pat = np.zeros(1, np.uint8)
    else:
        assert fill == "hostile", fill
        pat = np.frombuffer(SEQ_GARBAGE, np.uint8) if kind == "seq" else np.full(1, QUAL_GARBAGE, np.uint8)
    return pat[(np.arange(n) + phase) % len(pat)]


class DeviceBatch:
    """What device_batch uploaded: .batch (hpgq_batch_t of device pointers),
    .tensors / .host (name -> torch tensor / the numpy array it was made from),
    .mask_ptr (None without a mask)."""

    def __init__(self):
        self.tensors, self.host, self.batch, self.mask_ptr = {}, {}, None, None


def device_batch(reads, *, lead=0, seq_shift=0, qual_shift=0, lead_fill="hostile", slack_fill="hostile", mask=None):
    """`lead` garbage bytes before data_indices[0] (absolute offsets), the
    sequence / quality pointers moved off their alignment by seq_shift /
    qual_shift (0..3), exactly HPGQ_DEVICE_SLACK bytes after the data.  The
    garbage counts if a kernel takes it for data: sequence GCGTACGT...,
    quality 0x7F ("zero": zeros; bytes: that sequence pattern)."""
    import torch
    assert 0 <= seq_shift <= 3 and 0 <= qual_shift <= 3 and lead >= 0
    t = DeviceBatch()
    for name, data, shift in (("seq", reads.seq, seq_shift), ("qual", reads.qual, qual_shift)):
        t.host[name] = np.concatenate([_garbage(shift + lead, lead_fill, name), data,
                                       _garbage(H.DEVICE_SLACK, slack_fill, name)])
    t.host["idx"] = (reads.idx.astype(np.int64) + lead).astype(np.int32)
    if mask is not None:
        t.host["mask"] = np.ascontiguousarray(mask, np.uint8)
    for name, h in t.host.items():
        t.tensors[name] = torch.from_numpy(h.copy()).cuda() if h.size else torch.empty(0, dtype=torch.uint8, device="cuda")
        assert t.tensors[name].data_ptr() % 4 == 0
    torch.cuda.synchronize()
    t.batch = H.engine.device_batch(reads.n, t.tensors["seq"].data_ptr() + seq_shift,
                                    t.tensors["qual"].data_ptr() + qual_shift, t.tensors["idx"].data_ptr())
    if mask is not None:
        t.mask_ptr = t.tensors["mask"].data_ptr()
    return t


def inputs_unchanged(t):
    """seq, qual, idx and the mask are bit for bit what was uploaded, lead and slack included."""
    for name, h in t.host.items():
        np.testing.assert_array_equal(t.tensors[name].cpu().numpy(), h, err_msg=f"the kernel changed its input {name}")


class Guarded:
    """n_bytes of device memory filled with `poison`, inside a larger buffer
    the test owns: BAND bytes of a known pattern lie on each side.  The start
    has the residue `align` mod 4 (4: aligned).  check() asserts that both
    bands still hold the pattern and returns the interior's bytes."""
    BAND = 256

    def __init__(self, n_bytes, align, poison):
        import torch
        self.n = int(n_bytes)
        self.start = self.BAND + align % 4
        total = self.start + self.n + self.BAND
        self.pattern = ((np.arange(total) * 37 + 11) & 0xFF).astype(np.uint8)
        self.pattern[self.start:self.start + self.n] = poison
        self.poison = poison
        self.buf = torch.from_numpy(self.pattern.copy()).cuda()
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 4 == 0
        self.ptr = self.buf.data_ptr() + self.start

    def check(self):
        got = self.buf.cpu().numpy()
        a, b = self.start, self.start + self.n
        np.testing.assert_array_equal(got[:a], self.pattern[:a], err_msg="a store landed before the output")
        np.testing.assert_array_equal(got[b:], self.pattern[b:], err_msg="a store landed past the output")
        return got[a:b].copy()
