"""Engine / ChaosGame: Python handles over libhpgq contexts.

Host arrays are numpy; device buffers are passed as raw pointers (ints), so a
caller may own HBM through torch, hipMalloc or anything else.  Mirrors the
reference's worker-stage call shape: one call per batch, counters merged on
the device until read back (src/stats_fastq.c:202-253).
"""
import ctypes as C

import numpy as np

from ._abi import (lib, check, Params, Batch, Summary, GsInfo, QdistRow, DupLevels, AdaptInfo, ClipInfo, OvlInfo, OvlCorrectInfo, OvlMergeInfo, OVL_INSERT_BINS,
                   counters_len,
                   CGR_ALL_READS, ROUTES, E_PAIRING, QDIST_VALUES, DUP_LEVELS, HpgqError)

# Kernel route for new Engines (tests / A/B: a key of ROUTES, or None for the
# library's automatic chain).  Applied through hpgq_debug_set_route: the
# library itself reads no routing choice from the environment.
DEFAULT_ROUTE = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_batch(seq, qual, idx):
    """hpgq_batch_t over host numpy arrays (uint8, uint8, int32 of n+1)."""
    assert seq.dtype == np.uint8 and qual.dtype == np.uint8 and idx.dtype == np.int32
    assert seq.flags.c_contiguous and qual.flags.c_contiguous and idx.flags.c_contiguous
    b = Batch(len(idx) - 1, seq.ctypes.data, qual.ctypes.data, idx.ctypes.data)
    b._keep = (seq, qual, idx)   # the struct holds raw pointers: keep the arrays alive with it
    return b


def device_batch(num_reads, seq_ptr, qual_ptr, idx_ptr):
    return Batch(int(num_reads), int(seq_ptr), int(qual_ptr), int(idx_ptr))


class _Handle:
    """A libhpgq handle.  `_prefix` names the class's C functions: <prefix>_open,
    <prefix>_close and, where the C library has them, the pass-through methods
    below (a class whose prefix lacks one raises AttributeError from the
    library lookup)."""

    _prefix = None
    _h = None   # (the class's default: close and __del__ are safe when __init__ raised before the handle existed)

    def _open(self, *args):
        name = self._prefix + "_open"
        h = C.c_void_p()
        check(getattr(lib, name)(C.byref(h), *args), name)
        self._h = h

    def _call(self, what, *args):
        name = f"{self._prefix}_{what}"
        check(getattr(lib, name)(self._h, *args), name)

    def close(self):
        if self._h:
            getattr(lib, self._prefix + "_close")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._call("sync")

    def reset(self):
        self._call("reset")

    def set_max_workgroups(self, max_wg):
        """<prefix>_debug_set_max_workgroups: at most max_wg workgroups per
        launch (0: no limit); tests only."""
        self._call("debug_set_max_workgroups", int(max_wg))

    def count_device(self, batch, mask_ptr=None):
        self._call("count_device", C.byref(batch), mask_ptr)

    def reserve_length(self, max_len):
        """<prefix>_reserve_length: room for reads of up to max_len."""
        self._call("reserve_length", int(max_len))


class Engine(_Handle):
    """One hpgq_ctx: a HIP stream + device counters on `device`."""

    _prefix = "hpgq"

    def __init__(self, params, device=0, route=None):
        if not isinstance(params, Params):
            raise TypeError("params must be hpgfastq.Params")
        self.params = params
        self.lmax = params.lmax
        self.nsets = 2 if params.paired else 1
        self._open(device, C.byref(params))
        route = route if route is not None else DEFAULT_ROUTE
        if route is not None and route != "auto":
            self.set_route(route)

    def set_route(self, route):
        """hpgq_debug_set_route: 'auto', 'single' (catch-all alone), 'tri' /
        'hex' / 'wide' first, 'auto_fixed' (no adaptive first stage)."""
        check(lib.hpgq_debug_set_route(self._h, ROUTES[route]), "hpgq_debug_set_route")

    def stage_waves(self, stage, chain=0):
        """hpgq_debug_stage_waves -> (waves the stage launches at most, reads
        per unit it iterates over); stage 1..3, or 4 for the long-read tail's
        second pass.  HpgqError(-1) for a stage the chain does not have."""
        w, b = C.c_int(0), C.c_int(0)
        check(lib.hpgq_debug_stage_waves(self._h, int(chain), int(stage), C.byref(w), C.byref(b)),
              "hpgq_debug_stage_waves")
        return w.value, b.value

    @property
    def stream(self):
        return lib.hpgq_stream(self._h)

    @property
    def kernel_name(self):
        """The engine kernel instance this ctx launches."""
        return lib.hpgq_kernel_name(self._h).decode()

    @property
    def kernel_chain(self):
        """The ctx's kernel chain: first stage -> follow-up stages."""
        return lib.hpgq_kernel_chain(self._h).decode()

    def run_host(self, batch, batch2=None, mask=None, trim=None):
        """Host numpy batch; mask/trim are numpy outputs valid after sync()."""
        check(lib.hpgq_run_host(self._h, C.byref(batch), C.byref(batch2) if batch2 else None,
                                _ptr(mask), _ptr(trim)), "hpgq_run_host")

    def run_host_in_place(self, mates, mask=None, trim=None):
        """hpgq_host_batch + hpgq_run_host: each (seq u8, qual u8, idx i32 from 0)
        of `mates` is written straight into the ctx's staging slot (no copy in
        the library); mask/trim are numpy outputs valid after sync()."""
        bs = [Batch() for _ in mates]
        nb = [int(ix[-1]) for (_s, _q, ix) in mates]
        n = len(mates[0][2]) - 1
        check(lib.hpgq_host_batch(self._h, n, nb[0], nb[1] if len(mates) > 1 else 0, C.byref(bs[0]),
                                  C.byref(bs[1]) if len(mates) > 1 else None), "hpgq_host_batch")
        for b, (sq, ql, ix) in zip(bs, mates):
            C.memmove(b.data_indices, ix.ctypes.data, ix.nbytes)
            C.memmove(b.seq, sq.ctypes.data, int(ix[-1]))
            C.memmove(b.quality, ql.ctypes.data, int(ix[-1]))
        check(lib.hpgq_run_host(self._h, C.byref(bs[0]), C.byref(bs[1]) if len(mates) > 1 else None,
                                _ptr(mask), _ptr(trim)), "hpgq_run_host")

    def run_device(self, batch, batch2=None, mask_ptr=None, trim_ptr=None):
        check(lib.hpgq_run_device(self._h, C.byref(batch), C.byref(batch2) if batch2 else None,
                                  mask_ptr, trim_ptr), "hpgq_run_device")

    def counters(self):
        n = lib.hpgq_counters_size(self._h)
        out = np.zeros(n, dtype=np.uint64)
        check(lib.hpgq_read_counters(self._h, _ptr(out), n), "hpgq_read_counters")
        return out

    def counters_ext(self):
        """hpgq_read_counters_ext -> (counters of every merged read at full
        length in the layout of lmax_ext, lmax_ext).  Collective after
        allreduce() (every rank calls it)."""
        L = C.c_int32(0)
        check(lib.hpgq_read_counters_ext(self._h, None, 0, C.byref(L)), "hpgq_read_counters_ext")
        out = np.zeros(counters_len(L.value) * self.nsets, dtype=np.uint64)
        L2 = C.c_int32(0)
        check(lib.hpgq_read_counters_ext(self._h, _ptr(out), out.size, C.byref(L2)), "hpgq_read_counters_ext")
        assert L2.value == L.value
        return out, L.value

    def counters_device_ptr(self):
        return lib.hpgq_counters_device(self._h)

    def comm_init(self, nranks, rank, uid):
        check(lib.hpgq_comm_init(self._h, nranks, rank, uid), "hpgq_comm_init")

    def allreduce(self):
        check(lib.hpgq_allreduce(self._h), "hpgq_allreduce")

    def comm_count(self):
        """Ranks in the ctx's RCCL communicator (ncclCommCount)."""
        n = C.c_int(0)
        check(lib.hpgq_comm_count(self._h, C.byref(n)), "hpgq_comm_count")
        return n.value

    def process(self, seq, qual, idx, seq2=None, qual2=None, idx2=None):
        """Convenience: one host batch -> (mask, trim); counters accumulate."""
        n = len(idx) - 1
        b = host_batch(seq, qual, idx)
        b2 = host_batch(seq2, qual2, idx2) if self.params.paired else None
        mask = np.zeros(n, dtype=np.uint8)
        trim = np.zeros(n * self.nsets, dtype=np.uint32)
        self.run_host(b, b2, mask, trim)
        self.sync()
        return mask, trim


def comm_unique_id():
    buf = C.create_string_buffer(128)
    check(lib.hpgq_comm_unique_id(buf), "hpgq_comm_unique_id")
    return buf.raw


def summary(counter_set, lmax):
    s = Summary()
    arr = np.ascontiguousarray(counter_set[:counters_len(lmax)], dtype=np.uint64)
    check(lib.hpgq_counters_summary(_ptr(arr), lmax, C.byref(s)), "hpgq_counters_summary")
    return {f: getattr(s, f) for f, _ in Summary._fields_}


class ChaosGame(_Handle):
    """hpgq_cgr: chaos_game_fill_tables on the device (old/chaos_game.c:165)."""

    _prefix = "hpgq_cgr"

    def __init__(self, k, base_quality=33, device=0, path=0):
        self.k = k
        self.dim = 1 << k
        self._open(device, k, base_quality)
        self._call("set_path", path)

    @property
    def stream(self):
        return lib.hpgq_cgr_stream(self._h)

    def fill_device(self, batch, status_ptr=None, mode=CGR_ALL_READS):
        check(lib.hpgq_cgr_fill_device(self._h, C.byref(batch), status_ptr, mode),
              "hpgq_cgr_fill_device")

    def comm_init(self, nranks, rank, uid):
        """RCCL communicator for the table sum (uid from comm_unique_id())."""
        check(lib.hpgq_cgr_comm_init(self._h, nranks, rank, uid), "hpgq_cgr_comm_init")

    def allreduce(self):
        """u32 sum of every rank's tables and word count (hpgq_cgr_allreduce);
        tables() returns it until the next fill or reset."""
        check(lib.hpgq_cgr_allreduce(self._h), "hpgq_cgr_allreduce")

    def comm_count(self):
        n = C.c_int(0)
        check(lib.hpgq_cgr_comm_count(self._h, C.byref(n)), "hpgq_cgr_comm_count")
        return n.value

    def last_replays(self):
        return int(lib.hpgq_cgr_last_replays(self._h))

    def last_exact(self):
        """1 if the last synced fill ran the exact double simulation, 0 if the
        stream pass was proven exact (hpgq_cgr_last_exact)."""
        return int(lib.hpgq_cgr_last_exact(self._h))

    def tables(self):
        cells = self.dim * self.dim
        ts = np.zeros(cells, dtype=np.uint32)
        tq = np.zeros(cells, dtype=np.uint32)
        wc = np.zeros(1, dtype=np.uint32)
        check(lib.hpgq_cgr_read(self._h, _ptr(ts), _ptr(tq), _ptr(wc)), "hpgq_cgr_read")
        return ts.reshape(self.dim, self.dim), tq.reshape(self.dim, self.dim), int(wc[0])


def cgr_write_gs(path, k, table, word_count):
    """hpgq_cgr_write_gs: a genomic-signature file (header_gs_t + dim*dim u32)."""
    t = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
    check(lib.hpgq_cgr_write_gs(path.encode(), k, _ptr(t), word_count), "hpgq_cgr_write_gs")


def cgr_load_gs(path, k):
    """hpgq_cgr_load_gs -> (table u32 [dim*dim], ref_word_count)."""
    t = np.zeros(1 << (2 * k), dtype=np.uint32)
    w = np.zeros(1, dtype=np.uint32)
    check(lib.hpgq_cgr_load_gs(path.encode(), k, _ptr(t), _ptr(w)), "hpgq_cgr_load_gs")
    return t, int(w[0])


def cgr_table_dif(k, table_seq, fq_words, table_gs, ref_words):
    """hpgq_cgr_table_dif -> (int32 table_dif, highest, lowest)."""
    ts = np.ascontiguousarray(table_seq, dtype=np.uint32).reshape(-1)
    tg = np.ascontiguousarray(table_gs, dtype=np.uint32).reshape(-1)
    d = np.zeros(ts.size, dtype=np.int32)
    hl = np.zeros(2, dtype=np.int32)
    check(lib.hpgq_cgr_table_dif(k, _ptr(ts), fq_words, _ptr(tg), ref_words, _ptr(d),
                                 _ptr(hl), hl.ctypes.data + 4), "hpgq_cgr_table_dif")
    return d, int(hl[0]), int(hl[1])


def cgr_dif_stats(k, table_dif):
    d = np.ascontiguousarray(table_dif, dtype=np.int32).reshape(-1)
    ms = np.zeros(2, dtype=np.float64)
    check(lib.hpgq_cgr_dif_stats(k, _ptr(d), _ptr(ms), ms.ctypes.data + 8), "hpgq_cgr_dif_stats")
    return float(ms[0]), float(ms[1])


def cgr_normalize_quality(k, table_seq, table_q):
    ts = np.ascontiguousarray(table_seq, dtype=np.uint32).reshape(-1)
    tq = np.array(table_q, dtype=np.uint32).reshape(-1)
    check(lib.hpgq_cgr_normalize_quality(k, _ptr(ts), _ptr(tq)), "hpgq_cgr_normalize_quality")
    return tq


def cgr_write_pgm(path, k, table, norm):
    t = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
    check(lib.hpgq_cgr_write_pgm(path.encode(), k, _ptr(t), norm), "hpgq_cgr_write_pgm")


def cgr_write_images(report_dir, fq_path, k, table_seq, table_q, fq_words, table_dif=None):
    """hpgq_cgr_write_images: <dir>/<fq>_k=<k>_FG.pgm, _QQ.pgm (+ _FG_dif.pgm)."""
    ts = np.ascontiguousarray(table_seq, dtype=np.uint32).reshape(-1)
    tq = np.array(table_q, dtype=np.uint32).reshape(-1)
    d = None if table_dif is None else np.ascontiguousarray(table_dif, dtype=np.int32).reshape(-1)
    check(lib.hpgq_cgr_write_images(report_dir.encode(), fq_path.encode(), k, _ptr(ts), _ptr(tq),
                                    fq_words, _ptr(d) if d is not None else None),
          "hpgq_cgr_write_images")


class Kmers(_Handle):
    """hpgq_kmers: `stats --kmers` 5-mer counts per start position
    (merge src/stats_fastq.c:384-410; build-defined per-read rule)."""

    _prefix = "hpgq_kmers"

    def __init__(self, lmax, device=0, stream=None):
        self.lmax = lmax
        self.npos = max(lmax - 4, 0)
        self._open(device, lmax, stream)

    def by_pos(self):
        out = np.zeros((1024, self.npos), dtype=np.uint64)
        check(lib.hpgq_kmers_read(self._h, _ptr(out), out.size), "hpgq_kmers_read")
        return out

    def by_pos_ext(self):
        """hpgq_kmers_read_ext: every start, [1024, npos_ext]."""
        P = C.c_int32(0)
        check(lib.hpgq_kmers_read_ext(self._h, None, 0, C.byref(P)), "hpgq_kmers_read_ext")
        out = np.zeros((1024, P.value), dtype=np.uint64)
        check(lib.hpgq_kmers_read_ext(self._h, _ptr(out), out.size, C.byref(P)), "hpgq_kmers_read_ext")
        return out


class QualityDist(_Handle):
    """hpgq_qdist: `stats --quality-dist`, bases per (read position, raw quality
    byte) of the counted reads.  `rows` positions are reserved
    (reserve_length grows them); `base` is a speed hint: the 64 byte values from
    it are counted on chip.  sync(): HpgqError -4 after a counted read longer
    than the rows, until reset()."""

    _prefix = "hpgq_qdist"

    def __init__(self, rows, base=33, device=0, stream=None):
        self._open(device, rows, base, stream)

    def hist(self):
        """u64 [npos, 256], npos = the longest counted read (synchronises)."""
        P = C.c_int32(0)
        check(lib.hpgq_qdist_read(self._h, None, 0, C.byref(P)), "hpgq_qdist_read")
        out = np.zeros((P.value, QDIST_VALUES), dtype=np.uint64)
        check(lib.hpgq_qdist_read(self._h, _ptr(out), out.size, C.byref(P)), "hpgq_qdist_read")
        return out


def _qdist_table(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != QDIST_VALUES:
        raise ValueError("a quality-distribution table is (npos, 256) u64")
    return a


def qdist_add(dst, src):
    """hpgq_qdist_add: dst[:len(src)] += src, in place (dst: a C-contiguous
    (npos, 256) u64 array with at least src's rows)."""
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint64 and dst.flags.c_contiguous
            and dst.ndim == 2 and dst.shape[1] == QDIST_VALUES):
        raise ValueError("dst must be a C-contiguous (npos, 256) u64 array")
    src = _qdist_table(src)
    check(lib.hpgq_qdist_add(_ptr(dst), dst.shape[0], _ptr(src), src.shape[0]), "hpgq_qdist_add")
    return dst


def qdist_quantiles(hist, phred):
    """hpgq_qdist_quantiles: int64 [npos, 8] = count, min, P10, Q1, median, Q3,
    P90, max per position (qualities: (signed char)byte - phred)."""
    hist = _qdist_table(hist)
    rows = (QdistRow * max(hist.shape[0], 1))()
    check(lib.hpgq_qdist_quantiles(_ptr(hist), hist.shape[0], int(phred), rows), "hpgq_qdist_quantiles")
    out = np.zeros((hist.shape[0], 8), dtype=np.int64)
    for p in range(hist.shape[0]):
        r = rows[p]
        out[p, 1:] = (r.min, r.p10, r.q1, r.median, r.q3, r.p90, r.max)
        out.view(np.uint64)[p, 0] = r.count   # (a count of 2^63 or more: its two's complement)
    return out


class AdapterContent(_Handle):
    """hpgq_adapt: `stats --adapters`, per probe the counted reads whose first
    occurrence of it starts at each read position.  `probes`:
    byte strings of 8 .. 32 A C G T, at most 32 of them (None: the default
    set).  `rows` positions are reserved (reserve_length grows them).  sync():
    HpgqError -4 after a counted read longer than the rows, until reset()."""

    _prefix = "hpgq_adapt"

    def __init__(self, probes=None, rows=1024, device=0, stream=None):
        if probes is None:
            probes = [p for _, p in adapt_defaults()]
        self.probes = [p.encode() if isinstance(p, str) else bytes(p) for p in probes]
        arr = (C.c_char_p * max(len(self.probes), 1))(*self.probes)
        self._open(device, arr, len(self.probes), rows, stream)

    def table(self):
        """(first u64 [nprobes, npos], dict(reads, with_any, nprobes, npos)); npos =
        the longest counted read (synchronises)."""
        info = AdaptInfo()
        check(lib.hpgq_adapt_read(self._h, None, 0, C.byref(info)), "hpgq_adapt_read")
        out = np.zeros((info.nprobes, info.npos), dtype=np.uint64)
        check(lib.hpgq_adapt_read(self._h, _ptr(out), out.size, C.byref(info)), "hpgq_adapt_read")
        return out, dict(reads=int(info.reads), with_any=int(info.with_any), nprobes=int(info.nprobes),
                         npos=int(info.npos))


def adapt_add(dst, src):
    """hpgq_adapt_add: dst[:, :src.shape[1]] += src, in place (both C-contiguous
    (nprobes, npos) u64 arrays, dst with at least src's positions)."""
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint64 and dst.flags.c_contiguous and dst.ndim == 2):
        raise ValueError("dst must be a C-contiguous (nprobes, npos) u64 array")
    src = np.ascontiguousarray(src, dtype=np.uint64)
    if src.ndim != 2 or src.shape[0] != dst.shape[0]:
        raise ValueError("src must be (nprobes, npos) u64 with dst's probes")
    check(lib.hpgq_adapt_add(_ptr(dst), dst.shape[1], _ptr(src), src.shape[1], dst.shape[0]), "hpgq_adapt_add")
    return dst


def adapt_find(s, probe):
    """hpgq_adapt_find: the lowest position of probe in the bytes s, -1 if none
    (HpgqError -1 for a probe that breaks the rules)."""
    s = bytes(s)
    r = lib.hpgq_adapt_find(s, len(s), probe.encode() if isinstance(probe, str) else bytes(probe))
    if r == -2:
        raise HpgqError(-1, "hpgq_adapt_find")
    return int(r)


def adapt_defaults():
    """hpgq_adapt_default: [(name, probe)] of the default set, both bytes."""
    out = []
    for i in range(lib.hpgq_adapt_default(-1, None, None)):
        name, probe = C.c_char_p(), C.c_char_p()
        lib.hpgq_adapt_default(i, C.byref(name), C.byref(probe))
        out.append((name.value, probe.value))
    return out


def _probe_array(probes):
    if probes is None:
        probes = [p for _, p in adapt_defaults()]
    probes = [p.encode() if isinstance(p, str) else bytes(p) for p in probes]
    return probes, (C.c_char_p * max(len(probes), 1))(*probes)


class AdapterClip(_Handle):
    """hpgq_clip: `edit --clip-adapters`, every read cut at the lowest position at
    which a probe matches, whole or running off the read's end by at least
    `min_overlap` bases.  `probes` as AdapterContent's (None:
    the default set).  All pointers are device pointers (ints)."""

    _prefix = "hpgq_clip"

    def __init__(self, probes=None, min_overlap=8, device=0, stream=None):
        self.probes, arr = _probe_array(probes)
        self.min_overlap = int(min_overlap)
        self._open(device, arr, len(self.probes), self.min_overlap, stream)

    def find(self, batch, pos_ptr, probe_ptr=None):
        """hpgq_clip_find_device: pos u32 [n] and, unless None, probe u8 [n] (async)."""
        self._call("find_device", C.byref(batch), pos_ptr, probe_ptr)

    def clip_device(self, batch, seq_ptr, qual_ptr, idx_ptr, pos_ptr=None, probe_ptr=None):
        """hpgq_clip_device: the kept reads into the caller's buffers (async)."""
        self._call("device", C.byref(batch), seq_ptr, qual_ptr, idx_ptr, pos_ptr, probe_ptr)

    def clip_batch(self, batch):
        """hpgq_clip_batch_device: the kept reads as a Batch over buffers the
        handle owns, valid until the next clip_batch or close."""
        out = Batch()
        self._call("batch_device", C.byref(batch), C.byref(out))
        return out

    def info(self):
        """dict(reads, clipped, bases_removed, by_probe [nprobes], nprobes, min_overlap); synchronises."""
        i = ClipInfo()
        self._call("read", C.byref(i))
        return dict(reads=int(i.reads), clipped=int(i.clipped), bases_removed=int(i.bases_removed),
                    by_probe=[int(x) for x in i.by_probe[:i.nprobes]], nprobes=int(i.nprobes),
                    min_overlap=int(i.min_overlap))


def clip_find(s, probes=None, min_overlap=8):
    """hpgq_clip_find: (c, winning probe or -1) of the bytes s (HpgqError -1 for
    a set or a min_overlap that breaks the rules)."""
    s = bytes(s)
    probes, arr = _probe_array(probes)
    who = C.c_int(-1)
    c = lib.hpgq_clip_find(s, len(s), arr, len(probes), int(min_overlap), C.byref(who))
    if c == -2:
        raise HpgqError(-1, "hpgq_clip_find")
    return int(c), int(who.value)


class OverlapClip(_Handle):
    """hpgq_ovl: `edit --clip-overlap`, a pair's insert length from the overlap of
    mate 1 with the reverse complement of mate 2 (at least `min_overlap` facing
    bases, at most `max_mismatches` of them not complementary), both mates cut
    there.  `correct`: (phred, high, low) switches on the
    correction of the kept reads' facing bases, `inserts` the histogram of the
    insert lengths (§2.14); both are off by default and can be switched between
    any two calls.  All pointers are device pointers (ints)."""

    _prefix = "hpgq_ovl"

    def __init__(self, min_overlap=30, max_mismatches=5, correct=None, inserts=False, device=0, stream=None):
        self.min_overlap, self.max_mismatches = int(min_overlap), int(max_mismatches)
        self._open(device, self.min_overlap, self.max_mismatches, stream)
        if correct is not None:
            self.set_correct(correct)
        if inserts:
            self.count_inserts(True)

    def set_correct(self, correct):
        """hpgq_ovl_set_correct: clip_batch corrects from now on with correct =
        (phred, high, low); None: it does not."""
        if correct is None:
            self._call("set_correct", 0, 0, 0, 0)
        else:
            phred, high, low = correct
            self._call("set_correct", 1, int(phred), int(high), int(low))

    def count_inserts(self, on=True):
        """hpgq_ovl_count_inserts: every find and clip_batch counts its F* from now on (or no longer)."""
        self._call("count_inserts", int(bool(on)))

    def correct_info(self):
        """dict(corrected_pairs, corrected_bases [2], on, phred, high, low); synchronises."""
        i = OvlCorrectInfo()
        self._call("read_correct", C.byref(i))
        return dict(corrected_pairs=int(i.corrected_pairs), corrected_bases=[int(x) for x in i.corrected_bases],
                    on=bool(i.on), phred=int(i.phred), high=int(i.high), low=int(i.low))

    def last_inserts_ptr(self):
        """hpgq_ovl_last_inserts: the device pointer (int) to the F* (int32 [n]) of the last
        clip_batch while a switch was on, or of the last merge_batch; None otherwise; valid until the next call."""
        p = C.c_void_p()
        self._call("last_inserts", C.byref(p))
        return p.value

    def inserts(self):
        """hpgq_ovl_read_inserts: u64 [1025], pairs per F* (bin 0: analysed, no overlap); synchronises."""
        out = np.zeros(OVL_INSERT_BINS, dtype=np.uint64)
        self._call("read_inserts", _ptr(out))
        return out

    def find(self, mate1, mate2, insert_ptr=None, pos1_ptr=None, pos2_ptr=None):
        """hpgq_ovl_find_device: insert int32 [n], pos1 / pos2 u32 [n], each unless None (async)."""
        self._call("find_device", C.byref(mate1), C.byref(mate2), insert_ptr, pos1_ptr, pos2_ptr)

    def clip_batch(self, mate1, mate2):
        """hpgq_ovl_batch_device: both mates' kept reads as two Batches over buffers
        the handle owns, valid until the next clip_batch or close."""
        out1, out2 = Batch(), Batch()
        self._call("batch_device", C.byref(mate1), C.byref(mate2), C.byref(out1), C.byref(out2))
        return out1, out2

    def merge_batch(self, mate1, mate2):
        """hpgq_ovl_merge_device: (out1, out2, merged), the pairs
        without an overlap uncut as two Batches and the pairs with F* > 0 as one
        read each, all three compacted, in input order, over buffers the handle
        owns, valid until the next call or close.  last_inserts_ptr() is valid
        after it whatever the switches."""
        out1, out2, merged = Batch(), Batch(), Batch()
        self._call("merge_device", C.byref(mate1), C.byref(mate2), C.byref(out1), C.byref(out2), C.byref(merged))
        return out1, out2, merged

    def merge_info(self):
        """dict(merged_pairs, merged_bases, resolved [2]); synchronises."""
        i = OvlMergeInfo()
        self._call("read_merge", C.byref(i))
        return dict(merged_pairs=int(i.merged_pairs), merged_bases=int(i.merged_bases), resolved=[int(x) for x in i.resolved])

    def info(self):
        """dict(pairs, skipped, overlapping, clipped, bases_removed [2], min_overlap, max_mismatches); synchronises."""
        i = OvlInfo()
        self._call("read", C.byref(i))
        return dict(pairs=int(i.pairs), skipped=int(i.skipped), overlapping=int(i.overlapping), clipped=int(i.clipped),
                    bases_removed=[int(x) for x in i.bases_removed], min_overlap=int(i.min_overlap),
                    max_mismatches=int(i.max_mismatches))


def ovl_find(s1, s2, min_overlap=30, max_mismatches=5):
    """hpgq_ovl_find: F*, 0 or -1 (skipped) of the pair of byte strings
    (HpgqError -1 for parameters that break the rules)."""
    s1, s2 = bytes(s1), bytes(s2)
    f = lib.hpgq_ovl_find(s1, len(s1), s2, len(s2), int(min_overlap), int(max_mismatches))
    if f == -2:
        raise HpgqError(-1, "hpgq_ovl_find")
    return int(f)


def ovl_correct(s1, q1, s2, q2, F, phred=33, high=30, low=14):
    """hpgq_ovl_correct: §2.14's correction of one pair whose F* is F.  Returns
    (s1, q1, s2, q2, [bases changed in mate 1, in mate 2]), the four as new bytes
    (HpgqError -1 for parameters that break the rules or an F the pair cannot have)."""
    bufs = [C.create_string_buffer(bytes(x), max(len(x), 1)) for x in (s1, q1, s2, q2)]
    if len(s1) != len(q1) or len(s2) != len(q2):
        raise ValueError("a mate's quality is as long as its sequence")
    changed = (C.c_uint32 * 2)()
    r = lib.hpgq_ovl_correct(bufs[0], bufs[1], len(s1), bufs[2], bufs[3], len(s2), int(F), int(phred), int(high), int(low),
                             changed)
    if r == -2:
        raise HpgqError(-1, "hpgq_ovl_correct")
    out = [b.raw[:len(x)] for b, x in zip(bufs, (s1, q1, s2, q2))]
    assert r == changed[0] + changed[1]
    return (*out, [int(changed[0]), int(changed[1])])


def ovl_merge(s1, q1, s2, q2, F):
    """hpgq_ovl_merge: §2.15's merged read of one pair whose F* is F.  Returns
    (seq, qual, [bases resolved by mate 1, by mate 2]), both of F bytes (empty
    for F <= 0; HpgqError -1 for an F the pair cannot have)."""
    s1, q1, s2, q2 = (bytes(x) for x in (s1, q1, s2, q2))
    if len(s1) != len(q1) or len(s2) != len(q2):
        raise ValueError("a mate's quality is as long as its sequence")
    n = max(int(F), 0)
    seq, qual = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(n, 1))
    resolved = (C.c_uint32 * 2)()
    r = lib.hpgq_ovl_merge(s1, q1, len(s1), s2, q2, len(s2), int(F), seq, qual, resolved)
    if r == -2:
        raise HpgqError(-1, "hpgq_ovl_merge")
    assert r == n
    return seq.raw[:n], qual.raw[:n], [int(resolved[0]), int(resolved[1])]


def _levels_dict(lv):
    return dict(reads=int(lv.reads), distinct=int(lv.distinct), max_count=int(lv.max_count),
                distinct_at=[int(x) for x in lv.distinct_at], reads_at=[int(x) for x in lv.reads_at])


class Duplication(_Handle):
    """hpgq_dup: `stats --duplication`, the multiset {fingerprint -> count} of
    the counted reads' sequences in a device hash table.  The
    table starts at 2^log2_slots slots and doubles up to 2^log2_max_slots
    (count_device: HpgqError -3 when it would have to grow past that)."""

    _prefix = "hpgq_dup"

    def __init__(self, log2_slots=20, log2_max_slots=32, device=0, stream=None):
        self._open(device, log2_slots, log2_max_slots, stream)

    def levels(self):
        """dict: reads, distinct, max_count, distinct_at[16], reads_at[16] (synchronises)."""
        lv = DupLevels()
        check(lib.hpgq_dup_levels(self._h, C.byref(lv)), "hpgq_dup_levels")
        return _levels_dict(lv)

    def export(self):
        """(keys, counts): u64 arrays, the keys ascending (synchronises)."""
        n = C.c_size_t(0)
        check(lib.hpgq_dup_export(self._h, None, None, 0, C.byref(n)), "hpgq_dup_export")
        keys = np.zeros(n.value, dtype=np.uint64)
        counts = np.zeros(n.value, dtype=np.uint64)
        check(lib.hpgq_dup_export(self._h, _ptr(keys), _ptr(counts), n.value, C.byref(n)), "hpgq_dup_export")
        order = np.argsort(keys, kind="stable")
        return keys[order], counts[order]

    def import_(self, keys, counts):
        """Add counts[i] to the count of keys[i]: the merge of shards' tables."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if keys.ndim != 1 or keys.shape != counts.shape:
            raise ValueError("keys and counts are u64 vectors of one length")
        check(lib.hpgq_dup_import(self._h, _ptr(keys), _ptr(counts), keys.size), "hpgq_dup_import")

    def set_timing(self, on=True):
        check(lib.hpgq_dup_debug_set_timing(self._h, int(on)), "hpgq_dup_debug_set_timing")

    def last_times(self):
        """Measurement: (fingerprint kernel us, insert kernel us) of the last count_device."""
        a, b = C.c_float(0), C.c_float(0)
        check(lib.hpgq_dup_debug_last_times(self._h, C.byref(a), C.byref(b)), "hpgq_dup_debug_last_times")
        return a.value, b.value

    def keep_sequences(self, min_count, arena_bytes=1 << 28):
        """Keeping mode: from now on the bytes of every sequence
        whose count in this table reaches min_count are kept, once, in a device
        arena of arena_bytes.  Only on an empty table; 0 turns it off."""
        check(lib.hpgq_dup_keep_sequences(self._h, min_count, arena_bytes), "hpgq_dup_keep_sequences")

    def count_at_least(self, min_count=1):
        """How many sequences have count >= min_count (synchronises)."""
        total = C.c_size_t(0)
        check(lib.hpgq_dup_top(self._h, min_count, None, None, 0, C.byref(total)), "hpgq_dup_top")
        return total.value

    def top(self, n, min_count=1):
        """(keys, counts): the n most frequent sequences with count >= min_count,
        count descending, ties by key ascending (synchronises)."""
        n = min(int(n), self.count_at_least(min_count))
        keys = np.zeros(n, dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint64)
        total = C.c_size_t(0)
        check(lib.hpgq_dup_top(self._h, min_count, _ptr(keys), _ptr(counts), n, C.byref(total)), "hpgq_dup_top")
        return keys, counts

    def sequence(self, key):
        """The bytes kept for key in this table, or None (synchronises).
        HpgqError -3 after a representative did not fit in the arena."""
        n = C.c_int64(0)
        check(lib.hpgq_dup_sequence(self._h, key, None, 0, C.byref(n)), "hpgq_dup_sequence")
        if n.value < 0:
            return None
        buf = C.create_string_buffer(max(n.value, 1))
        check(lib.hpgq_dup_sequence(self._h, key, buf, n.value, C.byref(n)), "hpgq_dup_sequence")
        return buf.raw[:n.value]

    def kept(self):
        """Tests: (representatives held, the sum of their lengths)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib.hpgq_dup_debug_kept(self._h, C.byref(a), C.byref(b)), "hpgq_dup_debug_kept")
        return a.value, b.value

    def last_keep_time(self):
        """Measurement: the keep kernel's us of the last count_device (timing and keeping on)."""
        a = C.c_float(0)
        check(lib.hpgq_dup_debug_last_keep_time(self._h, C.byref(a)), "hpgq_dup_debug_last_keep_time")
        return a.value

    def info(self):
        """Tests: (log2 of the slots now, growths since the table was opened)."""
        k, r = C.c_int(0), C.c_int64(0)
        check(lib.hpgq_dup_debug_info(self._h, C.byref(k), C.byref(r)), "hpgq_dup_debug_info")
        return k.value, r.value

    def fingerprints(self, batch):
        """Tests: the fingerprint of every read of a device batch, nothing inserted."""
        out = np.zeros(batch.num_reads, dtype=np.uint64)
        check(lib.hpgq_dup_debug_fingerprints(self._h, C.byref(batch), _ptr(out)), "hpgq_dup_debug_fingerprints")
        return out


def dup_fingerprint(data):
    """hpgq_dup_fingerprint: the 64-bit fingerprint of a sequence's bytes."""
    data = bytes(data)
    return int(lib.hpgq_dup_fingerprint(data, len(data)))


def dup_level_bounds():
    return [int(lib.hpgq_dup_level_bound(i)) for i in range(DUP_LEVELS)]


def dup_levels_of(counts):
    """hpgq_dup_levels_of: the levels of a list of counts (host only)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    lv = DupLevels()
    check(lib.hpgq_dup_levels_of(_ptr(counts), counts.size, C.byref(lv)), "hpgq_dup_levels_of")
    return _levels_dict(lv)


def dup_top_of(keys, counts, n, min_count=1):
    """hpgq_dup_top_of: (keys, counts, total) of the n most frequent pairs with
    count >= min_count, count descending, ties by key ascending (host only)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    if keys.ndim != 1 or keys.shape != counts.shape:
        raise ValueError("keys and counts are u64 vectors of one length")
    n = min(int(n), keys.size)
    ok, oc = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    total = C.c_size_t(0)
    check(lib.hpgq_dup_top_of(_ptr(keys), _ptr(counts), keys.size, min_count, _ptr(ok), _ptr(oc), n, C.byref(total)),
          "hpgq_dup_top_of")
    m = min(n, total.value)
    return ok[:m], oc[:m], total.value


class Signature(_Handle):
    """hpgq_gs: the genomic signature of FASTA text, the table
    a --gs-filename file holds.  The text may be cut anywhere between add()s."""

    _prefix = "hpgq_gs"

    def __init__(self, k, device=0, stream=None):
        self.k = k
        self.dim = 1 << k
        self._open(device, k, stream)

    def add(self, text):
        """bytes-like host text (staged; reusable on return) or a device uint8
        tensor (async: keep it alive until sync(), table() or info())."""
        if hasattr(text, "data_ptr"):
            if not text.is_cuda or text.element_size() != 1 or not text.is_contiguous():
                raise ValueError("device text must be a contiguous 1-byte tensor on the GPU")
            check(lib.hpgq_gs_add_device(self._h, text.data_ptr() if text.numel() else None,
                                         text.numel()), "hpgq_gs_add_device")
        else:
            b = bytes(text)
            check(lib.hpgq_gs_add_host(self._h, b, len(b)), "hpgq_gs_add_host")

    def table(self):
        """u32 [dim, dim], [co_x][co_y] (synchronises)."""
        t = np.zeros(self.dim * self.dim, dtype=np.uint32)
        check(lib.hpgq_gs_read(self._h, _ptr(t), None), "hpgq_gs_read")
        return t.reshape(self.dim, self.dim)

    def info(self):
        """{'words', 'bases', 'ns', 'sequences'} (synchronises)."""
        i = GsInfo()
        check(lib.hpgq_gs_read(self._h, None, C.byref(i)), "hpgq_gs_read")
        return {f: int(getattr(i, f)) for f, _ in GsInfo._fields_}


def complete_prefix(buf, at_eof=False):
    """hpgq_fastq_complete_prefix: bytes of `buf` holding whole FASTQ records."""
    return int(lib.hpgq_fastq_complete_prefix(buf, len(buf), 1 if at_eof else 0))


def record_prefix(buf, max_records):
    """hpgq_fastq_record_prefix: (bytes, records) of the first min(max_records,
    whole records in `buf`) four-line records, counted from buf[0]."""
    r = C.c_int64(0)
    n = lib.hpgq_fastq_record_prefix(buf, len(buf), max_records, C.byref(r))
    return int(n), int(r.value)


class Parser(_Handle):
    """hpgq_parser: FASTQ text -> device batch (parsing half of fastq_fread_se,
    src/stats_fastq.c:183, on the GPU)."""

    _prefix = "hpgq_parser"

    def __init__(self, device=0, stream=None):
        self._open(device, stream)
        self.num_reads = 0

    def parse(self, text):
        """Host bytes (whole records) -> device Batch (valid until the next parse)."""
        b = Batch()
        check(lib.hpgq_parse_host(self._h, text, len(text), C.byref(b)), "hpgq_parse_host")
        self.num_reads = int(b.num_reads)
        return b

    def parse_interleaved(self, text):
        """Host bytes of interleaved mates -> (mate 1, mate 2) device batches
        (records 2i and 2i+1); records() then gives all records in text order."""
        b1, b2 = Batch(), Batch()
        check(lib.hpgq_parse_host_interleaved(self._h, text, len(text), C.byref(b1), C.byref(b2)),
              "hpgq_parse_host_interleaved")
        self.num_reads = 2 * int(b1.num_reads)
        return b1, b2

    def pair_check(self, other=None):
        """hpgq_parse_pair_check over the last parse of this parser and `other`
        (None: this parser's interleaved parse): -1 when every pair is in step,
        else the first bad pair."""
        bad = C.c_int64(-1)
        rc = lib.hpgq_parse_pair_check(self._h, other._h if other is not None else None, C.byref(bad))
        if rc != E_PAIRING:
            check(rc, "hpgq_parse_pair_check")
        return int(bad.value)

    @property
    def max_length(self):
        """The longest record of the last parse (hpgq_parser_max_length)."""
        return int(lib.hpgq_parser_max_length(self._h))

    def records(self):
        n = self.num_reads
        out = {k: np.zeros(n, np.uint32) for k in ("start", "seq", "plus", "qual")}
        check(lib.hpgq_parse_records(self._h, _ptr(out["start"]), _ptr(out["seq"]),
                                     _ptr(out["plus"]), _ptr(out["qual"])), "hpgq_parse_records")
        return out
