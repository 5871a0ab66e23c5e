"""
``Engine``: one MI355X context holding fragments resident in HBM and running
the per-window kernels through the C ABI (``include/ftk.h``).

This is the host-side object the ``finaletoolkit_amd.frag`` functions drive.
It replaces the reference's "open the file per window, stream Python tuples"
feeder (``utils/_frag_generator.py:112-130``) by "decode once, keep the SoA in
HBM, answer every window in one launch".
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L


def _win(values, open_value):
    if isinstance(values, np.ndarray) and values.dtype == np.int32:
        return np.ascontiguousarray(values)
    if hasattr(values, "data_ptr"):  # int32 torch tensor (host or device), passed through by address
        return values
    return np.ascontiguousarray([open_value if v is None else int(v) for v in values], dtype=np.int32)


_SAVGOL = {}


def savgol_operators(window: int, deg: int):
    """Savitzky-Golay taps and the edge-fit matrices of ``scipy.signal.savgol_filter(mode="interp")``:
    ``coef`` [window] (interior correlation taps) and ``edge`` [2*half, window] whose first ``half`` rows
    map the first ``window`` samples to the first ``half`` outputs and whose last ``half`` rows map the last
    ``window`` samples to the last ``half`` outputs (polyfit + polyval is linear in the samples)."""
    key = (int(window), int(deg))
    if key not in _SAVGOL:
        from scipy.signal import savgol_coeffs
        if window % 2 == 0:
            raise ValueError("savgol_window_size must be odd")
        coef = np.ascontiguousarray(savgol_coeffs(window, deg), dtype=np.float64)
        half = window // 2
        x = np.arange(window)
        eye = np.eye(window)
        edge = np.zeros((2 * half, window))
        for j in range(window):
            p = np.polyfit(x, eye[j], deg)
            edge[:half, j] = np.polyval(p, np.arange(0, half))
            edge[half:, j] = np.polyval(p, np.arange(window - half, window))
        _SAVGOL[key] = (coef, np.ascontiguousarray(edge))
    return _SAVGOL[key]


class _HostBlock:
    """Owner of one host block of the library's result caches (``ftk_host_alloc``: page-locked;
    ``ftk_host_alloc_pageable``: ordinary memory); numpy arrays made from it keep it alive through
    ``__array_interface__`` and the block goes back to the library's cache with the last of them."""

    def __init__(self, lib, nbytes: int, pinned: bool = True):
        p = C.c_void_p()
        rc = (lib.ftk_host_alloc if pinned else lib.ftk_host_alloc_pageable)(int(nbytes), C.byref(p))
        if rc != 0:
            raise L.FtkError(rc, lib.ftk_fragtable_error().decode())
        self._lib, self._ptr = lib, p.value
        self.__array_interface__ = {"data": (p.value, False), "shape": (int(nbytes),), "typestr": "|u1", "version": 3}

    def __del__(self):
        if getattr(self, "_ptr", None):
            try:
                self._lib.ftk_host_free(self._ptr)
            except Exception:  # interpreter shutdown: the library object may already be gone
                pass
            self._ptr = None


# results of at least this many bytes are handed out in page-locked memory (their device -> host copy is the
# long leg of a per-base call); smaller ones are ordinary numpy arrays
PINNED_RESULT_MIN = 8 << 20
_PINNED_RESULTS = __import__("os").environ.get("FTK_PINNED_RESULTS", "1") != "0"
# ftk_wps sends a host output of this many positions or more across the link as int16 and lets the host threads widen
# it into the output (ftk_api.hip, kNarrowMin; FTK_WPS_NARROW_WIRE=0 keeps the plain copy): the device never writes
# such an output, so page-locking it buys nothing and costs 0.2 ms per MB in a process's first call
NARROW_WIRE_MIN = 1 << 22
_NARROW_WIRE = __import__("os").environ.get("FTK_WPS_NARROW_WIRE", "1") != "0"


def _checked_policy(policy: str) -> str:
    if policy not in L.POLICY:
        from .exceptions import InvalidInputError
        raise InvalidInputError(f"{policy} is not a valid policy")
    return policy


class RegionMask:
    """One contig's region masks for the export (``Engine.mask_keep`` / ``format_rows`` / ``write_contig``):
    ``whitelist`` / ``blacklist`` are ``(starts, ends)`` of sorted, disjoint intervals or ``None`` (no such mask; an
    EMPTY whitelist keeps nothing); ``policy`` is ``"midpoint"`` or ``"any"`` and serves both."""
    __slots__ = ("whitelist", "blacklist", "policy")

    def __init__(self, whitelist=None, blacklist=None, policy="midpoint"):
        self.whitelist, self.blacklist, self.policy = whitelist, blacklist, policy


class Engine:
    def __init__(self, device: int = 0):
        self.lib = L.load()
        ctx = C.c_void_p()
        rc = self.lib.ftk_ctx_create(int(device), C.byref(ctx))
        if rc != L.FTK_OK:
            raise L.FtkError(rc, self.lib.ftk_last_error(None).decode())
        self.ctx = ctx
        self.device = int(device)
        self._ids: dict[str, int] = {}
        self._next_id = 0
        self._bam: dict[str, bool] = {}
        # results whose device -> host copy may still be in flight (wps_async), by token: the engine keeps
        # the page-locked block alive until the copy is known to be done, whatever the caller drops
        self._pending: dict[int, np.ndarray] = {}

    # -- plumbing -------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            if self._pending:
                self.lib.ftk_ctx_sync(self.ctx)  # no DMA may outlive its target block
                self._pending.clear()
            self.lib.ftk_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def result_array(self, n: int, dtype, pinned: bool = True) -> np.ndarray:
        """Uninitialised result array of ``n`` elements: page-locked (``ftk_host_alloc``) when large, so that
        the copy back from the device is one DMA; the memory returns to the library's cache when the array
        (and every view of it) is gone.  ``pinned=False``: a recycled block of ordinary memory
        (``ftk_host_alloc_pageable``) for results the host threads fill."""
        dt = np.dtype(dtype)
        nbytes = int(n) * dt.itemsize
        if nbytes < PINNED_RESULT_MIN or not _PINNED_RESULTS:
            return np.empty(int(n), dt)
        try:
            return np.asarray(_HostBlock(self.lib, nbytes, pinned)).view(dt)
        except L.FtkError as e:
            if e.code != L.FTK_ERR_OOM:
                raise
            return np.empty(int(n), dt)  # the limit on page-locked results is reached: ordinary memory

    def _check(self, rc):
        if rc != L.FTK_OK:
            raise L.FtkError(rc, self.lib.ftk_last_error(self.ctx).decode())

    def set_stream(self, hip_stream: Optional[int]):
        self._check(self.lib.ftk_ctx_set_stream(self.ctx, C.c_void_p(hip_stream or 0)))

    def sync(self):
        self._check(self.lib.ftk_ctx_sync(self.ctx))
        self._pending.clear()

    def scratch_fill(self, byte: Optional[int] = None) -> int:
        """Diagnostics (``ftk_ctx_scratch_fill``): fill the context's scratch block as it stands with ``byte`` (0 .. 255;
        ``None``: fill nothing) on the context's stream and return the block's size in bytes.  No result of any call may
        depend on what the block held."""
        n = C.c_int64()
        self._check(self.lib.ftk_ctx_scratch_fill(self.ctx, -1 if byte is None else int(byte), C.byref(n)))
        return int(n.value)

    def timer_start(self):
        self._check(self.lib.ftk_timer_start(self.ctx))

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self.lib.ftk_timer_stop(self.ctx, C.byref(ms)))
        return float(ms.value)

    def event_record(self, slot: int):
        self._check(self.lib.ftk_event_record(self.ctx, int(slot)))

    def event_elapsed_ms(self, slot_a: int, slot_b: int) -> float:
        ms = C.c_float()
        self._check(self.lib.ftk_event_elapsed_ms(self.ctx, int(slot_a), int(slot_b), C.byref(ms)))
        return float(ms.value)

    # -- fragments ------------------------------------------------------------
    def _new_id(self, name: str) -> int:
        """Contig id of ``name``; fresh ids are never reused (released ids must not alias live contigs)."""
        if name not in self._ids:
            self._ids[name] = self._next_id
            self._next_id += 1
        return self._ids[name]

    def _load(self, name: str, call):
        """Run ``call(cid)``, the C calls of one load into ``name``'s id.  A refused load leaves no contig under the
        name: the library drops the id's old columns before it validates the new ones (upload_common), so the name
        goes too, whether it was new or a reload.  Its id is spent; a later load of the name gets a fresh one."""
        cid = self._new_id(name)
        try:
            call(cid)
        except Exception:
            self._ids.pop(name, None)
            self._bam.pop(name, None)
            self.lib.ftk_frags_release(self.ctx, cid)  # (refused before the drop, or after the columns went in)
            raise
        return cid

    def contig_id(self, name: str) -> int:
        if name not in self._ids:
            raise KeyError(name)
        return self._ids[name]

    def has_contig(self, name: str) -> bool:
        return name in self._ids

    @property
    def contigs(self):
        return list(self._ids)

    def is_bam(self, name: str) -> bool:
        return self._bam.get(name, False)

    def load_contig(self, name: str, start, end, mapq, strand=None, r1_start=None, r1_end=None):
        """Upload one contig's start-sorted fragments (host numpy arrays)."""
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        strand = None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)
        n = len(start)
        if not (len(end) == n and len(mapq) == n and (strand is None or len(strand) == n)):
            raise ValueError("fragment columns differ in length")
        r1s = None if r1_start is None else np.ascontiguousarray(r1_start, dtype=np.int32)
        r1e = None if r1_start is None else np.ascontiguousarray(r1_end, dtype=np.int32)

        def call(cid):
            self._check(self.lib.ftk_frags_from_host(self.ctx, cid, L.ptr(start), L.ptr(end), L.ptr(mapq),
                                                     L.ptr(strand), n))
            if r1s is not None:
                self._check(self.lib.ftk_frags_set_read1(self.ctx, cid, L.ptr(r1s), L.ptr(r1e), n))
        cid = self._load(name, call)
        self._bam[name] = r1s is not None
        return cid

    def load_contig_from_table(self, name: str, table, index: int, is_bam: bool):
        """Upload contig ``index`` of a decoded ``ftk_fragtable`` (page-locked columns -> HBM)."""
        cid = self._load(name, lambda cid: self._check(self.lib.ftk_frags_from_table(self.ctx, cid, table, int(index))))
        # an empty BAM contig carries no read1 columns: plain fetch mode is equivalent
        self._bam[name] = bool(is_bam) and self.lib.ftk_fragtable_contig_rows(table, int(index)) > 0
        return cid

    def load_contig_device(self, name: str, d_start, d_end, d_mapq, d_strand, n: int):
        """Adopt columns already in HBM (torch tensors or raw device addresses)."""
        cid = self._load(name, lambda cid: self._check(self.lib.ftk_frags_from_device(
            self.ctx, cid, L.ptr(d_start), L.ptr(d_end), L.ptr(d_mapq), L.ptr(d_strand), int(n))))
        self._bam[name] = False
        return cid

    def set_read1(self, name: str, r1_start, r1_end, n: int):
        """Read1 spans of a resident contig's fragments (host arrays, torch tensors or raw device addresses): the contig
        then answers with the BAM fetch rule (io/alignment.py:245)."""
        self._check(self.lib.ftk_frags_set_read1(self.ctx, self.contig_id(name), L.ptr(r1_start), L.ptr(r1_end), int(n)))
        self._bam[name] = True

    def info(self, name: str):
        n, ml, me = C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self.lib.ftk_frags_info(self.ctx, self.contig_id(name), C.byref(n), C.byref(ml), C.byref(me)))
        return int(n.value), int(ml.value), int(me.value)

    def frags_packed(self, name: str) -> bool:
        """Does the resident contig hold the packed (length, mapq) column (``ftk_frags_packed``)?  Calls whose filter
        allows it read that column instead of ``end`` and ``mapq``."""
        present = C.c_int32()
        self._check(self.lib.ftk_frags_packed(self.ctx, self.contig_id(name), C.byref(present), None, None))
        return bool(present.value)

    def release(self, name: str):
        self._check(self.lib.ftk_frags_release(self.ctx, self._ids.pop(name)))
        self._bam.pop(name, None)

    @staticmethod
    def _interval_pair(starts, stops, flat=True):
        """``(s, e, ps, pe)``: the int64 arrays of an interval list and the pointers the library takes for them (those
        of a stand-in when the list is empty).  ``flat``: the arrays have to be one-dimensional too.  (Two error texts,
        one per kind of caller: tests match on both, so they stay apart.)"""
        s = np.ascontiguousarray(starts, dtype=np.int64)
        e = np.ascontiguousarray(stops, dtype=np.int64)
        if flat and (s.shape != e.shape or s.ndim != 1):
            raise ValueError("starts and stops should be one-dimensional and equal in length")
        if s.shape != e.shape:
            raise ValueError("starts and stops differ in length")
        keep = np.empty(1, np.int64)
        return s, e, L.ptr(s if len(s) else keep), L.ptr(e if len(s) else keep)

    def _library_records(self, call, *dtypes):
        """``call(*outputs)`` with the output arguments of one record set per dtype - a block pointer per column, then
        the count - and the library's blocks home: a list of record arrays, one per dtype.  The blocks are freed
        whatever happens."""
        sets = [([C.c_void_p() for _ in dt.names], C.c_int64()) for dt in dtypes]
        try:
            self._check(call(*[a for ptrs, n in sets for a in (*[C.byref(p) for p in ptrs], C.byref(n))]))
            recs = []
            for dt, (ptrs, n) in zip(dtypes, sets):
                rec = np.zeros(n.value, dt)
                for col, p in zip(dt.names, ptrs):
                    if n.value:  # (one copy: out of the library's block into the records)
                        rec[col] = np.frombuffer((C.c_char * (n.value * dt[col].itemsize)).from_address(p.value), dt[col])
                recs.append(rec)
        finally:
            for ptrs, _ in sets:
                for p in ptrs:
                    if p.value:
                        self.lib.ftk_buffer_free(p.value)
        return recs

    def _filter(self, name, quality_threshold, min_length, max_length, intersect_policy):
        return L.make_filter(quality_threshold, min_length, max_length, intersect_policy,
                             L.FETCH_BAM_READ1 if self.is_bam(name) else L.FETCH_TABIX)

    # -- features -------------------------------------------------------------
    def window_counts(self, name: str, starts: Sequence, stops: Sequence, quality_threshold=30, min_length=None,
                      max_length=None, intersect_policy="midpoint", out=None):
        """a5: fragments per window (frag/_coverage.py:117-130)."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        res = np.zeros(len(ws), np.int64) if out is None else out
        self._check(self.lib.ftk_window_counts(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws),
                                               C.byref(f), L.ptr(res)))
        return res

    def delfi_counts(self, name: str, starts, stops, quality_threshold=30, bl_start=None, bl_end=None, gaps=None):
        """a10: DELFI short/long/num_frags per window (frag/_delfi.py:443-472)."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        n_bl = 0 if bl_start is None else len(bl_start)
        bs = None if n_bl == 0 else np.ascontiguousarray(bl_start, dtype=np.int32)
        be = None if n_bl == 0 else np.ascontiguousarray(bl_end, dtype=np.int32)
        g = L.make_gaps(gaps)
        sh = np.zeros(len(ws), np.int64)
        lg = np.zeros(len(ws), np.int64)
        nf = np.zeros(len(ws), np.int64)
        self._check(self.lib.ftk_delfi_counts(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws),
                                              int(quality_threshold), L.ptr(bs), L.ptr(be), n_bl, C.byref(g),
                                              L.ptr(sh), L.ptr(lg), L.ptr(nf)))
        return sh, lg, nf

    def fraglen_hist(self, name: str, starts, stops, len_lo: int, n_bins: int, quality_threshold=30,
                     min_length=None, max_length=None, intersect_policy="midpoint"):
        """a9: per-window length histogram (frag/_frag_length.py:147-153)."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        hist = np.zeros((len(ws), int(n_bins)), np.uint32)
        over = np.zeros(len(ws), np.int64)
        self._check(self.lib.ftk_fraglen_hist(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws),
                                              C.byref(f), int(len_lo), int(n_bins), L.ptr(hist), L.ptr(over)))
        return hist, over

    def fraglen_stats(self, name: str, starts, stops, len_lo: int, n_bins: int, short_cut: int, quality_threshold=30,
                      min_length=None, max_length=None, intersect_policy="midpoint"):
        """a9: per-window length statistics computed on the device from the histogram rows (frag/_frag_length.py:156-172,
        202-224): float64 ``[n_win, 7]`` = mean median stdev min max count n_short; count 0 = no passing fragment."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        out = np.zeros((len(ws), 7), np.float64)
        self._check(self.lib.ftk_fraglen_stats(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws), C.byref(f),
                                               int(len_lo), int(n_bins), int(short_cut), L.ptr(out)))
        return out

    def window_features(self, name: str, starts, stops, quality_threshold=30, min_length=None, max_length=None,
                        intersect_policy="midpoint", coverage=True, hist=None, delfi=None):
        """Coverage / length histogram / DELFI counts of the same windows in ONE pass
        (``ftk_window_features``).  ``hist=(len_lo, n_bins)``; ``delfi=dict(quality_threshold=,
        bl_start=, bl_end=, gaps=)``.  Returns a dict of the requested arrays."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        n = len(ws)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        out = {}
        cov = np.zeros(n, np.int64) if coverage else None
        h = o = None
        len_lo = n_bins = 0
        if hist is not None:
            len_lo, n_bins = int(hist[0]), int(hist[1])
            h, o = np.zeros((n, n_bins), np.uint32), np.zeros(n, np.int64)
        sh = lg = bs = be = None
        n_bl, q, g = 0, 0, L.make_gaps(None)
        if delfi is not None:
            sh, lg = np.zeros(n, np.int64), np.zeros(n, np.int64)
            q = int(delfi.get("quality_threshold", 30))
            if delfi.get("bl_start") is not None and len(delfi["bl_start"]):
                bs = np.ascontiguousarray(delfi["bl_start"], dtype=np.int32)
                be = np.ascontiguousarray(delfi["bl_end"], dtype=np.int32)
                n_bl = len(bs)
            g = L.make_gaps(delfi.get("gaps"))
        self._check(self.lib.ftk_window_features(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), n, C.byref(f),
                                                 L.ptr(cov), len_lo, n_bins, L.ptr(h), L.ptr(o), q, L.ptr(bs),
                                                 L.ptr(be), n_bl, C.byref(g), L.ptr(sh), L.ptr(lg)))
        if coverage:
            out["coverage"] = cov
        if hist is not None:
            out["hist"], out["overflow"] = h, o
        if delfi is not None:
            out["short"], out["long"] = sh, lg
        return out

    def window_features_wps(self, name: str, starts, stops, wps_out, wps_start: int, wps_stop: int, chrom_size: int,
                            quality_threshold=30, min_length=None, max_length=None, intersect_policy="midpoint",
                            coverage=None, hist=None, hist_bins=None, overflow=None, delfi_q=30, bl_start=None,
                            bl_end=None, gaps=None, short=None, long=None, window_size=120, wps_min_length=120,
                            wps_max_length=180, wps_quality=30):
        """``window_features`` followed by ``wps`` of the same contig as ONE launch when the request allows it
        (``ftk_window_features_wps``: feature blocks first, WPS tiles behind them); every output is a device
        pointer / tensor or a host numpy array the caller allocated, ``wps_out`` must live on the device for the
        merged launch (a host array runs the two launches)."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        len_lo, n_bins = hist_bins if hist_bins is not None else (0, 0)
        bs = be = None
        n_bl = 0
        if bl_start is not None and len(bl_start):
            bs = np.ascontiguousarray(bl_start, dtype=np.int32)
            be = np.ascontiguousarray(bl_end, dtype=np.int32)
            n_bl = len(bs)
        g = L.make_gaps(gaps)
        self._check(self.lib.ftk_window_features_wps(
            self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws), C.byref(f), L.ptr(coverage), int(len_lo),
            int(n_bins), L.ptr(hist), L.ptr(overflow), int(delfi_q), L.ptr(bs), L.ptr(be), n_bl, C.byref(g), L.ptr(short),
            L.ptr(long), int(wps_start), int(wps_stop), int(chrom_size), int(window_size), int(wps_min_length),
            int(wps_max_length), int(wps_quality), L.ptr(wps_out)))

    def all_features_wps(self, name: str, starts, stops, chrom_size: int, quality_threshold=30, hist_bins=(0, 1001),
                         delfi_q=30, bl_start=None, bl_end=None, gaps=None, window_size=120, wps_min_length=120,
                         wps_max_length=180, wps_quality=30):
        """Every feature of the windows AND the WPS of every base of the contig, in host memory, from ONE launch
        (``window_features_wps``: coverage, length histogram + overflow, DELFI short / long; scores of
        ``[0, chrom_size)``) - BASELINE config 5's "all features fused single pass" as this engine serves it.
        Returns ``(features dict, scores int64)``."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        n = len(ws)
        f = dict(coverage=np.zeros(n, np.int64), hist=np.zeros((n, int(hist_bins[1])), np.uint32), overflow=np.zeros(n, np.int64),
                 short=np.zeros(n, np.int64), long=np.zeros(n, np.int64))
        size = int(chrom_size)
        w = self.result_array(size, np.int64, pinned=not (_NARROW_WIRE and size >= NARROW_WIRE_MIN))
        self.window_features_wps(name, ws, we, w, 0, size, size, quality_threshold, coverage=f["coverage"], hist=f["hist"],
                                 hist_bins=hist_bins, overflow=f["overflow"], delfi_q=delfi_q, bl_start=bl_start, bl_end=bl_end,
                                 gaps=gaps, short=f["short"], long=f["long"], window_size=window_size,
                                 wps_min_length=wps_min_length, wps_max_length=wps_max_length, wps_quality=wps_quality)
        return f, w

    def feature_batch(self, items, quality_threshold=30, min_length=None, max_length=None,
                      intersect_policy="midpoint"):
        """Prepare a multi-contig window-feature batch (``ftk_window_features_batch``): ``items`` is a list of
        dicts ``name, starts, stops[, bl_start, bl_end, gaps]``.  Returns an opaque handle holding the C item
        array (and the arrays it points to) for ``window_features_batch``."""
        n = len(items)
        arr = (L.FeatureItem * n)()
        keep = []
        for i, it in enumerate(items):
            ws, we = _win(it["starts"], L.OPEN_LO), _win(it["stops"], L.OPEN_HI)
            g = L.make_gaps(it.get("gaps"))
            bs = be = None
            if it.get("bl_start") is not None and len(it["bl_start"]):
                bs = np.ascontiguousarray(it["bl_start"], dtype=np.int32)
                be = np.ascontiguousarray(it["bl_end"], dtype=np.int32)
            keep.append((ws, we, bs, be, g))
            arr[i].contig_id = self.contig_id(it["name"])
            arr[i].n_win = len(ws)
            arr[i].w_start = ws.ctypes.data
            arr[i].w_end = we.ctypes.data
            arr[i].bl_start = None if bs is None else bs.ctypes.data
            arr[i].bl_end = None if be is None else be.ctypes.data
            arr[i].n_bl = 0 if bs is None else len(bs)
            arr[i].gaps = C.pointer(g)
        f = L.make_filter(quality_threshold, min_length, max_length, intersect_policy,
                          L.FETCH_BAM_READ1 if items and self.is_bam(items[0]["name"]) else L.FETCH_TABIX)
        return dict(arr=arr, n=n, keep=keep, filter=f, rows=int(sum(len(k[0]) for k in keep)))

    def window_features_batch(self, batch, coverage=None, hist=None, hist_bins=None, overflow=None, delfi_q=30,
                              short=None, long=None):
        """Run a prepared batch; every output is a device pointer (int) or a host numpy array sized for
        ``batch["rows"]`` rows (``hist``: rows x n_bins uint32 with ``hist_bins=(len_lo, n_bins)``), or None."""
        len_lo, n_bins = hist_bins if hist_bins is not None else (0, 0)
        self._check(self.lib.ftk_window_features_batch(
            self.ctx, batch["arr"], batch["n"], C.byref(batch["filter"]), L.ptr(coverage), int(len_lo), int(n_bins),
            L.ptr(hist), L.ptr(overflow), int(delfi_q), L.ptr(short), L.ptr(long)))

    def wps_window_features(self, name: str, chrom_size: int, win_start: int, win_len: int, n_win: int,
                            window_size=120, min_length=120, max_length=180, quality_threshold=30, wps_out=None,
                            feat_quality=30, feat_min_length=None, feat_max_length=None, coverage=None, hist=None,
                            hist_bins=None, overflow=None, delfi_q=30, bl_start=None, bl_end=None, gaps=None,
                            short=None, long=None):
        """Whole-contig WPS and the window features of the regular tiling ``[win_start + k*win_len, ...)`` in ONE
        pass (``ftk_wps_window_features``).  Outputs: numpy arrays or device pointers; returns ``wps_out``
        (allocated on the host when None)."""
        if wps_out is None:
            wps_out = np.zeros(int(chrom_size), np.int64)
        f = self._filter(name, feat_quality, feat_min_length, feat_max_length, "midpoint")
        len_lo, n_bins = hist_bins if hist_bins is not None else (0, 0)
        bs = be = None
        n_bl = 0
        if bl_start is not None and len(bl_start):
            bs = np.ascontiguousarray(bl_start, dtype=np.int32)
            be = np.ascontiguousarray(bl_end, dtype=np.int32)
            n_bl = len(bs)
        g = L.make_gaps(gaps)
        self._check(self.lib.ftk_wps_window_features(
            self.ctx, self.contig_id(name), 0, int(chrom_size), int(chrom_size), int(window_size), int(min_length),
            int(max_length), int(quality_threshold), L.ptr(wps_out), int(win_start), int(win_len), int(n_win),
            C.byref(f), L.ptr(coverage), int(len_lo), int(n_bins), L.ptr(hist), L.ptr(overflow), int(delfi_q),
            L.ptr(bs), L.ptr(be), n_bl, C.byref(g), L.ptr(short), L.ptr(long)))
        return wps_out

    def wps_batch(self, names, starts, stops, chrom_sizes, out_offsets, out, window_size=120, min_length=120,
                  max_length=180, quality_threshold=30):
        """WPS of several (contig, interval) pairs in one launch into the device buffer ``out``."""
        ids = np.array([self.contig_id(n) for n in names], np.int32)
        s = np.ascontiguousarray(starts, dtype=np.int64)
        e = np.ascontiguousarray(stops, dtype=np.int64)
        cs = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
        oo = np.ascontiguousarray(out_offsets, dtype=np.int64)
        self._check(self.lib.ftk_wps_batch(self.ctx, L.ptr(ids), L.ptr(s), L.ptr(e), L.ptr(cs), L.ptr(oo), len(ids),
                                           int(window_size), int(min_length), int(max_length), int(quality_threshold),
                                           L.ptr(out)))

    def frag_lengths(self, name: str, start, stop, quality_threshold=30, min_length=None, max_length=None,
                     intersect_policy="midpoint"):
        """Lengths of one window's passing fragments in file order."""
        ws = L.OPEN_LO if start is None else int(start)
        we = L.OPEN_HI if stop is None else int(stop)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        n = C.c_int64()
        cid = self.contig_id(name)
        cap = 1 << 16
        while True:
            out = np.zeros(cap, np.int32)
            self._check(self.lib.ftk_frag_lengths(self.ctx, cid, ws, we, C.byref(f), L.ptr(out), cap, C.byref(n)))
            if n.value <= cap:
                return out[: n.value].copy()
            cap = int(n.value)

    def frag_select(self, name: str, start, stop, quality_threshold=30, min_length=None, max_length=None,
                    intersect_policy="midpoint"):
        """(start, end, mapq, strand) of one window's passing fragments in file order."""
        ws = L.OPEN_LO if start is None else int(start)
        we = L.OPEN_HI if stop is None else int(stop)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        n = C.c_int64()
        cid = self.contig_id(name)
        cap = 1 << 16
        while True:
            s = np.zeros(cap, np.int32)
            e = np.zeros(cap, np.int32)
            q = np.zeros(cap, np.uint8)
            st = np.zeros(cap, np.uint8)
            self._check(self.lib.ftk_frag_select(self.ctx, cid, ws, we, C.byref(f), L.ptr(s), L.ptr(e), L.ptr(q),
                                                 L.ptr(st), cap, C.byref(n)))
            if n.value <= cap:
                k = n.value
                return s[:k].copy(), e[:k].copy(), q[:k].copy(), st[:k].copy()
            cap = int(n.value)

    # -- export: columns -> rows -> BGZF on the device (csrc/ftk_fragtext.hip) ----------------------------------
    @staticmethod
    def _export_args(print_name, quality_threshold, min_length, max_length, layout):
        if layout not in L.LAYOUT:
            raise ValueError(f"layout must be one of {sorted(L.LAYOUT)}, not {layout!r}")
        f = L.make_filter(quality_threshold, min_length, max_length)
        return str(print_name).encode(), f.mapq_min, f.min_len, f.max_len, L.LAYOUT[layout]

    @staticmethod
    def _mask_struct(mask):
        """``(ftk_region_mask or None, the arrays it points into)`` of a ``RegionMask`` / ``None``."""
        if mask is None:
            return None, ()
        m = L.RegionMask()
        keep = []
        for tag, pair in (("wl", mask.whitelist), ("bl", mask.blacklist)):
            if pair is None:
                setattr(m, "n_" + tag, -1 if tag == "wl" else 0)
                continue
            s = np.ascontiguousarray(pair[0], dtype=np.int32)
            e = np.ascontiguousarray(pair[1], dtype=np.int32)
            if s.ndim != 1 or s.shape != e.shape:
                raise ValueError("a mask's starts and ends must be two 1-d arrays of one length")
            keep += [s, e]
            setattr(m, tag + "_start", s.ctypes.data)
            setattr(m, tag + "_end", e.ctypes.data)
            setattr(m, "n_" + tag, len(s))
        m.policy = mask.policy if isinstance(mask.policy, int) else L.POLICY[_checked_policy(mask.policy)]
        return m, keep

    def mask_lds_intervals(self) -> int:
        """Intervals of one mask a workgroup of the mask kernel stages in LDS (``kMaskLdsIntervals``); a tile whose
        rows can touch more searches the global arrays."""
        return int(self.lib.ftk_mask_lds_intervals())

    def mask_keep(self, name: str, mask):
        """``(bool[n], kept)``: which rows of resident contig ``name`` the region mask keeps (in the whitelist, if
        any, and not in the blacklist, if any) - the mask kernel alone, without the MAPQ / length rule
        (``ftk_frags_mask_keep``)."""
        n = self.info(name)[0]
        out = np.zeros(n, np.uint8)
        kept = C.c_int64()
        m, alive = self._mask_struct(mask if mask is not None else RegionMask())
        self._check(self.lib.ftk_frags_mask_keep(self.ctx, self.contig_id(name), C.byref(m), L.ptr(out), C.byref(kept)))
        del alive
        return out.astype(bool), int(kept.value)

    def format_rows(self, name: str, print_name: str, quality_threshold=30, min_length=None, max_length=None,
                    layout="frag", mask=None):
        """``(text bytes, rows)``: the kept fragments of resident contig ``name`` as rows that carry ``print_name``,
        formatted on the device (``ftk_frags_format_rows``; with a ``RegionMask``: ``ftk_frags_format_rows_masked``)."""
        args = self._export_args(print_name, quality_threshold, min_length, max_length, layout)
        out, n, rows = C.c_void_p(), C.c_int64(), C.c_int64()
        if mask is None:
            self._check(self.lib.ftk_frags_format_rows(self.ctx, self.contig_id(name), *args, C.byref(out), C.byref(n),
                                                       C.byref(rows)))
        else:
            m, alive = self._mask_struct(mask)
            self._check(self.lib.ftk_frags_format_rows_masked(self.ctx, self.contig_id(name), *args, C.byref(out),
                                                              C.byref(n), C.byref(rows), C.byref(m)))
            del alive
        try:
            return C.string_at(out.value, n.value), int(rows.value)
        finally:
            self.lib.ftk_buffer_free(out.value)

    def bgzf_deflate(self, data: bytes, write_eof: bool = True):
        """``(BGZF image bytes, block offsets int64[n_blocks + 1])`` of ``data``, deflated on the device
        (``ftk_bgzf_deflate_device``)."""
        n = len(data)
        n_blocks = -(-n // 0xFF00)
        cap = n + 31 * n_blocks + 28  # the stored bound: 18 header + 5 stored-block header + 8 trailer per member
        out = np.empty(max(cap, 1), np.uint8)
        offs = np.zeros(n_blocks + 1, np.int64)
        got = C.c_int64()
        src = np.frombuffer(data, np.uint8) if n else None
        self._check(self.lib.ftk_bgzf_deflate_device(self.ctx, L.ptr(src), n, L.ptr(out), cap, C.byref(got), L.ptr(offs),
                                                     int(bool(write_eof))))
        return out[: got.value].tobytes(), offs

    def write_contig(self, name: str, print_name: str, path: str, quality_threshold=30, min_length=None,
                     max_length=None, layout="frag", append=False, write_eof=False, deflate_on_host=False,
                     mask=None) -> dict:
        """Append the kept rows of resident contig ``name`` to ``path`` as BGZF members built on the device
        (``ftk_frags_write``).  Returns ``rows``, ``text_bytes``, ``first_off`` / ``end_off`` (file offsets), the
        tabix inputs ``linear`` (uint64 virtual offsets per 16 kb window) and ``runs`` = ``(bin int32[], begin
        uint64[], end uint64[])``, and ``stage_ms`` (format, deflate + CRC, compaction, copy, write).  ``mask``: a
        ``RegionMask`` added to the keep rule (``ftk_frags_write_masked``; its kernel counts into ``stage_ms[0]``)."""
        args = self._export_args(print_name, quality_threshold, min_length, max_length, layout)
        res = L.ExportResult()
        tail = (str(path).encode(), int(bool(append)), int(bool(write_eof)), int(bool(deflate_on_host)), C.byref(res))
        if mask is None:
            self._check(self.lib.ftk_frags_write(self.ctx, self.contig_id(name), *args, *tail))
        else:
            m, alive = self._mask_struct(mask)
            self._check(self.lib.ftk_frags_write_masked(self.ctx, self.contig_id(name), *args, *tail, C.byref(m)))
            del alive

        def take(p, n, dtype):
            if not p or n == 0:
                return np.zeros(0, dtype)
            try:
                return np.frombuffer(C.string_at(p, n * np.dtype(dtype).itemsize), dtype).copy()
            finally:
                self.lib.ftk_buffer_free(p)
        nr = int(res.n_runs)
        return dict(rows=int(res.n_rows), text_bytes=int(res.text_bytes), first_off=int(res.first_off),
                    end_off=int(res.end_off), linear=take(res.linear, int(res.n_linear), np.uint64),
                    runs=(take(res.run_bin, nr, np.int32), take(res.run_beg, nr, np.uint64), take(res.run_end, nr, np.uint64)),
                    stage_ms=[float(v) for v in res.stage_ms])

    def wps(self, name: str, start: int, stop: int, chrom_size: int, window_size=120, min_length=120,
            max_length=180, quality_threshold=30, out=None):
        """a7: WPS per base of [start, stop) (frag/_wps.py:156-188)."""
        n_pos = max(int(stop) - int(start), 0)
        if out is None:  # (every element is written by the call)
            res = self.result_array(n_pos, np.int64, pinned=not (_NARROW_WIRE and n_pos >= NARROW_WIRE_MIN))
        else:
            res = out
        self._check(self.lib.ftk_wps(self.ctx, self.contig_id(name), int(start), int(stop), int(chrom_size),
                                     int(window_size), int(min_length), int(max_length), int(quality_threshold),
                                     L.ptr(res)))
        return res

    def wps_async(self, name: str, start: int, stop: int, chrom_size: int, window_size=120, min_length=120,
                  max_length=180, quality_threshold=30):
        """``wps`` with the copy-back off the caller's path (``ftk_wps_async``): returns ``(scores, token)``
        at once; ``scores`` (page-locked) is valid after ``result_wait(token)``.  Loading and scoring the next
        contig overlaps the copy of this one; two results can be in flight."""
        n_pos = max(int(stop) - int(start), 0)
        res = self.result_array(n_pos, np.int64)
        tok = C.c_int(-1)
        self._check(self.lib.ftk_wps_async(self.ctx, self.contig_id(name), int(start), int(stop), int(chrom_size),
                                           int(window_size), int(min_length), int(max_length), int(quality_threshold),
                                           L.ptr(res), C.byref(tok)))
        if tok.value >= 0:
            # tokens count up; two results can be in flight (token & 1 is the library's buffer): an array registered
            # under an older token is complete - the library waited for that buffer's copy before reusing it
            self._pending[int(tok.value)] = res
            for old in [t for t in self._pending if t < tok.value - 1]:
                del self._pending[old]
        return res, int(tok.value)

    def result_wait(self, token: int):
        self._check(self.lib.ftk_result_wait(self.ctx, int(token)))
        self._pending.pop(int(token), None)

    def wps_intervals(self, name: str, starts, stops, chrom_size: int, window_size=120, min_length=120,
                      max_length=180, quality_threshold=30):
        """a8: WPS of many intervals of one contig in one launch; returns
        (scores, offsets) with interval i at scores[offsets[i]:offsets[i+1]]."""
        s = np.ascontiguousarray(starts, dtype=np.int64)
        e = np.ascontiguousarray(stops, dtype=np.int64)
        lens = np.maximum(e - s, 0)
        offs = np.zeros(len(s) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        out = self.result_array(int(offs[-1]), np.int64)  # the intervals tile it: every element is written
        if len(s) and offs[-1] > 0:
            self._check(self.lib.ftk_wps_intervals(self.ctx, self.contig_id(name), L.ptr(s), L.ptr(e), len(s),
                                                   L.ptr(np.ascontiguousarray(offs[:-1])), int(chrom_size),
                                                   int(window_size), int(min_length), int(max_length),
                                                   int(quality_threshold), L.ptr(out)))
        return out, offs

    def cleavage_intervals(self, name: str, starts, stops, min_length=None, max_length=None, quality_threshold=30):
        """Cleavage proportion (percent) per base of many intervals of one contig in one launch
        (frag/_cleavage_profile.py:33-90,204-216); returns (proportions f64, offsets)."""
        s = np.ascontiguousarray(starts, dtype=np.int64)
        e = np.ascontiguousarray(stops, dtype=np.int64)
        offs = np.zeros(len(s) + 1, np.int64)
        np.cumsum(np.maximum(e - s, 0), out=offs[1:])
        out = self.result_array(int(offs[-1]), np.float64)  # the intervals tile it: every element is written
        if len(s) and offs[-1] > 0:
            self._check(self.lib.ftk_cleavage_intervals(
                self.ctx, self.contig_id(name), L.ptr(s), L.ptr(e), len(s), L.ptr(np.ascontiguousarray(offs[:-1])),
                L.LEN_OPEN if min_length is None else max(int(min_length), 0),
                L.LEN_OPEN if max_length is None else int(max_length), int(quality_threshold), L.ptr(out)))
        return out, offs

    def cleavage(self, name: str, start: int, stop: int, min_length=None, max_length=None, quality_threshold=30, out=None):
        """Cleavage proportion (percent) per base of ONE interval (``ftk_cleavage``: the tiles are numbered by the grid, no
        descriptor arrays); ``out``: a float64 host array or device tensor / address of ``stop - start`` elements."""
        n = max(int(stop) - int(start), 0)
        res = self.result_array(n, np.float64) if out is None else out
        if n:
            self._check(self.lib.ftk_cleavage(self.ctx, self.contig_id(name), int(start), int(stop),
                                              L.LEN_OPEN if min_length is None else max(int(min_length), 0),
                                              L.LEN_OPEN if max_length is None else int(max_length), int(quality_threshold),
                                              L.ptr(res)))
        return res

    # -- per-base depth track (csrc/ftk_depth.hip) ------------------------------------
    @staticmethod
    def _depth_args(start, stop, min_length, max_length, quality_threshold):
        f = L.make_filter(quality_threshold, min_length, max_length)
        return int(start), int(stop), f.min_len, f.max_len, f.mapq_min

    def depth(self, name: str, start: int, stop: int, quality_threshold=30, min_length=None, max_length=None, out=None):
        """Kept fragments covering each base of ``[start, stop)`` of resident contig ``name`` (``ftk_depth``): int32,
        one value per base; ``out``: an int32 host array or device tensor / address of ``stop - start`` elements."""
        n = max(int(stop) - int(start), 0)
        res = self.result_array(n, np.int32) if out is None else out
        dst = res if n or out is not None else np.empty(1, np.int32)  # (an empty region still has its arguments checked)
        self._check(self.lib.ftk_depth(self.ctx, self.contig_id(name),
                                       *self._depth_args(start, stop, min_length, max_length, quality_threshold), L.ptr(dst)))
        return res

    def depth_runs(self, name: str, start: int, stop: int, quality_threshold=30, min_length=None, max_length=None,
                   include_zero=False):
        """``(run_start, run_end, run_depth)`` int32: the maximal intervals of constant depth inside ``[start, stop)``,
        run-length encoded on the device (``ftk_depth_runs``); runs of depth 0 only with ``include_zero``."""
        ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        n = C.c_int64()
        self._check(self.lib.ftk_depth_runs(self.ctx, self.contig_id(name),
                                            *self._depth_args(start, stop, min_length, max_length, quality_threshold),
                                            int(bool(include_zero)), *[C.byref(p) for p in ptrs], C.byref(n)))
        cols = []
        for p in ptrs:
            try:
                cols.append(np.frombuffer(C.string_at(p.value, n.value * 4), np.int32).copy() if n.value else np.zeros(0, np.int32))
            finally:
                if p.value:
                    self.lib.ftk_buffer_free(p.value)
        return tuple(cols)

    # -- fragment length x GC tables (csrc/ftk_gcbias.hip) -------------------------------
    def frag_gc(self, name: str, rid: int, quality_threshold=30, min_length=None, max_length=None, out=None) -> np.ndarray:
        """G + C bases of every fragment of resident contig ``name`` in reference image ``rid`` (``ftk_frag_gc``;
        the image needs its layout): int16, one value per fragment in resident order, ``-1`` for a fragment that
        fails the MAPQ / length rule, leaves the contig, is longer than 1000 bases or spans an N.  ``out``: an int16
        host array or device tensor of as many elements as the contig has fragments."""
        n = self.info(name)[0]
        res = self.result_array(n, np.int16) if out is None else out
        dst = res if n or out is not None else np.empty(1, np.int16)
        f = L.make_filter(quality_threshold, min_length, max_length)
        self._check(self.lib.ftk_frag_gc(self.ctx, self.contig_id(name), int(rid), f.min_len, f.max_len, f.mapq_min, L.ptr(dst)))
        return res

    def frag_gc_table(self, name: str, rid: int, len_lo: int, len_hi: int, quality_threshold=30):
        """``(table, n_skipped)``: the observed length x GC table of resident contig ``name`` (``ftk_frag_gc_table``) -
        ``table[L - len_lo, g]`` = fragments of length ``L`` with ``g`` G + C bases, int64 of shape
        ``(len_hi - len_lo + 1, len_hi + 1)`` - and the fragments of those lengths whose GC count is undefined."""
        shape = (max(int(len_hi) - int(len_lo) + 1, 1), max(int(len_hi) + 1, 1))
        table = np.empty(shape, np.int64)
        skipped = C.c_int64()
        self._check(self.lib.ftk_frag_gc_table(self.ctx, self.contig_id(name), int(rid), int(len_lo), int(len_hi),
                                               int(quality_threshold), L.ptr(table), C.byref(skipped)))
        return table, int(skipped.value)

    def ref_gc_table(self, rid: int, pos_lo: int, pos_hi: int, len_lo: int, len_hi: int, stride: int = 1) -> np.ndarray:
        """The expected length x GC table of reference image ``rid`` (``ftk_ref_gc_table``): ``table[L - len_lo, g]`` =
        positions ``p`` of ``[pos_lo, pos_hi)`` with ``p % stride == 0`` whose window ``[p, p + L)`` lies inside the
        contig, holds no N and has ``g`` G + C bases."""
        shape = (max(int(len_hi) - int(len_lo) + 1, 1), max(int(len_hi) + 1, 1))
        table = np.empty(shape, np.int64)
        self._check(self.lib.ftk_ref_gc_table(self.ctx, int(rid), int(pos_lo), int(pos_hi), int(len_lo), int(len_hi),
                                              int(stride), L.ptr(table)))
        return table

    # -- end context: base and base-pair profiles around fragment ends (csrc/ftk_endcontext.hip) ----
    def end_context_lds_classes(self, half_width: int) -> int:
        """Length classes one workgroup of the end-context kernel keeps in LDS at ``half_width``
        (``ftk_end_context_lds_classes``); a call with more classes spreads them over further rows of its grid."""
        return int(self.lib.ftk_end_context_lds_classes(int(half_width)))

    def end_context(self, name: str, rid: int, half_width: int, length_edges, quality_threshold=30, anchor="ends", out=None):
        """``(table, n_kept)`` of resident contig ``name`` against reference image ``rid`` (``ftk_end_context``; the rule
        is in ``include/ftk.h``, "end context"): ``table[c, k, o + half_width, 5 * x + y]`` = kept fragments of length
        class ``c`` (``length_edges[c] <= L < length_edges[c + 1]``) whose reading of kind ``k`` (0: the U end on the +
        strand, 1: the D end on the - strand; ``anchor="centre"``: the same readings around the fragment's centre) has
        base ``x`` at offset ``o`` and base ``y`` at ``o + 1`` (A C G T N = 0 .. 4), int64 of shape
        ``(n_classes, 2, 2 * half_width, 25)``; ``n_kept[c]``: the kept fragments of class ``c``, int64.  ``out``: an
        int64 host array or device tensor of that many elements to write the table into (returned as passed)."""
        if anchor not in L.CONTEXT_ANCHOR:
            raise ValueError(f"invalid anchor ({anchor!r}): 'ends' or 'centre'")
        edges = np.asarray(length_edges, dtype=np.int64).ravel()
        if len(edges) < 2 or edges.min() < 1 or edges.max() > 1 << 30:
            raise ValueError("length_edges: at least two values within [1, 2**30]")
        edges32 = np.ascontiguousarray(edges, dtype=np.int32)
        n_classes = len(edges) - 1
        shape = (n_classes, 2, 2 * max(int(half_width), 0), 25)
        table = np.empty(shape, np.int64) if out is None else out
        n_kept = np.empty(n_classes, np.int64)
        self._check(self.lib.ftk_end_context(self.ctx, self.contig_id(name), int(rid), int(half_width), L.ptr(edges32), n_classes,
                                             int(quality_threshold), L.CONTEXT_ANCHOR[anchor], L.ptr(table), L.ptr(n_kept)))
        return table, n_kept

    def ref_context(self, rid: int, pos_lo: int, pos_hi: int) -> np.ndarray:
        """The background of ``end_context`` (``ftk_ref_context``): int64 ``[25]``, cell ``5 * x + y`` = positions ``p`` of
        ``[pos_lo, pos_hi)`` inside the contig with base ``x`` at ``p`` and base ``y`` at ``p + 1`` (A C G T N = 0 .. 4; the
        base behind the contig's end is N)."""
        out = np.empty(25, np.int64)
        self._check(self.lib.ftk_ref_context(self.ctx, int(rid), int(pos_lo), int(pos_hi), L.ptr(out)))
        return out

    # -- motif x length: end-motif counts per fragment length (csrc/ftk_motiflen.hip) ----
    def motif_length_lds_rows(self, k: int) -> int:
        """Length rows one workgroup of the motif x length kernel keeps in LDS at motif length ``k``
        (``ftk_motif_length_lds_rows``; 0 for ``k`` outside 1 .. 4); a call with more rows walks them in bands of that many."""
        return int(self.lib.ftk_motif_length_lds_rows(int(k)))

    def motif_length_table(self, name: str, rid: int, k: int, shift: int, len_lo: int, len_hi: int, len_bin: int = 1,
                           quality_threshold=30):
        """``(table, n_kept)`` of resident contig ``name`` against reference image ``rid`` (``ftk_motif_length_table``; the
        rule is in ``include/ftk.h``, "motif x length"): ``table[kind, r, code]`` = kept fragments (``mapq >=
        quality_threshold``, ``len_lo <= L <= len_hi``) of length row ``r = (L - len_lo) // len_bin`` whose reading of ``kind``
        (0: ``base(s + shift + i)``, the U end on the + strand; 1: ``comp(base(e - 1 - shift - i))``, the D end on the -
        strand; ``i = 0 .. k-1``) has that code - first base most significant, ``A C G T`` = 0 .. 3, column ``4 ** k`` for a
        reading with an N or off the contig - int64 of shape ``(2, n_rows, 4 ** k + 1)``; ``n_kept[r]``: the kept fragments
        of row ``r``, int64.  Every row of either kind sums to ``n_kept[r]``."""
        k, lo, hi, b = int(k), int(len_lo), int(len_hi), int(len_bin)
        n_rows = (hi - lo) // b + 1 if b >= 1 and hi >= lo else 1
        if not 1 <= n_rows <= L.MOTIFLEN_MAX_ROWS or not 1 <= k <= L.MOTIFLEN_MAX_K:
            shape = (2, 1, 1)  # (the call refuses these arguments and writes nothing)
        else:
            shape = (2, n_rows, 4 ** k + 1)
        table = np.empty(shape, np.int64)
        n_kept = np.empty(shape[1], np.int64)
        self._check(self.lib.ftk_motif_length_table(self.ctx, self.contig_id(name), int(rid), k, int(shift), lo, hi, b,
                                                    int(quality_threshold), L.ptr(table), L.ptr(n_kept)))
        return table, n_kept

    # -- co-fragmentation: pairwise KS numerators of length histograms (csrc/ftk_cofrag.hip) ----
    def hist_ks_shape(self):
        """``(T, chunk)`` of the tiled pair kernel (``ftk_hist_ks_shape``): the edge of the pair tile one workgroup
        computes and the lengths it stages per LDS chunk."""
        t, c = C.c_int32(), C.c_int32()
        self._check(self.lib.ftk_hist_ks_shape(C.byref(t), C.byref(c)))
        return int(t.value), int(c.value)

    def hist_ks(self, hist, out=None, at=True):
        """``(K, at, n)`` of the histogram rows ``hist`` (``ftk_hist_ks``; the rule is in ``include/ftk.h``,
        "co-fragmentation"): ``hist`` is a uint32 host array or device tensor of shape ``(N, n_bins)``;
        ``K[i, j] = max over l of |C(i, l) n(j) - C(j, l) n(i)|`` (int64, ``N x N``, symmetric: the two-sample KS statistic
        is ``K / (n(i) n(j))``), ``at[i, j]`` the smallest ``l`` that attains it (int32; ``None`` with ``at=False``) and
        ``n`` the row sums (int64), each of which must be below 2**31.  ``out``: an int64 host array or device tensor of
        ``N * N`` elements to write K into (returned as passed); ``at`` may likewise be an int32 array or tensor."""
        if isinstance(hist, np.ndarray) or not hasattr(hist, "data_ptr"):
            hist = np.ascontiguousarray(hist, dtype=np.uint32)
        if len(hist.shape) != 2:
            raise ValueError("hist: rows of cells, shape (N, n_bins)")
        n_rows, n_bins = int(hist.shape[0]), int(hist.shape[1])
        k = np.empty((n_rows, n_rows), np.int64) if out is None else out
        if at is True:
            at = np.empty((n_rows, n_rows), np.int32)
        elif at is False:
            at = None
        n = np.empty(n_rows, np.int64)
        self._check(self.lib.ftk_hist_ks(self.ctx, L.ptr(hist), n_rows, n_bins, L.ptr(k), L.ptr(at), L.ptr(n)))
        return k, at, n

    def cofrag(self, name: str, starts, stops, len_lo: int, n_bins: int, quality_threshold=30, min_length=None, max_length=None,
               intersect_policy="midpoint", out=None, at=True):
        """``(K, at, n, overflow)`` of the windows of resident contig ``name`` (``ftk_cofrag``): what ``hist_ks`` gives on
        the rows of ``fraglen_hist`` with the same arguments, and that call's overflow column - the histograms are
        built and compared on the device and never leave it.  ``out`` / ``at`` as in ``hist_ks``."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        n_win = len(ws)
        k = np.empty((n_win, n_win), np.int64) if out is None else out
        if at is True:
            at = np.empty((n_win, n_win), np.int32)
        elif at is False:
            at = None
        n, over = np.empty(n_win, np.int64), np.empty(n_win, np.int64)
        self._check(self.lib.ftk_cofrag(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), n_win, C.byref(f), int(len_lo),
                                        int(n_bins), L.ptr(k), L.ptr(at), L.ptr(n), L.ptr(over)))
        return k, at, n, over

    # -- per-fragment weights and their sums per window (csrc/ftk_weights.hip) ----------
    def set_weights(self, name: str, w):
        """Attach one weight per fragment to resident contig ``name`` (``ftk_frags_set_weights``): uint32 in units of
        2^-16 (``_lib.WEIGHT_ONE`` = 1.0), in resident order; a host array or a uint32 / int32 device tensor of as many
        elements as the contig has fragments.  The column stays on the device until the contig is released or loaded
        again."""
        if not hasattr(w, "data_ptr"):
            w = np.ascontiguousarray(w, dtype=np.uint32)
        n = int(w.numel()) if hasattr(w, "numel") else len(w)
        self._check(self.lib.ftk_frags_set_weights(self.ctx, self.contig_id(name), L.ptr(w), n))

    def weights(self, name: str, out=None) -> np.ndarray:
        """The weight column of resident contig ``name`` (``ftk_frags_weights``): uint32, one per fragment.  ``out``: a
        host array or device tensor of as many 4-byte elements as the contig has fragments.  ``FtkError`` when the
        contig has no column."""
        n = self.info(name)[0]
        res = np.empty(n, np.uint32) if out is None else out
        dst = res if n or out is not None else np.empty(1, np.uint32)
        self._check(self.lib.ftk_frags_weights(self.ctx, self.contig_id(name), L.ptr(dst)))
        return res

    def set_gc_weights(self, name: str, rid: int, len_lo: int, len_hi: int, table, quality_threshold=30) -> int:
        """Weights from a length x GC table (``ftk_frags_set_gc_weights``): fragment ``i`` of resident contig ``name``
        gets ``table[L - len_lo, g]`` when ``mapq >= quality_threshold``, its length ``L`` lies in ``[len_lo, len_hi]``
        and its span has a GC count ``g`` in reference image ``rid`` (as ``frag_gc``), else 0.  ``table``: uint32 of
        shape ``(len_hi - len_lo + 1, len_hi + 1)``, e.g. ``utils.gc_weights(bias)``.  Returns ``n_zero``: fragments
        that pass the MAPQ / length rule and got weight 0.  Replaces a column already attached."""
        table = np.ascontiguousarray(table, dtype=np.uint32)
        if table.shape != (int(len_hi) - int(len_lo) + 1, int(len_hi) + 1):
            raise ValueError(f"table should have shape {(int(len_hi) - int(len_lo) + 1, int(len_hi) + 1)}, not {table.shape}")
        n_zero = C.c_int64()
        self._check(self.lib.ftk_frags_set_gc_weights(self.ctx, self.contig_id(name), int(rid), int(len_lo), int(len_hi),
                                                      int(quality_threshold), L.ptr(table), C.byref(n_zero)))
        return int(n_zero.value)

    def weighted_window_sums(self, name: str, starts: Sequence, stops: Sequence, quality_threshold=30, min_length=None,
                             max_length=None, intersect_policy="midpoint"):
        """``(sums, n_weighted)`` int64 per window (``ftk_weighted_window_sums``): the sum of the weights, in units of
        2^-16, of the fragments ``window_counts`` counts for the window under the same arguments, and how many of
        them have a weight above 0."""
        ws, we = _win(starts, L.OPEN_LO), _win(stops, L.OPEN_HI)
        f = self._filter(name, quality_threshold, min_length, max_length, intersect_policy)
        sums = np.zeros(len(ws), np.int64)
        n_weighted = np.zeros(len(ws), np.int64)
        self._check(self.lib.ftk_weighted_window_sums(self.ctx, self.contig_id(name), L.ptr(ws), L.ptr(we), len(ws),
                                                      C.byref(f), L.ptr(sums), L.ptr(n_weighted)))
        return sums, n_weighted

    # -- site-aggregated midpoint profiles (csrc/ftk_siteprofile.hip) --------------------
    @staticmethod
    def _site_inputs(centres, flip, groups):
        """The sites of a site call as its leading arguments, ``(centre, flip, group, n_sites)`` - contiguous int32 /
        uint8 / int32 behind the pointers, NULL for an array that was not given or has no site - and ``out``, which
        gives an output array's pointer: for one without an element that of a spare cell (the call fails or writes
        nothing)."""
        c = np.ascontiguousarray(centres, dtype=np.int32)
        fl = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8)
        gr = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        for other, what in ((fl, "flip"), (gr, "groups")):
            if other is not None and other.shape != c.shape:
                raise ValueError(f"{what} should have one entry per site")
        keep = np.empty(1, np.int64)
        sites = tuple(L.ptr(a) if a is not None and len(c) else None for a in (c, fl, gr)) + (len(c),)
        return sites, lambda a, _alive=(c, fl, gr): L.ptr(a if a.size else keep)  # (`out` keeps the arrays behind `sites`)

    def site_profile(self, name: str, centres: Sequence, flip=None, groups=None, n_groups: int = 1, half_width: int = 1000,
                     bin_size: int = 1, quality_threshold=30, min_length=None, max_length=None, weighted: bool = False):
        """``(sums, counts)`` int64 of shape ``(n_groups, 2 * half_width // bin_size)`` (``ftk_site_profile``): the
        midpoint profile of resident contig ``name`` around the sites ``centres``, aggregated per group.  A fragment with
        ``mapq >= quality_threshold`` and a length in ``[min_length, max_length]`` whose midpoint ``(start + end) >> 1``
        lies ``d`` in ``[-half_width, half_width)`` from site ``i`` adds 1 to ``counts[groups[i], k]`` and its weight,
        in units of 2^-16, to ``sums[groups[i], k]``, ``k = (d + half_width) // bin_size`` - counted from the other end
        where ``flip[i]`` is set (a site on the - strand).  ``weighted=False``: every fragment weighs ``_lib.WEIGHT_ONE``
        and the contig needs no weight column.  ``flip=None``: no site is flipped; ``groups=None``: all in group 0.  Sites
        come in any order and are independent: one listed twice counts twice."""
        sites, out = self._site_inputs(centres, flip, groups)
        n_bins = 2 * int(half_width) // max(int(bin_size), 1)
        shape = (max(int(n_groups), 0), min(max(n_bins, 0), 4096))
        sums, counts = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self._check(self.lib.ftk_site_profile(
            self.ctx, self.contig_id(name), *sites, int(n_groups), int(half_width), int(bin_size),
            int(quality_threshold), -1 if min_length is None else int(min_length), -1 if max_length is None else int(max_length),
            int(bool(weighted)), out(sums), out(counts)))
        return sums, counts

    # -- fragment length x offset maps around sites (csrc/ftk_vplot.hip) ----------------
    def site_vplot(self, name: str, centres: Sequence, flip=None, groups=None, n_groups: int = 1, half_width: int = 500,
                   bin_size: int = 5, len_lo: int = 50, len_hi: int = 349, len_bin: int = 5, mapq_min=30, weighted: bool = False):
        """``(sums, counts)`` int64 of shape ``(n_groups, n_rows, n_bins)`` (``ftk_site_vplot``), ``n_rows = (len_hi -
        len_lo + 1) // len_bin`` and ``n_bins = 2 * half_width // bin_size``: the V-plot of resident contig ``name``
        around the sites ``centres``, aggregated per group.  A fragment with ``mapq >= mapq_min`` and a length ``L`` in
        ``[len_lo, len_hi]`` whose midpoint ``(start + end) >> 1`` lies ``d`` in ``[-half_width, half_width)`` from site
        ``i`` adds 1 to ``counts[groups[i], r, k]`` and its weight, in units of 2^-16, to ``sums[groups[i], r, k]``, ``r
        = (L - len_lo) // len_bin`` and ``k = (d + half_width) // bin_size`` - ``k`` counted from the other end where
        ``flip[i]`` is set; the length axis is never reversed.  ``weighted``, ``flip``, ``groups`` and the sites' order:
        as in ``site_profile``."""
        sites, out = self._site_inputs(centres, flip, groups)
        n_bins = 2 * int(half_width) // max(int(bin_size), 1)
        n_rows = (int(len_hi) - int(len_lo) + 1) // max(int(len_bin), 1)
        shape = [max(int(n_groups), 0), min(max(n_rows, 0), 4096), min(max(n_bins, 0), 4096)]
        if shape[0] * shape[1] * shape[2] > 1 << 28:  # (the call fails and writes nothing)
            shape[0] = 0
        sums, counts = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self._check(self.lib.ftk_site_vplot(
            self.ctx, self.contig_id(name), *sites, int(n_groups), int(half_width), int(bin_size),
            int(len_lo), int(len_hi), int(len_bin), int(mapq_min), int(bool(weighted)), out(sums), out(counts)))
        return sums, counts

    # -- fragment-end profiles and OCF window sums around sites (csrc/ftk_siteends.hip) --
    def site_ends(self, name: str, centres: Sequence, flip=None, groups=None, n_groups: int = 1, half_width: int = 1000,
                  bin_size: int = 1, quality_threshold=30, min_length=None, max_length=None, weighted: bool = False, peak=None,
                  flank: int = 10):
        """``(sums, counts)`` int64 of shape ``(n_groups, 2, n_bins)`` (``ftk_site_ends``), ``n_bins = 2 * half_width //
        bin_size``: where the fragments of resident contig ``name`` END around the sites ``centres``, aggregated per group.
        A fragment ``[start, end)`` with ``mapq >= quality_threshold`` and a length in ``[min_length, max_length]`` has its
        U end on base ``start`` and its D end on base ``end - 1``; an end ``d`` in ``[-half_width, half_width)`` from site
        ``i`` adds 1 to ``counts[groups[i], t, k]`` and the fragment's weight, in units of 2^-16, to ``sums[groups[i], t,
        k]``, ``t`` = 0 (U) or 1 (D) and ``k = (d + half_width) // bin_size`` - where ``flip[i]`` is set, ``k`` is counted
        from the other end and the tracks change places.  With ``peak`` given, ``(sums, counts, site_sums, site_counts)``:
        the last two int64 of shape ``(n_sites, 4)`` in the order of ``centres`` - ``left_up, left_down, right_up,
        right_down``, the U and D ends with ``d`` in ``[-peak - flank, -peak + flank]`` and in ``[peak - flank, peak +
        flank]``, in genome orientation (``flip`` is not applied; ``0 <= flank < peak``, ``peak + flank < half_width``).
        ``OCF = (left_down - left_up) + (right_up - right_down)``.  ``weighted``, ``flip``, ``groups`` and the sites'
        order: as in ``site_profile``."""
        sites, out = self._site_inputs(centres, flip, groups)
        n_bins = 2 * int(half_width) // max(int(bin_size), 1)
        shape = [max(int(n_groups), 0), 2, min(max(n_bins, 0), 4096)]
        if shape[0] * shape[1] * shape[2] > 1 << 28:  # (the call fails and writes nothing)
            shape[0] = 0
        sums, counts = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        per_site = peak is not None
        site_sums, site_counts = np.zeros((sites[3], 4), np.int64), np.zeros((sites[3], 4), np.int64)
        self._check(self.lib.ftk_site_ends(
            self.ctx, self.contig_id(name), *sites, int(n_groups), int(half_width), int(bin_size),
            int(quality_threshold), -1 if min_length is None else int(min_length), -1 if max_length is None else int(max_length),
            int(bool(weighted)), int(peak) if per_site else 0, int(flank) if per_site else 0, out(sums), out(counts),
            out(site_sums) if per_site else None, out(site_counts) if per_site else None))
        return (sums, counts, site_sums, site_counts) if per_site else (sums, counts)

    # -- periodograms of score runs (csrc/ftk_spectrum.hip) --------------------------------
    @staticmethod
    def _spectrum_outputs(n_iv, periods, out, ssw_out):
        """The periods as int32 and the two outputs of a spectrum call: fresh host arrays, or the caller's float64
        ``out`` (``n_iv * n_per * 2`` elements: re, im) and ``ssw_out`` (``n_iv``) - host arrays or device tensors."""
        per = np.ascontiguousarray(periods, dtype=np.int32).reshape(-1)
        res = np.zeros((n_iv, len(per)), np.complex128) if out is None else out
        ssw = np.zeros(n_iv, np.float64) if ssw_out is None else ssw_out
        return per, res, ssw

    def track_spectrum(self, scores, offsets, periods, taper=0.1, detrend=True, out=None, ssw_out=None):
        """``(spectrum complex128 [n_iv, n_per], ssw float64 [n_iv])`` of the int64 score runs
        ``scores[offsets[i]:offsets[i+1]]`` at the integer ``periods`` (``ftk_track_spectrum``; the rule is in
        ``include/ftk.h``): each run less its mean (``detrend``) under a split cosine bell of fraction ``taper``, summed
        against ``exp(-2j pi (n mod p) / p)`` in float64; ``ssw`` is the bell's sum of squares, so ``abs(spectrum) ** 2 /
        ssw`` is the power.  ``scores``: a host array, a device tensor or a device address.  A ``(run, period)`` value
        does not depend on what else the call asks for."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        n_iv = max(len(offs) - 1, 0)
        if not (isinstance(scores, (int, np.integer)) or hasattr(scores, "data_ptr")):
            scores = np.ascontiguousarray(scores, dtype=np.int64)
        per, res, ssw = self._spectrum_outputs(n_iv, periods, out, ssw_out)
        keep = np.empty(1, np.int64)  # (a pointer for arrays without an element: the call fails or reads nothing)
        self._check(self.lib.ftk_track_spectrum(
            self.ctx, L.ptr(int(scores) if isinstance(scores, np.integer) else scores), L.ptr(offs if len(offs) else keep), n_iv,
            L.ptr(per if len(per) else keep.view(np.int32)), len(per), float(taper), int(bool(detrend)), L.ptr(res), L.ptr(ssw)))
        return res, ssw

    def wps_spectrum(self, name: str, starts, stops, chrom_size: int, periods, window_size=120, min_length=120,
                     max_length=180, quality_threshold=30, taper=0.1, detrend=True, batch_bases=None, out=None, ssw_out=None):
        """``track_spectrum`` of the WPS of the intervals ``[starts[i], stops[i])`` of resident contig ``name``
        (``ftk_wps_spectrum``): the scores of ``wps_intervals`` with the same arguments, written to device scratch and
        transformed there, ``batch_bases`` bases of intervals at a time (``None``: the library's choice) - no per-base
        value reaches the host.  The same bits as ``track_spectrum(*wps_intervals(...), periods, ...)``."""
        s, _, ps, pe = self._interval_pair(starts, stops, flat=False)
        per, res, ssw = self._spectrum_outputs(len(s), periods, out, ssw_out)
        keep = np.empty(1, np.int64)
        self._check(self.lib.ftk_wps_spectrum(
            self.ctx, self.contig_id(name), ps, pe, len(s), int(chrom_size),
            int(window_size), int(min_length), int(max_length), int(quality_threshold),
            L.ptr(per if len(per) else keep.view(np.int32)), len(per), float(taper), int(bool(detrend)),
            0 if batch_bases is None else int(batch_bases), L.ptr(res), L.ptr(ssw)))
        return res, ssw

    # -- nucleosome calls from adjusted score runs (csrc/ftk_peaks.hip) ----------------------
    PEAK_DTYPE = np.dtype([("run", np.int32), ("start", np.int64), ("stop", np.int64), ("summit", np.int64),
                           ("height", np.float64), ("area", np.float64)])

    def _peaks_call(self, fn, n_runs, *args):
        """Calls ``fn(ctx, *args, outputs...)`` of the peaks pair and takes the library's blocks home:
        ``(calls, stats)`` - a ``PEAK_DTYPE`` record array ordered by ``(run, start)`` and the int64 counters
        ``[n_runs, 6]`` (regions, open, short, long, flat, calls)."""
        stats = np.zeros((n_runs, 6), np.int64)
        keep = np.empty(1, np.int64)
        calls, = self._library_records(lambda *out: fn(self.ctx, *args, *out, L.ptr(stats if n_runs else keep)), self.PEAK_DTYPE)
        return calls, stats

    def track_peaks(self, scores, offsets, skip=0, max_gap=5, min_region=50, short_max=150, max_region=450):
        """``(calls, stats)``: nucleosome calls of the float64 score runs ``scores[offsets[i]:offsets[i+1]]``
        (``ftk_track_peaks``; the rule is in ``include/ftk.h``, "peaks"): regions of positive scores joined over gaps of
        at most ``max_gap`` inside ``[skip, n - skip)``, the windows above the region's median, the window of largest
        area for a region of up to ``short_max`` positions and every window of ``min_region .. short_max`` positions for
        a longer one (up to ``max_region``).  ``calls``: a record array (``Engine.PEAK_DTYPE``: run, start, stop, summit,
        height, area; positions count from the run's start) ordered by ``(run, start)``; ``stats``: int64 ``[n_runs, 6]``
        (regions, open, short, long, flat, calls).  ``scores``: a host array, a device tensor or a device address."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        n_runs = max(len(offs) - 1, 0)
        if not (isinstance(scores, (int, np.integer)) or hasattr(scores, "data_ptr")):
            scores = np.ascontiguousarray(scores, dtype=np.float64)
        keep = np.empty(1, np.int64)
        return self._peaks_call(
            self.lib.ftk_track_peaks, n_runs, L.ptr(int(scores) if isinstance(scores, np.integer) else scores),
            L.ptr(offs if len(offs) else keep), n_runs, int(skip), int(max_gap), int(min_region), int(short_max), int(max_region))

    def wps_peaks(self, name: str, starts, stops, chrom_size: int, window_size=120, min_length=120, max_length=180,
                  quality_threshold=30, median_window_size=1000, savgol_window_size=21, savgol_poly_deg=2, savgol=True,
                  max_gap=5, min_region=50, short_max=150, max_region=450, batch_bases=None):
        """``track_peaks`` of the adjusted WPS of the intervals ``[starts[i], stops[i])`` of resident contig ``name``
        (``ftk_wps_peaks``): the scores of ``wps_intervals``, the running median and Savitzky-Golay pass of
        ``wps_adjust`` and the calls, in device scratch, ``batch_bases`` bases of intervals at a time (``None``: the
        library's choice) - no per-base value reaches the host.  ``skip`` is ``savgol_window_size // 2`` (0 without
        ``savgol``).  A call's ``run`` is its interval's number and its positions are contig positions.  An interval
        shorter than ``median_window_size + max(savgol_window_size, 1)`` has no callable track: no call, zero counters.
        The same calls as ``track_peaks(wps_adjust(*wps_intervals(...)), ...)`` with positions moved to the contig."""
        s, _, ps, pe = self._interval_pair(starts, stops, flat=False)
        sw = int(savgol_window_size) if savgol else 0
        coef = edge = None
        if sw:
            coef, edge = savgol_operators(sw, int(savgol_poly_deg))
        return self._peaks_call(
            self.lib.ftk_wps_peaks, len(s), self.contig_id(name), ps, pe, len(s),
            int(chrom_size), int(window_size), int(min_length), int(max_length), int(quality_threshold),
            int(median_window_size), sw, L.ptr(coef), L.ptr(edge), int(max_gap), int(min_region), int(short_max),
            int(max_region), 0 if batch_bases is None else int(batch_bases))

    # -- preferred fragment ends (csrc/ftk_prefends.hip) ----------------------------------------
    PREFERRED_END_DTYPE = np.dtype([("run", np.int32), ("pos", np.int64), ("kind", np.int32), ("count", np.int32),
                                    ("total", np.int64), ("n_w", np.int32)])

    def preferred_ends(self, name: str, starts, stops, chrom_size: int, half=500, mode="combined", min_count=2, thresholds=None,
                       min_length=None, max_length=None, quality_threshold=30):
        """``(calls, stats)``: the preferred ends of the intervals ``[starts[i], stops[i])`` of resident contig ``name``
        (``ftk_preferred_ends``; the rule is in ``include/ftk.h``, "preferred ends"): the positions whose end count ``e``
        is at least ``min_count`` and whose window total ``T`` over ``half`` bases on either side satisfies
        ``T * 2**20 <= thresholds[min(e, len(thresholds) - 1)] * n_w``.  ``mode``: ``"combined"`` (U + D ends, kind 2) or
        ``"split"`` (U ends, kind 0, and D ends, kind 1, each against its own total).  ``thresholds``: the ``uint64``
        table (``None``: ``utils.preferred_end_thresholds()``).  ``calls``: a record array
        (``Engine.PREFERRED_END_DTYPE``: run, pos, kind, count, total, n_w; ``run`` the interval's number, ``pos`` a
        contig position) ordered by ``(run, pos, kind)``; ``stats``: int64 ``[n_intervals, 6]`` (U ends, D ends, tested
        a, tested b, calls a, calls b)."""
        s, _, ps, pe = self._interval_pair(starts, stops)
        if mode not in ("combined", "split"):
            raise ValueError(f"invalid mode ({mode!r}): 'combined' or 'split'")
        if thresholds is None:
            from .utils import preferred_end_thresholds
            thresholds = preferred_end_thresholds()
        thr = np.ascontiguousarray(thresholds, dtype=np.uint64)
        if thr.ndim != 1:
            raise ValueError("thresholds should be one-dimensional")
        n_iv = len(s)
        stats = np.zeros((n_iv, 6), np.int64)
        keep = np.empty(1, np.int64)
        calls, = self._library_records(lambda *out: self.lib.ftk_preferred_ends(
            self.ctx, self.contig_id(name), ps, pe, n_iv, int(chrom_size),
            int(half), int(mode == "split"), int(min_count), L.ptr(thr if len(thr) else keep), len(thr),
            L.LEN_OPEN if min_length is None else int(min_length), L.LEN_OPEN if max_length is None else int(max_length),
            int(quality_threshold), *out, L.ptr(stats if n_iv else keep)), self.PREFERRED_END_DTYPE)
        return calls, stats

    # -- IFS fragmentation hotspots (csrc/ftk_hotspots.hip) ---------------------------------------
    IFS_WINDOW_DTYPE = np.dtype([("run", np.int32), ("pos", np.int64), ("count", np.int32), ("ifs", np.int64),
                                 ("bg1", np.int64), ("nb1", np.int32), ("bg2", np.int64), ("nb2", np.int32)])
    HOTSPOT_DTYPE = np.dtype([("run", np.int32), ("start", np.int64), ("stop", np.int64), ("n_windows", np.int32),
                              ("summit", np.int64), ("ifs", np.int64), ("count", np.int32), ("bg1", np.int64),
                              ("nb1", np.int32)])

    @staticmethod
    def ifs_window_ranges(starts, stops, chrom_size: int, step: int, m: int):
        """``(k_lo, n)``: the first window and the number of windows of every interval ``[starts[i], stops[i])`` (rule 2 of
        "IFS hotspots" in ``include/ftk.h``: window ``k`` belongs iff ``starts[i] <= k * step`` and its span ends at or
        before ``stops[i]``)."""
        s = np.asarray(starts, dtype=np.int64)
        e = np.asarray(stops, dtype=np.int64)
        step, m, size = int(step), int(m), int(chrom_size)
        n_bins = -(-size // step)
        k_lo = -(-s // step)
        k_hi = np.where(e == size, n_bins - m, np.minimum(e // step - m, n_bins - m))
        return k_lo, np.maximum(k_hi - k_lo + 1, 0)

    def ifs_track(self, name: str, starts, stops, chrom_size: int, step=20, m=10, mean_length=167, min_length=None,
                  max_length=None, quality_threshold=30, device=False):
        """``(n, ifs, offsets)``: the midpoint count ``n`` (int32) and the integer IFS ``I`` (int64, in units of
        ``1 / mean_length``) of every window of the intervals ``[starts[i], stops[i])`` of resident contig ``name``
        (``ftk_ifs_track``; the rule is in ``include/ftk.h``, "IFS hotspots"), interval ``i`` at
        ``[offsets[i], offsets[i + 1])``.  ``device``: the two arrays stay on the GPU (torch tensors)."""
        s, e, ps, pe = self._interval_pair(starts, stops)
        if not 1 <= int(step) <= 65535 or not 1 <= int(m) <= L.IFS_MAX_WINDOW_BINS or not 0 <= int(chrom_size) < 1 << 30:
            count = np.zeros(len(s), np.int64)  # (the library refuses the call below)
        else:
            count = self.ifs_window_ranges(s, e, chrom_size, step, m)[1]
        offs = np.zeros(len(s) + 1, np.int64)
        np.cumsum(count, out=offs[1:])
        total = int(offs[-1])
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            n_out = torch.zeros(total, dtype=torch.int32, device=dev)
            i_out = torch.zeros(total, dtype=torch.int64, device=dev)
        else:
            n_out = np.zeros(total, np.int32)
            i_out = np.zeros(total, np.int64)
        keep = np.empty(1, np.int64)
        self._check(self.lib.ftk_ifs_track(
            self.ctx, self.contig_id(name), ps, pe, len(s),
            L.ptr(np.ascontiguousarray(offs[:-1]) if len(s) else keep), int(chrom_size), int(step), int(m), int(mean_length),
            L.LEN_OPEN if min_length is None else int(min_length), L.LEN_OPEN if max_length is None else int(max_length),
            int(quality_threshold), L.ptr(n_out) if total else None, L.ptr(i_out) if total else None))
        return n_out, i_out, offs

    def ifs_totals(self, name: str, chrom_size: int, min_length=None, max_length=None, quality_threshold=30):
        """``(N, S)``: the number and the length sum of the passing fragments of resident contig ``name`` whose midpoint
        lies in ``[0, chrom_size)`` (``ftk_ifs_totals``, reduced on the GPU) - Python integers."""
        n, sm = C.c_int64(), C.c_int64()
        self._check(self.lib.ftk_ifs_totals(
            self.ctx, self.contig_id(name), int(chrom_size), L.LEN_OPEN if min_length is None else int(min_length),
            L.LEN_OPEN if max_length is None else int(max_length), int(quality_threshold), C.byref(n), C.byref(sm)))
        return int(n.value), int(sm.value)

    def ifs_hotspots(self, name: str, starts, stops, chrom_size: int, step=20, m=10, mean_length=167, h1=125, h2=250,
                     min_count=0, thresholds=None, global_mean=0, join=None, min_windows=1, min_length=None, max_length=None,
                     quality_threshold=30):
        """``(windows, hotspots, stats)``: the IFS hotspots of the intervals ``[starts[i], stops[i])`` of resident contig
        ``name`` (``ftk_ifs_hotspots``; the rule is in ``include/ftk.h``, "IFS hotspots"): the windows of ``m`` bins of
        ``step`` bases whose integer IFS is significantly low against the backgrounds of ``h1`` and ``h2`` bins on either
        side (``h2 = 0``: one background) and against ``global_mean`` (0: off), merged over gaps of up to ``join``
        windows (``None``: ``m + 200 // step``, at least 1).  ``thresholds``: the table (``None``:
        ``utils.ifs_thresholds()``).  ``windows``: the called windows (``Engine.IFS_WINDOW_DTYPE``) ordered by ``(run,
        pos)``; ``hotspots``: ``Engine.HOTSPOT_DTYPE`` records ordered by ``(run, start)``; ``stats``: int64
        ``[n_intervals, 6]`` (windows, tested, called, hotspots kept, hotspots dropped, bases covered)."""
        s, _, ps, pe = self._interval_pair(starts, stops)
        if thresholds is None:
            from .utils import ifs_thresholds
            thresholds = ifs_thresholds()
        thr = np.ascontiguousarray(thresholds, dtype=np.uint64)
        if thr.ndim != 1:
            raise ValueError("thresholds should be one-dimensional")
        if join is None:
            join = max(int(m) + 200 // max(int(step), 1), 1)
        n_iv = len(s)
        stats = np.zeros((n_iv, 6), np.int64)
        keep = np.empty(1, np.int64)
        windows, hotspots = self._library_records(lambda *out: self.lib.ftk_ifs_hotspots(
            self.ctx, self.contig_id(name), ps, pe, n_iv, int(chrom_size),
            int(step), int(m), int(mean_length), int(h1), int(h2), int(min_count), L.ptr(thr if len(thr) else keep), len(thr),
            int(global_mean), int(join), int(min_windows),
            L.LEN_OPEN if min_length is None else int(min_length), L.LEN_OPEN if max_length is None else int(max_length),
            int(quality_threshold), *out, L.ptr(stats if n_iv else keep)), self.IFS_WINDOW_DTYPE, self.HOTSPOT_DTYPE)
        return windows, hotspots, stats

    # -- WPS post-processing --------------------------------------------------------
    def wps_adjust(self, scores, offsets, median_window_size=1000, mean=False, edge_sub=None, savgol_window_size=21,
                   savgol_poly_deg=2, savgol=True, out=None):
        """Running median/mean subtraction + Savitzky-Golay pass over score runs laid end to end
        (frag/_adjust_wps.py:25-50,119-140).  ``scores`` is a host float64 array or a device pointer
        (int) to one; run ``i`` is ``scores[offsets[i]:offsets[i+1]]`` and yields ``len_i - W`` values at
        ``offsets[i] - i*W`` of the result.  Raises ValueError where the reference does (window longer
        than a run, odd median window, Savitzky-Golay window longer than the filtered run)."""
        W = int(median_window_size)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        n_iv = len(offs) - 1
        lens = np.diff(offs)
        if W % 2 or W < 2:
            # data[W//2:-(W//2)] and the n-W running values only line up for even W (numpy broadcast error)
            raise ValueError(f"median_window_size ({W}) must be even: operands could not be broadcast together")
        if n_iv and W > int(lens.min()):
            raise ValueError(f"median_window_size ({W}) cannot be greater than the length of interval "
                             f"({int(lens.min())}).")
        sw = int(savgol_window_size) if savgol else 0
        coef = edge = None
        if sw:
            if n_iv and sw > int(lens.min()) - W:
                raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
            coef, edge = savgol_operators(sw, int(savgol_poly_deg))
        total_out = int(offs[-1]) - n_iv * W if n_iv else 0
        if isinstance(scores, (int, np.integer)):
            sp = C.c_void_p(int(scores))
        else:
            scores = np.ascontiguousarray(scores, dtype=np.float64)
            sp = L.ptr(scores)
        res = np.empty(total_out, np.float64) if out is None else out
        op = C.c_void_p(int(res)) if isinstance(res, (int, np.integer)) else L.ptr(res)
        sub = None if edge_sub is None else np.ascontiguousarray(edge_sub, dtype=np.float64)
        if n_iv and total_out >= 0:
            self._check(self.lib.ftk_wps_adjust(self.ctx, sp, L.ptr(offs), n_iv, W, int(bool(mean)),
                                                None if sub is None else L.ptr(sub), sw,
                                                None if coef is None else L.ptr(coef),
                                                None if edge is None else L.ptr(edge), op))
        return res

    # -- reference images (DELFI GC on the device) ----------------------------------
    def ref_upload(self, key, image: np.ndarray, kind: int) -> int:
        """Upload a contig's reference image (uint8); returns the ref id, cached by ``key`` (2 images kept)."""
        refs = self.__dict__.setdefault("_refs", {})
        if key in refs:
            return refs[key]
        while len(refs) >= 2:  # images are up to ~250 MB each
            old_key = next(iter(refs))
            self.__dict__.setdefault("_ref_layouts", set()).discard(refs[old_key])
            self._check(self.lib.ftk_ref_release(self.ctx, refs.pop(old_key)))
        rid = self.__dict__.setdefault("_next_ref", 0)
        self._next_ref = rid + 1
        image = np.ascontiguousarray(image, dtype=np.uint8)
        self._check(self.lib.ftk_ref_upload(self.ctx, rid, L.ptr(image), len(image), int(kind)))
        refs[key] = rid
        return rid

    def ref_upload_file(self, key, path: str, offset: int, n_bytes: int, kind: int) -> int:
        """``ref_upload`` of ``n_bytes`` at ``offset`` of a file, read by the library (several read threads,
        page-locked chunks, asynchronous copies); cached by ``key`` like ``ref_upload``."""
        refs = self.__dict__.setdefault("_refs", {})
        if key in refs:
            return refs[key]
        while len(refs) >= 2:
            old_key = next(iter(refs))
            self.__dict__.setdefault("_ref_layouts", set()).discard(refs[old_key])
            self._check(self.lib.ftk_ref_release(self.ctx, refs.pop(old_key)))
        rid = self.__dict__.setdefault("_next_ref", 0)
        self._next_ref = rid + 1
        self._check(self.lib.ftk_ref_upload_file(self.ctx, rid, str(path).encode(), int(offset), int(n_bytes), int(kind)))
        refs[key] = rid
        return rid

    def ref_set_layout(self, rid: int, chrom_len: int, line_bases: int = 0, line_width: int = 0, n_starts=None,
                       n_ends=None):
        """Geometry of an uploaded image: FASTA line layout or the 2bit record's N blocks."""
        ns = np.ascontiguousarray(n_starts if n_starts is not None else [], dtype=np.int32)
        ne = np.ascontiguousarray(n_ends if n_ends is not None else [], dtype=np.int32)
        self._check(self.lib.ftk_ref_set_layout(self.ctx, rid, int(chrom_len), int(line_bases), int(line_width),
                                                L.ptr(ns) if len(ns) else None, L.ptr(ne) if len(ne) else None,
                                                len(ns)))

    def motif_counts(self, name: str, rid: int, starts, stops, k: int, fwd_offset: int, rev_offset: int,
                     both_strands: bool, negative_strand: bool, guard: int, rev_oob_is_error: bool,
                     quality_threshold: int, bam: bool = False):
        """k-mer histograms per window (frag/_end_motifs.py:118-176, frag/_breakpoint_motifs.py:124-185);
        returns (counts uint32 [n_win, 4**k], fetched fragments per window, reverse-end errors per window)."""
        ws = np.ascontiguousarray(starts, dtype=np.int32)
        we = np.ascontiguousarray(stops, dtype=np.int32)
        n = len(ws)
        counts = np.zeros((n, 4 ** int(k)), np.uint32)
        nfrag = np.zeros(n, np.int64)
        err = np.zeros(n, np.int64)
        if n:
            m = L.Motif(int(k), int(fwd_offset), int(rev_offset), int(bool(both_strands)),
                        int(bool(negative_strand)), int(guard), int(bool(rev_oob_is_error)))
            self._check(self.lib.ftk_motif_counts(self.ctx, self.contig_id(name), rid, L.ptr(ws), L.ptr(we), n,
                                                  C.byref(m), int(quality_threshold),
                                                  L.FETCH_BAM_READ1 if bam else L.FETCH_TABIX, L.ptr(counts),
                                                  L.ptr(nfrag), L.ptr(err)))
        return counts, nfrag, err

    def ref_gc_counts(self, rid: int, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.int64)
        hi = np.ascontiguousarray(hi, dtype=np.int64)
        out = np.zeros(len(lo), np.int64)
        if len(lo):
            self._check(self.lib.ftk_ref_gc_counts(self.ctx, rid, L.ptr(lo), L.ptr(hi), len(lo), L.ptr(out)))
        return out

