"""
Output writers of the per-base features on the library's host threads (``csrc/ftk_writers.cpp``).

The reference prints one Python f-string per base (``frag/_wps.py:208-229``, ``frag/_multi_wps.py:328-341``) and
hands bigWig entries to pyBigWig (``:300-325``); after a 0.2 ms kernel that is seconds to minutes of
interpreter time for a chromosome.  Here the same bytes are formatted in C on all usable cores, ``.gz``
outputs are written as gzip members compressed in parallel (the decompressed stream is identical; a gzip
file carries a timestamp, so compressed bytes never were reproducible), and bigWig data sections are built
and deflated natively.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

GZIP_LEVEL = 6


class TextBuffer:
    """Bytes formatted by the library (owned by it until ``free``)."""

    def __init__(self, lib, ptr, n):
        self._lib, self.ptr, self.n = lib, ptr, int(n)

    def tobytes(self) -> bytes:
        return C.string_at(self.ptr, self.n)

    def write(self, path: str, gzip_level: int = 0, append: bool = False, threads: int = 0):
        rc = self._lib.ftk_file_write(str(path).encode(), self.ptr, self.n, int(gzip_level), int(threads), int(append))
        if rc != L.FTK_OK:
            raise OSError(self._lib.ftk_fragtable_error().decode())

    def gzip_bytes(self, gzip_level: int = GZIP_LEVEL, threads: int = 0) -> bytes:
        """The gzip members ``write(path, gzip_level)`` would put into the file, as bytes (a rank that does not own
        the output file hands them to the one that does)."""
        if self.n == 0:
            return b""
        out, n = C.c_void_p(), C.c_int64()
        rc = self._lib.ftk_gzip_members(self.ptr, self.n, int(gzip_level), int(threads), C.byref(out), C.byref(n))
        if rc != L.FTK_OK:
            raise L.FtkError(rc, self._lib.ftk_fragtable_error().decode())
        try:
            return C.string_at(out.value, n.value)
        finally:
            self._lib.ftk_buffer_free(out.value)

    def free(self):
        if self.ptr:
            self._lib.ftk_buffer_free(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _call(fn, *args) -> TextBuffer:
    lib = L.load()
    out, n = C.c_void_p(), C.c_int64()
    rc = getattr(lib, fn)(*args, C.byref(out), C.byref(n))
    if rc != L.FTK_OK:
        raise L.FtkError(rc, lib.ftk_fragtable_error().decode())
    return TextBuffer(lib, out.value, n.value)


def wig_body(values, threads: int = 0) -> TextBuffer:
    """``"".join(f"{v}\\n" for v in values)`` for int64 values."""
    v = np.ascontiguousarray(values, dtype=np.int64)
    return _call("ftk_format_wig_i64", L.ptr(v), len(v), int(threads))


def _runs(starts, offsets, n_values):
    st = np.ascontiguousarray(starts, dtype=np.int64)
    if offsets is None:
        offs = np.array([0, n_values], np.int64)
    else:
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if len(offs) != len(st) + 1:
        raise ValueError("offsets must hold one entry more than starts")
    return st, offs


def bedgraph_rows(contig: str, starts, values, offsets=None, threads: int = 0) -> TextBuffer:
    """``contig  pos  pos+1  value`` per base of every run (run ``k`` = ``values[offsets[k]:offsets[k+1]]``
    starting at ``starts[k]``; one run when ``offsets`` is None and ``starts`` a single position); int64 values
    as ``str(int)``, float64 values as ``repr(float)``."""
    v = np.asarray(values)
    flt = v.dtype.kind == "f"
    v = np.ascontiguousarray(v, dtype=np.float64 if flt else np.int64)
    st, offs = _runs(np.atleast_1d(starts), offsets, len(v))
    return _call("ftk_format_bedgraph_f64" if flt else "ftk_format_bedgraph_i64", str(contig).encode(), L.ptr(st),
                 L.ptr(offs), len(st), L.ptr(v), int(threads))


def bedgraph_batches(contig: str, starts, values, offsets=None, max_values: int = 8 << 20, threads: int = 0):
    """``bedgraph_rows`` in pieces of at most ``max_values`` rows (about 25 bytes each), cut at run boundaries
    and inside runs longer than that: a generator of ``TextBuffer`` whose concatenation is the full text, so a
    whole chromosome of per-base rows never sits in memory at once."""
    v = np.asarray(values)
    st, offs = _runs(np.atleast_1d(starts), offsets, len(v))
    k, n_runs = 0, len(st)
    while k < n_runs:
        a = int(offs[k])
        if offs[k + 1] - a > max_values:  # one long run: its own pieces
            for o in range(a, int(offs[k + 1]), max_values):
                e = min(o + max_values, int(offs[k + 1]))
                yield bedgraph_rows(contig, [int(st[k]) + (o - a)], v[o:e], None, threads)
            k += 1
            continue
        j = int(np.searchsorted(offs, a + max_values, side="right")) - 1  # last run end within the budget
        j = min(max(j, k + 1), n_runs)
        yield bedgraph_rows(contig, st[k:j], v[a:int(offs[j])], offs[k:j + 1] - a, threads)
        k = j


def bedgraph_runs(contig: str, run_start, run_end, run_depth, threads: int = 0) -> TextBuffer:
    """``contig  start  end  depth`` per run of a depth track (``Engine.depth_runs``; int32 columns)."""
    s_ = np.ascontiguousarray(run_start, dtype=np.int32)
    e_ = np.ascontiguousarray(run_end, dtype=np.int32)
    d_ = np.ascontiguousarray(run_depth, dtype=np.int32)
    if not (s_.ndim == 1 and s_.shape == e_.shape == d_.shape):
        raise ValueError("run columns differ in length")
    return _call("ftk_format_bedgraph_runs", str(contig).encode(), L.ptr(s_), L.ptr(e_), L.ptr(d_), len(s_), int(threads))


def write_text(path: str, data: bytes, gzip_level: int = 0, append: bool = False, threads: int = 0):
    """Plain or gzip-member write of a Python bytes object (headers and other small pieces)."""
    lib = L.load()
    rc = lib.ftk_file_write(str(path).encode(), data, len(data), int(gzip_level), int(threads), int(append))
    if rc != L.FTK_OK:
        raise OSError(lib.ftk_fragtable_error().decode())


def bigwig_sections(chrom_id: int, starts, values, offsets=None, items_per_section: int = 16384, level: int = 6,
                    threads: int = 0):
    """fixedStep data sections of one ``addEntries(chrom, start, values=..., span=1, step=1)`` call per run.
    Returns ``(blob bytes, table int64[n_sec, 3] = start end compressed_bytes, stats float64[n_sec, 4] = min max
    sum sumsq)``."""
    lib = L.load()
    v = np.asarray(values)
    kind = 1 if v.dtype.kind == "f" else 0
    v = np.ascontiguousarray(v, dtype=np.float64 if kind else np.int64)
    st, offs = _runs(np.atleast_1d(starts), offsets, len(v))
    out, out_len, n_sec = C.c_void_p(), C.c_int64(), C.c_int64()
    table, stats = C.c_void_p(), C.c_void_p()
    rc = lib.ftk_bigwig_fixedstep_sections(int(chrom_id), L.ptr(st), L.ptr(offs), len(st), L.ptr(v), kind,
                                           int(items_per_section), int(level), int(threads), C.byref(out),
                                           C.byref(out_len), C.byref(n_sec), C.byref(table), C.byref(stats))
    if rc != L.FTK_OK:
        raise L.FtkError(rc, lib.ftk_fragtable_error().decode())
    try:
        blob = C.string_at(out.value, out_len.value)
        k = int(n_sec.value)
        tab = np.ctypeslib.as_array(C.cast(table, C.POINTER(C.c_int64)), (max(k, 1) * 3,))[:k * 3].reshape(k, 3).copy()
        sts = np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_double)), (max(k, 1) * 4,))[:k * 4].reshape(k, 4).copy()
    finally:
        for q in (out, table, stats):
            lib.ftk_buffer_free(q.value)
    return blob, tab, sts


def frag_rows(contig: str, start, end, mapq, strand, bed6: bool = False, threads: int = 0) -> TextBuffer:
    """Fragment-file rows ``contig  start  end  mapq  +|-`` (``bed6``: a ``.`` name column before mapq)."""
    s_ = np.ascontiguousarray(start, dtype=np.int32)
    e_ = np.ascontiguousarray(end, dtype=np.int32)
    q_ = np.ascontiguousarray(mapq, dtype=np.uint8)
    t_ = np.ascontiguousarray(strand, dtype=np.uint8)
    if not (len(s_) == len(e_) == len(q_) == len(t_)):
        raise ValueError("fragment columns differ in length")
    return _call("ftk_format_frag_rows", str(contig).encode(), L.ptr(s_), L.ptr(e_), L.ptr(q_), L.ptr(t_), len(s_),
                 int(bool(bed6)), int(threads))


def bgzf_write(path: str, data, level: int = 6, append: bool = False, write_eof: bool = True, threads: int = 0):
    """Write ``data`` (bytes or a ``TextBuffer``) as BGZF blocks compressed in parallel; returns the file offset
    of every data block plus the offset behind the last one (int64 array)."""
    lib = L.load()
    if isinstance(data, TextBuffer):
        ptr, n = C.c_void_p(data.ptr), data.n
    else:
        ptr, n = data, len(data)
    offs = np.zeros(-(-n // 0xFF00) + 1, np.int64)
    rc = lib.ftk_bgzf_write(str(path).encode(), ptr, n, int(level), int(threads), int(append), int(write_eof), L.ptr(offs))
    if rc != L.FTK_OK:
        raise OSError(lib.ftk_fragtable_error().decode())
    return offs


# ---------------------------------------------------------------------------------------------------------------
# Row files of the interval commands.  What the formats ARE is the reference's contract (suffix rules, column order,
# header lines, `str()` / `repr()` of every value: frag/_coverage.py:262-296, frag/_frag_length.py:466-490,607-632);
# how they are produced is ours: the rows of a call are one string, written once (`.gz`: as gzip members, compressed
# by the library's threads - the decompressed stream is what `gzip.open(..., "wt")` would have held).
# ---------------------------------------------------------------------------------------------------------------
def _emit(output_file: str, text: str, plain: tuple, gz: tuple, bad_suffix: str) -> None:
    """``text`` to ``output_file``: ``"-"`` = stdout, a name ending in one of ``gz`` = gzip, in one of ``plain`` = as
    is (``plain=None``: any other name), else ``ValueError(bad_suffix)``."""
    import sys
    if output_file == "-":
        sys.stdout.write(text)
    elif gz and output_file.endswith(gz):
        write_text(output_file, text.encode(), GZIP_LEVEL)
    elif plain is None or output_file.endswith(plain):
        with open(output_file, "w") as fh:
            fh.write(text)
    else:
        raise ValueError(bad_suffix)


def check_suffix(output_file: str, suffixes: tuple, message: str) -> None:
    if not (output_file == "-" or output_file.endswith(suffixes)):
        raise ValueError(message)


def write_coverage_rows(output_file: str, intervals, values) -> None:
    """``contig start stop name value`` per interval (``.bedgraph``: no name column); ``.bed`` / ``.bedgraph`` /
    ``.bed.gz`` / ``-``."""
    message = "output_file should have .bed or .bed.gz as suffix"
    check_suffix(output_file, (".bed", ".bedgraph", ".bed.gz"), message)
    if output_file.endswith(".bedgraph"):
        text = "".join([f"{c}\t{a}\t{b}\t{v}\n" for (c, a, b, _), v in zip(intervals, values)])
    else:
        text = "".join([f"{c}\t{a}\t{b}\t{n}\t{v}\n" for (c, a, b, n), v in zip(intervals, values)])
    _emit(output_file, text, (".bed", ".bedgraph"), (".bed.gz",), message)


def write_length_bins(output_file: str, bins, counts, bin_size: int, stats=None) -> None:
    """The ``min max count`` table of ``frag_length_bins`` (+ ``#name: value`` lines when ``stats`` is given); any
    file name, ``.gz`` = gzip, ``-`` = stdout."""
    rows = ["min\tmax\tcount\n"]
    rows += [f"{lo}\t{lo + bin_size - 1}\t{n}\n" for lo, n in zip(bins, counts)]
    if stats:
        rows += [f"#{name}: {value}\n" for name, value in stats]
    _emit(output_file, "".join(rows), None, (".gz",), "")


def write_length_stats(output_file: str, results, short_reads: int, lines=None) -> None:
    """The per-interval statistics table of ``frag_length_intervals``: a header line, then the eleven fields of every
    result, tab-separated, ``str()`` of each (``lines``: the rows already formatted, one per result); ``.bed`` /
    ``.bedgraph`` / ``.bed.gz`` / ``-``."""
    message = "The output file should have .bed or .bed.gz as as suffix."
    check_suffix(output_file, (".bed", ".bedgraph", ".bed.gz"), message)
    head = f"contig\tstart\tstop\tname\tmean\tmedian\tstdev\tmin\tmax\tcount\ts{short_reads}\n"
    if lines is None or any(ln is None for ln in lines):
        lines = [f"{r[0]}\t{r[1]}\t{r[2]}\t{r[3]}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\t{r[8]}\t{r[9]}\t{r[10]}" for r in results]
    body = "\n".join(lines)
    _emit(output_file, head + body + "\n", (".bed", ".bedgraph"), (".bed.gz",), message)


GC_BIAS_SUFFIXES = (".tsv", ".tsv.gz")


def gc_bias_text(min_length: int, observed, expected, bias) -> str:
    """The rows of a length x GC table (``utils.frag_gc_bias``): the header ``length gc observed expected bias``, then one
    row per cell with ``observed > 0 or expected > 0``, lengths ascending, the bias as ``repr(float)`` (``nan`` where it
    is undefined)."""
    observed = np.asarray(observed)
    expected = np.asarray(expected)
    bias = np.asarray(bias, dtype=np.float64)
    if not (observed.ndim == 2 and observed.shape == expected.shape == bias.shape):
        raise ValueError("observed, expected and bias differ in shape")
    rows = ["length\tgc\tobserved\texpected\tbias\n"]
    ri, gi = np.nonzero((observed > 0) | (expected > 0))
    rows += [f"{int(r) + int(min_length)}\t{int(g)}\t{int(observed[r, g])}\t{int(expected[r, g])}\t{float(bias[r, g])!r}\n"
             for r, g in zip(ri, gi)]
    return "".join(rows)


def write_gc_bias_table(output_file: str, min_length: int, observed, expected, bias) -> None:
    """``gc_bias_text`` to ``output_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith(GC_BIAS_SUFFIXES):
        raise ValueError(message)
    _emit(output_file, gc_bias_text(min_length, observed, expected, bias), (".tsv",), (".tsv.gz",), message)


def write_gc_coverage_rows(output_file: str, intervals, count, corrected) -> None:
    """``contig start stop name count corrected`` per interval (``utils.frag_gc_coverage``), ``corrected`` with six
    decimals or ``nan``; ``.bed`` as text, ``.bed.gz`` as gzip."""
    message = "output_file should have .bed or .bed.gz as suffix"
    if not output_file.endswith((".bed", ".bed.gz")):
        raise ValueError(message)
    text = "".join([f"{c}\t{a}\t{b}\t{n}\t{int(k)}\t{'nan' if x != x else format(float(x), '.6f')}\n"
                    for (c, a, b, n), k, x in zip(intervals, count, corrected)])
    _emit(output_file, text, (".bed",), (".bed.gz",), message)


def write_site_profile_rows(output_file: str, profile) -> None:
    """``group n_sites offset count corrected`` per (group, bin) of a ``utils.SiteProfile`` behind the header line
    ``#group n_sites offset count corrected``, in group order then bin order, ``corrected`` with six decimals; ``.tsv``
    as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["#group\tn_sites\toffset\tcount\tcorrected\n"]
    for g, name in enumerate(profile.groups):
        rows += [f"{name}\t{int(profile.n_sites[g])}\t{int(o)}\t{int(k)}\t{format(float(x), '.6f')}\n"
                 for o, k, x in zip(profile.offsets, profile.count[g], profile.corrected[g])]
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_vplot_rows(output_file: str, vplot) -> None:
    """``group n_sites length offset count corrected`` per cell of a ``utils.VPlot`` behind the header line ``#group
    n_sites length offset count corrected``, in group order, then row order, then bin order, ``corrected`` with six
    decimals; ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["#group\tn_sites\tlength\toffset\tcount\tcorrected\n"]
    for g, name in enumerate(vplot.groups):
        head = f"{name}\t{int(vplot.n_sites[g])}\t"
        for r, length in enumerate(vplot.lengths):
            rows += [f"{head}{int(length)}\t{int(o)}\t{int(k)}\t{format(float(x), '.6f')}\n"
                     for o, k, x in zip(vplot.offsets, vplot.count[g, r], vplot.corrected[g, r])]
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_ocf_rows(output_file: str, ocf) -> None:
    """``group n_sites left_up left_down right_up right_down ocf_count ocf`` per group of a ``utils.OCF`` behind the header
    line ``#group n_sites left_up left_down right_up right_down ocf_count ocf``: the four window counts summed over the
    group's sites, the score from the counts and the (corrected) score with six decimals; ``.tsv`` as text, ``.tsv.gz`` as
    gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["#group\tn_sites\tleft_up\tleft_down\tright_up\tright_down\tocf_count\tocf\n"]
    rows += [f"{name}\t{int(ocf.n_sites[g])}\t" + "\t".join(str(int(x)) for x in ocf.windows_count[g])
             + f"\t{int(ocf.ocf_count[g])}\t{format(float(ocf.ocf[g]), '.6f')}\n" for g, name in enumerate(ocf.groups)]
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_end_profile_rows(output_file: str, ocf) -> None:
    """``group n_sites offset up_count down_count up_corrected down_corrected`` per (group, bin) of a ``utils.OCF`` behind
    the header line of those names with a ``#`` in front, in group order then bin order, the corrected columns with six
    decimals; ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "profile_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["#group\tn_sites\toffset\tup_count\tdown_count\tup_corrected\tdown_corrected\n"]
    for g, name in enumerate(ocf.groups):
        rows += [f"{name}\t{int(ocf.n_sites[g])}\t{int(o)}\t{int(u)}\t{int(d)}\t{format(float(x), '.6f')}\t{format(float(y), '.6f')}\n"
                 for o, u, d, x, y in zip(ocf.offsets, ocf.up_count[g], ocf.down_count[g], ocf.up_corrected[g], ocf.down_corrected[g])]
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_site_ocf_rows(output_file: str, sites, site_windows_count, site_ocf) -> None:
    """``contig centre name strand left_up left_down right_up right_down ocf`` per site of ``sites`` (``utils.read_sites``)
    behind the header line of those names with a ``#`` in front, in the site file's order: the four window COUNTS of the
    site (``site_windows_count``, int64 ``(n_sites, 4)``) and its score ``site_ocf`` with six decimals.  Sites whose score
    is NaN - those on skipped contigs - are left out.  ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "site_output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["#contig\tcentre\tname\tstrand\tleft_up\tleft_down\tright_up\tright_down\tocf\n"]
    rows += [f"{c}\t{int(centre)}\t{name}\t{strand}\t" + "\t".join(str(int(x)) for x in w) + f"\t{format(float(s), '.6f')}\n"
             for (c, centre, name, strand), w, s in zip(sites, site_windows_count, site_ocf) if s == s]
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_wps_spectrum_rows(output_file: str, spectrum) -> None:
    """One row per interval of a ``utils.WpsSpectrum``, in its order, behind the header line ``contig start stop name
    n_bases band_mean p<min> ... p<max>``: the interval, its bases, the band's mean power and the power at every period,
    floats with six significant digits or ``nan``; ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)

    def num(x):
        return "nan" if x != x else format(float(x), ".6g")
    rows = ["\t".join(["contig", "start", "stop", "name", "n_bases", "band_mean"] + [f"p{int(p)}" for p in spectrum.periods]) + "\n"]
    for (c, a, b, name), n, mean, row in zip(spectrum.intervals, spectrum.n_bases, spectrum.band_mean, spectrum.power):
        rows.append("\t".join([str(c), str(a), str(b), str(name), str(int(n)), num(mean)] + [num(x) for x in row]) + "\n")
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_wps_peaks_rows(output_file: str, peaks) -> None:
    """One row per call of a ``utils.WpsPeaks``, ordered by interval and start, without a header line: ``contig start stop
    name centre summit height area`` - ``[start, stop)`` the call's window, ``name`` its interval's name (``.`` in
    whole-contig mode), ``centre = start + (stop - start) // 2``, the floats with six significant digits; ``.bed`` as text,
    ``.bed.gz`` as gzip."""
    message = "output_file should have .bed or .bed.gz as suffix"
    if not output_file.endswith((".bed", ".bed.gz")):
        raise ValueError(message)
    rows = []
    for i, a, b, summit, height, area in peaks.calls.tolist():
        c, _, _, name = peaks.intervals[i]
        rows.append(f"{c}\t{a}\t{b}\t{name}\t{a + (b - a) // 2}\t{summit}\t{format(height, '.6g')}\t{format(area, '.6g')}\n")
    _emit(output_file, "".join(rows), (".bed",), (".bed.gz",), message)


def write_wps_peaks_summary(output_file: str, peaks) -> None:
    """One row per interval of a ``utils.WpsPeaks``, in its order, behind the header line ``contig start stop name callable
    regions open short long flat calls median_spacing``: the interval, the positions of its callable track, the six
    counters of the rule and the median distance between consecutive call centres (six significant digits, ``nan`` below
    two calls); ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "summary_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["contig\tstart\tstop\tname\tcallable\tregions\topen\tshort\tlong\tflat\tcalls\tmedian_spacing\n"]
    for (c, a, b, name), n, stats, gap in zip(peaks.intervals, peaks.callable, peaks.stats, peaks.median_spacing):
        rows.append("\t".join([str(c), str(a), str(b), str(name), str(int(n))] + [str(int(x)) for x in stats]
                              + ["nan" if gap != gap else format(float(gap), ".6g")]) + "\n")
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def write_preferred_end_rows(output_file: str, ends) -> None:
    """One row per call of a ``utils.PreferredEnds``, ordered by interval, position and kind, without a header line:
    ``contig pos pos+1 name kind count window_total expected neglog10_p`` - ``name`` the interval's name (``.`` in
    whole-contig mode), ``kind`` ``U`` / ``D`` / ``B`` (both ends, combined mode), ``expected = window_total / n_w`` the
    mean of the Poisson model, ``p = P(X >= count)`` under it (``scipy.special.gammainc(count, expected)``), both computed
    here for the calls alone, the floats with six significant digits; ``.bed`` as text, ``.bed.gz`` as gzip."""
    message = "output_file should have .bed or .bed.gz as suffix"
    if not output_file.endswith((".bed", ".bed.gz")):
        raise ValueError(message)
    calls = ends.calls
    rows = []
    if len(calls):
        from scipy.special import gammainc
        expected = calls["total"].astype(np.float64) / calls["n_w"].astype(np.float64)
        with np.errstate(divide="ignore"):
            score = -np.log10(gammainc(calls["count"].astype(np.float64), expected))
        for (i, pos, kind, count, total, _), m, s in zip(calls.tolist(), expected.tolist(), score.tolist()):
            c, _, _, name = ends.intervals[i]
            rows.append(f"{c}\t{pos}\t{pos + 1}\t{name}\t{'UDB'[kind]}\t{count}\t{total}\t{format(m, '.6g')}\t{format(s + 0.0, '.6g')}\n")
    _emit(output_file, "".join(rows), (".bed",), (".bed.gz",), message)


def write_preferred_end_summary(output_file: str, ends) -> None:
    """One row per interval of a ``utils.PreferredEnds``, in its order, behind the header line ``contig start stop name
    u_ends d_ends tested_a tested_b calls_a calls_b share``: the interval, the six counters of the rule and the share of
    its ends that lie on called positions (six significant digits, ``nan`` without ends); ``.tsv`` as text, ``.tsv.gz`` as
    gzip."""
    message = "summary_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["contig\tstart\tstop\tname\tu_ends\td_ends\ttested_a\ttested_b\tcalls_a\tcalls_b\tshare\n"]
    for (c, a, b, name), stats, share in zip(ends.intervals, ends.stats, ends.share):
        rows.append("\t".join([str(c), str(a), str(b), str(name)] + [str(int(x)) for x in stats]
                              + ["nan" if share != share else format(float(share), ".6g")]) + "\n")
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


def _ifs_floats(res, rec):
    """``(ifs, expected, neglog10_p)`` of IFS records (hotspot summits or called windows): ``ifs = I / L``, ``expected =
    B m / (n_b L)`` - the first background's mean IFS per window - and ``p = P(X <= floor(I / L))`` under a Poisson model
    of that mean (``scipy.special.gammaincc``), computed here from the integers for the records alone."""
    from scipy.special import gammaincc
    L = res.mean_length[rec["interval"]].astype(np.float64)
    ifs = rec["ifs"].astype(np.float64) / L
    expected = rec["bg1"].astype(np.float64) * res.window_bins / (rec["nb1"].astype(np.float64) * L)
    q = (rec["ifs"] // res.mean_length[rec["interval"]]).astype(np.float64)
    with np.errstate(divide="ignore"):
        score = -np.log10(gammaincc(q + 1.0, expected))
    return ifs.tolist(), expected.tolist(), score.tolist()


def write_hotspot_rows(output_file: str, res) -> None:
    """One row per hotspot of a ``utils.IfsHotspots``, ordered by interval and start, without a header line: ``contig start
    stop name n_windows summit ifs count expected neglog10_p`` - ``name`` the interval's name (``.`` in whole-contig mode),
    ``summit`` the start of the hotspot's called window of smallest IFS, and that window's ``ifs = I / L``, fragment
    ``count``, ``expected = B m / (n_b L)`` (the mean IFS per window of its first background) and Poisson lower tail of
    ``floor(ifs)``, the floats with six significant digits; ``.bed`` as text, ``.bed.gz`` as gzip."""
    message = "output_file should have .bed or .bed.gz as suffix"
    if not output_file.endswith((".bed", ".bed.gz")):
        raise ValueError(message)
    hot = res.hotspots
    rows = []
    if len(hot):
        for (i, a, b, nw, summit, _, count, _, _), x, m, s in zip(hot.tolist(), *_ifs_floats(res, hot)):
            c, _, _, name = res.intervals[i]
            rows.append(f"{c}\t{a}\t{b}\t{name}\t{nw}\t{summit}\t{format(x, '.6g')}\t{count}\t{format(m, '.6g')}\t{format(s + 0.0, '.6g')}\n")
    _emit(output_file, "".join(rows), (".bed",), (".bed.gz",), message)


def write_hotspot_windows(output_file: str, res) -> None:
    """One row per called window of a ``utils.IfsHotspots``, ordered by interval and start, without a header line: ``contig
    start stop name count ifs expected neglog10_p`` with the columns of ``write_hotspot_rows``; ``.bed`` as text,
    ``.bed.gz`` as gzip."""
    message = "windows_file should have .bed or .bed.gz as suffix"
    if not output_file.endswith((".bed", ".bed.gz")):
        raise ValueError(message)
    win = res.windows
    rows = []
    if len(win):
        for (i, a, b, count, *_), x, m, s in zip(win.tolist(), *_ifs_floats(res, win)):
            c, _, _, name = res.intervals[i]
            rows.append(f"{c}\t{a}\t{b}\t{name}\t{count}\t{format(x, '.6g')}\t{format(m, '.6g')}\t{format(s + 0.0, '.6g')}\n")
    _emit(output_file, "".join(rows), (".bed",), (".bed.gz",), message)


def write_hotspot_summary(output_file: str, res) -> None:
    """One row per interval of a ``utils.IfsHotspots``, in its order, behind the header line ``contig start stop name
    mean_length global_mean windows tested called hotspots dropped bases``: the interval, its contig's ``L`` and mean IFS
    per window (six significant digits; ``nan`` when the test did not use it) and the six counters of the rule; ``.tsv``
    as text, ``.tsv.gz`` as gzip."""
    message = "summary_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith((".tsv", ".tsv.gz")):
        raise ValueError(message)
    rows = ["contig\tstart\tstop\tname\tmean_length\tglobal_mean\twindows\ttested\tcalled\thotspots\tdropped\tbases\n"]
    for (c, a, b, name), L, gm, stats in zip(res.intervals, res.mean_length, res.global_mean, res.stats):
        rows.append("\t".join([str(c), str(a), str(b), str(name), str(int(L)), "nan" if gm == 0 else format(int(gm) / 1024.0, ".6g")]
                              + [str(int(x)) for x in stats]) + "\n")
    _emit(output_file, "".join(rows), (".tsv",), (".tsv.gz",), message)


END_CONTEXT_SUFFIXES = (".tsv", ".tsv.gz")
END_CONTEXT_HEADER = "length_lo\tlength_hi\tend\toffset\tmotif\tcount\tfrequency\tenrichment\n"
END_CONTEXT_MOTIFS = tuple("ACGTN") + tuple(a + b for a in "ACGT" for b in "ACGT")


def end_context_text(res) -> str:
    """The rows of a ``utils.EndContext``: the header ``length_lo length_hi end offset motif count frequency enrichment``,
    then, per length class ``[length_lo, length_hi)``, per end (``U`` / ``D``; ``+`` / ``-`` when the anchor is the
    centre) and per offset, the motifs ``A C G T N`` and ``AA AC ... TT`` that have a count or a background count (N: the
    reference's N positions).  ``frequency`` and ``enrichment`` are ``repr(float)`` of ``res.frequency(k)`` and
    ``res.enrichment(k)``, ``nan`` where they are undefined and for N."""
    w = int(res.half_width)
    mono, dinuc = res.mono, res.dinuc
    count = np.concatenate([mono, dinuc], axis=-1)
    nan = np.full(mono.shape[:-1] + (1,), np.nan)
    freq = np.concatenate([res.frequency(1), nan, res.frequency(2)], axis=-1)
    enr = np.concatenate([res.enrichment(1), nan, res.enrichment(2)], axis=-1)
    bg_n = int(np.asarray(res.background).reshape(5, 5)[4].sum())
    bg = np.concatenate([res.background_counts(1), np.full((2, 1), bg_n, np.int64), res.background_counts(2)], axis=-1)
    ends = "UD" if res.anchor == "ends" else "+-"
    rows = [END_CONTEXT_HEADER]
    for c in range(count.shape[0]):
        for k in range(2):
            head = f"{int(res.length_edges[c])}\t{int(res.length_edges[c + 1])}\t{ends[k]}\t"
            for j in range(2 * w):
                rows += [f"{head}{j - w}\t{END_CONTEXT_MOTIFS[m]}\t{int(count[c, k, j, m])}\t{float(freq[c, k, j, m])!r}\t{float(enr[c, k, j, m])!r}\n"
                         for m in np.flatnonzero((count[c, k, j] > 0) | (bg[k] > 0))]
    return "".join(rows)


def write_end_context_rows(output_file: str, res) -> None:
    """``end_context_text`` to ``output_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith(END_CONTEXT_SUFFIXES):
        raise ValueError(message)
    _emit(output_file, end_context_text(res), (".tsv",), (".tsv.gz",), message)


MOTIF_LENGTH_SUFFIXES = (".tsv", ".tsv.gz")
MOTIF_LENGTH_HEADER = "length_lo\tlength_hi\tend\tmotif\tcount\tfrequency\n"
MOTIF_LENGTH_SUMMARY_HEADER = "length_lo\tlength_hi\tn_frags\tundefined_u\tundefined_d\tmds_u\tmds_d\tmds\n"


def motif_length_text(res) -> str:
    """The rows of a ``utils.MotifLengths``: the header ``length_lo length_hi end motif count frequency``, then one row per
    non-zero cell - per length row (the lengths ``length_lo .. length_hi``, both inclusive), per end (``U`` / ``D``) and per
    motif in the order of ``gen_kmers``, the undefined column last, written ``N``.  ``frequency`` is ``repr(float)`` of
    ``res.frequency()``, ``nan`` for N."""
    table, names = np.asarray(res.table), list(res.motifs()) + ["N"]
    freq = np.concatenate([res.frequency(), np.full(table.shape[:2] + (1,), np.nan)], axis=-1)
    first, b = res.lengths(), int(res.length_bin)
    rows = [MOTIF_LENGTH_HEADER]
    for r in np.flatnonzero(table.any(axis=(0, 2))):
        for kind in range(2):
            head = f"{int(first[r])}\t{int(first[r]) + b - 1}\t{'UD'[kind]}\t"
            rows += [f"{head}{names[m]}\t{int(table[kind, r, m])}\t{float(freq[kind, r, m])!r}\n" for m in np.flatnonzero(table[kind, r])]
    return "".join(rows)


def motif_length_summary_text(res) -> str:
    """One row per length row of a ``utils.MotifLengths`` that holds a fragment: the header ``length_lo length_hi n_frags
    undefined_u undefined_d mds_u mds_d mds``, the undefined readings of either end and ``repr(float)`` of ``res.mds()``."""
    table, mds = np.asarray(res.table), res.mds()
    first, b = res.lengths(), int(res.length_bin)
    rows = [MOTIF_LENGTH_SUMMARY_HEADER]
    rows += [f"{int(first[r])}\t{int(first[r]) + b - 1}\t{int(res.n_kept[r])}\t{int(table[0, r, -1])}\t{int(table[1, r, -1])}\t"
             f"{float(mds[0, r])!r}\t{float(mds[1, r])!r}\t{float(mds[2, r])!r}\n" for r in np.flatnonzero(np.asarray(res.n_kept))]
    return "".join(rows)


def write_motif_length_rows(output_file: str, res) -> None:
    """``motif_length_text`` to ``output_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith(MOTIF_LENGTH_SUFFIXES):
        raise ValueError(message)
    _emit(output_file, motif_length_text(res), (".tsv",), (".tsv.gz",), message)


def write_motif_length_summary(output_file: str, res) -> None:
    """``motif_length_summary_text`` to ``output_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "summary_file should have .tsv or .tsv.gz as suffix"
    if not output_file.endswith(MOTIF_LENGTH_SUFFIXES):
        raise ValueError(message)
    _emit(output_file, motif_length_summary_text(res), (".tsv",), (".tsv.gz",), message)


COFRAG_TRACK_HEADER ="contig\tstart\tstop\tn_frags\toverflow\tvalid\tpc1\n"
COFRAG_PAIRS_HEADER = "contig\tstart_i\tstart_j\tn_i\tn_j\tks_num\td\tat\tz\tneglog10_p\tcorr\n"


def cofrag_track_text(results) -> str:
    """The bins of ``utils.CoFragmentation`` results, contig by contig: the header ``contig start stop n_frags overflow
    valid pc1``, ``valid`` as 0 / 1, ``pc1`` as ``repr(float)`` (``nan`` at a bin that is not valid)."""
    rows = [COFRAG_TRACK_HEADER]
    for r in results:
        rows += [f"{r.contig}\t{int(a)}\t{int(b)}\t{int(n)}\t{int(o)}\t{int(v)}\t{float(p)!r}\n"
                 for a, b, n, o, v, p in zip(r.starts, r.stops, r.n, r.overflow, r.valid, r.pc1)]
    return "".join(rows)


def cofrag_pairs_text(results) -> str:
    """The bin pairs ``i < j`` of ``utils.CoFragmentation`` results, row-major: the header ``contig start_i start_j n_i n_j
    ks_num d at z neglog10_p corr``; the floats as ``repr(float)``, ``nan`` where a bin of the pair is not valid."""
    rows = [COFRAG_PAIRS_HEADER]
    for r in results:
        for i in range(len(r.n)):
            rows += [f"{r.contig}\t{int(r.starts[i])}\t{int(r.starts[j])}\t{int(r.n[i])}\t{int(r.n[j])}\t{int(r.K[i, j])}\t"
                     f"{float(r.D[i, j])!r}\t{int(r.at[i, j])}\t{float(r.z[i, j])!r}\t{float(r.neglog10_p[i, j])!r}\t"
                     f"{float(r.corr[i, j])!r}\n" for j in range(i + 1, len(r.n))]
    return "".join(rows)


def write_cofrag_track(output_file: str, results) -> None:
    """``cofrag_track_text`` to ``output_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "output_file should have .tsv or .tsv.gz as suffix"
    check_suffix(output_file, (".tsv", ".tsv.gz"), message)
    _emit(output_file, cofrag_track_text(results), (".tsv",), (".tsv.gz",), message)


def write_cofrag_pairs(pairs_file: str, results) -> None:
    """``cofrag_pairs_text`` to ``pairs_file``: ``.tsv`` as text, ``.tsv.gz`` as gzip."""
    message = "pairs_file should have .tsv or .tsv.gz as suffix"
    check_suffix(pairs_file, (".tsv", ".tsv.gz"), message)
    _emit(pairs_file, cofrag_pairs_text(results), (".tsv",), (".tsv.gz",), message)
