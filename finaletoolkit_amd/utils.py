"""
Host-side helpers of the hot path with the reference's names and semantics
(``src/finaletoolkit/utils/utils.py`` and ``utils/_frag_generator.py``):
chrom.sizes / BED readers, ``overlaps``, and the fragment stream
(``frag_generator`` / ``frag_array``), which here is a device-side ordered
selection (``ftk_frag_select``) instead of a per-row Python predicate.
"""
from __future__ import annotations

import itertools
from pathlib import Path
from typing import Generator, NamedTuple, Tuple

import numpy as np

from .exceptions import InvalidInputError
from .source import get_engine, open_source

__all__ = ["chrom_sizes_to_list", "chrom_sizes_to_dict", "get_intervals", "overlaps", "frags_in_region", "frag_generator",
           "frag_array", "frag_export", "frag_filter", "frag_gc_coverage", "frag_site_profile", "frag_vplot", "VPlot", "frag_ocf", "OCF", "frag_wps_spectrum", "WpsSpectrum", "frag_wps_peaks", "WpsPeaks", "frag_preferred_ends", "PreferredEnds", "preferred_end_thresholds", "frag_hotspots", "IfsHotspots", "ifs_thresholds", "frag_end_context", "EndContext", "frag_motif_lengths", "MotifLengths", "read_sites", "gc_weights", "read_gc_bias_table", "read_region_mask", "agg_bw", "gen_kmers", "reverse_complement", "validate_compatible_contigs", "valid_interval",
           "_none_eq", "_none_geq", "_none_leq"]

FragTuple = Tuple[str, int, int, int, bool]


def chrom_sizes_to_list(chrom_sizes_file) -> list[tuple[str, int]]:
    """utils/utils.py:53-73."""
    out = []
    with open(chrom_sizes_file, "r") as fh:
        for line in fh:
            if line != "\n":
                chrom, size = line.strip().split("\t")
                out.append((chrom, int(size)))
    return out


def chrom_sizes_to_dict(chrom_sizes_file) -> dict[str, int]:
    """utils/utils.py:76-94."""
    return dict(chrom_sizes_to_list(chrom_sizes_file))


def get_intervals(interval_file) -> list[tuple[str, int, int, str]]:
    """BED reader (utils/utils.py:310-343): skips ``#``/``track``/``browser``/blank
    lines and rows with < 3 columns; missing name -> ``'.'``."""
    intervals = []
    with open(interval_file, "r") as bed:
        for line in bed:
            if line.startswith(("#", "track", "browser")) or not line.strip():
                continue
            parts = line.strip().split("\t")
            if len(parts) < 3:
                continue
            intervals.append((parts[0], int(parts[1]), int(parts[2]), parts[3] if len(parts) > 3 else "."))
    return intervals


def overlaps(contigs_1, starts_1, stops_1, contigs_2, starts_2, stops_2):
    """Does each interval of set 1 overlap any interval of set 2 on the same
    contig?  (utils/utils.py:346-382; grouped by contig instead of an
    n1 x n2 broadcast.)"""
    contigs_1 = np.asarray(contigs_1)
    starts_1 = np.asarray(starts_1)
    stops_1 = np.asarray(stops_1)
    contigs_2 = np.asarray(contigs_2)
    starts_2 = np.asarray(starts_2)
    stops_2 = np.asarray(stops_2)
    out = np.zeros(contigs_1.shape[0], dtype=bool)
    for c in np.unique(contigs_1):
        m1 = contigs_1 == c
        m2 = contigs_2 == c
        if not m2.any():
            continue
        s1 = starts_1[m1][:, None]
        e1 = stops_1[m1][:, None]
        out[m1] = np.any((s1 < stops_2[m2][None]) & (e1 > starts_2[m2][None]), axis=1)
    return out


def gen_kmers(k: int, bases: str = "ACGT") -> list[str]:
    """All ``len(bases)**k`` k-mers in lexicographic order (utils/utils.py:388-410)."""
    if k < 0:
        raise ValueError("k must be non-negative")
    return ["".join(t) for t in itertools.product(bases, repeat=k)]


def frags_in_region(frag_array, start: int, stop: int):
    """Rows of a ``frag_array`` result with ``start < stop_`` and ``stop >= start_`` (utils/utils.py:160-183;
    note the inclusive lower test)."""
    keep = (frag_array["start"] < stop) & (frag_array["stop"] >= start)
    return frag_array[keep]


def _check_policy(intersect_policy: str):
    if intersect_policy not in ("midpoint", "any"):
        raise InvalidInputError(f"{intersect_policy} is not a valid policy")


def _check_region(contig, start, stop):
    # utils/_frag_generator.py:105-110
    if contig is None and not (start is None and stop is None):
        if not (start == 0 and stop is None):
            raise InvalidInputError("contig should be specified if start or stop given.")


def _region_contigs(src, contig):
    """Contigs a fetch(contig, ...) touches, in file order, with their bounds
    semantics: ``contig=None`` iterates the whole file and pysam ignores
    start/stop (io/alignment.py:245,273-279)."""
    if contig is None:
        src.load_all()
        return [c for c in src.contigs if c in src.loaded], True
    return [contig], False


def frag_generator(input_file, contig, quality_threshold: int = 30, start=None, stop=None, min_length=None,
                   max_length=None, intersect_policy: str = "midpoint", verbose=False,
                   reference_file=None) -> Generator[FragTuple, None, None]:
    """Stream ``(contig, start, stop, mapq, is_forward)`` of the fragments
    passing the shared predicate (utils/_frag_generator.py:58-141)."""
    _check_policy(intersect_policy)
    _check_region(contig, start, stop)
    src = open_source(input_file)
    src.check_fetch(contig, start, stop)
    eng = get_engine()
    names, whole = _region_contigs(src, contig)
    for c in names:
        key = src.require(c)
        s, e, q, st = eng.frag_select(key, None if whole else start, None if whole else stop, quality_threshold,
                                      min_length, max_length, intersect_policy)
        for i in range(len(s)):
            yield (c, int(s[i]), int(e[i]), int(q[i]), bool(st[i]))


def frag_array(input_file, contig: str, quality_threshold: int = 30, start=None, stop=None, min_length=None,
               max_length=None, intersect_policy: str = "midpoint", verbose: bool = False, reference_file=None):
    """Structured ``[('start','i8'),('stop','i8'),('strand','?')]`` array of the
    passing fragments (utils/utils.py:186-255)."""
    _check_policy(intersect_policy)
    _check_region(contig, start, stop)
    src = open_source(input_file)
    src.check_fetch(contig, start, stop)
    eng = get_engine()
    names, whole = _region_contigs(src, contig)
    parts = []
    for c in names:
        s, e, _, st = eng.frag_select(src.require(c) if whole else src.require_interval(c, start, stop, 1), None if whole else start, None if whole else stop,
                                      quality_threshold, min_length, max_length, intersect_policy)
        a = np.zeros(len(s), dtype=[("start", "i8"), ("stop", "i8"), ("strand", "?")])
        a["start"], a["stop"], a["strand"] = s, e, st.astype(bool)
        parts.append(a)
    if not parts:
        return np.zeros(0, dtype=[("start", "i8"), ("stop", "i8"), ("strand", "?")])
    return np.concatenate(parts)


_EXPORT_LAYOUTS = ("frag", "bed6", "bed3")


COORD_BOUND = 1 << 30  # the project's coordinate bound (a contig's columns hold values below it)


def read_region_mask(bed_file) -> dict:
    """A whitelist / blacklist BED (plain or gzip; the first three columns) as ``{contig: (starts int32[], ends
    int32[])}``, sorted, with overlapping intervals merged - neither intersect policy can tell the merged set from the
    given one (``merge_intervals``; touching intervals stay apart).  Blank lines and lines that start with ``#``, ``track`` or ``browser`` are skipped; a row
    with fewer than three columns, a coordinate that is no integer, ``start < 0``, ``stop <= start`` or ``stop >
    2**30`` is a ``ValueError`` that names the file and the line."""
    import gzip
    import os
    path = os.fspath(bed_file)
    with open(path, "rb") as fh:
        zipped = fh.read(2) == b"\x1f\x8b"
    per = {}
    with (gzip.open if zipped else open)(path, "rt") as fh:
        for no, line in enumerate(fh, 1):
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            parts = line.split()
            if len(parts) < 3:
                raise ValueError(f"{path}, line {no}: a BED row needs three columns, found {len(parts)}")
            try:
                a, b = int(parts[1]), int(parts[2])
            except ValueError:
                raise ValueError(f"{path}, line {no}: coordinates {parts[1]!r}, {parts[2]!r} are not integers") from None
            if a < 0:
                raise ValueError(f"{path}, line {no}: start {a} < 0")
            if b <= a:
                raise ValueError(f"{path}, line {no}: stop {b} <= start {a}")
            if b > COORD_BOUND:
                raise ValueError(f"{path}, line {no}: stop {b} > 2**30, the coordinate bound")
            per.setdefault(parts[0], []).append((a, b))
    return {c: merge_intervals(*zip(*iv)) for c, iv in per.items()}


def merge_intervals(starts, ends):
    """``(starts, ends)`` int32, sorted by start, OVERLAPPING intervals made one: sorted and disjoint.  Intervals that
    only touch (``[a, b)``, ``[b, c)``) stay two: under the ``any`` policy a zero-length fragment ``[b, b)`` is in
    neither of them (``b > a and b < b`` fails, so does ``b > b``) but would be in ``[a, c)``; every other fragment,
    and every fragment under ``midpoint``, is in the one exactly when it is in one of the two."""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    if len(s) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    o = np.argsort(s, kind="stable")
    s, e = s[o], np.maximum.accumulate(e[o])
    first = np.concatenate(([True], s[1:] >= e[:-1]))  # opens a run: starts at or behind the end of everything in front
    last = np.concatenate((first[1:], [True]))
    return s[first].astype(np.int32), e[last].astype(np.int32)


def _check_export_args(input_file, output_file, layout) -> str:
    import os

    from . import writers
    output_file = os.fspath(output_file)
    writers.check_suffix(output_file, (".gz", ".bgz"), "output_file should have .gz or .bgz as suffix")
    if output_file == "-":
        raise ValueError("output_file should have .gz or .bgz as suffix")
    if layout not in _EXPORT_LAYOUTS:
        raise ValueError(f"layout must be one of {_EXPORT_LAYOUTS}, not {layout!r}")
    if os.path.abspath(os.fspath(input_file)) == os.path.abspath(output_file) or (
            os.path.exists(output_file) and os.path.exists(os.fspath(input_file)) and os.path.samefile(input_file, output_file)):
        raise ValueError("input_file and output_file are the same file")
    return output_file


def _one_or_all(contig) -> dict:
    """The ``ContigFeed`` arguments of a command that takes ``contig=None`` (every contig of the file) or one name, which
    the file must then hold: the ``ValueError`` of every other command otherwise."""
    return {} if contig is None else dict(names=[str(contig)], require=[str(contig)])


def _export(label, input_file, output_file, contig, quality_threshold, min_length, max_length, layout, workers, verbose,
            whitelist=None, blacklist=None, intersect_policy="midpoint") -> dict:
    """The body of ``frag_export`` and ``frag_filter`` (arguments checked by the caller): every contig of the feed goes
    through ``Engine.write_contig``; ``whitelist`` / ``blacklist`` are ``read_region_mask`` results or ``None``."""
    import sys
    import time

    from . import bgzf
    from .engine import RegionMask
    from .source import ContigFeed
    t0 = time.time()
    eng = get_engine()
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    written, index, first = {}, [], True
    with ContigFeed(input_file, workers, **_one_or_all(contig)) as feed:
        for src, c in feed:
            mask = None
            if whitelist is not None or blacklist is not None:
                mask = RegionMask(None if whitelist is None else whitelist.get(c, none),
                                  None if blacklist is None else blacklist.get(c), intersect_policy)
            res = eng.write_contig(src.key(c), c, output_file, quality_threshold, min_length, max_length, layout,
                                   append=not first, mask=mask)
            first = False
            written[c] = res["rows"]
            index.append(dict(name=c, v_begin=res["first_off"] << 16, v_end=res["end_off"] << 16, rows=res["rows"],
                              linear=res["linear"], runs=res["runs"]))
            if verbose:
                sys.stderr.write(f"{label}: {c}: {res['rows']} rows, {res['text_bytes']} bytes of text -> "
                                 f"{res['end_off'] - res['first_off']} bytes\n")
    with open(output_file, "ab" if not first else "wb") as fh:
        fh.write(bgzf._EOF)
    bgzf.write_tabix(output_file + ".tbi", index)
    if verbose:
        sys.stderr.write(f"{label}: {sum(written.values())} rows in {time.time() - t0:.3f} s\n")
    return written


def frag_export(input_file, output_file, contig=None, quality_threshold: int = 30, min_length=None, max_length=None,
                layout: str = "frag", workers=None, verbose=False) -> dict:
    """Write the fragments of ``input_file`` (BAM, or a fragment file / BED6) that pass ``mapq >= quality_threshold``
    and ``min_length <= length <= max_length`` as a tabix-indexed BGZF file ``output_file`` (+ ``.tbi``): rows
    ``contig start end mapq strand`` (``layout="frag"``), with a ``.`` name column (``"bed6"``) or ``contig start
    end`` alone (``"bed3"``), sorted by start within a contig, contigs in the order of the input.  Rows are formatted
    and deflated on the GPU, contig by contig as the input is decoded (``ftk_frags_write``).  Returns
    ``{contig: rows written}`` for the contigs visited (``contig``: that one alone)."""
    output_file = _check_export_args(input_file, output_file, layout)
    return _export("frag_export", input_file, output_file, contig, quality_threshold, min_length, max_length, layout,
                   workers, verbose)


def frag_filter(input_file, output_file, whitelist_file=None, blacklist_file=None, intersect_policy: str = "midpoint",
                contig=None, quality_threshold: int = 30, min_length=None, max_length=None, layout: str = "frag",
                workers=None, verbose=False) -> dict:
    """``frag_export`` with region masks: a fragment is written when it passes the MAPQ / length rule, is IN
    ``whitelist_file`` (a BED; if given) and is NOT in ``blacklist_file`` (if given).  A fragment is in a BED when one
    of its intervals ``[r_start, r_stop)`` on the fragment's contig holds ``frag_generator``'s own rule for
    ``intersect_policy``: ``"midpoint"``: ``r_start <= (start + stop) // 2 < r_stop``; ``"any"``: ``stop > r_start
    and start < r_stop``.  One policy serves both masks.  Rows are whole fragments, each written at most once, in the
    order ``frag_export`` writes them (this is not bedtools' ``-f 0.5`` clipping of the reference's ``filter_file``).
    The mask test is a kernel in front of the device formatter (``ftk_frags_write_masked``).  Every contig of the
    input is visited; one the whitelist does not name yields 0 rows.  Returns ``{contig: rows written}``; with both
    masks ``None`` the file and its index are ``frag_export``'s byte for byte."""
    output_file = _check_export_args(input_file, output_file, layout)
    _check_policy(intersect_policy)
    whitelist = None if whitelist_file is None else read_region_mask(whitelist_file)
    blacklist = None if blacklist_file is None else read_region_mask(blacklist_file)
    return _export("frag_filter", input_file, output_file, contig, quality_threshold, min_length, max_length, layout,
                   workers, verbose, whitelist, blacklist, intersect_policy)


_DEPTH_PLAIN, _DEPTH_GZ = (".bedgraph", ".bg"), (".bedgraph.gz", ".bg.gz")


def frag_depth(input_file, contig, start=None, stop=None, quality_threshold: int = 30, min_length=None, max_length=None,
               workers=None) -> np.ndarray:
    """Per-base depth of ``contig:[start, stop)``: an int32 array with, for every base, the number of fragments with
    ``frag_start <= base < frag_stop`` that pass ``mapq >= quality_threshold`` and ``min_length <= length <=
    max_length`` (``ftk_depth``).  ``start=None``: 0.  ``stop=None``: the contig length of the BAM header, or for a
    fragment file (whose index holds no lengths) the largest fragment end.  With both bounds given, a fragment file
    is read through its index for the interval alone (``FragSource.require_interval``); a BAM is decoded for the
    whole contig, because its index finds fragments by their read1 and a fragment can cover a base of the interval
    while its read1 lies outside it."""
    contig = str(contig)
    a = 0 if start is None else int(start)
    if a < 0 or (stop is not None and int(stop) < a):
        raise ValueError(f"invalid coordinates: start ({a}), stop ({stop})")
    src = open_source(input_file, workers)
    eng = get_engine()
    if stop is None or src.is_bam:
        key = src.require(contig)
        b = int(stop) if stop is not None else (src.lengths.get(contig) or eng.info(key)[2])
    else:
        b = int(stop)
        key = src.require_interval(contig, a, b)
    return eng.depth(key, a, max(a, b), quality_threshold, min_length, max_length)


def frag_depth_track(input_file, output_file, contig=None, quality_threshold: int = 30, min_length=None, max_length=None,
                     include_zero: bool = False, workers=None, verbose=False) -> dict:
    """Write the depth track of ``input_file`` (see ``frag_depth``) as bedGraph rows ``contig start end depth``, one
    per maximal interval of constant depth, for every contig in the order of the file (``contig``: that one alone;
    with ``include_zero`` the rows of a contig wait in host memory until every contig in front of it has been
    written).  The intervals are built on the GPU (``ftk_depth_runs``), contig by contig as the input is decoded, and only they
    come back to the host.  ``output_file`` ends in ``.bedgraph`` / ``.bg`` (text) or ``.bedgraph.gz`` / ``.bg.gz``
    (gzip).  Intervals of depth 0 are left out (``genomecov -bg``) unless ``include_zero`` (``-bga``), which makes the
    rows tile each contig.  A contig spans ``[0, length)`` with the length of the BAM header, or up to its largest
    fragment end for a fragment file; one without kept fragments writes nothing, or one row of depth 0 with
    ``include_zero`` when its length is known.  Returns ``n_runs`` (rows written), ``n_fragments`` (fragments that
    pass the MAPQ / length rule), ``bases_covered`` (bases of depth > 0) and ``max_depth``."""
    import os
    import sys
    import time

    from . import writers
    from .source import ContigFeed
    output_file = os.fspath(output_file)
    zipped = output_file.endswith(_DEPTH_GZ)
    if not zipped and not output_file.endswith(_DEPTH_PLAIN):
        raise ValueError("output_file should have .bedgraph, .bg, .bedgraph.gz or .bg.gz as suffix")
    level = writers.GZIP_LEVEL if zipped else 0
    t0 = time.time()
    eng = get_engine()
    out = dict(n_runs=0, n_fragments=0, bases_covered=0, max_depth=0)
    state = dict(first=True, next=0)
    pending = {}  # include_zero: rows of contigs that became resident ahead of an earlier contig of the file

    def emit(text):
        with text:
            text.write(output_file, level, append=not state["first"], threads=workers or 0)
        state["first"] = False

    def flush(src, everything):
        # Contigs with fragments become resident in file order; the ones a BAM header lists without a single
        # fragment only once the file has been read.  Without include_zero those write nothing, so rows go out as
        # they arrive; with it every contig of the header has a row, and rows wait for the contigs in front of them.
        names = src.contigs if contig is None else [str(contig)]
        while state["next"] < len(names) and (names[state["next"]] in pending or everything):
            text = pending.pop(names[state["next"]], None)
            if text is not None:
                emit(text)
            state["next"] += 1

    with ContigFeed(input_file, workers, **_one_or_all(contig)) as feed:
        for src, c in feed:
            key = src.key(c)
            length = src.lengths.get(c)
            rs, re_, rd = eng.depth_runs(key, 0, length or eng.info(key)[2], quality_threshold, min_length, max_length,
                                         include_zero)
            if not length and not rd.any():  # nothing kept and no length to span: no row
                rs, re_, rd = rs[:0], re_[:0], rd[:0]
            text = writers.bedgraph_runs(c, rs, re_, rd, workers or 0)
            if include_zero:
                pending[c] = text
                flush(src, False)
            else:
                emit(text)
            kept = int(eng.window_counts(key, [None], [None], quality_threshold, min_length, max_length)[0])
            out["n_runs"] += len(rs)
            out["n_fragments"] += kept
            out["bases_covered"] += int((re_ - rs)[rd > 0].sum(dtype=np.int64))
            out["max_depth"] = max(out["max_depth"], int(rd.max()) if len(rd) else 0)
            if verbose:
                sys.stderr.write(f"frag_depth_track: {c}: {kept} fragments, {len(rs)} runs\n")
        flush(feed.finish(), True)
    if state["first"]:
        writers.write_text(output_file, b"", level)
    if verbose:
        sys.stderr.write(f"frag_depth_track: {out['n_runs']} runs in {time.time() - t0:.3f} s\n")
    return out


class GCBias(NamedTuple):
    """Result of ``frag_gc_bias``: tables of shape ``(max_length - min_length + 1, max_length + 1)``, row
    ``L - min_length``, column ``g`` = G + C bases."""
    min_length: int
    max_length: int
    observed: np.ndarray   # int64: fragments of length L with g G + C bases
    expected: np.ndarray   # int64: reference windows of length L with g G + C bases
    bias: np.ndarray       # float64: (observed / observed.sum()) / (expected / expected.sum())
    n_fragments: int       # observed.sum()
    n_skipped: int         # fragments of those lengths without a GC count (off the contig, or over an N)
    skipped_contigs: tuple  # contigs of the input the reference does not hold


def gc_bias_ratio(observed, expected) -> np.ndarray:
    """``(observed / observed.sum()) / (expected / expected.sum())`` in float64: NaN where ``expected == 0``, all NaN
    when either table sums to 0."""
    obs = np.asarray(observed, dtype=np.float64)
    exp = np.asarray(expected, dtype=np.float64)
    if obs.shape != exp.shape:
        raise ValueError("observed and expected differ in shape")
    bias = np.full(obs.shape, np.nan)
    so, se = obs.sum(), exp.sum()
    if so > 0 and se > 0:
        ok = exp > 0
        bias[ok] = (obs[ok] / so) / (exp[ok] / se)
    return bias


def _check_gc_bias_args(output_file, min_length, max_length, stride, expected):
    from . import _lib as L
    from . import writers
    if int(min_length) < 1 or int(max_length) < int(min_length) or int(max_length) > L.GC_MAX_LEN:
        raise ValueError(f"invalid lengths: 1 <= min_length ({min_length}) <= max_length ({max_length}) <= {L.GC_MAX_LEN} is required")
    if int(stride) < 1:
        raise ValueError(f"invalid stride ({stride}): at least 1")
    shape = (int(max_length) - int(min_length) + 1, int(max_length) + 1)
    if expected is not None:
        expected = np.asarray(expected)
        if expected.shape != shape or expected.dtype.kind not in "iu":
            raise ValueError(f"expected should be an integer array of shape {shape}")
        expected = expected.astype(np.int64)
    if output_file is not None and not str(output_file).endswith(writers.GC_BIAS_SUFFIXES):
        raise ValueError("output_file should have .tsv or .tsv.gz as suffix")
    return shape, expected


def _over_reference_contigs(label, input_file, reference_file, contig, workers, verbose, one_contig) -> tuple:
    """The walk ``frag_gc_bias`` and ``frag_end_context`` share: every contig of the input (``contig``: that one alone,
    which the file must hold) that ``reference_file`` holds too, handed to ``one_contig(engine, key, image id, name,
    size) -> note`` as it becomes resident, its reference image resident with its layout; ``note`` ends the contig's
    verbose line.  Contigs the reference lacks are skipped with one ``UserWarning`` and returned."""
    import sys
    import warnings

    from .reference import ReferenceGenome
    from .source import ContigFeed
    eng = get_engine()
    missing = []
    with ContigFeed(input_file, workers, **_one_or_all(contig)) as feed, ReferenceGenome(reference_file) as ref:
        for src, c in feed:
            if c not in ref.chroms:
                missing.append(c)
                continue
            note = one_contig(eng, src.key(c), ref.device_image(eng, c, with_layout=True), c, ref.chroms[c])
            if verbose:
                sys.stderr.write(f"{label}: {c}: {note}\n")
    if missing:
        warnings.warn(f"{label}: contigs not in the reference were skipped: " + ", ".join(missing), UserWarning)
    return tuple(missing)


def frag_gc_bias(input_file, reference_file, output_file=None, contig=None, min_length: int = 100, max_length: int = 220,
                 quality_threshold: int = 30, stride: int = 1, expected=None, workers=None, verbose=False) -> GCBias:
    """Fragment length x GC bias of ``input_file`` against ``reference_file`` (``.2bit`` or FASTA), the measurement of
    deepTools ``computeGCBias``, Griffin and GCparagon, counted on the GPU contig by contig as the input is decoded.

    ``observed[L - min_length, g]``: fragments with ``mapq >= quality_threshold`` and length ``L`` in ``[min_length,
    max_length]`` whose reference span ``[start, end)`` holds ``g`` G / C bases (either case).  ``expected[...]``:
    positions ``p`` of every contig with ``p % stride == 0`` whose window ``[p, p + L)`` holds ``g``.  A span or window
    that leaves the contig or holds an N (2bit: the record's N blocks; FASTA: any base but ACGTacgt) counts nowhere;
    such fragments are ``n_skipped``.  ``bias = (observed / observed.sum()) / (expected / expected.sum())``, NaN where
    ``expected == 0``.  ``max_length`` is at most 1000.

    ``stride``: the expected table samples every ``stride``-th position; at ``stride=1`` it takes every window of
    every contig (see ``docs/experiments.md`` for what that costs).  ``expected``: an int64 table of the right shape
    to use instead, e.g. an earlier result's ``.expected`` - it depends only on the reference, the lengths and the
    stride.  Contigs of the input that the reference lacks are skipped with one ``UserWarning`` and listed in
    ``skipped_contigs``.  ``output_file`` (``.tsv`` / ``.tsv.gz``): ``length gc observed expected bias`` rows of the
    cells with ``observed > 0 or expected > 0``.

    Per-fragment weights ``1 / bias[L - min_length, g]`` and the GC-corrected coverage of intervals they give:
    ``frag_gc_coverage`` (which takes this result, or its TSV, as ``bias``); ``gc_weights`` turns the bias table into the
    weight table ``Engine.set_gc_weights`` attaches to a resident contig."""
    import os
    import sys
    import time

    from . import writers
    shape, given = _check_gc_bias_args(output_file, min_length, max_length, stride, expected)
    lo, hi, stride = int(min_length), int(max_length), int(stride)
    t0 = time.time()
    observed = np.zeros(shape, np.int64)
    exp_sum = np.zeros(shape, np.int64) if given is None else given
    n_skipped = 0

    def one_contig(eng, key, rid, name, size):
        nonlocal n_skipped
        table, skipped = eng.frag_gc_table(key, rid, lo, hi, quality_threshold)
        observed[...] += table
        n_skipped += skipped
        if given is None:
            exp_sum[...] += eng.ref_gc_table(rid, 0, size, lo, hi, stride)
        return f"{int(table.sum())} fragments, {skipped} skipped"
    missing = _over_reference_contigs("frag_gc_bias", input_file, reference_file, contig, workers, verbose, one_contig)
    res = GCBias(lo, hi, observed, exp_sum, gc_bias_ratio(observed, exp_sum), int(observed.sum()), int(n_skipped), missing)
    if output_file is not None:
        writers.write_gc_bias_table(os.fspath(output_file), lo, res.observed, res.expected, res.bias)
    if verbose:
        sys.stderr.write(f"frag_gc_bias: {res.n_fragments} fragments in {time.time() - t0:.3f} s\n")
    return res


def _check_min_bias(min_bias):
    if not float(min_bias) >= 2.0 ** -15:
        raise ValueError(f"invalid min_bias ({min_bias}): at least 2**-15")


def gc_weights(bias, min_bias: float = 0.05) -> np.ndarray:
    """The weight table of a bias table (a ``GCBias`` or a float array): uint32 in units of 2^-16, ``floor(65536 / bias +
    0.5)`` per cell, 0 where the bias is NaN or below ``min_bias`` (a cell with hardly any observed fragments would
    otherwise give each of them a huge weight).  ``min_bias`` is at least 2^-15, which keeps every weight within 2^31
    units."""
    _check_min_bias(min_bias)
    b = np.asarray(bias.bias if isinstance(bias, GCBias) else bias, dtype=np.float64)
    out = np.zeros(b.shape, np.uint32)
    ok = ~np.isnan(b) & (b >= float(min_bias))
    out[ok] = np.floor(65536.0 / b[ok] + 0.5).astype(np.uint32)
    return out


def read_gc_bias_table(path, min_length: int, max_length: int) -> GCBias:
    """The ``GCBias`` of a TSV written by ``frag_gc_bias`` / ``writers.write_gc_bias_table`` (``.gz``: gzip) for the
    lengths ``[min_length, max_length]``.  The file holds ``repr(float)`` of every bias, so the tables come back exactly;
    cells it does not list are ``0 / 0 / nan``.  A row of another length, or with more G + C than ``max_length``, raises
    ``ValueError``.  ``n_skipped`` is 0 and ``skipped_contigs`` empty: the file does not hold them."""
    import gzip
    import os
    lo, hi = int(min_length), int(max_length)
    if lo < 1 or hi < lo:
        raise ValueError(f"invalid lengths: 1 <= min_length ({min_length}) <= max_length ({max_length}) is required")
    shape = (hi - lo + 1, hi + 1)
    observed, expected, bias = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.full(shape, np.nan)
    path = os.fspath(path)
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        if head != ["length", "gc", "observed", "expected", "bias"]:
            raise ValueError(f"{path}: not a length x GC bias table (header {head})")
        for line in fh:
            if not line.strip():
                continue
            length, g, o, e, b = line.rstrip("\n").split("\t")
            length, g = int(length), int(g)
            if not (lo <= length <= hi and 0 <= g <= hi):
                raise ValueError(f"{path}: row length {length}, gc {g} lies outside the lengths [{lo}, {hi}]")
            observed[length - lo, g], expected[length - lo, g], bias[length - lo, g] = int(o), int(e), float(b)
    return GCBias(lo, hi, observed, expected, bias, int(observed.sum()), 0, ())


def _weight_table(input_file, reference_file, bias, lo, hi, quality_threshold, stride, min_bias, workers, verbose) -> np.ndarray:
    """``gc_weights`` of what a command was given as ``bias`` for the lengths ``[lo, hi]``: a ``GCBias``, the path of its TSV
    (``read_gc_bias_table``), or ``None`` - then ``frag_gc_bias`` of the input runs first with the same lengths, MAPQ cut
    and ``stride``, its warning about contigs the reference lacks left to the command, which reports them itself."""
    import warnings
    if bias is None:
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="frag_gc_bias: contigs not in the reference", category=UserWarning)
            bias = frag_gc_bias(input_file, reference_file, None, None, lo, hi, quality_threshold, stride, None, workers, verbose)
    elif not isinstance(bias, GCBias):
        bias = read_gc_bias_table(bias, lo, hi)
    return gc_weights(bias, min_bias)


class GCCoverage(NamedTuple):
    """Result of ``frag_gc_coverage``, one entry per interval of the interval file, in its order."""
    intervals: list           # (contig, start, stop, name)
    count: np.ndarray         # int64: fragments the interval counts (``frag.coverage``'s number)
    corrected: np.ndarray     # float64: the sum of their weights; NaN on a contig the reference lacks
    n_weighted: np.ndarray    # int64: those with a weight above 0
    n_zero: int               # fragments of the visited contigs that pass the MAPQ / length rule and got weight 0
    skipped_contigs: tuple    # contigs with intervals that the reference does not hold


_GC_COVERAGE_SUFFIXES = (".bed", ".bed.gz")


def _check_gc_coverage_args(output_file, bias, min_length, max_length, intersect_policy, min_bias, stride):
    _check_gc_bias_args(None, min_length, max_length, stride, None)
    _check_policy(intersect_policy)
    _check_min_bias(min_bias)
    if output_file is not None and not str(output_file).endswith(_GC_COVERAGE_SUFFIXES):
        raise ValueError("output_file should have .bed or .bed.gz as suffix")
    if isinstance(bias, GCBias) and (bias.min_length, bias.max_length) != (int(min_length), int(max_length)):
        raise ValueError(f"the bias table holds lengths [{bias.min_length}, {bias.max_length}], not "
                         f"[{min_length}, {max_length}]")


def frag_gc_coverage(input_file, reference_file, interval_file, output_file=None, bias=None, min_length: int = 100,
                     max_length: int = 220, quality_threshold: int = 30, intersect_policy: str = "midpoint",
                     min_bias: float = 0.05, stride: int = 1, workers=None, verbose=False) -> GCCoverage:
    """GC-bias-corrected fragment coverage of every interval of ``interval_file`` (BED): what Griffin, ichorCNA-style
    copy-number work and DELFI-style features start from, with the correction applied per FRAGMENT, so no bin-level
    LOESS is involved.

    Every fragment with ``mapq >= quality_threshold`` and a length ``L`` in ``[min_length, max_length]`` whose reference
    span holds ``g`` G / C bases weighs ``1 / bias[L - min_length, g]`` (``gc_weights``: rounded to units of 2^-16; 0
    where the bias is undefined or below ``min_bias``, and for a span that leaves the contig or holds an N).  Per
    interval, ``count`` is the number of such fragments the interval counts under ``intersect_policy`` (the number
    ``frag.coverage`` reports with the same arguments), ``corrected`` the sum of their weights and ``n_weighted`` how
    many of them weigh more than 0.  The weights are summed as integers on the GPU, contig by contig as the input is
    decoded (``Engine.set_gc_weights``, ``Engine.weighted_window_sums``), so ``corrected`` is exact and does not
    depend on the order of the fragments.

    ``bias``: a ``GCBias`` (from ``frag_gc_bias``), the path of its TSV (``read_gc_bias_table``), or ``None`` - then
    ``frag_gc_bias(input_file, reference_file, ...)`` runs first with the same lengths, MAPQ cut and ``stride``.  A
    ``GCBias`` of other lengths raises ``ValueError``.

    No further normalisation is applied.  With ``1 / bias`` of the SAME sample the weights of all fragments sum to
    ``n_fragments * (share of the expected windows whose cell has observed fragments)`` - each cell contributes
    ``observed * (expected / expected.sum()) / (observed / observed.sum())`` - so the mean weight is close to 1 and
    ``corrected`` stays on the scale of ``count``; it falls below 1 by the cells ``min_bias`` removes.

    Contigs with intervals that the reference lacks: one ``UserWarning``, their intervals keep their ``count`` and get
    ``corrected = nan``.  An interval on a contig the input lacks raises ``ValueError``, as in ``frag.coverage``.
    ``output_file`` (``.bed`` / ``.bed.gz``): rows ``contig start stop name count corrected`` in the interval file's
    order, ``corrected`` with six decimals or ``nan``."""
    import os
    import sys
    import time
    import warnings

    from . import _lib as L
    from . import writers
    from .reference import ReferenceGenome
    from .source import ContigFeed
    _check_gc_coverage_args(output_file, bias, min_length, max_length, intersect_policy, min_bias, stride)
    lo, hi = int(min_length), int(max_length)
    t0 = time.time()
    table = _weight_table(input_file, reference_file, bias, lo, hi, quality_threshold, stride, min_bias, workers, verbose)
    intervals = get_intervals(interval_file)
    by_contig: dict[str, list[int]] = {}
    for i, iv in enumerate(intervals):
        by_contig.setdefault(iv[0], []).append(i)
    starts = np.array([iv[1] for iv in intervals], dtype=np.int64)
    stops = np.array([iv[2] for iv in intervals], dtype=np.int64)
    count = np.zeros(len(intervals), np.int64)
    units = np.zeros(len(intervals), np.int64)
    n_weighted = np.zeros(len(intervals), np.int64)
    no_reference = np.zeros(len(intervals), bool)
    n_zero, missing, left = 0, [], dict(by_contig)
    eng = get_engine()
    # (require: contigs the file does not hold get the ValueError of frag.coverage)
    with ContigFeed(input_file, workers, names=list(by_contig), require=left) as feed, ReferenceGenome(reference_file) as ref:
        for src, c in feed:
            idx = left.pop(c, None)
            if idx is None:
                continue
            key = src.key(c)
            idx = np.asarray(idx, dtype=np.int64)
            order = idx[np.argsort(starts[idx], kind="stable")]
            ws, we = starts[order].astype(np.int32), stops[order].astype(np.int32)
            args = (quality_threshold, lo, hi, intersect_policy)
            count[order] = eng.window_counts(key, ws, we, *args)
            if c not in ref.chroms:
                missing.append(c)
                no_reference[order] = True
                continue
            rid = ref.device_image(eng, c, with_layout=True)
            zeros = eng.set_gc_weights(key, rid, lo, hi, table, quality_threshold)
            units[order], n_weighted[order] = eng.weighted_window_sums(key, ws, we, *args)
            n_zero += zeros
            if verbose:
                sys.stderr.write(f"frag_gc_coverage: {c}: {len(order)} intervals, {zeros} fragments of weight 0\n")
    if missing:
        warnings.warn("frag_gc_coverage: contigs not in the reference were not corrected: " + ", ".join(missing), UserWarning)
    corrected = units / float(L.WEIGHT_ONE)
    corrected[no_reference] = np.nan
    res = GCCoverage(intervals, count, corrected, n_weighted, int(n_zero), tuple(missing))
    if output_file is not None:
        writers.write_gc_coverage_rows(os.fspath(output_file), intervals, count, corrected)
    if verbose:
        sys.stderr.write(f"frag_gc_coverage: {len(intervals)} intervals in {time.time() - t0:.3f} s\n")
    return res


def read_sites(site_file) -> list[tuple[str, int, str, str]]:
    """``(contig, centre, name, strand)`` per row of a ``.bed`` / ``.bed.gz`` file of sites: the lines ``get_intervals``
    skips are skipped (``#`` / ``track`` / ``browser`` / blank lines, rows with < 3 columns); the centre is ``(start +
    stop) // 2``, the name column 4 or ``'.'``, the strand ``'-'`` only when column 6 is ``-``, else ``'+'``."""
    import gzip
    import os
    path = os.fspath(site_file)
    sites = []
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")) as bed:
        for line in bed:
            if line.startswith(("#", "track", "browser")) or not line.strip():
                continue
            parts = line.strip().split("\t")
            if len(parts) < 3:
                continue
            sites.append((parts[0], (int(parts[1]) + int(parts[2])) // 2, parts[3] if len(parts) > 3 else ".",
                          "-" if len(parts) > 5 and parts[5] == "-" else "+"))
    return sites


class SiteProfile(NamedTuple):
    """Result of ``frag_site_profile``: one row of ``2 * half_width // bin_size`` bins per group of sites."""
    groups: tuple             # names in order of first appearance (``by_name``), else ``("all",)``
    n_sites: np.ndarray       # int64 per group: the sites used (those on contigs that were not skipped)
    offsets: np.ndarray       # int64 per bin: its first offset from the site's centre, ``-half_width + k * bin_size``
    count: np.ndarray         # int64 (n_groups, n_bins): fragment midpoints
    corrected: np.ndarray     # float64 (n_groups, n_bins): the sum of their weights (``count`` without a reference)
    skipped_contigs: tuple    # contigs with sites that the input, or the reference, does not hold


SITE_PROFILE_MAX_BINS = 4096  # the bins one profile may have (``ftk_site_profile``)


def _check_site_profile_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, min_bias, stride):
    _check_suffix(output_file, "output_file", "tsv")
    half_width, bin_size = int(half_width), int(bin_size)
    if not 1 <= half_width <= 1 << 20:
        raise ValueError(f"invalid half_width ({half_width}): between 1 and 2**20")
    if bin_size < 1 or (2 * half_width) % bin_size:
        raise ValueError(f"invalid bin_size ({bin_size}): it should divide 2 * half_width = {2 * half_width}")
    if 2 * half_width // bin_size > SITE_PROFILE_MAX_BINS:
        raise ValueError(f"{2 * half_width // bin_size} bins: at most {SITE_PROFILE_MAX_BINS} (a larger bin_size, or a smaller half_width)")
    if reference_file is None:
        if bias is not None:
            raise ValueError("bias needs reference_file: without a reference the profile is not corrected")
        if min_length is not None and max_length is not None and int(min_length) > int(max_length):
            raise ValueError(f"invalid lengths: min_length ({min_length}) <= max_length ({max_length}) is required")
    else:
        _check_gc_coverage_args(None, bias, min_length, max_length, "midpoint", min_bias, stride)


def frag_site_profile(input_file, site_file, output_file=None, reference_file=None, bias=None, half_width: int = 1000,
                      bin_size: int = 1, min_length: int = 100, max_length: int = 220, quality_threshold: int = 30,
                      by_name: bool = False, normalize: bool = False, min_bias: float = 0.05, stride: int = 1, workers=None,
                      verbose=False) -> SiteProfile:
    """Fragment-midpoint profile around the sites of ``site_file`` (``.bed`` / ``.bed.gz``, ``read_sites``), aggregated
    over the sites and, with ``reference_file``, GC-corrected per fragment: the nucleosome profile Griffin computes around
    transcription-factor binding sites, TSSs or open chromatin.

    A fragment with ``mapq >= quality_threshold`` and a length in ``[min_length, max_length]`` whose midpoint ``(start +
    end) >> 1`` lies ``d`` in ``[-half_width, half_width)`` from a site's centre counts in bin ``(d + half_width) //
    bin_size`` of the site's group, counted from the other end for a site on the ``-`` strand, so that offsets run 5' to
    3' of the site.  ``bin_size`` divides ``2 * half_width`` and gives at most 4096 bins.  Sites are independent: a
    fragment near two sites counts for both.  ``by_name``: one group per name (column 4), in order of first appearance;
    else one group ``"all"``.  Every fragment of a contig is eligible - a BAM and the fragment file exported from it give
    the same profile.  The profile is accumulated as integers on the GPU, contig by contig as the input is decoded
    (``Engine.site_profile``), and summed over the contigs on the host, so it is exact.

    With ``reference_file`` (``.2bit`` / FASTA) every fragment weighs ``1 / bias[L - min_length, g]`` as in
    ``frag_gc_coverage`` (``gc_weights``, ``min_bias``); ``bias`` is a ``GCBias``, the path of its TSV, or ``None`` - then
    ``frag_gc_bias(input_file, reference_file, ...)`` runs first with the same lengths, MAPQ cut and ``stride``.  Without
    a reference ``bias`` must be ``None`` and ``corrected`` equals ``count``.  ``normalize``: every group's ``corrected``
    row is divided by its mean (a row whose mean is 0 stays 0).

    Contigs with sites that the input does not hold, and - when correcting - contigs that the reference does not hold,
    are skipped with one ``UserWarning`` each kind, listed in ``skipped_contigs`` and their sites left out of ``n_sites``.
    ``output_file`` (``.tsv`` / ``.tsv.gz``): ``writers.write_site_profile_rows``."""
    import os
    import sys
    import time

    from . import _lib as L
    from . import writers
    _check_site_profile_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, min_bias, stride)
    H, b = int(half_width), int(bin_size)
    n_bins = 2 * H // b
    t0 = time.time()

    def one_contig(eng, key, centre, flip, group, n_groups, weighted):
        return eng.site_profile(key, centre, flip, group, n_groups, H, b, quality_threshold, min_length, max_length, weighted=weighted)
    groups, n_sites, count, units, skipped, n_read = _sites_over_contigs(
        "frag_site_profile", one_contig, (n_bins,), input_file, site_file, reference_file, bias, min_length, max_length,
        quality_threshold, by_name, min_bias, stride, workers, verbose)
    corrected = units / float(L.WEIGHT_ONE)
    if normalize:
        mean = corrected.mean(axis=1, keepdims=True)
        corrected = np.divide(corrected, mean, out=np.zeros_like(corrected), where=mean != 0)
    res = SiteProfile(groups, n_sites, -H + b * np.arange(n_bins, dtype=np.int64), count, corrected, skipped)
    if output_file is not None:
        writers.write_site_profile_rows(os.fspath(output_file), res)
    if verbose:
        sys.stderr.write(f"frag_site_profile: {n_read} sites in {time.time() - t0:.3f} s\n")
    return res


def _sites_over_contigs(what, one_contig, cell_shape, input_file, site_file, reference_file, bias, min_length, max_length,
                        quality_threshold, by_name, min_bias, stride, workers, verbose, max_cells=None, per_site=None):
    """The driver ``frag_site_profile``, ``frag_vplot`` and ``frag_ocf`` share: the sites read and grouped, the bias table
    made ready, one ``ContigFeed`` pass with ``set_gc_weights`` per contig when there is a reference, ``one_contig(eng,
    key, centre, flip, group, n_groups, weighted) -> (sums, counts)`` of shape ``(n_groups,) + cell_shape`` per contig
    summed on the host, and the two warnings (named after ``what``).  ``max_cells``: the cells all groups together may
    have, checked once the site file has given the groups.  ``per_site``: a callable; ``one_contig`` may then return
    further per-site arrays behind ``(sums, counts)``, in the order of the sites it was given, and ``per_site(idx, *those)``
    is called once per visited contig with the indices of the contig's sites among the sites read - the sites of skipped
    contigs never get a call.  Returns ``(groups, n_sites, count, units, skipped_contigs, sites
    read)``."""
    import sys
    import warnings

    from .source import ContigFeed
    sites = read_sites(site_file)  # read and checked before the input is walked for anything
    if any(not 0 <= s[1] < COORD_BOUND for s in sites):
        raise ValueError(f"{site_file}: a site's centre lies outside [0, 2**30)")
    if max_cells is not None:
        n_groups = max(len({s[2] for s in sites}), 1) if by_name else 1
        if n_groups * int(np.prod(cell_shape)) > max_cells:
            raise ValueError(f"{n_groups} groups of {' x '.join(str(n) for n in cell_shape)} cells: at most {max_cells} cells in all")
    table = None
    if reference_file is not None:
        table = _weight_table(input_file, reference_file, bias, int(min_length), int(max_length), quality_threshold, stride,
                              min_bias, workers, verbose)
    names: dict[str, int] = {}
    if by_name:
        for s in sites:
            names.setdefault(s[2], len(names))
    groups = tuple(names) if by_name else ("all",)
    by_contig: dict[str, list[int]] = {}
    for i, s in enumerate(sites):
        by_contig.setdefault(s[0], []).append(i)
    centre = np.array([s[1] for s in sites], dtype=np.int64)
    flip = np.array([s[3] == "-" for s in sites], dtype=np.uint8)
    group = np.array([names[s[2]] if by_name else 0 for s in sites], dtype=np.int32)
    shape = (len(groups),) + tuple(cell_shape)
    count, units, n_sites = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(len(groups), np.int64)
    no_reference, left = [], dict(by_contig)
    if sites:
        from contextlib import nullcontext

        from .reference import ReferenceGenome
        eng = get_engine()
        with ContigFeed(input_file, workers, names=list(by_contig)) as feed, \
                (ReferenceGenome(reference_file) if table is not None else nullcontext()) as ref:
            for src, c in feed:
                idx = left.pop(c, None)
                if idx is None:
                    continue
                if ref is not None and c not in ref.chroms:
                    no_reference.append(c)
                    continue
                key = src.key(c)
                idx = np.asarray(idx, dtype=np.int64)
                if ref is not None:
                    rid = ref.device_image(eng, c, with_layout=True)
                    eng.set_gc_weights(key, rid, int(min_length), int(max_length), table, quality_threshold)
                sums, counts, *rest = one_contig(eng, key, centre[idx], flip[idx], group[idx], len(groups), ref is not None)
                if per_site is not None:
                    per_site(idx, *rest)
                units += sums
                count += counts
                n_sites += np.bincount(group[idx], minlength=len(groups))
                if verbose:
                    sys.stderr.write(f"{what}: {c}: {len(idx)} sites, {int(counts.sum())} {'midpoints' if per_site is None else 'ends'}\n")
    if left:
        warnings.warn(f"{what}: contigs not in the input were skipped: " + ", ".join(left), UserWarning)
    if no_reference:
        warnings.warn(f"{what}: contigs not in the reference were skipped: " + ", ".join(no_reference), UserWarning)
    return groups, n_sites, count, units, tuple(left) + tuple(no_reference), len(sites)


class VPlot(NamedTuple):
    """Result of ``frag_vplot``: per group of sites, ``n_rows`` length rows of ``2 * half_width // bin_size`` offset bins."""
    groups: tuple             # names in order of first appearance (``by_name``), else ``("all",)``
    n_sites: np.ndarray       # int64 per group: the sites used (those on contigs that were not skipped)
    offsets: np.ndarray       # int64 per bin: its first offset from the site's centre, ``-half_width + k * bin_size``
    lengths: np.ndarray       # int64 per row: its first length, ``min_length + r * length_bin``
    count: np.ndarray         # int64 (n_groups, n_rows, n_bins): fragment midpoints
    corrected: np.ndarray     # float64 (n_groups, n_rows, n_bins): the sum of their weights (``count`` without a reference)
    skipped_contigs: tuple    # contigs with sites that the input, or the reference, does not hold


VPLOT_MAX_ROWS = 4096     # the length rows one matrix may have (``ftk_site_vplot``)
VPLOT_MAX_CELLS = 1 << 28  # groups x rows x bins of one call


def _check_vplot_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, length_bin, min_bias, stride):
    if min_length is None or max_length is None:
        raise ValueError("invalid lengths: min_length and max_length bound the length axis and cannot be None")
    _check_site_profile_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, min_bias, stride)
    lo, hi, lb = int(min_length), int(max_length), int(length_bin)
    if not 0 <= lo <= hi < 1 << 16:
        raise ValueError(f"invalid lengths: 0 <= min_length ({lo}) <= max_length ({hi}) < 2**16 is required")
    if lb < 1 or (hi - lo + 1) % lb:
        raise ValueError(f"invalid length_bin ({lb}): it should divide max_length - min_length + 1 = {hi - lo + 1}")
    if (hi - lo + 1) // lb > VPLOT_MAX_ROWS:
        raise ValueError(f"{(hi - lo + 1) // lb} length rows: at most {VPLOT_MAX_ROWS} (a larger length_bin, or a narrower range)")


def frag_vplot(input_file, site_file, output_file=None, reference_file=None, bias=None, half_width: int = 500, bin_size: int = 5,
               min_length: int = 50, max_length: int = 349, length_bin: int = 5, quality_threshold: int = 30,
               by_name: bool = False, normalize: bool = False, min_bias: float = 0.05, stride: int = 1, workers=None,
               verbose=False) -> VPlot:
    """V-plot around the sites of ``site_file`` (``.bed`` / ``.bed.gz``, ``read_sites``): fragment length against the
    midpoint's offset from the site, aggregated over the sites and, with ``reference_file``, GC-corrected per fragment.
    It shows whether the signal at a binding site comes from nucleosome-sized fragments flanking it or from short
    sub-nucleosomal ones sitting on the factor itself - what ``frag_site_profile``, with its one axis, cannot.

    A fragment with ``mapq >= quality_threshold`` and a length ``L`` in ``[min_length, max_length]`` whose midpoint
    ``(start + end) >> 1`` lies ``d`` in ``[-half_width, half_width)`` from a site's centre counts in row ``(L -
    min_length) // length_bin`` and column ``(d + half_width) // bin_size`` of the site's group - the column counted from
    the other end for a site on the ``-`` strand; the length axis is never reversed.  ``bin_size`` divides ``2 *
    half_width`` and gives at most 4096 bins; ``length_bin`` divides ``max_length - min_length + 1`` and gives at most
    4096 rows; groups x rows x bins is at most 2**28.  Sites, groups (``by_name``), skipped contigs, the bias (``bias``,
    ``min_bias``, ``stride``) and exactness are as in ``frag_site_profile``: one pass over the input, one
    ``Engine.site_vplot`` call per contig, summed on the host.  ``normalize``: every group's ``corrected`` matrix is
    divided by its mean (a matrix whose mean is 0 stays 0).  ``output_file`` (``.tsv`` / ``.tsv.gz``):
    ``writers.write_vplot_rows``."""
    import os
    import sys
    import time

    from . import _lib as L
    from . import writers
    _check_vplot_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, length_bin, min_bias, stride)
    H, b, lo, hi, lb = int(half_width), int(bin_size), int(min_length), int(max_length), int(length_bin)
    n_bins, n_rows = 2 * H // b, (hi - lo + 1) // lb
    t0 = time.time()

    def one_contig(eng, key, centre, flip, group, n_groups, weighted):
        return eng.site_vplot(key, centre, flip, group, n_groups, H, b, lo, hi, lb, quality_threshold, weighted=weighted)
    groups, n_sites, count, units, skipped, n_read = _sites_over_contigs(
        "frag_vplot", one_contig, (n_rows, n_bins), input_file, site_file, reference_file, bias, lo, hi, quality_threshold,
        by_name, min_bias, stride, workers, verbose, VPLOT_MAX_CELLS)
    corrected = units / float(L.WEIGHT_ONE)
    if normalize:
        mean = corrected.mean(axis=(1, 2), keepdims=True)
        corrected = np.divide(corrected, mean, out=np.zeros_like(corrected), where=mean != 0)
    res = VPlot(groups, n_sites, -H + b * np.arange(n_bins, dtype=np.int64), lo + lb * np.arange(n_rows, dtype=np.int64), count,
                corrected, skipped)
    if output_file is not None:
        writers.write_vplot_rows(os.fspath(output_file), res)
    if verbose:
        sys.stderr.write(f"frag_vplot: {n_read} sites in {time.time() - t0:.3f} s\n")
    return res


class OCF(NamedTuple):
    """Result of ``frag_ocf``: per group of sites the U / D end profiles and the OCF score, and every site's score."""
    groups: tuple               # names in order of first appearance (``by_name``), else ``("all",)``
    n_sites: np.ndarray         # int64 per group: the sites used (those on contigs that were not skipped)
    offsets: np.ndarray         # int64 per bin: its first offset from the site's centre, ``-half_width + k * bin_size``
    up_count: np.ndarray        # int64 (n_groups, n_bins): U ends (fragment starts), 5' to 3' of the sites
    down_count: np.ndarray      # int64 (n_groups, n_bins): D ends (last bases of the fragments)
    up_corrected: np.ndarray    # float64 (n_groups, n_bins): the sum of their weights (``up_count`` without a reference)
    down_corrected: np.ndarray  # float64 (n_groups, n_bins)
    windows_count: np.ndarray   # int64 (n_groups, 4): left_up, left_down, right_up, right_down summed over the group's sites
    ocf_count: np.ndarray       # int64 per group: (left_down - left_up) + (right_up - right_down) of ``windows_count``
    ocf: np.ndarray             # float64 per group: the same from the weighted sums (``ocf_count`` without a reference)
    site_ocf: np.ndarray        # float64 per site, in the site file's order; NaN for the sites of skipped contigs
    skipped_contigs: tuple      # contigs with sites that the input, or the reference, does not hold


OCF_MAX_CELLS = 1 << 28  # groups x 2 tracks x bins of one call


def _check_ocf_args(output_file, profile_file, site_output_file, reference_file, bias, half_width, bin_size, peak, flank, min_length,
                    max_length, min_bias, stride):
    _check_site_profile_args(output_file, reference_file, bias, half_width, bin_size, min_length, max_length, min_bias, stride)
    _check_suffix(profile_file, "profile_file", "tsv")
    _check_suffix(site_output_file, "site_output_file", "tsv")
    if peak is None or flank is None:
        raise ValueError("invalid windows: peak and flank cannot be None")
    H, p, w = int(half_width), int(peak), int(flank)
    if p < 1:
        raise ValueError(f"invalid peak ({p}): at least 1")
    if not 0 <= w < p:
        raise ValueError(f"invalid flank ({w}): 0 <= flank < peak = {p} is required")
    if p + w >= H:
        raise ValueError(f"invalid windows: peak + flank = {p + w} should be below half_width = {H}")


def frag_ocf(input_file, site_file, output_file=None, profile_file=None, site_output_file=None, reference_file=None, bias=None,
             half_width: int = 1000, bin_size: int = 1, peak: int = 60, flank: int = 10, min_length: int = 50, max_length: int = 350,
             quality_threshold: int = 30, by_name: bool = False, normalize: bool = False, min_bias: float = 0.05, stride: int = 1,
             workers=None, verbose=False) -> OCF:
    """Orientation-aware cfDNA fragmentation (OCF, Sun et al., Genome Research 2019) around the sites of ``site_file``
    (``.bed`` / ``.bed.gz``, ``read_sites``): where fragments END relative to tissue-specific open-chromatin centres.
    Upstream (U) and downstream (D) fragment ends pile up on opposite sides of an open site; their signed difference in
    two small windows at ``-peak`` and ``+peak`` is the tissue-of-origin score.

    A fragment ``[start, end)`` with ``mapq >= quality_threshold`` and a length in ``[min_length, max_length]`` has its U
    end on base ``start`` and its D end on base ``end - 1``.  Profile: an end ``d`` in ``[-half_width, half_width)`` from a
    site's centre counts in bin ``(d + half_width) // bin_size`` of ``up_count`` or ``down_count`` of the site's group.
    The profile is STRAND-AWARE, as in ``frag_site_profile``: for a site on the ``-`` strand the bins are counted from the
    other end and U and D change places, so that offsets run 5' to 3' of the site and "up" is upstream of it.  Score: per
    site, ``left_up`` / ``left_down`` are the U / D ends with ``d`` in ``[-peak - flank, -peak + flank]`` and ``right_up``
    / ``right_down`` those in ``[peak - flank, peak + flank]``, and ``OCF = (left_down - left_up) + (right_up -
    right_down)``.  Mirroring a site swaps left with right and U with D, which leaves the score as it is - it is
    strand-free, and so is a group's ``ocf``, the sum of its sites' scores.  ``0 <= flank < peak``, ``peak + flank <
    half_width``.  Everything is accumulated as integers on the GPU, contig by contig as the input is decoded
    (``Engine.site_ends``), and summed on the host, so it is exact.

    Sites, groups (``by_name``), skipped contigs (two ``UserWarning`` kinds), and the GC correction (``reference_file``,
    ``bias`` as a ``GCBias``, the path of its TSV or ``None``, ``min_bias``, ``stride``) are exactly as in
    ``frag_site_profile``; without a reference the corrected arrays equal the counts.  ``normalize``: both corrected
    tracks and ``ocf`` of a group are divided by the mean of the group's corrected profile over both tracks (a mean of 0
    leaves zeros).  ``site_ocf`` holds every site's score from the weighted sums, NaN for the sites of skipped contigs.

    Files (``.tsv`` / ``.tsv.gz``): ``output_file`` one row per group (``writers.write_ocf_rows``), ``profile_file`` the
    end profiles (``writers.write_end_profile_rows``), ``site_output_file`` one row per site
    (``writers.write_site_ocf_rows``)."""
    import os
    import sys
    import time

    from . import _lib as L
    from . import writers
    _check_ocf_args(output_file, profile_file, site_output_file, reference_file, bias, half_width, bin_size, peak, flank, min_length,
                    max_length, min_bias, stride)
    H, b, p, w = int(half_width), int(bin_size), int(peak), int(flank)
    n_bins = 2 * H // b
    t0 = time.time()
    sites = read_sites(site_file)  # (read again by the driver: the per-site arrays and the site file's rows need them here)
    site_units, site_count = np.zeros((len(sites), 4), np.int64), np.zeros((len(sites), 4), np.int64)
    seen = np.zeros(len(sites), bool)

    def one_contig(eng, key, centre, flip, group, n_groups, weighted):
        return eng.site_ends(key, centre, flip, group, n_groups, H, b, quality_threshold, min_length, max_length, weighted=weighted,
                             peak=p, flank=w)

    def per_site(idx, site_sums, site_counts):
        site_units[idx], site_count[idx], seen[idx] = site_sums, site_counts, True
    groups, n_sites, count, units, skipped, n_read = _sites_over_contigs(
        "frag_ocf", one_contig, (2, n_bins), input_file, site_file, reference_file, bias, min_length, max_length, quality_threshold,
        by_name, min_bias, stride, workers, verbose, OCF_MAX_CELLS, per_site)
    sign = np.array([-1, 1, 1, -1], np.int64)  # left_up, left_down, right_up, right_down
    site_score = (site_units * sign).sum(axis=1)
    site_ocf = site_score / float(L.WEIGHT_ONE)
    site_ocf[~seen] = np.nan
    names = {name: g for g, name in enumerate(groups)}
    group_of = np.array([names[s[2]] if by_name else 0 for s in sites], dtype=np.int64)
    windows_count, ocf_units = np.zeros((len(groups), 4), np.int64), np.zeros(len(groups), np.int64)
    np.add.at(windows_count, group_of[seen], site_count[seen])
    np.add.at(ocf_units, group_of[seen], site_score[seen])
    corrected = units / float(L.WEIGHT_ONE)
    ocf = ocf_units / float(L.WEIGHT_ONE)
    if normalize:
        mean = corrected.mean(axis=(1, 2), keepdims=True)
        corrected = np.divide(corrected, mean, out=np.zeros_like(corrected), where=mean != 0)
        ocf = np.divide(ocf, mean[:, 0, 0], out=np.zeros_like(ocf), where=mean[:, 0, 0] != 0)
    res = OCF(groups, n_sites, -H + b * np.arange(n_bins, dtype=np.int64), count[:, 0], count[:, 1], corrected[:, 0], corrected[:, 1],
              windows_count, (windows_count * sign).sum(axis=1), ocf, site_ocf, skipped)
    if output_file is not None:
        writers.write_ocf_rows(os.fspath(output_file), res)
    if profile_file is not None:
        writers.write_end_profile_rows(os.fspath(profile_file), res)
    if site_output_file is not None:
        writers.write_site_ocf_rows(os.fspath(site_output_file), sites, site_count, site_ocf)
    if verbose:
        sys.stderr.write(f"frag_ocf: {n_read} sites in {time.time() - t0:.3f} s\n")
    return res


class WpsSpectrum(NamedTuple):
    """Result of ``frag_wps_spectrum``, one row per interval of the interval file, in its order."""
    intervals: list           # (contig, start, stop, name)
    periods: np.ndarray       # int64: min_period .. max_period
    power: np.ndarray         # float64 (n_intervals, n_periods): (re^2 + im^2) / ssw; NaN for an empty interval
    band_mean: np.ndarray     # float64 per interval: the mean of ``power`` over the periods inside ``band``
    n_bases: np.ndarray       # int64 per interval: the bases transformed, ``max(stop - start, 0)``


SPECTRUM_MAX_PERIODS = 1024          # periods of one call (``ftk_wps_spectrum``)
SPECTRUM_PERIOD_RANGE = (2, 4096)
SPECTRUM_MAX_BASES = 1 << 22         # bases of one interval


def _is_alignment_file(input_file) -> bool:
    import os
    return isinstance(input_file, (str, os.PathLike)) and str(input_file).endswith((".sam", ".bam", ".cram"))


def _check_suffix(path, what, kind):
    """``path`` (``None``: no file) should end in ``.kind`` or ``.kind.gz``."""
    if path is not None and not str(path).endswith((f".{kind}", f".{kind}.gz")):
        raise ValueError(f"{what} should have .{kind} or .{kind}.gz as suffix")


def _check_length_bounds(min_length, max_length):
    if min_length is not None and int(min_length) < 0:
        raise ValueError(f"invalid min_length ({min_length}): it should not be negative")
    if max_length is not None and int(max_length) < 0:
        raise ValueError(f"invalid max_length ({max_length}): it should not be negative")
    if min_length is not None and max_length is not None and int(min_length) > int(max_length):
        raise ValueError(f"min_length ({min_length}) exceeds max_length ({max_length})")


def _check_chrom_sizes_given(input_file, chrom_sizes):
    if chrom_sizes is None and not _is_alignment_file(input_file):
        raise ValueError("chrom_sizes must be specified for BED/Fragment files")


def _over_regions(label, input_file, interval_file, chrom_sizes, workers, verbose, dtypes, row, one_contig, finish, vet=None,
                  whole_contigs=True):
    """The walk of the region commands (``frag_wps_spectrum``, ``frag_wps_peaks``, ``frag_preferred_ends``,
    ``frag_hotspots``): the intervals of ``interval_file`` grouped by contig - or, without one, every contig of the input
    as one interval ``(contig, 0, size, ".")`` in the order the contigs are met (``whole_contigs`` off: the command has no
    such mode and the interval file is required) - handed to the command contig by contig
    as the input is decoded, and the command's answers put back into the intervals' order.

    ``one_contig(engine, key, size, spans, whole) -> (records, rows, note)`` is the command's part: ``spans`` are the
    ``(start, stop)`` of the contig's intervals; ``records`` holds one record array per dtype of ``dtypes`` whose field
    ``interval`` numbers the spans from 0, in order inside every span; ``rows`` one row of ``row = (width, dtype)`` values
    per span; ``note`` ends the contig's verbose line.  ``finish(intervals, records, rows) -> (result, note)`` gets the
    records of all contigs ordered by interval, the rows as an ``(n_intervals, width)`` array, builds the result and
    writes its files.  ``vet(intervals)`` may refuse the interval file's rows before anything else is looked at.

    Chromosome sizes: the BAM header, else the ``chrom_sizes`` file.  A contig that is not in ``chrom_sizes`` raises
    ``ValueError`` before the engine is used, one the input lacks raises the ``ValueError`` of ``frag.coverage``."""
    import sys
    import time

    from .source import ContigFeed
    t0 = time.time()
    sizes = None if _is_alignment_file(input_file) else chrom_sizes_to_dict(chrom_sizes)
    whole = whole_contigs and interval_file is None
    intervals = [] if whole else get_intervals(interval_file)
    if vet is not None:
        vet(intervals)
    by_contig: dict[str, list[int]] = {}
    for i, iv in enumerate(intervals):
        by_contig.setdefault(iv[0], []).append(i)
    if sizes is not None:
        for c in by_contig:
            if c not in sizes:
                raise ValueError(f"{c} is not in chrom_sizes")
    parts, rows = [[] for _ in dtypes], {}
    left = dict(by_contig)
    eng = get_engine()
    # (require: contigs the file does not hold get the ValueError of frag.coverage)
    with ContigFeed(input_file, workers, names=None if whole else list(by_contig), require=left) as feed:
        for src, c in feed:
            if whole:
                if sizes is not None and c not in sizes:
                    raise ValueError(f"{c} is not in chrom_sizes")
                idx = [len(intervals)]
            else:
                idx = left.pop(c, None)
                if idx is None:
                    continue
            size = int(src.lengths[c]) if sizes is None else int(sizes[c])
            if whole:
                intervals.append((c, 0, size, "."))
            records, c_rows, note = one_contig(eng, src.key(c), size, [intervals[i][1:3] for i in idx], whole)
            which = np.asarray(idx, np.int64)
            for part, rec in zip(parts, records):
                rec["interval"] = which[rec["interval"]]
                part.append(rec)
            rows.update(zip(idx, c_rows))
            if verbose:
                sys.stderr.write(f"{label}: {c}: {len(idx)} intervals, {note}\n")
    records = []
    for part, dt in zip(parts, dtypes):  # (an interval's records are in order already)
        rec = np.concatenate(part) if part else np.zeros(0, dt)
        records.append(rec[np.argsort(rec["interval"], kind="stable")])
    n = len(intervals)
    res, note = finish(intervals, records, np.array([rows[i] for i in range(n)], row[1]).reshape(n, row[0]))
    if verbose:
        sys.stderr.write(f"{label}: {n} intervals{note} in {time.time() - t0:.3f} s\n")
    return res


def _to_interval_records(dtype, calls, **fields):
    """The engine's records ``calls`` as ``dtype`` records: ``interval`` from ``run``, ``fields`` as given, every other
    field under its own name."""
    rec = np.zeros(len(calls), dtype)
    for name in dtype.names:
        rec[name] = fields[name] if name in fields else calls["run" if name == "interval" else name]
    return rec


def _check_wps_spectrum_args(input_file, chrom_sizes, output_file, min_period, max_period, band, taper):
    _check_suffix(output_file, "output_file", "tsv")
    lo, hi = int(min_period), int(max_period)
    if lo > hi:
        raise ValueError(f"invalid periods: min_period ({lo}) is above max_period ({hi})")
    if lo < SPECTRUM_PERIOD_RANGE[0] or hi > SPECTRUM_PERIOD_RANGE[1]:
        raise ValueError(f"invalid periods: [{lo}, {hi}] leaves the range {SPECTRUM_PERIOD_RANGE[0]} .. {SPECTRUM_PERIOD_RANGE[1]}")
    if hi - lo + 1 > SPECTRUM_MAX_PERIODS:
        raise ValueError(f"invalid periods: {hi - lo + 1} of them, at most {SPECTRUM_MAX_PERIODS}")
    try:
        b0, b1 = (int(b) for b in band)
    except (TypeError, ValueError):
        raise ValueError(f"invalid band ({band!r}): a pair of periods") from None
    if not lo <= b0 <= b1 <= hi:
        raise ValueError(f"invalid band ({b0}, {b1}): it should lie inside the periods [{lo}, {hi}]")
    if not 0.0 <= float(taper) <= 0.5:
        raise ValueError(f"invalid taper ({taper}): a fraction in [0, 0.5]")
    _check_chrom_sizes_given(input_file, chrom_sizes)


def frag_wps_spectrum(input_file, interval_file, chrom_sizes=None, output_file=None, min_period: int = 120, max_period: int = 280,
                      band=(193, 199), window_size: int = 120, min_length: int = 120, max_length: int = 180,
                      quality_threshold: int = 30, taper: float = 0.1, workers=None, verbose=False) -> WpsSpectrum:
    """Periodicity of the windowed protection score over every interval of ``interval_file`` (BED; gene bodies, as a rule):
    the periodogram of the interval's WPS at every integer period from ``min_period`` to ``max_period`` bases, and its
    mean over ``band`` - the 193-199 bp intensity that follows nucleosome spacing and, through it, expression and
    tissue of origin.

    Per interval, the WPS of ``frag.wps`` with the same ``window_size``, lengths and ``quality_threshold`` has its mean
    removed, is tapered by a split cosine bell over a fraction ``taper`` of the interval at either end, and is summed
    against ``exp(-2j pi (n mod p) / p)`` for every period ``p``, all in float64 (the rule: ``include/ftk.h``,
    "spectrum").  ``power = |X_p|^2 / sum(bell^2)``; an empty interval has ``power = nan``.  The scores are written and
    transformed on the GPU, contig by contig as the input is decoded (``Engine.wps_spectrum``): no per-base value comes
    back to the host.  Strand is ignored - power is unchanged by reversing a run.

    Chromosome sizes (the WPS ignores fragments that leave the contig): the BAM header, else the ``chrom_sizes`` file,
    else ``ValueError``.  An interval on a contig the input lacks raises ``ValueError``, as in ``frag.coverage``; an
    interval of more than 2**22 bases raises too.  ``output_file`` (``.tsv`` / ``.tsv.gz``):
    ``writers.write_wps_spectrum_rows``."""
    import os

    from . import writers
    _check_wps_spectrum_args(input_file, chrom_sizes, output_file, min_period, max_period, band, taper)
    periods = np.arange(int(min_period), int(max_period) + 1, dtype=np.int64)

    def bases(intervals):
        return np.array([max(iv[2] - iv[1], 0) for iv in intervals], np.int64)

    def vet(intervals):
        n_bases = bases(intervals)
        if len(n_bases) and int(n_bases.max()) > SPECTRUM_MAX_BASES:
            raise ValueError(f"interval {intervals[int(n_bases.argmax())][:3]} holds more than {SPECTRUM_MAX_BASES} bases")

    def one_contig(eng, key, size, spans, whole):
        a, b = (np.array(v, np.int64) for v in zip(*spans))
        spectrum, ssw = eng.wps_spectrum(key, a, b, size, periods, window_size, min_length, max_length, quality_threshold, taper, True)
        return (), np.column_stack([spectrum, ssw]), f"{int(np.maximum(b - a, 0).sum())} bases"

    def finish(intervals, records, rows):
        spectrum, ssw, n_bases = rows[:, :-1], rows[:, -1].real, bases(intervals)
        with np.errstate(divide="ignore", invalid="ignore"):
            power = (spectrum.real ** 2 + spectrum.imag ** 2) / ssw[:, None]
        power[(ssw == 0) | (n_bases == 0)] = np.nan
        in_band = (periods >= int(band[0])) & (periods <= int(band[1]))
        band_mean = power[:, in_band].mean(axis=1) if len(intervals) else np.zeros(0)
        res = WpsSpectrum(intervals, periods, power, band_mean, n_bases)
        if output_file is not None:
            writers.write_wps_spectrum_rows(os.fspath(output_file), res)
        return res, ""
    return _over_regions("frag_wps_spectrum", input_file, interval_file, chrom_sizes, workers, verbose, (),
                         (len(periods) + 1, np.complex128), one_contig, finish, vet, whole_contigs=False)


class WpsPeaks(NamedTuple):
    """Result of ``frag_wps_peaks``, one row of ``stats`` / ``callable`` / ``median_spacing`` per interval (of the interval
    file, in its order; whole-contig mode: per contig of the input, in the order the contigs were met)."""
    intervals: list             # (contig, start, stop, name)
    calls: np.ndarray           # WPS_PEAK_DTYPE records ordered by (interval, start); contig positions
    stats: np.ndarray           # int64 (n_intervals, 6): regions, open, short, long, flat, calls
    callable: np.ndarray        # int64 per interval: positions of its callable track
    median_spacing: np.ndarray  # float64 per interval: median distance between consecutive call centres; nan below two calls


WPS_PEAK_DTYPE = np.dtype([("interval", np.int64), ("start", np.int64), ("stop", np.int64), ("summit", np.int64),
                           ("height", np.float64), ("area", np.float64)])
PEAKS_MAX_GAP = 63                # FTK_PEAKS_MAX_GAP
PEAKS_MAX_REGION = 1024           # FTK_PEAKS_MAX_REGION
PEAKS_MAX_MEDIAN_WINDOW = 2048    # the running median of ``ftk_wps_adjust``


def _check_wps_peaks_args(input_file, chrom_sizes, output_file, summary_file, median_window_size, savgol_window_size,
                          savgol_poly_deg, savgol, max_gap, min_region, short_max, max_region, chunk_size):
    _check_suffix(output_file, "output_file", "bed")
    _check_suffix(summary_file, "summary_file", "tsv")
    W = int(median_window_size)
    if W < 2 or W % 2 or W > PEAKS_MAX_MEDIAN_WINDOW:
        raise ValueError(f"invalid median_window_size ({W}): an even number in [2, {PEAKS_MAX_MEDIAN_WINDOW}]")
    if savgol:
        sw, deg = int(savgol_window_size), int(savgol_poly_deg)
        if sw < 3 or sw % 2 == 0:
            raise ValueError(f"invalid savgol_window_size ({sw}): an odd number, 3 at least")
        if not 0 <= deg < sw:
            raise ValueError(f"invalid savgol_poly_deg ({deg}): it should be below savgol_window_size ({sw})")
    if not 0 <= int(max_gap) <= PEAKS_MAX_GAP:
        raise ValueError(f"invalid max_gap ({max_gap}): 0 .. {PEAKS_MAX_GAP}")
    if not 1 <= int(min_region) <= int(short_max) <= int(max_region) <= PEAKS_MAX_REGION:
        raise ValueError(f"invalid region lengths ({min_region}, {short_max}, {max_region}): 1 <= min_region <= short_max <= "
                         f"max_region <= {PEAKS_MAX_REGION}")
    if int(chunk_size) < 1:
        raise ValueError(f"invalid chunk_size ({chunk_size}): at least 1")
    _check_chrom_sizes_given(input_file, chrom_sizes)


def _median_spacing(starts, stops) -> float:
    centres = starts + (stops - starts) // 2
    return float(np.median(np.diff(centres))) if len(centres) >= 2 else float("nan")


def frag_wps_peaks(input_file, interval_file=None, chrom_sizes=None, output_file=None, summary_file=None, window_size: int = 120,
                   min_length: int = 120, max_length: int = 180, quality_threshold: int = 30, median_window_size: int = 1000,
                   savgol_window_size: int = 21, savgol_poly_deg: int = 2, savgol: bool = True, max_gap: int = 5,
                   min_region: int = 50, short_max: int = 150, max_region: int = 450, chunk_size: int = 1 << 20, workers=None,
                   verbose=False) -> WpsPeaks:
    """Nucleosome calls from the adjusted windowed protection score (Snyder et al. 2016): per interval of
    ``interval_file`` (BED), or over every contig of the input when there is none, the WPS of ``frag.wps`` is adjusted as
    ``frag.adjust_wps`` does (running median over ``median_window_size``, Savitzky-Golay with ``savgol_window_size`` /
    ``savgol_poly_deg`` unless ``savgol`` is off) and called by the rule of ``include/ftk.h``, "peaks": regions of positive
    adjusted score joined over gaps of up to ``max_gap``, their windows above the region's median, the window of largest
    area in a region of up to ``short_max`` positions and every window of ``min_region .. short_max`` positions in a
    longer one (up to ``max_region``).  All of it runs on the GPU, contig by contig as the input is decoded
    (``Engine.wps_peaks``): only the calls come back to the host.

    An interval's callable track is what the adjustment leaves of it - ``median_window_size / 2 + savgol_window_size // 2``
    positions less at either end; an interval too short for one has no call.  Whole-contig mode cuts a contig into
    chunks of ``chunk_size`` positions, each widened by ``median_window_size / 2 + savgol_window_size // 2 + max_region +
    max_gap + 1`` on both sides, and keeps a call with the chunk that holds its ``start``: the calls do not depend on
    ``chunk_size``.  (The counters other than ``calls`` are summed over the chunks there: a region inside an overlap
    counts in both.)

    Chromosome sizes: the BAM header, else the ``chrom_sizes`` file, else ``ValueError``.  An interval on a contig the
    input lacks raises ``ValueError``, as in ``frag.coverage``.  ``output_file`` (``.bed`` / ``.bed.gz``):
    ``writers.write_wps_peaks_rows``; ``summary_file`` (``.tsv`` / ``.tsv.gz``): ``writers.write_wps_peaks_summary``."""
    import os

    from . import writers
    _check_wps_peaks_args(input_file, chrom_sizes, output_file, summary_file, median_window_size, savgol_window_size,
                          savgol_poly_deg, savgol, max_gap, min_region, short_max, max_region, chunk_size)
    W, sw = int(median_window_size), int(savgol_window_size) if savgol else 0
    skip, chunk = sw // 2, int(chunk_size)
    pad = W // 2 + skip + int(max_region) + int(max_gap) + 1
    args = dict(window_size=window_size, min_length=min_length, max_length=max_length, quality_threshold=quality_threshold,
                median_window_size=W, savgol_window_size=savgol_window_size, savgol_poly_deg=savgol_poly_deg, savgol=bool(savgol),
                max_gap=max_gap, min_region=min_region, short_max=short_max, max_region=max_region)

    def one_contig(eng, key, size, spans, whole):
        if whole:  # padded chunks; a call stays with the chunk that holds its start
            core = np.arange(0, max(size, 1), chunk, dtype=np.int64)
            core_end = np.minimum(core + chunk, size)
            calls, stats = eng.wps_peaks(key, np.maximum(core - pad, 0), np.minimum(core_end + pad, size), size, **args)
            calls = calls[(calls["start"] >= core[calls["run"]]) & (calls["start"] < core_end[calls["run"]])]
            stats = stats.sum(axis=0, keepdims=True)
            stats[0, 5] = len(calls)
            part = _to_interval_records(WPS_PEAK_DTYPE, calls, interval=0)
        else:
            calls, stats = eng.wps_peaks(key, [a for a, _ in spans], [b for _, b in spans], size, **args)
            part = _to_interval_records(WPS_PEAK_DTYPE, calls)
        return (part,), stats, f"{len(part)} calls"

    def finish(intervals, records, stats):
        calls, n = records[0], len(intervals)
        lens = np.array([max(iv[2] - iv[1], 0) for iv in intervals], np.int64)
        callable_ = np.where(lens >= W + max(sw, 1), lens - W - 2 * skip, 0)
        bounds = np.searchsorted(calls["interval"], np.arange(n + 1))
        spacing = np.array([_median_spacing(calls["start"][a:b], calls["stop"][a:b]) for a, b in zip(bounds[:-1], bounds[1:])], np.float64)
        res = WpsPeaks(intervals, calls, stats, callable_, spacing)
        if output_file is not None:
            writers.write_wps_peaks_rows(os.fspath(output_file), res)
        if summary_file is not None:
            writers.write_wps_peaks_summary(os.fspath(summary_file), res)
        return res, f", {len(calls)} calls"
    return _over_regions("frag_wps_peaks", input_file, interval_file, chrom_sizes, workers, verbose, (WPS_PEAK_DTYPE,), (6, np.int64),
                         one_contig, finish)


class PreferredEnds(NamedTuple):
    """Result of ``frag_preferred_ends``, one row of ``stats`` / ``share`` per interval (of the interval file, in its order;
    whole-contig mode: per contig of the input, in the order the contigs were met)."""
    intervals: list      # (contig, start, stop, name)
    calls: np.ndarray    # PREFERRED_END_DTYPE records ordered by (interval, pos, kind); contig positions
    stats: np.ndarray    # int64 (n_intervals, 6): U ends, D ends, tested a, tested b, calls a, calls b
    share: np.ndarray    # float64 per interval: the share of its ends that lie on called positions; nan without ends


PREFERRED_END_DTYPE = np.dtype([("interval", np.int64), ("pos", np.int64), ("kind", np.int32), ("count", np.int32),
                                ("total", np.int64), ("n_w", np.int32)])
PREFENDS_MAX_HALF = 2048   # FTK_PREFENDS_MAX_HALF
PREFENDS_MAX_THR = 4096    # FTK_PREFENDS_MAX_THR
PREFENDS_SCALE_BITS = 20   # a table entry is a mean in units of 2^-20 ends per base


def preferred_end_thresholds(alpha: float = 0.01, n: int = 256) -> np.ndarray:
    """The ``uint64`` table of ``Engine.preferred_ends`` for a Poisson test at level ``alpha``: ``thr[0] = 0`` and, for
    ``1 <= k < n``, ``thr[k]`` is the largest integer ``q`` in ``[0, k * 2**20]`` with ``P(X >= k | Poisson(q / 2**20)) <
    alpha`` - the largest mean, in units of 2^-20 ends per base, at which ``k`` ends on one base are still significant.
    ``P(X >= k | Poisson(m))`` is the regularised lower incomplete gamma function ``gammainc(k, m)``, which grows with
    ``m``, so ``q`` is found by bisection over the integers.  Counts of ``n - 1`` and more share the last entry."""
    alpha, n = float(alpha), int(n)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"invalid alpha ({alpha}): it should lie inside (0, 1)")
    if not 2 <= n <= PREFENDS_MAX_THR:
        raise ValueError(f"invalid n ({n}): 2 .. {PREFENDS_MAX_THR}")
    from scipy.special import gammainc
    k = np.arange(1, n, dtype=np.int64)
    unit = float(1 << PREFENDS_SCALE_BITS)

    def ok(q):
        return gammainc(k.astype(np.float64), q / unit) < alpha
    lo = np.zeros(n - 1, np.int64)          # ok(lo) holds: P = 0
    hi = k << PREFENDS_SCALE_BITS           # the search ends here
    top = ok(hi)
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        good = ok(mid)
        lo = np.where(good, mid, lo)
        hi = np.where(good, hi, mid)
    thr = np.zeros(n, np.uint64)
    thr[1:] = np.where(top, k << PREFENDS_SCALE_BITS, lo).astype(np.uint64)
    return thr


def _check_preferred_ends_args(input_file, chrom_sizes, output_file, summary_file, half_window, alpha, min_count, min_length,
                               max_length, chunk_size):
    _check_suffix(output_file, "output_file", "bed")
    _check_suffix(summary_file, "summary_file", "tsv")
    if not 1 <= int(half_window) <= PREFENDS_MAX_HALF:
        raise ValueError(f"invalid half_window ({half_window}): 1 .. {PREFENDS_MAX_HALF}")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"invalid alpha ({alpha}): it should lie inside (0, 1)")
    if int(min_count) < 1:
        raise ValueError(f"invalid min_count ({min_count}): at least 1")
    _check_length_bounds(min_length, max_length)
    if int(chunk_size) < 1:
        raise ValueError(f"invalid chunk_size ({chunk_size}): at least 1")
    _check_chrom_sizes_given(input_file, chrom_sizes)


def frag_preferred_ends(input_file, interval_file=None, chrom_sizes=None, output_file=None, summary_file=None,
                        half_window: int = 500, alpha: float = 0.01, min_count: int = 2, split: bool = False, min_length=None,
                        max_length=None, quality_threshold: int = 30, chunk_size: int = 1 << 22, workers=None,
                        verbose=False) -> PreferredEnds:
    """Preferred fragment-end coordinates (Chan et al. 2016, Jiang et al. 2018; ``split``: U and D ends apart, Sun et al.
    2019): per interval of ``interval_file`` (BED), or over every contig of the input when there is none, the positions on
    which at least ``min_count`` fragments end and significantly more than a Poisson model predicts whose mean is the end
    density of the window of ``half_window`` bases on either side (``alpha``: the level of the one-sided test).  The rule
    is stated in ``include/ftk.h``, "preferred ends"; the test becomes an integer comparison with the table of
    ``preferred_end_thresholds(alpha)``.  Every base is tested on the GPU, contig by contig as the input is decoded
    (``Engine.preferred_ends``): only the calls come back to the host.

    Windows read the contig, not the interval: whole-contig mode cuts a contig into chunks of ``chunk_size`` positions
    without overlap and the result does not depend on ``chunk_size``.  BED intervals are clipped to the contig.

    Chromosome sizes: the BAM header, else the ``chrom_sizes`` file, else ``ValueError``.  An interval on a contig the
    input lacks raises ``ValueError``, as in ``frag.coverage``.  ``output_file`` (``.bed`` / ``.bed.gz``):
    ``writers.write_preferred_end_rows``; ``summary_file`` (``.tsv`` / ``.tsv.gz``): ``writers.write_preferred_end_summary``."""
    import os

    from . import writers
    _check_preferred_ends_args(input_file, chrom_sizes, output_file, summary_file, half_window, alpha, min_count, min_length,
                               max_length, chunk_size)
    chunk = int(chunk_size)
    args = dict(half=int(half_window), mode="split" if split else "combined", min_count=int(min_count),
                thresholds=preferred_end_thresholds(alpha), min_length=min_length, max_length=max_length,
                quality_threshold=quality_threshold)

    def one_contig(eng, key, size, spans, whole):
        if whole:  # chunks without overlap, one after the other: the calls are in position order
            cut = np.arange(0, max(size, 1), chunk, dtype=np.int64)
            calls, stats = eng.preferred_ends(key, cut, np.minimum(cut + chunk, size), size, **args)
            stats = stats.sum(axis=0, keepdims=True)
            part = _to_interval_records(PREFERRED_END_DTYPE, calls, interval=0)
        else:
            a = np.clip(np.array([a for a, _ in spans], np.int64), 0, size)
            b = np.clip(np.array([b for _, b in spans], np.int64), a, size)
            calls, stats = eng.preferred_ends(key, a, b, size, **args)
            part = _to_interval_records(PREFERRED_END_DTYPE, calls)
        return (part,), stats, f"{len(part)} calls"

    def finish(intervals, records, stats):
        calls, n = records[0], len(intervals)
        on_calls = np.bincount(calls["interval"], weights=calls["count"], minlength=n)[:n] if n else np.zeros(0)
        ends = (stats[:, 0] + stats[:, 1]).astype(np.float64)
        share = np.divide(on_calls, ends, out=np.full(n, np.nan), where=ends > 0)
        res = PreferredEnds(intervals, calls, stats, share)
        if output_file is not None:
            writers.write_preferred_end_rows(os.fspath(output_file), res)
        if summary_file is not None:
            writers.write_preferred_end_summary(os.fspath(summary_file), res)
        return res, f", {len(calls)} calls"
    return _over_regions("frag_preferred_ends", input_file, interval_file, chrom_sizes, workers, verbose, (PREFERRED_END_DTYPE,),
                         (6, np.int64), one_contig, finish)


class IfsHotspots(NamedTuple):
    """Result of ``frag_hotspots``, one row of ``stats`` / ``mean_length`` / ``global_mean`` per interval (of the interval
    file, in its order; whole-contig mode: per contig of the input, in the order the contigs were met)."""
    intervals: list          # (contig, start, stop, name)
    hotspots: np.ndarray     # HOTSPOT_DTYPE records ordered by (interval, start); contig positions
    windows: np.ndarray      # IFS_WINDOW_DTYPE records, the called windows, ordered by (interval, start)
    stats: np.ndarray        # int64 (n_intervals, 6): windows, tested, called, hotspots kept, hotspots dropped, bases covered
    mean_length: np.ndarray  # int64 per interval: L of its contig
    global_mean: np.ndarray  # int64 per interval: its contig's mean IFS per window in units of 2^-10 (0: not used)
    step: int                # bases per bin
    window_bins: int         # m


HOTSPOT_DTYPE = np.dtype([("interval", np.int64), ("start", np.int64), ("stop", np.int64), ("n_windows", np.int32),
                          ("summit", np.int64), ("ifs", np.int64), ("count", np.int32), ("bg1", np.int64), ("nb1", np.int32)])
IFS_WINDOW_DTYPE = np.dtype([("interval", np.int64), ("start", np.int64), ("stop", np.int64), ("count", np.int32),
                             ("ifs", np.int64), ("bg1", np.int64), ("nb1", np.int32), ("bg2", np.int64), ("nb2", np.int32)])
IFS_MAX_WINDOW_BINS = 64   # FTK_IFS_MAX_WINDOW_BINS
IFS_MAX_REACH = 1024       # FTK_IFS_MAX_REACH
IFS_MAX_THR = 4096         # FTK_IFS_MAX_THR
IFS_MAX_JOIN = 1024        # FTK_IFS_MAX_JOIN
IFS_SCALE_BITS = 10        # a table entry is a mean IFS per window in units of 2^-10


def ifs_thresholds(alpha: float = 1e-5, n: int = 256) -> np.ndarray:
    """The ``uint64`` table of ``Engine.ifs_hotspots`` for a Poisson lower-tail test at level ``alpha``: ``thr[q]`` is the
    smallest integer ``t`` with ``P(X <= q | Poisson(t / 1024)) <= alpha`` - the smallest mean, in units of 2^-10, at which
    an integer IFS of ``q`` is significantly low.  ``P(X <= q | Poisson(x))`` is the regularised upper incomplete gamma
    function ``gammaincc(q + 1, x)``, which falls as ``x`` grows, so ``t`` is found by bisection over the integers between 0
    (where it is 1) and a Chernoff bound ``q + A + sqrt(A^2 + 2 q A) + 1`` with ``A = -ln(alpha)`` (where it is at most
    ``alpha``: asserted)."""
    alpha, n = float(alpha), int(n)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"invalid alpha ({alpha}): it should lie inside (0, 1)")
    if not 1 <= n <= IFS_MAX_THR:
        raise ValueError(f"invalid n ({n}): 1 .. {IFS_MAX_THR}")
    from scipy.special import gammaincc
    q = np.arange(n, dtype=np.float64)
    unit = float(1 << IFS_SCALE_BITS)

    def ok(t):
        return gammaincc(q + 1.0, t / unit) <= alpha
    A = -np.log(alpha)
    lo = np.zeros(n, np.int64)  # ok(lo) fails: P = 1
    hi = np.ceil((q + A + np.sqrt(A * A + 2.0 * q * A) + 1.0) * unit).astype(np.int64)
    assert np.all(ok(hi)), "the upper bracket of ifs_thresholds is not significant"
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        good = ok(mid)
        hi = np.where(good, mid, hi)
        lo = np.where(good, lo, mid)
    return hi.astype(np.uint64)


def _check_hotspots_args(input_file, chrom_sizes, output_file, windows_file, summary_file, step, window, background, alpha,
                         mean_length, min_count, join, min_windows, min_length, max_length):
    _check_suffix(output_file, "output_file", "bed")
    _check_suffix(windows_file, "windows_file", "bed")
    _check_suffix(summary_file, "summary_file", "tsv")
    step, window = int(step), int(window)
    if not 1 <= step <= 65535:
        raise ValueError(f"invalid step ({step}): 1 .. 65535")
    if window < step or window % step:
        raise ValueError(f"invalid window ({window}): a positive multiple of step ({step})")
    m = window // step
    if m > IFS_MAX_WINDOW_BINS:
        raise ValueError(f"invalid window ({window}): at most {IFS_MAX_WINDOW_BINS} steps")
    try:
        bg = [int(b) for b in background]
    except TypeError:
        bg = [int(background)]
    if not 1 <= len(bg) <= 2:
        raise ValueError("background should hold one or two widths")
    h = [b // (2 * step) for b in bg]
    if h[0] < 1:
        raise ValueError(f"invalid background ({bg[0]}): at least two steps")
    if len(h) == 2 and h[1] < h[0]:
        raise ValueError(f"invalid background ({bg}): the second width should not be below the first")
    if max(h) + m > IFS_MAX_REACH:
        raise ValueError(f"invalid background ({bg}): half of it and the window exceed {IFS_MAX_REACH} steps")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"invalid alpha ({alpha}): it should lie inside (0, 1)")
    if mean_length is not None and not 1 <= int(mean_length) <= 65535:
        raise ValueError(f"invalid mean_length ({mean_length}): 1 .. 65535")
    if int(min_count) < 0:
        raise ValueError(f"invalid min_count ({min_count}): it should not be negative")
    if join is not None and not 1 <= int(join) <= IFS_MAX_JOIN:
        raise ValueError(f"invalid join ({join}): 1 .. {IFS_MAX_JOIN}")
    if int(min_windows) < 1:
        raise ValueError(f"invalid min_windows ({min_windows}): at least 1")
    _check_length_bounds(min_length, max_length)
    _check_chrom_sizes_given(input_file, chrom_sizes)
    return m, h[0], (h[1] if len(h) == 2 else 0)


def frag_hotspots(input_file, interval_file=None, chrom_sizes=None, output_file=None, windows_file=None, summary_file=None,
                  step: int = 20, window: int = 200, background=(5000, 10000), alpha: float = 1e-5, mean_length=None,
                  use_global: bool = True, min_count: int = 0, join=None, min_windows: int = 1, min_length=None,
                  max_length=None, quality_threshold: int = 30, workers=None, verbose=False) -> IfsHotspots:
    """Fragmentation hotspots from the Integrated Fragmentation Score (Zhou et al. 2022, CRAG): per interval of
    ``interval_file`` (BED), or over every contig of the input when there is none, the windows of ``window`` bases sliding
    by ``step`` whose IFS - ``n * (1 + mean fragment length in the window / mean fragment length on the contig)`` over the
    fragments with their midpoint in the window - is significantly low (Poisson lower tail at level ``alpha``) against
    the mean IFS of the ``background`` widths around the window (one or two, in bases; half-widths ``b // (2 * step)``
    steps) and, with ``use_global``, of the contig; called windows at most ``join`` steps apart (default
    ``window // step + 200 // step``) merge into a hotspot, and a hotspot of fewer than ``min_windows`` windows is dropped.
    The rule is stated in ``include/ftk.h``, "IFS hotspots"; the test becomes an integer comparison with the table of
    ``ifs_thresholds(alpha)``.  Every window is scored and tested on the GPU, contig by contig as the input is decoded
    (``Engine.ifs_hotspots``): only the called windows come back to the host.

    ``mean_length``: ``L`` of the rule; ``None``: per contig, the rounded mean length of the passing fragments with a
    midpoint on the contig.  That mean and the contig's mean IFS (``global_mean``) come from one reduction on the GPU
    (``Engine.ifs_totals``).  Backgrounds read the contig, not the interval.  BED intervals are clipped to the contig.

    Chromosome sizes: the BAM header, else the ``chrom_sizes`` file, else ``ValueError``.  An interval on a contig the
    input lacks raises ``ValueError``, as in ``frag.coverage``.  ``output_file`` (``.bed`` / ``.bed.gz``):
    ``writers.write_hotspot_rows``; ``windows_file``: ``writers.write_hotspot_windows``; ``summary_file`` (``.tsv`` /
    ``.tsv.gz``): ``writers.write_hotspot_summary``."""
    import os

    from . import writers
    m, h1, h2 = _check_hotspots_args(input_file, chrom_sizes, output_file, windows_file, summary_file, step, window, background,
                                     alpha, mean_length, min_count, join, min_windows, min_length, max_length)
    step = int(step)
    join = max(m + 200 // step, 1) if join is None else int(join)
    filt = dict(min_length=min_length, max_length=max_length, quality_threshold=quality_threshold)
    thr = ifs_thresholds(alpha)

    def one_contig(eng, key, size, spans, whole):
        a = np.clip(np.array([a for a, _ in spans], np.int64), 0, size)
        b = np.clip(np.array([b for _, b in spans], np.int64), a, size)
        L, gm = mean_length, 0
        if L is None or use_global:
            N, S = eng.ifs_totals(key, size, **filt)
            if L is None:
                L = min(max((2 * S + N) // (2 * N), 1), 65535) if N else 1
            L = int(L)
            n_bins = -(-size // step)
            if use_global and n_bins:
                gm = (N * L + S) * m * 1024 // (n_bins * L)
        L = int(L)
        win, hot, stats = eng.ifs_hotspots(key, a, b, size, step=step, m=m, mean_length=L, h1=h1, h2=h2, min_count=int(min_count),
                                           thresholds=thr, global_mean=gm, join=join, min_windows=int(min_windows), **filt)
        hp = _to_interval_records(HOTSPOT_DTYPE, hot)
        wp = _to_interval_records(IFS_WINDOW_DTYPE, win, start=win["pos"], stop=np.minimum(win["pos"] + m * step, size))
        rows = np.column_stack([stats, np.full(len(stats), L, np.int64), np.full(len(stats), gm, np.int64)])
        return (hp, wp), rows, f"L = {L}, {len(wp)} called windows, {len(hp)} hotspots"

    def finish(intervals, records, rows):
        hotspots, windows = records
        stats, mean_rows, glob_rows = (np.ascontiguousarray(a) for a in (rows[:, :6], rows[:, 6], rows[:, 7]))
        res = IfsHotspots(intervals, hotspots, windows, stats, mean_rows, glob_rows, step, m)
        if output_file is not None:
            writers.write_hotspot_rows(os.fspath(output_file), res)
        if windows_file is not None:
            writers.write_hotspot_windows(os.fspath(windows_file), res)
        if summary_file is not None:
            writers.write_hotspot_summary(os.fspath(summary_file), res)
        return res, f", {len(hotspots)} hotspots"
    return _over_regions("frag_hotspots", input_file, interval_file, chrom_sizes, workers, verbose, (HOTSPOT_DTYPE, IFS_WINDOW_DTYPE),
                         (8, np.int64), one_contig, finish)


class EndContext(NamedTuple):
    """Result of ``frag_end_context``: base and base-pair counts at every offset of a window around the fragment ends (or
    centres), per length class and per kind of reading.  Bases are ``A C G T N`` = 0 .. 4."""
    table: np.ndarray        # int64 (n_classes, 2, 2 * half_width, 25): cell 5 * x + y = base x at offset o, base y at o + 1
    n_kept: np.ndarray       # int64 per class: the kept fragments; every row table[c, k, j] sums to n_kept[c]
    background: np.ndarray   # int64 [25]: cell 5 * x + y = reference positions p with base x at p and base y at p + 1
    half_width: int          # W: offsets run over [-W, W), row j = o + W; o >= 0 lies inside the fragment
    length_edges: tuple      # class c holds the lengths length_edges[c] <= L < length_edges[c + 1]
    anchor: str              # "ends": kind 0 = U end on the + strand, kind 1 = D end on the - strand; "centre"
    skipped_contigs: tuple   # contigs of the input the reference does not hold

    @property
    def mono(self) -> np.ndarray:
        """int64 ``(n_classes, 2, 2 * half_width, 5)``: the base at each offset (the marginal over the second base)."""
        return self.table.reshape(self.table.shape[:-1] + (5, 5)).sum(axis=-1)

    @property
    def dinuc(self) -> np.ndarray:
        """int64 ``(n_classes, 2, 2 * half_width, 16)``: cell ``4 * x + y`` of the pairs with both bases defined, in the
        order ``AA AC AG AT CA ... TT``."""
        t = self.table.reshape(self.table.shape[:-1] + (5, 5))[..., :4, :4]
        return np.ascontiguousarray(t).reshape(self.table.shape[:-1] + (16,))

    def background_counts(self, k: int) -> np.ndarray:
        """int64 ``(2, 4 ** k)``: per kind of reading, how often each motif of ``k`` defined bases is read on that kind's
        strand of the reference - kind 0: the motif's count on the + strand; kind 1: the count of its reverse complement
        on the + strand."""
        bg = np.asarray(self.background, dtype=np.int64).reshape(5, 5)
        if k == 1:
            plus = bg.sum(axis=1)[:4]
            return np.stack([plus, plus[::-1]])
        if k == 2:
            plus = bg[:4, :4]
            return np.stack([plus.reshape(16), plus[::-1, ::-1].T.reshape(16)])
        raise ValueError(f"invalid k ({k}): 1 or 2")

    def frequency(self, k: int) -> np.ndarray:
        """float64 ``(n_classes, 2, 2 * half_width, 4 ** k)``: ``count[m] / sum(count[m'] for the 4 ** k defined motifs
        m')`` per row, ``count`` = ``mono[..., :4]`` (k = 1) or ``dinuc`` (k = 2); NaN where a row has no defined motif."""
        if k not in (1, 2):
            raise ValueError(f"invalid k ({k}): 1 or 2")
        count = (self.mono[..., :4] if k == 1 else self.dinuc).astype(np.float64)
        total = count.sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(total > 0, count / total, np.nan)

    def enrichment(self, k: int) -> np.ndarray:
        """float64 ``(n_classes, 2, 2 * half_width, 4 ** k)``:
        ``enrichment[c, kind, j, m] = frequency(k)[c, kind, j, m] / (B[kind, m] / B[kind].sum())`` with ``B =
        background_counts(k)`` - the motif's frequency among the defined motifs of its row over its frequency among the
        defined motifs of the reference read on the same strand (kind 1: the reverse complement's count on the + strand).
        NaN where the row has no defined motif, the background has none, or ``B[kind, m] == 0``."""
        freq = self.frequency(k)
        b = self.background_counts(k).astype(np.float64)
        tot = b.sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            bf = np.where((tot > 0) & (b > 0), b / tot, np.nan)
            return freq / bf[None, :, None, :]


def _check_end_context_args(output_file, half_width, length_edges, anchor):
    from . import _lib as L
    from . import writers
    if not 1 <= int(half_width) <= L.CONTEXT_MAX_HALF:
        raise ValueError(f"invalid half_width ({half_width}): 1 .. {L.CONTEXT_MAX_HALF}")
    edges = tuple(int(v) for v in length_edges)
    if not 2 <= len(edges) <= L.CONTEXT_MAX_CLASSES + 1:
        raise ValueError(f"invalid length_edges: 2 .. {L.CONTEXT_MAX_CLASSES + 1} values bound 1 .. {L.CONTEXT_MAX_CLASSES} classes")
    if edges[0] < 1 or edges[-1] > 1 << 30 or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"invalid length_edges {edges}: strictly ascending within [1, 2**30]")
    if anchor not in L.CONTEXT_ANCHOR:
        raise ValueError(f"invalid anchor ({anchor!r}): 'ends' or 'centre'")
    if output_file is not None and not str(output_file).endswith(writers.END_CONTEXT_SUFFIXES):
        raise ValueError("output_file should have .tsv or .tsv.gz as suffix")
    return edges


def frag_end_context(input_file, reference_file, output_file=None, contig=None, quality_threshold: int = 30, half_width: int = 32,
                     length_edges=(1, 150, 221, 1001), anchor: str = "ends", workers=None, verbose=False) -> EndContext:
    """Nucleotide and dinucleotide profiles around the fragment ends of ``input_file`` against ``reference_file``
    (``.2bit`` or FASTA), per fragment length class: the first figure of a cfDNA cleavage analysis and the first QC plot
    of library-prep end bias.  Counted on the GPU in one pass per contig as the input is decoded.

    A fragment ``[s, e)`` of length ``L`` with ``mapq >= quality_threshold`` and ``length_edges[0] <= L <
    length_edges[-1]`` belongs to the class ``c`` with ``length_edges[c] <= L < length_edges[c + 1]`` (at most 8 classes)
    and gives two readings over the offsets ``o`` of ``[-half_width, half_width]``: kind 0 ``= base(s + o)``, the U end read
    5'->3' on the + strand, and kind 1 ``= complement(base(e - 1 - o))``, the D end read 5'->3' on the - strand.  ``o >= 0``
    lies inside the fragment, ``o < 0`` in front of it.  ``anchor="centre"`` takes the same readings around ``s + L // 2`` and
    ``e - 1 - L // 2`` instead.  ``table[c, kind, o + half_width, 5 * x + y]`` counts the readings with base ``x`` at ``o``
    and ``y`` at ``o + 1`` (``A C G T N`` = 0 .. 4; N: outside the contig, a 2bit N block, or a FASTA byte other than
    ACGTacgt).  ``background[5 * x + y]`` counts the reference positions of the contigs used in the same way.

    Contigs of the input that the reference lacks are skipped with one ``UserWarning`` and listed in ``skipped_contigs``.
    Returns an ``EndContext``: see its ``mono``, ``dinuc``, ``frequency(k)`` and ``enrichment(k)``.  ``output_file`` (``.tsv``
    / ``.tsv.gz``): ``writers.write_end_context_rows``."""
    import os
    import sys
    import time

    from . import writers
    edges = _check_end_context_args(output_file, half_width, length_edges, anchor)
    w = int(half_width)
    t0 = time.time()
    table = np.zeros((len(edges) - 1, 2, 2 * w, 25), np.int64)
    n_kept = np.zeros(len(edges) - 1, np.int64)
    background = np.zeros(25, np.int64)

    def one_contig(eng, key, rid, name, size):
        t, k = eng.end_context(key, rid, w, edges, quality_threshold, anchor)
        table[...] += t
        n_kept[...] += k
        background[...] += eng.ref_context(rid, 0, size)
        return f"{int(k.sum())} fragments"
    missing = _over_reference_contigs("frag_end_context", input_file, reference_file, contig, workers, verbose, one_contig)
    res = EndContext(table, n_kept, background, w, edges, str(anchor), missing)
    if output_file is not None:
        writers.write_end_context_rows(os.fspath(output_file), res)
    if verbose:
        sys.stderr.write(f"frag_end_context: {int(n_kept.sum())} fragments in {time.time() - t0:.3f} s\n")
    return res


class MotifLengths(NamedTuple):
    """Result of ``frag_motif_lengths``: end-motif (or breakpoint-motif) counts per fragment length row and per kind of
    reading (0: the U end on the + strand, 1: the D end on the - strand).  Row ``r`` holds the lengths ``min_length + r *
    length_bin .. min_length + (r + 1) * length_bin - 1``; column ``4 ** k`` counts the readings with an N or off the contig."""
    table: np.ndarray        # int64 (2, n_rows, 4 ** k + 1): motifs in the order of gen_kmers(k), then "undefined"
    n_kept: np.ndarray       # int64 per row: the kept fragments; every row table[kind, r] sums to n_kept[r]
    k: int
    kind: str                # "end" or "breakpoint"
    min_length: int          # the first length of row 0
    length_bin: int          # lengths per row
    skipped_contigs: tuple   # contigs of the input the reference does not hold

    def lengths(self) -> np.ndarray:
        """int64 per row: the first length of the row."""
        return int(self.min_length) + int(self.length_bin) * np.arange(len(self.n_kept), dtype=np.int64)

    def motifs(self) -> list:
        """The names of the first ``4 ** k`` columns: ``gen_kmers(k, "ACGT")``."""
        return gen_kmers(int(self.k), "ACGT")

    def frequency(self) -> np.ndarray:
        """float64 ``(2, n_rows, 4 ** k)``: each motif's share among the defined motifs of its row; NaN where a row has none."""
        count = np.asarray(self.table)[..., :-1].astype(np.float64)
        total = count.sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(total > 0, count / total, np.nan)

    def mds(self) -> np.ndarray:
        """float64 ``(3, n_rows)``: the motif diversity score ``-sum f ln f / ln(4 ** k)`` (``0 ln 0 = 0``) of the U ends, of
        the D ends and of both pooled, per row; NaN where a row has no defined motif."""
        t = np.asarray(self.table)[..., :-1].astype(np.float64)
        count = np.concatenate([t, t.sum(axis=0, keepdims=True)], axis=0)
        total = count.sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(total > 0, count / total, np.nan)
            logs = np.log(f, out=np.zeros_like(f), where=f > 0)  # (NaN > 0 is False: the NaN comes back through f * logs)
        return (0.0 - (f * logs).sum(axis=-1)) / np.log(4.0 ** int(self.k))  # (0.0 - x: a single motif gives 0.0, not -0.0)

    def pooled(self, lo: int, hi: int) -> np.ndarray:
        """int64 ``(2, 4 ** k + 1)``: the rows of the lengths ``lo .. hi`` summed - what an end-motif count restricted to
        that size selection gives.  ``lo`` must start a row and ``hi`` end one (the last row may be narrower than
        ``length_bin``: any ``hi`` inside it ends it)."""
        lo, hi, first, b = int(lo), int(hi), int(self.min_length), int(self.length_bin)
        last = first + b * len(self.n_kept) - 1
        if lo > hi or lo < first or hi > last or (lo - first) % b or ((hi + 1 - first) % b and hi <= last - b):
            raise ValueError(f"invalid length range ({lo}, {hi}): whole rows of {b} lengths within {first} .. {last}")
        return np.asarray(self.table)[:, (lo - first) // b:(hi - first) // b + 1].sum(axis=1)


def _check_motif_length_args(output_file, summary_file, k, kind, min_length, max_length, length_bin):
    from . import _lib as L
    from . import writers
    k, lo, hi, b = int(k), int(min_length), int(max_length), int(length_bin)
    if not 1 <= k <= L.MOTIFLEN_MAX_K:
        raise ValueError(f"invalid k ({k}): 1 .. {L.MOTIFLEN_MAX_K}")
    if kind not in ("end", "breakpoint"):
        raise ValueError(f"invalid kind ({kind!r}): 'end' or 'breakpoint'")
    if kind == "breakpoint" and k % 2:
        raise ValueError(f"invalid k ({k}): a breakpoint motif has k / 2 bases either side of the end, k must be even")
    if lo < 1 or hi < lo or hi > 1 << 30 or b < 1:
        raise ValueError(f"invalid lengths ({lo} .. {hi} in rows of {b}): 1 <= min_length <= max_length <= 2**30, length_bin >= 1")
    n_rows = (hi - lo) // b + 1
    if n_rows > L.MOTIFLEN_MAX_ROWS:
        raise ValueError(f"invalid lengths ({lo} .. {hi} in rows of {b}): {n_rows} rows, at most {L.MOTIFLEN_MAX_ROWS}")
    for what, path in (("output_file", output_file), ("summary_file", summary_file)):
        if path is not None and not str(path).endswith(writers.MOTIF_LENGTH_SUFFIXES):
            raise ValueError(f"{what} should have .tsv or .tsv.gz as suffix")
    return k, (0 if kind == "end" else -(k // 2)), lo, hi, b, n_rows


def frag_motif_lengths(input_file, reference_file, output_file=None, summary_file=None, contig=None, k: int = 4, kind: str = "end",
                       min_length: int = 1, max_length: int = 1000, length_bin: int = 1, quality_threshold: int = 30,
                       workers=None, verbose=False) -> MotifLengths:
    """End-motif counts of ``input_file`` against ``reference_file`` (``.2bit`` or FASTA) per fragment length: the table
    behind "motif frequency against fragment size" and the motif diversity score per length, counted on the GPU in one
    pass per contig as the input is decoded.

    A fragment ``[s, e)`` of length ``L`` with ``mapq >= quality_threshold`` and ``min_length <= L <= max_length`` falls
    into row ``(L - min_length) // length_bin`` (at most 1024 rows) and gives two readings of ``k`` bases (1 .. 4): the U end
    on the + strand, ``base(s + shift + i)``, and the D end on the - strand, ``complement(base(e - 1 - shift - i))``, ``i
    = 0 .. k-1``.  ``kind="end"``: ``shift = 0``, the end motifs; ``kind="breakpoint"`` (even ``k``): ``shift = -k // 2``, the
    breakpoint motifs - the two k-mers ``end_motifs`` / ``breakpoint_motifs`` read.  A reading with an N (a 2bit N block, a
    FASTA byte other than ACGTacgt) or a base off the contig counts in the last column, "undefined"; no fragment is dropped.

    Contigs of the input that the reference lacks are skipped with one ``UserWarning`` and listed in ``skipped_contigs``.
    Returns a ``MotifLengths``: see its ``lengths``, ``motifs``, ``frequency``, ``mds`` and ``pooled``.  ``output_file``
    (``.tsv`` / ``.tsv.gz``): ``writers.write_motif_length_rows``; ``summary_file``: ``writers.write_motif_length_summary``."""
    import os
    import sys
    import time

    from . import writers
    k, shift, lo, hi, b, n_rows = _check_motif_length_args(output_file, summary_file, k, kind, min_length, max_length, length_bin)
    t0 = time.time()
    table = np.zeros((2, n_rows, 4 ** k + 1), np.int64)
    n_kept = np.zeros(n_rows, np.int64)

    def one_contig(eng, key, rid, name, size):
        t, kept = eng.motif_length_table(key, rid, k, shift, lo, hi, b, quality_threshold)
        table[...] += t
        n_kept[...] += kept
        return f"{int(kept.sum())} fragments"
    missing = _over_reference_contigs("frag_motif_lengths", input_file, reference_file, contig, workers, verbose, one_contig)
    res = MotifLengths(table, n_kept, k, str(kind), lo, b, missing)
    if output_file is not None:
        writers.write_motif_length_rows(os.fspath(output_file), res)
    if summary_file is not None:
        writers.write_motif_length_summary(os.fspath(summary_file), res)
    if verbose:
        sys.stderr.write(f"frag_motif_lengths: {int(n_kept.sum())} fragments in {time.time() - t0:.3f} s\n")
    return res


class CoFragmentation(NamedTuple):
    """Result of ``frag_cofragmentation`` for one contig: the pairwise Kolmogorov-Smirnov distances between the fragment
    length distributions of its bins and the compartment track read off them.  ``N`` bins; the matrices are ``N x N``."""
    contig: str
    starts: np.ndarray      # int64 [N]: bin k is [starts[k], stops[k])
    stops: np.ndarray       # int64 [N]
    n: np.ndarray           # int64 [N]: fragments of the bin inside the length range
    overflow: np.ndarray    # int64 [N]: fragments of the bin that passed the filter outside the histogram's range
    K: np.ndarray           # int64: the KS numerator, max over lengths of |C(i, l) n(j) - C(j, l) n(i)|
    at: np.ndarray          # int32: the smallest fragment LENGTH at which that maximum is attained (min_length where K = 0)
    valid: np.ndarray       # bool [N]: n >= min_count
    D: np.ndarray           # float64: the KS statistic K / (n(i) n(j)); NaN where either bin is not valid
    z: np.ndarray           # float64: D sqrt(n(i) n(j) / (n(i) + n(j))); NaN likewise
    neglog10_p: np.ndarray  # float64: ks_neglog10_p(z); NaN likewise
    corr: np.ndarray        # float64: Pearson correlation of the rows of the chosen distance over the valid bins; NaN elsewhere
    pc1: np.ndarray         # float64 [N]: unit eigenvector of corr's largest eigenvalue, largest component positive; NaN at invalid bins


def ks_neglog10_p(z) -> np.ndarray:
    """``-log10 Q(z)`` of the Kolmogorov distribution, ``Q(z) = 2 sum_{k >= 1} (-1)^(k - 1) exp(-2 k^2 z^2)`` summed over
    ``k`` to 200 in float64: 0 for ``z < 0.04`` (where Q is 1 to the last bit); for ``z >= 1`` evaluated as
    ``(2 z^2 - ln(2 (1 - e^(-6 z^2) + e^(-16 z^2) - ...))) / ln 10``, which stays finite where Q underflows.  NaN stays
    NaN.  Any shape; returns float64 of that shape."""
    z = np.asarray(z, dtype=np.float64)
    flat = z.ravel()
    out = np.zeros(flat.shape, np.float64)
    out[np.isnan(flat)] = np.nan
    hi = np.flatnonzero(flat >= 1.0)
    if len(hi):
        # (k = 20: exp(-2 * 399) is 0 in float64, as is every later term of the 200)
        k = np.arange(1, 21, dtype=np.float64)
        sign = np.where(k % 2 == 1, 1.0, -1.0)
        for lo in range(0, len(hi), 1 << 16):
            idx = hi[lo:lo + (1 << 16)]
            z2 = flat[idx] ** 2
            t = (sign * np.exp(-2.0 * (k * k - 1.0) * z2[:, None])).sum(axis=1)
            out[idx] = (2.0 * z2 - np.log(2.0 * t)) / np.log(10.0)
    mid = np.flatnonzero((flat >= 0.04) & (flat < 1.0))
    if len(mid):
        mid = mid[np.argsort(flat[mid], kind="stable")]
        for lo in range(0, len(mid), 1 << 14):
            idx = mid[lo:lo + (1 << 14)]
            zz = flat[idx]
            # the terms with 2 k^2 z^2 > 760 are exactly 0 in float64: leaving them out changes nothing
            kmax = int(min(200, np.ceil(np.sqrt(380.0) / zz[0]) + 1))
            k = np.arange(1, kmax + 1, dtype=np.float64)
            sign = np.where(k % 2 == 1, 1.0, -1.0)
            q = 2.0 * (sign * np.exp(-2.0 * (k * k) * (zz * zz)[:, None])).sum(axis=1)
            out[idx] = -np.log10(np.clip(q, np.finfo(np.float64).tiny, 1.0))
    return out.reshape(z.shape)


def cofrag_bins(size: int, bin_size: int, contig: str = "the contig"):
    """``(starts, stops)`` of the bins ``[k * bin_size, min((k + 1) * bin_size, size))`` of a contig of ``size`` bases, int64;
    ``ValueError`` when there are more than 4096 (``FTK_COFRAG_MAX_BINS``)."""
    from . import _lib as L
    if int(bin_size) < 1:
        raise ValueError("bin_size must be at least 1")
    n_bins = -(-max(int(size), 0) // int(bin_size))
    if n_bins > L.COFRAG_MAX_BINS:
        raise ValueError(f"{contig}: {n_bins} bins of {int(bin_size)} bases; at most {L.COFRAG_MAX_BINS} bins per contig are "
                         f"supported - use a larger bin_size")
    starts = np.arange(n_bins, dtype=np.int64) * int(bin_size)
    return starts, np.minimum(starts + int(bin_size), int(size))


def cofrag_host_part(contig, starts, stops, n, overflow, K, at, len_lo: int, min_count: int = 1000, distance: str = "d") -> CoFragmentation:
    """The host's arithmetic of ``frag_cofragmentation`` on what the device returned (``Engine.cofrag`` / ``hist_ks``):
    the mask, ``D``, ``z``, ``neglog10_p``, the row correlation of the chosen distance and its first principal
    component.  ``at`` comes in as an index ``l`` and leaves as the length ``len_lo + l``."""
    if distance not in ("d", "z"):
        raise ValueError(f"invalid distance ({distance!r}): 'd' or 'z'")
    n = np.asarray(n, dtype=np.int64)
    K = np.asarray(K, dtype=np.int64)
    N = len(n)
    valid = n >= max(int(min_count), 1)
    pair = valid[:, None] & valid[None, :]
    nf = n.astype(np.float64)
    prod, tot = nf[:, None] * nf[None, :], nf[:, None] + nf[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.where(pair, K.astype(np.float64) / prod, np.nan)
        z = np.where(pair, D * np.sqrt(prod / tot), np.nan)
    p = np.full((N, N), np.nan)
    iu = np.triu_indices(N)
    p[iu] = ks_neglog10_p(z[iu])
    p.T[iu] = p[iu]
    corr = np.full((N, N), np.nan)
    pc1 = np.full(N, np.nan)
    v = np.flatnonzero(valid)
    if len(v) >= 3:
        m = (D if distance == "d" else z)[np.ix_(v, v)]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.corrcoef(m)
        corr[np.ix_(v, v)] = c
        w, vec = np.linalg.eigh(np.nan_to_num(c))
        e = vec[:, int(np.argmax(w))]
        if e[int(np.argmax(np.abs(e)))] < 0:
            e = -e
        pc1[v] = e
    return CoFragmentation(str(contig), np.asarray(starts, np.int64), np.asarray(stops, np.int64), n, np.asarray(overflow, np.int64),
                           K, (np.asarray(at, np.int32) + np.int32(len_lo)).astype(np.int32), valid, D, z, p, corr, pc1)


def frag_cofragmentation(input_file, bin_size: int = 500_000, contigs=None, chrom_sizes=None, min_length: int = 50,
                         max_length: int = 1000, quality_threshold: int = 30, min_count: int = 1000, distance: str = "d",
                         output_file=None, pairs_file=None, workers=None, verbose=False) -> list:
    """The co-fragmentation map of Liu et al. 2019: every contig of ``input_file`` (or those of ``contigs``) is cut into
    bins ``[k * bin_size, min((k + 1) * bin_size, chrom_size))``, the length distributions (``min_length .. max_length``, at
    most 4096 lengths) of the fragments with their midpoint in each bin are compared pair by pair with the two-sample
    Kolmogorov-Smirnov statistic, the rows of that distance matrix (``distance``: ``"d"`` the statistic, ``"z"`` scaled by
    ``sqrt(n_i n_j / (n_i + n_j))``) are correlated over the bins with at least ``min_count`` fragments, and the first
    principal component is the A/B-compartment track.  The histograms are built and compared on the GPU, contig by contig
    as the input is decoded (``Engine.cofrag``; the rule is in ``include/ftk.h``, "co-fragmentation"): the integer matrix K
    comes back, the float arithmetic on its N^2 values is the host's.  Needs no site list, reference or second sample.

    Chromosome sizes: the BAM header, else the ``chrom_sizes`` file, else ``ValueError``.  A contig of more than 4096 bins
    raises ``ValueError``.  Returns one ``CoFragmentation`` per contig, in the order the contigs are met.  ``output_file``
    (``.tsv`` / ``.tsv.gz``): ``writers.write_cofrag_track``; ``pairs_file``: ``writers.write_cofrag_pairs``."""
    import os
    import sys
    import time

    from . import _lib as L
    from . import writers
    from .source import ContigFeed
    _check_suffix(output_file, "output_file", "tsv")
    _check_suffix(pairs_file, "pairs_file", "tsv")
    if distance not in ("d", "z"):
        raise ValueError(f"invalid distance ({distance!r}): 'd' or 'z'")
    if int(bin_size) < 1:
        raise ValueError("bin_size must be at least 1")
    len_lo, n_len = int(min_length), int(max_length) - int(min_length) + 1
    if len_lo < 0 or n_len < 1 or n_len > L.COFRAG_MAX_LEN_BINS:
        raise ValueError(f"min_length .. max_length must hold 1 to {L.COFRAG_MAX_LEN_BINS} lengths from 0 up")
    if not _is_alignment_file(input_file) and chrom_sizes is None:
        raise ValueError("chrom_sizes is needed for an input without a header")
    t0 = time.time()
    sizes = None if _is_alignment_file(input_file) else chrom_sizes_to_dict(chrom_sizes)
    names = None if contigs is None else list(contigs)
    if sizes is not None and names is not None:
        for c in names:
            if c not in sizes:
                raise ValueError(f"{c} is not in chrom_sizes")
    results = []
    eng = get_engine()
    with ContigFeed(input_file, workers, names=names, require=() if names is None else names) as feed:
        for src, c in feed:
            if names is not None and c not in names:
                continue
            if sizes is not None and c not in sizes:
                raise ValueError(f"{c} is not in chrom_sizes")
            size = int(src.lengths[c]) if sizes is None else int(sizes[c])
            starts, stops = cofrag_bins(size, bin_size, c)
            if len(starts) == 0:
                continue
            K, at, n, over = eng.cofrag(src.key(c), starts, stops, len_lo, n_len, quality_threshold, len_lo, int(max_length))
            results.append(cofrag_host_part(c, starts, stops, n, over, K, at, len_lo, min_count, distance))
            if verbose:
                sys.stderr.write(f"frag_cofragmentation: {c}: {len(starts)} bins, {int(results[-1].valid.sum())} valid\n")
    if output_file is not None:
        writers.write_cofrag_track(os.fspath(output_file), results)
    if pairs_file is not None:
        writers.write_cofrag_pairs(os.fspath(pairs_file), results)
    if verbose:
        sys.stderr.write(f"frag_cofragmentation: {len(results)} contigs in {time.time() - t0:.3f} s\n")
    return results


def agg_bw(input_file, interval_file, output_file, median_window_size: int = 1, mean: bool = False,
           verbose: bool = False) -> np.ndarray:
    """Aggregate a bigWig signal across strand-oriented intervals (reference: ``utils/_agg_bw.py:18-146``):
    every interval's per-base values (NaN -> 0) are trimmed by the upstream median filter's window
    (``values[w // 2 : -w // 2]`` - with ``w = 0`` that slice is empty and every interval is skipped, as in the
    reference), flipped for ``-`` strand intervals, and summed; ``mean`` divides by the intervals added.  A host
    utility downstream of ``adjust_wps`` - file reading and a few vector additions, no kernel."""
    import gzip
    import time
    from sys import stderr

    from .bigwig import BigWigFile
    t0 = time.time()
    if not (str(interval_file).endswith(".bed") or str(interval_file).endswith(".bed.gz")):
        raise ValueError("Invalid filetype for interval_file.")
    intervals = []
    opener = gzip.open if str(interval_file).endswith(".gz") else open
    with opener(interval_file, "rt") as fh:
        for line in fh:
            f = line.split("\t")
            intervals.append((f[0], int(f[1]), int(f[2]), f[5].strip()))
    with BigWigFile(str(input_file)) as bw:
        interval_size = intervals[0][2] - intervals[0][1] - median_window_size
        agg = np.zeros(interval_size, dtype=np.int64)
        added = 0
        for contig, start, stop, strand in intervals:
            try:
                values = np.nan_to_num(bw.values(contig, start, stop), nan=0)
            except RuntimeError as e:
                print(e)
                continue
            trimmed = values[median_window_size // 2: -median_window_size // 2]
            if trimmed.shape[0] != interval_size:
                print(f"Trimmed size {trimmed.shape[0]} for {contig}:{start}-{stop} is not equal to "
                      f"interval size {interval_size}. Skipping.")
                continue
            if strand == "+":
                agg = agg + trimmed
                added += 1
            elif strand == "-":
                agg = agg + np.flip(trimmed)
                added += 1
            elif verbose:
                stderr.write("A segment without strand was encountered. Skipping.")
    if mean:
        agg = agg / added
    if not str(output_file).endswith("wig"):
        raise ValueError("The output_file is an unaccepted type. Must be a wiggle file ending in .wig")
    with open(output_file, "wt") as out:
        out.write(f"fixedStep\tchrom=.\tstart={-interval_size // 2}\tstep={1}\tspan={interval_size}\n")
        for score in agg:
            out.write(f"{score}\n")
    if verbose:
        stderr.write(f"Aggregating bigWig took {time.time() - t0} s to complete\n")
    return agg


# ---- small pure helpers of the reference's utility layer (kept so that `finaletoolkit.utils.<name>` resolves) --------
from .validation import valid_interval, validate_compatible_contigs  # noqa: E402

_COMPLEMENT = str.maketrans("ACGTacgt", "TGCATGCA")


def reverse_complement(kmer: str) -> str:
    """utils/utils.py:413-437: the reverse complement of a DNA string - A/C/G/T in either case give the upper-case
    complement, every other character (``N``) stays what it is."""
    return kmer.translate(_COMPLEMENT)[::-1]


def _none_leq(a, b) -> bool:
    """utils/_comparison.py: ``a <= b`` where a missing operand means "unbounded" (true)."""
    return a is None or b is None or a <= b


def _none_geq(a, b) -> bool:
    return a is None or b is None or a >= b


def _none_eq(a, b) -> bool:
    return a is None or b is None or a == b
