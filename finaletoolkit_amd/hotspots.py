"""
Command line of ``utils.frag_hotspots``: BAM / fragment file [+ intervals (BED)] -> fragmentation hotspots from the
Integrated Fragmentation Score - of every interval, or of every contig of the input - every window scored and
Poisson-tested on the GPU.

    python -m finaletoolkit_amd.hotspots IN.frag.gz OUT.bed.gz --chrom-sizes hg38.chrom.sizes --summary OUT.tsv
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.hotspots",
                                 description="write the IFS fragmentation hotspots of intervals or whole contigs")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="hotspots (.bed or .bed.gz)")
    ap.add_argument("--intervals", dest="interval_file", default=None, metavar="BED",
                    help="intervals to call (.bed or .bed.gz; column 4: name); without it every contig is called whole")
    ap.add_argument("--windows", dest="windows_file", default=None, metavar="F", help="the called windows (.bed or .bed.gz)")
    ap.add_argument("--summary", dest="summary_file", default=None, metavar="F",
                    help="per-interval mean length, mean IFS and counters (.tsv or .tsv.gz)")
    ap.add_argument("--chrom-sizes", dest="chrom_sizes", default=None, metavar="F",
                    help="chromosome sizes (needed for a fragment file; a BAM carries them in its header)")
    ap.add_argument("--step", dest="step", type=int, default=20, metavar="N", help="bases a window slides by")
    ap.add_argument("--window", dest="window", type=int, default=200, metavar="N",
                    help="bases per window, a multiple of the step (at most 64 steps)")
    ap.add_argument("--background", dest="background", type=int, nargs=2, default=(5000, 10000), metavar="N",
                    help="widths in bases of the two local backgrounds around a window")
    ap.add_argument("--alpha", dest="alpha", type=float, default=1e-5, metavar="X", help="level of the one-sided Poisson test")
    ap.add_argument("--mean-length", dest="mean_length", type=int, default=None, metavar="N",
                    help="mean fragment length the IFS is scaled by (default: each contig's own)")
    ap.add_argument("--no-global", dest="use_global", action="store_false", help="do not test against the contig's mean IFS")
    ap.add_argument("--min-count", dest="min_count", type=int, default=0, metavar="N", help="fewest fragments in a tested window")
    ap.add_argument("--join", dest="join", type=int, default=None, metavar="N",
                    help="called windows at most this many steps apart merge (default: window / step + 200 / step)")
    ap.add_argument("--min-windows", dest="min_windows", type=int, default=1, metavar="N", help="fewest called windows of a hotspot")
    ap.add_argument("--min-length", dest="min_length", type=int, default=None, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=None, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="N")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="N")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = vars(build_parser().parse_args(argv))
    args["background"] = tuple(args["background"])
    from .utils import frag_hotspots
    frag_hotspots(**args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
