"""
Command line of ``utils.frag_wps_peaks``: BAM / fragment file [+ intervals (BED)] -> nucleosome calls from the adjusted
WPS - of every interval, or of every contig of the input - scored, adjusted and called on the GPU.

    python -m finaletoolkit_amd.peaks IN.frag.gz OUT.bed.gz --chrom-sizes hg38.chrom.sizes --summary OUT.tsv
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.peaks",
                                 description="write nucleosome calls from the adjusted WPS of intervals or whole contigs")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="calls (.bed or .bed.gz)")
    ap.add_argument("--intervals", dest="interval_file", default=None, metavar="BED",
                    help="intervals to call (.bed or .bed.gz; column 4: name); without it every contig is called whole")
    ap.add_argument("--summary", dest="summary_file", default=None, metavar="F",
                    help="per-interval counters and call spacing (.tsv or .tsv.gz)")
    ap.add_argument("--chrom-sizes", dest="chrom_sizes", default=None, metavar="F",
                    help="chromosome sizes (needed for a fragment file; a BAM carries them in its header)")
    ap.add_argument("--window-size", dest="window_size", type=int, default=120, metavar="N")
    ap.add_argument("--min-length", dest="min_length", type=int, default=120, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=180, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="N")
    ap.add_argument("--median-window-size", dest="median_window_size", type=int, default=1000, metavar="N")
    ap.add_argument("--savgol-window-size", dest="savgol_window_size", type=int, default=21, metavar="N")
    ap.add_argument("--savgol-poly-deg", dest="savgol_poly_deg", type=int, default=2, metavar="N")
    ap.add_argument("--no-savgol", dest="savgol", action="store_false", help="call on the median-subtracted score")
    ap.add_argument("--max-gap", dest="max_gap", type=int, default=5, metavar="N",
                    help="positions without a positive score a region may bridge (0 .. 63)")
    ap.add_argument("--min-region", dest="min_region", type=int, default=50, metavar="N")
    ap.add_argument("--short-max", dest="short_max", type=int, default=150, metavar="N",
                    help="a region up to this long yields its one best window")
    ap.add_argument("--max-region", dest="max_region", type=int, default=450, metavar="N", help="longer regions are not called (<= 1024)")
    ap.add_argument("--chunk-size", dest="chunk_size", type=int, default=1 << 20, metavar="N",
                    help="positions per chunk of a contig called whole")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="N")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = vars(build_parser().parse_args(argv))
    from .utils import frag_wps_peaks
    frag_wps_peaks(**args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
