"""
Command line of ``utils.frag_depth_track``: BAM / fragment file -> bedGraph depth track, one row per interval of
constant depth, run-length encoded on the GPU.

    python -m finaletoolkit_amd.depth IN.frag.gz OUT.bedgraph.gz -q 30 --min-length 120 --max-length 180
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.depth",
                                 description="write the per-base fragment depth of a file as a bedGraph track")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="output file (.bedgraph / .bg, or .bedgraph.gz / .bg.gz)")
    ap.add_argument("-c", "--contig", default=None, help="this contig only")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--min-length", dest="min_length", type=int, default=None, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=None, metavar="N")
    ap.add_argument("--include-zero", dest="include_zero", action="store_true",
                    help="keep the intervals of depth 0, so that the rows tile every contig")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_depth_track
    frag_depth_track(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
