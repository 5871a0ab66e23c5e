"""
Command line of ``utils.frag_ocf``: BAM / fragment file + sites (BED) [+ reference (.2bit / FASTA)] -> the OCF score of
every group of sites (orientation-aware cfDNA fragmentation), with the fragment-end profiles and the per-site scores on
request, GC-corrected per fragment, counted on the GPU.

    python -m finaletoolkit_amd.ocf IN.frag.gz sites.bed.gz OUT.tsv.gz --profile ends.tsv.gz --per-site sites.tsv.gz --by-name
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.ocf",
                                 description="write the OCF scores of the sites of a BED file, per group of sites")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("site_file", metavar="SITES", help="sites (.bed or .bed.gz; column 4: name, column 6: strand)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.tsv or .tsv.gz): one row per group")
    ap.add_argument("--profile", dest="profile_file", default=None, metavar="F",
                    help="also write the U / D end profiles per group (.tsv or .tsv.gz)")
    ap.add_argument("--per-site", dest="site_output_file", default=None, metavar="F",
                    help="also write the window counts and the score of every site (.tsv or .tsv.gz)")
    ap.add_argument("--reference", dest="reference_file", default=None, metavar="REF",
                    help="reference genome (.2bit or FASTA): correct every fragment for GC bias")
    ap.add_argument("--bias", dest="bias", default=None, metavar="TSV",
                    help="length x GC bias table written by finaletoolkit_amd.gcbias (default: measured from IN first)")
    ap.add_argument("--half-width", dest="half_width", type=int, default=1000, metavar="N")
    ap.add_argument("--bin-size", dest="bin_size", type=int, default=1, metavar="N")
    ap.add_argument("--peak", dest="peak", type=int, default=60, metavar="N", help="distance of the two windows from the centre")
    ap.add_argument("--flank", dest="flank", type=int, default=10, metavar="N", help="half width of the two windows")
    ap.add_argument("--min-length", dest="min_length", type=int, default=50, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=350, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--by-name", dest="by_name", action="store_true", help="one score per site name (column 4)")
    ap.add_argument("--normalize", dest="normalize", action="store_true",
                    help="divide every group's profiles and score by the mean of its profiles")
    ap.add_argument("--min-bias", dest="min_bias", type=float, default=0.05, metavar="X",
                    help="cells with a bias below X get weight 0")
    ap.add_argument("--stride", dest="stride", type=int, default=1, metavar="N",
                    help="without --bias: sample every N-th reference position for the expected table")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_ocf
    frag_ocf(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
