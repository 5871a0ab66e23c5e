"""
Command line of ``utils.frag_gc_coverage``: BAM / fragment file + reference (.2bit / FASTA) + intervals (BED) -> the
GC-bias-corrected coverage of every interval, the fragment weights applied and summed on the GPU.

    python -m finaletoolkit_amd.gccov IN.frag.gz hg38.2bit bins.bed OUT.bed.gz --bias bias.tsv.gz -q 30
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.gccov",
                                 description="write the GC-bias-corrected fragment coverage of BED intervals")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("reference_file", metavar="REF", help="reference genome (.2bit or FASTA)")
    ap.add_argument("interval_file", metavar="INTERVALS", help="intervals (BED)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.bed or .bed.gz)")
    ap.add_argument("--bias", dest="bias", default=None, metavar="TSV",
                    help="length x GC bias table written by finaletoolkit_amd.gcbias (default: measured from IN first)")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--min-length", dest="min_length", type=int, default=100, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=220, metavar="N")
    ap.add_argument("--policy", dest="intersect_policy", choices=("midpoint", "any"), default="midpoint")
    ap.add_argument("--min-bias", dest="min_bias", type=float, default=0.05, metavar="X",
                    help="cells with a bias below X get weight 0")
    ap.add_argument("--stride", dest="stride", type=int, default=1, metavar="N",
                    help="without --bias: sample every N-th reference position for the expected table")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_gc_coverage
    frag_gc_coverage(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
