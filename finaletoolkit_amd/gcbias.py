"""
Command line of ``utils.frag_gc_bias``: BAM / fragment file + reference (.2bit / FASTA) -> the fragment length x GC
table (observed, expected, bias) as TSV, counted on the GPU.

    python -m finaletoolkit_amd.gcbias IN.frag.gz hg38.2bit OUT.tsv.gz -q 30 --min-length 100 --max-length 220
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.gcbias",
                                 description="write the fragment length x GC bias table of a file as TSV")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("reference_file", metavar="REF", help="reference genome (.2bit or FASTA)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.tsv or .tsv.gz)")
    ap.add_argument("-c", "--contig", default=None, help="this contig only")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--min-length", dest="min_length", type=int, default=100, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=220, metavar="N")
    ap.add_argument("--stride", dest="stride", type=int, default=1, metavar="N",
                    help="sample every N-th reference position for the expected table")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_gc_bias
    frag_gc_bias(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
