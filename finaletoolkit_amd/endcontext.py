"""
Command line of ``utils.frag_end_context``: BAM / fragment file + reference (.2bit / FASTA) -> the nucleotide and
dinucleotide profiles around the fragment ends, per fragment length class, as TSV, counted on the GPU.

    python -m finaletoolkit_amd.endcontext IN.frag.gz hg38.2bit OUT.tsv.gz -q 30 --half-width 32 --length-edges 1 150 221 1001
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.endcontext",
                                 description="write the base and base-pair profiles around a file's fragment ends as TSV")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("reference_file", metavar="REF", help="reference genome (.2bit or FASTA)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.tsv or .tsv.gz)")
    ap.add_argument("-c", "--contig", default=None, help="this contig only")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--half-width", dest="half_width", type=int, default=32, metavar="N",
                    help="offsets -N .. N - 1 around each end (at most 128)")
    ap.add_argument("--length-edges", dest="length_edges", type=int, nargs="+", default=(1, 150, 221, 1001), metavar="N",
                    help="ascending bounds of the fragment length classes: class c holds edges[c] <= length < edges[c + 1]")
    ap.add_argument("--anchor", choices=("ends", "centre"), default="ends",
                    help="read around the fragment ends, or around the fragment centre")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    args.length_edges = tuple(args.length_edges)
    from .utils import frag_end_context
    frag_end_context(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
