"""
Command line of ``utils.frag_cofragmentation``: BAM / fragment file -> the co-fragmentation map of every contig (pairwise
Kolmogorov-Smirnov distances between the fragment length distributions of large bins, compared on the GPU) and the
compartment track read off it, as TSV.

    python -m finaletoolkit_amd.cofrag IN.frag.gz OUT.tsv.gz --pairs PAIRS.tsv.gz --bin-size 500000 --chrom-sizes hg38.chrom.sizes
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.cofrag",
                                 description="write the co-fragmentation compartment track (and the bin pairs) of a file as TSV")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="track file (.tsv or .tsv.gz): contig start stop n_frags overflow valid pc1")
    ap.add_argument("--pairs", dest="pairs_file", default=None, metavar="F", help="also write the bin pairs i < j (.tsv or .tsv.gz)")
    ap.add_argument("--bin-size", dest="bin_size", type=int, default=500_000, metavar="N")
    ap.add_argument("--contigs", dest="contigs", nargs="+", default=None, metavar="C", help="these contigs only")
    ap.add_argument("--chrom-sizes", dest="chrom_sizes", default=None, metavar="F", help="needed for an input without a header")
    ap.add_argument("--min-length", dest="min_length", type=int, default=50, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=1000, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="N")
    ap.add_argument("--min-count", dest="min_count", type=int, default=1000, metavar="N",
                    help="a bin with fewer fragments takes no part in the correlation")
    ap.add_argument("--distance", choices=("d", "z"), default="d",
                    help="correlate the KS statistic, or the statistic scaled by sqrt(n_i n_j / (n_i + n_j))")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_cofragmentation
    frag_cofragmentation(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
