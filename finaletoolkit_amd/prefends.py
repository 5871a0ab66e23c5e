"""
Command line of ``utils.frag_preferred_ends``: BAM / fragment file [+ intervals (BED)] -> preferred fragment-end
coordinates - of every interval, or of every contig of the input - every base Poisson-tested on the GPU.

    python -m finaletoolkit_amd.prefends IN.frag.gz OUT.bed.gz --chrom-sizes hg38.chrom.sizes --summary OUT.tsv
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.prefends",
                                 description="write the preferred fragment-end coordinates of intervals or whole contigs")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="calls (.bed or .bed.gz)")
    ap.add_argument("--intervals", dest="interval_file", default=None, metavar="BED",
                    help="intervals to call (.bed or .bed.gz; column 4: name); without it every contig is called whole")
    ap.add_argument("--summary", dest="summary_file", default=None, metavar="F",
                    help="per-interval counters and the share of ends on called positions (.tsv or .tsv.gz)")
    ap.add_argument("--chrom-sizes", dest="chrom_sizes", default=None, metavar="F",
                    help="chromosome sizes (needed for a fragment file; a BAM carries them in its header)")
    ap.add_argument("--half-window", dest="half_window", type=int, default=500, metavar="N",
                    help="bases on either side of a position that make up its window (1 .. 2048)")
    ap.add_argument("--alpha", dest="alpha", type=float, default=0.01, metavar="X", help="level of the one-sided Poisson test")
    ap.add_argument("--min-count", dest="min_count", type=int, default=2, metavar="N", help="fewest ends on a called position")
    ap.add_argument("--split", dest="split", action="store_true", help="test U and D ends apart (default: their sum)")
    ap.add_argument("--min-length", dest="min_length", type=int, default=None, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=None, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="N")
    ap.add_argument("--chunk-size", dest="chunk_size", type=int, default=1 << 22, metavar="N",
                    help="positions per chunk of a contig called whole")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="N")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = vars(build_parser().parse_args(argv))
    from .utils import frag_preferred_ends
    frag_preferred_ends(**args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
