"""
Command line of ``utils.frag_wps_spectrum``: BAM / fragment file + intervals (BED) -> the periodogram of every
interval's WPS at the integer periods of a range and its mean over a band, scored and transformed on the GPU.

    python -m finaletoolkit_amd.spectrum IN.frag.gz genes.bed OUT.tsv.gz --chrom-sizes hg38.chrom.sizes
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.spectrum",
                                 description="write the WPS periodogram of every interval of a BED file")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("interval_file", metavar="INTERVALS", help="intervals (.bed or .bed.gz; column 4: name)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.tsv or .tsv.gz)")
    ap.add_argument("--chrom-sizes", dest="chrom_sizes", default=None, metavar="F",
                    help="chromosome sizes (needed for a fragment file; a BAM carries them in its header)")
    ap.add_argument("--min-period", dest="min_period", type=int, default=120, metavar="N")
    ap.add_argument("--max-period", dest="max_period", type=int, default=280, metavar="N")
    ap.add_argument("--band", dest="band", type=int, nargs=2, default=(193, 199), metavar=("LO", "HI"),
                    help="periods whose mean power is reported as band_mean")
    ap.add_argument("--window-size", dest="window_size", type=int, default=120, metavar="N")
    ap.add_argument("--min-length", dest="min_length", type=int, default=120, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=180, metavar="N")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="N")
    ap.add_argument("--taper", dest="taper", type=float, default=0.1, metavar="X",
                    help="fraction of an interval under the cosine bell at either end (0 .. 0.5)")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="N")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = vars(build_parser().parse_args(argv))
    args["band"] = tuple(args["band"])
    from .utils import frag_wps_spectrum
    frag_wps_spectrum(**args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
