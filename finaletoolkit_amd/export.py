"""
Command line of ``utils.frag_export``: BAM / fragment file -> filtered, tabix-indexed fragment file, formatted and
deflated on the GPU.

    python -m finaletoolkit_amd.export IN.bam OUT.frag.gz -q 30 --min-length 120 --max-length 180
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.export",
                                 description="export fragments to a tabix-indexed BGZF fragment file")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("output_file", metavar="OUT", help="output file (.gz / .bgz); OUT.tbi is written next to it")
    ap.add_argument("-c", "--contig", default=None, help="export this contig only")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("--min-length", dest="min_length", type=int, default=None, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=None, metavar="N")
    ap.add_argument("--layout", choices=["frag", "bed6", "bed3"], default="frag")
    ap.add_argument("-t", "--threads", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_export
    frag_export(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
