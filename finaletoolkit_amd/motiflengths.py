"""
Command line of ``utils.frag_motif_lengths``: BAM / fragment file + reference (.2bit / FASTA) -> the end-motif (or
breakpoint-motif) counts per fragment length as TSV, and the motif diversity score per length, counted on the GPU.

    python -m finaletoolkit_amd.motiflengths IN.frag.gz hg38.2bit OUT.tsv.gz --summary MDS.tsv -k 4 --max-length 600 -q 30
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m finaletoolkit_amd.motiflengths",
                                 description="write a file's end-motif counts per fragment length as TSV")
    ap.add_argument("input_file", metavar="IN", help="BAM, or a tabix-indexed fragment file / BED6")
    ap.add_argument("reference_file", metavar="REF", help="reference genome (.2bit or FASTA)")
    ap.add_argument("output_file", metavar="OUT", help="output file (.tsv or .tsv.gz): one row per non-zero cell")
    ap.add_argument("--summary", dest="summary_file", default=None, metavar="F",
                    help="per-length summary (.tsv or .tsv.gz): fragments, undefined readings, motif diversity scores")
    ap.add_argument("-c", "--contig", default=None, help="this contig only")
    ap.add_argument("-k", dest="k", type=int, default=4, metavar="N", help="motif length, 1 .. 4")
    ap.add_argument("--kind", choices=("end", "breakpoint"), default="end",
                    help="end motifs (the first k bases of each end) or breakpoint motifs (k / 2 bases either side of it)")
    ap.add_argument("--min-length", dest="min_length", type=int, default=1, metavar="N")
    ap.add_argument("--max-length", dest="max_length", type=int, default=1000, metavar="N")
    ap.add_argument("--length-bin", dest="length_bin", type=int, default=1, metavar="N",
                    help="lengths per row (at most 1024 rows)")
    ap.add_argument("-q", "--min-mapq", dest="quality_threshold", type=int, default=30, metavar="Q")
    ap.add_argument("-w", "--workers", dest="workers", type=int, default=None, metavar="WORKERS")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_motif_lengths
    frag_motif_lengths(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
