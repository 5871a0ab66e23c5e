"""
Command line of ``utils.frag_filter``: BAM / fragment file -> fragment file filtered by MAPQ, length and region masks
(a whitelist and / or a blacklist BED), tabix-indexed, masked, formatted and deflated on the GPU.

    python -m finaletoolkit_amd.filter IN.bam OUT.frag.gz --whitelist panel.bed --blacklist encode.bed -q 30
"""
from __future__ import annotations

import sys


def build_parser():
    from .export import build_parser as export_parser
    ap = export_parser()
    ap.prog = "python -m finaletoolkit_amd.filter"
    ap.description = "filter fragments by MAPQ, length and region masks into a tabix-indexed BGZF fragment file"
    ap.add_argument("--whitelist", dest="whitelist_file", default=None, metavar="BED",
                    help="keep only fragments in these regions")
    ap.add_argument("--blacklist", dest="blacklist_file", default=None, metavar="BED",
                    help="drop fragments in these regions")
    ap.add_argument("-p", "--intersect-policy", dest="intersect_policy", choices=["midpoint", "any"], default="midpoint",
                    help="when a fragment is in a region: its midpoint lies in it, or any base overlaps it")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .utils import frag_filter
    frag_filter(**vars(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
