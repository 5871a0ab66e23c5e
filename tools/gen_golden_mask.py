"""
TEST INFRASTRUCTURE -- needs the reference package (imported through ``oracle.refstub.install()``).

Golden rows for the region-mask export (``utils.frag_filter``): the fragments come from the IMPORTED reference's
``frag_generator`` and the reference's own ``_make_intersect_checker`` (utils/_frag_generator.py:21-55) is applied per
mask interval - a row is in a mask when the checker holds for at least one interval of the row's contig; it is kept
when it is in the whitelist (if any) and not in the blacklist (if any).  Inputs: ``tests/data/12.3444.b37.frag.gz`` and
a small three-contig fragment file built by ``finaletoolkit_amd.synth`` from the recipe recorded in the fixture (the
tests rebuild it).  Mask sets hold overlapping, touching, unsorted and duplicate intervals, intervals placed on the
rows' own midpoints and ends, a contig the input lacks and an input contig the set lacks; both policies; whitelist
only, blacklist only, both.  Writes ``tests/golden/export_mask.json.gz`` (data only; byte-identical on every run).

Usage:  python tools/gen_golden_mask.py
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refstub  # noqa: E402

refstub.install()
from finaletoolkit.utils._frag_generator import _make_intersect_checker, frag_generator  # noqa: E402

from finaletoolkit_amd import bgzf, synth  # noqa: E402

SYNTH = dict(contigs=[["chrA", 240_000, 600, 901], ["chrB", 180_000, 500, 902], ["chrC", 100_000, 300, 903]])  # name, size, rows, seed
FILES = {"fixture": dict(path="tests/data/12.3444.b37.frag.gz", quality_threshold=0),
         "synth": dict(recipe=SYNTH, quality_threshold=30)}


def write_synth(path, recipe=SYNTH):
    """The synthetic input of the fixture (the tests call this recipe too, through their own copy of these lines)."""
    bgzf.write_frag_gz(path, [(n, *synth.synth_contig(size, seed=seed, n=rows)) for n, size, rows, seed in recipe["contigs"]])


def mask_sets(rows, seed):
    """{name: [[contig, start, stop], ...]} as they go into the BED files, in this (unsorted) order."""
    rng = np.random.default_rng(seed)
    contigs = list(dict.fromkeys(r[0] for r in rows))
    sparse, edges, messy = [], [], []
    for c in contigs:
        mine = [r for r in rows if r[0] == c]
        lo, hi = min(r[1] for r in mine), max(r[2] for r in mine)
        span = max((hi - lo) // 6, 50)
        sparse += [[c, lo + span, lo + 2 * span], [c, lo + 4 * span, lo + 4 * span + span // 2]]
        for k, r in enumerate(mine[::3]):  # intervals on the rows' own midpoints and ends
            mid = (r[1] + r[2]) // 2
            edges.append([[c, mid, mid + 1], [c, max(mid - 7, 0), mid], [c, mid + 1, mid + 9], [c, r[2], r[2] + 5],
                          [c, max(r[1] - 5, 0), r[1] + 1], [c, r[2] - 1, r[2] + 3]][k % 6])
    for c in contigs[:-1] if len(contigs) > 1 else contigs:  # (the last contig of a multi-contig input is not named)
        mine = [r for r in rows if r[0] == c]
        lo, hi = min(r[1] for r in mine), max(r[2] for r in mine)
        for _ in range(12):
            a = int(rng.integers(lo, hi))
            w = int(rng.integers(20, max((hi - lo) // 10, 40)))
            messy += [[c, a, a + w], [c, a + w, a + w + 30], [c, a + w // 2, a + w + 10]]  # touching, overlapping
        messy.append(messy[-1])  # a duplicate
    order = rng.permutation(len(messy))
    messy = [messy[i] for i in order] + [["chrNotInTheInput", 10, 500]]
    return {"sparse": sparse, "edges": edges[::-1], "messy": messy}


def in_mask(check, row, intervals):
    return any(check(a, b, row[1], row[2]) for c, a, b in intervals if c == row[0])


def text(rows):
    return "".join(f"{c}\t{s}\t{e}\t{q}\t{'+' if fwd else '-'}\n" for c, s, e, q, fwd in rows)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, spec in FILES.items():
            if "path" in spec:
                path = os.path.join(ROOT, spec["path"])
            else:
                path = os.path.join(tmp, "synth.frag.gz")
                write_synth(path)
            q = spec["quality_threshold"]
            rows = [tuple(r) for r in frag_generator(path, None, quality_threshold=q)]
            sets = mask_sets(rows, seed=len(rows))
            cases = []
            for policy in ("midpoint", "any"):
                check = _make_intersect_checker(policy)
                for wl, bl in (("sparse", None), (None, "sparse"), ("messy", None), (None, "messy"), ("edges", None),
                               (None, "edges"), ("messy", "edges"), ("sparse", "messy"), ("edges", "sparse")):
                    kept = [r for r in rows if (wl is None or in_mask(check, r, sets[wl]))
                            and (bl is None or not in_mask(check, r, sets[bl]))]
                    cases.append(dict(policy=policy, whitelist=wl, blacklist=bl, n=len(kept), rows=text(kept)))
            out[tag] = dict(spec, masks=sets, all_rows=text(rows), cases=cases)
    raw = json.dumps(out, sort_keys=True, separators=(",", ":")).encode()
    path = os.path.join(ROOT, "tests", "golden", "export_mask.json.gz")
    with open(path, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0, compresslevel=9) as gz:
        gz.write(raw)
    print("wrote", path, os.path.getsize(path), "bytes;",
          {t: (len(v["cases"]), [c["n"] for c in v["cases"]]) for t, v in out.items()})


if __name__ == "__main__":
    main()
