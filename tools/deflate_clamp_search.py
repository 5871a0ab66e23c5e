#!/usr/bin/env python3
"""Find texts for ``CLAMP_CASES`` of ``tests/test_gpu_deflate_choices.py``: one-block inputs whose dynamic header makes
the device compressor's code-length code over-subscribe when its Shannon lengths are cut to 7 bits (the only way into
the ``kraft > cap`` loop of ``code_lengths`` in ``csrc/ftk_fragtext.hip``).  Needs a GPU.

    python tools/deflate_clamp_search.py --seconds 120 --seed 1

Each printed line is ``fill total (lengths, counts, seed, permute)``: paste the tuple into ``CLAMP_CASES``."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import deflate_tokens as D  # noqa: E402
from test_gpu_deflate_choices import class_block  # noqa: E402
from test_gpu_frag_export import split_members  # noqa: E402

COUNTS = (1, 2, 3, 4, 8, 16, 32, 64, 128)


def header_fill(payload):
    """``(fill, total)`` of the first block's header: the Shannon lengths of its code-length symbols, cut at 7, in
    units of 2^-7 (above 128: over-subscribed); ``None`` for a block that is not dynamic."""
    b = D.inflate(payload)[0][0]
    if b.btype != "dynamic":
        return None
    syms = [s for s, _ in b.cl_symbols]
    total = len(syms)
    counts = [syms.count(s) for s in set(syms)]
    return sum(1 << (7 - min(7, next(l for l in range(1, 16) if (c << l) >= total))) for c in counts), total


def search(deflate, seconds, seed):
    """``deflate(text) -> (image, offs)`` (``Engine.bgzf_deflate``); yields ``(fill, total, case)``."""
    rnd = random.Random(seed)
    t0 = time.time()
    while time.time() - t0 < seconds:
        lengths = rnd.sample(range(4, 13), rnd.randint(5, 8))
        counts = [rnd.choice(COUNTS) for _ in lengths]
        size = sum(c << (13 - ln) for c, ln in zip(counts, lengths))
        if not (200 <= sum(counts) <= 254 and 6000 < size <= 8191):
            continue
        case = (tuple(lengths), tuple(counts), rnd.randint(0, 10**6), rnd.random() < 0.5)
        image, _ = deflate(class_block(*case))
        got = header_fill(split_members(image[:-28])[0][0])
        if got and got[0] > 128:
            yield got[0], got[1], case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from finaletoolkit_amd.engine import Engine
    with Engine(0) as eng:
        for fill, total, case in search(eng.bgzf_deflate, args.seconds, args.seed):
            print(fill, total, case, flush=True)


if __name__ == "__main__":
    main()
