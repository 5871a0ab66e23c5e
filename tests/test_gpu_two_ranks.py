"""GPU: the multi-rank product path with HIP compute.  Two rank processes share GPU 0 (exchange over gloo
host copies, what a 1-GPU box allows); each decodes and counts only ITS contigs on the device, the bin vectors
meet in one all-gather, and every rank must return exactly what a single process returns
(reference fan-out: frag/_delfi.py:289-300, frag/_coverage.py:212-248).  Also: ``bench.py --gpus N`` starts N
ranks or fails loudly -- it never benchmarks fewer GPUs than asked for."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = H.ROOT

WORKER = r"""
import os, pickle, sys, warnings
sys.path.insert(0, {root!r})
from finaletoolkit_amd import frag, sharding
rank, world = sharding.init_from_env()
d = {tmp!r}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    df = frag.delfi(d + "/g.frag.gz", d + "/cs.genome", d + "/bins.txt", d + "/ref.fa", blacklist_file=d + "/bl.bed",
                    gap_file=d + "/gaps.bed", no_gc_correct=True, remove_nocov=False, merge_bins=False,
                    output_file=d + f"/delfi_w{{world}}.tsv")
    from finaletoolkit_amd import source as _src
    loaded_delfi = sorted(k.split(":", 1)[1] for k in _src.get_engine().contigs)  # whole contigs this rank decoded for it
    regions = [r[1:] for r in _src.REGION_READS]                                   # ... and the parts of contigs
    merged = frag.delfi(d + "/g.frag.gz", d + "/cs.genome", d + "/bins.txt", d + "/ref.fa", gap_file=d + "/gaps.bed",
                        no_gc_correct=True, remove_nocov=False, merge_bins=True)
cov = frag.coverage(d + "/g.frag.gz", d + "/iv.bed", d + f"/cov_w{{world}}.bed", normalize=True, scale_factor=1e6)
raw = frag.coverage(d + "/g.frag.gz", d + "/iv.bed", None, intersect_policy="any", min_length=100, max_length=220)
from finaletoolkit_amd.source import get_engine
loaded = sorted(k.split(":", 1)[1] for k in get_engine().contigs)
pickle.dump(dict(rank=rank, world=world, delfi=df, merged=merged, cov=[tuple(c) for c in cov],
                 raw=[tuple(c) for c in raw], loaded=loaded, loaded_delfi=loaded_delfi, regions=regions),
            open(d + f"/out_w{{world}}_r{{rank}}.pkl", "wb"))
sharding.finalize()
"""

# the other fan-outs of the reference (frag/_multi_wps.py:196-198, _frag_length.py:571-593, _cleavage_profile.py:372,
# _motif_common.py:635-685): per-base outputs assembled by rank 0 from the ranks' compressed pieces, statistics and
# k-mer tables gathered
WORKER2 = r"""
import os, pickle, sys, warnings
sys.path.insert(0, {root!r})
os.environ["FTK_SHARD_OVERHEAD_BASES"] = "0"  # contigs under 1 Mb: the shares are cut by the intervals' span alone
os.environ["FTK_UNIT_BASES"] = "20000"        # ... and the per-base commands' units hold a few intervals each
from finaletoolkit_amd import frag, sharding, source
rank, world = sharding.init_from_env()
d = {tmp!r}
o = d + f"/w{{world}}_"
trail = {{}}  # command -> (contigs this rank decoded WHOLE for it, regions it read through the index)
def ran(name, call):
    source.close_all()            # every command starts with nothing resident
    del source.REGION_READS[:]
    out = call()
    trail[name] = (sorted(k.split(":", 1)[1] for k in source.get_engine().contigs if "@" not in k),
                   [tuple(r[1:]) for r in source.REGION_READS])
    return out
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    ran("wps.bw", lambda: frag.multi_wps(d + "/g.frag.gz", d + "/sites.bed", d + "/cs.genome", o + "wps.bw", interval_size=3000))
    ran("wps.bed.gz", lambda: frag.multi_wps(d + "/g.frag.gz", d + "/sites.bed", d + "/cs.genome", o + "wps.bed.gz",
                                             interval_size=800, window_size=61, min_length=100, max_length=200))
    ran("clv.bw", lambda: frag.multi_cleavage_profile(d + "/g.frag.gz", d + "/clv.bed", d + "/cs.genome", left=20, right=30,
                                                      output_file=o + "clv.bw"))
    ran("clv2.bw", lambda: frag.multi_cleavage_profile(d + "/g.frag.gz", d + "/clv_unsorted.bed", d + "/cs.genome",
                                                       output_file=o + "clv2.bw"))
    ran("clv.bed.gz", lambda: frag.multi_cleavage_profile(d + "/g.frag.gz", d + "/clv.bed", d + "/cs.genome", min_length=100,
                                                          max_length=250, output_file=o + "clv.bed.gz"))
    fli = ran("fli", lambda: frag.frag_length_intervals(d + "/g.frag.gz", d + "/iv.bed", o + "fli.bed", min_length=50,
                                                        max_length=400))
    flb = ran("flb", lambda: frag.frag_length_bins(d + "/g.frag.gz", output_file=o + "flb.tsv", bin_size=5,
                                                   summary_stats=True, short_fraction=150))
    flb1 = ran("flb1", lambda: frag.frag_length_bins(d + "/g.frag.gz", contig="c3", start=1000, stop=300000,
                                                     output_file=o + "flb1.tsv"))
    em = ran("em", lambda: frag.end_motifs(d + "/g.frag.gz", d + "/ref.fa", k=3, output_file=o + "em.tsv"))
    iem = ran("iem", lambda: frag.interval_end_motifs(d + "/g.frag.gz", d + "/ref.fa", d + "/iv.bed", k=2, both_strands=False,
                                                      output_file=o + "iem.tsv"))
    ibm = ran("ibm", lambda: frag.interval_breakpoint_motifs(d + "/g.frag.gz", d + "/ref.fa", d + "/iv.bed", k=4,
                                                             output_file=o + "ibm.csv"))
    cov = ran("cov", lambda: frag.coverage(d + "/g.frag.gz", d + "/iv.bed", o + "cov.bed", intersect_policy="any"))
    one = ran("one", lambda: frag.wps(d + "/g.frag.gz", "c2", 5000, 9000, 700000, output_file=o + "one.wig"))
pickle.dump(dict(rank=rank, world=world, fli=[tuple(x) for x in fli], flb=(list(map(int, flb[0])), list(flb[1])),
                 flb1=(list(map(int, flb1[0])), list(flb1[1])), em=list(em), iem=[(iv, dict(f)) for iv, f in iem],
                 ibm=[(iv, dict(f)) for iv, f in ibm], one=one.tolist(), cov=[tuple(c) for c in cov], trail=trail),
            open(d + f"/out2_w{{world}}_r{{rank}}.pkl", "wb"))
sharding.finalize()
"""


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from finaletoolkit_amd import bgzf, synth
    d = tmp_path_factory.mktemp("two_ranks")
    sizes = {"c1": 900_000, "c2": 700_000, "c3": 420_000, "c4": 350_000, "c5": 130_000}
    rows = []
    for i, (c, n) in enumerate(sizes.items()):
        s, e, q, st = synth.synth_contig(n, depth=6.0, seed=900 + i)
        rows.append((c, s, e, q, st))
    bgzf.write_frag_gz(d / "g.frag.gz", rows, level=1, with_index=True)
    (d / "cs.genome").write_text("".join(f"{c}\t{n}\n" for c, n in sizes.items()))
    (d / "bins.txt").write_text("".join(f"{c}\t{a}\t{min(a + 9_999, n)}\n" for c, n in sizes.items()
                                        for a in range(0, n, 10_000)))
    seqs = {}
    rng = np.random.default_rng(4)
    for c, n in sizes.items():
        seqs[c] = np.frombuffer(b"ACGTNacgt", np.uint8)[rng.integers(0, 9, n)].tobytes().decode()
    H.write_fasta(d / "ref.fa", seqs)
    (d / "gaps.bed").write_text("".join(
        f"{c}\t0\t10000\ttelomere\n{c}\t{n // 2 // 10000 * 10000}\t{n // 2 // 10000 * 10000 + 30000}\tcentromere\n"
        f"{c}\t{n - 10000}\t{n}\ttelomere\n" for c, n in sizes.items()))
    bl = []
    for c, n in sizes.items():
        for a in rng.integers(0, n - 3000, 25):
            bl.append(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(100, 2500))}\n")
    (d / "bl.bed").write_text("".join(bl))
    iv = []
    for c, n in sizes.items():
        for k, a in enumerate(rng.integers(0, n - 5000, 40)):
            iv.append(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(1, 5000))}\t{c}_{k}\n")
    rng.shuffle(iv)  # interval order is file order, not contig order
    (d / "iv.bed").write_text("".join(iv))
    (d / "worker.py").write_text(WORKER.format(root=ROOT, tmp=str(d)))
    (d / "worker2.py").write_text(WORKER2.format(root=ROOT, tmp=str(d)))
    # WPS sites in file (not contig) order, some overlapping their neighbours, one on a contig the genome lacks
    sites = []
    for c, n in sizes.items():
        for a in np.sort(rng.integers(0, n - 2000, 30)):
            sites.append(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(1, 1500))}\n")
    sites.insert(7, "cX\t100\t200\n")
    order = rng.permutation(len(sizes))
    names = list(sizes)
    by_c = {c: [x for x in sites if x.split("\t")[0] == c] for c in names + ["cX"]}
    (d / "sites.bed").write_text("".join("".join(by_c[names[i]]) for i in order) + "".join(by_c["cX"]))
    # cleavage intervals: sorted and merged-on-overlap in one file; contigs out of header order in the other (pyBigWig
    # refuses a contig that comes back: those intervals are skipped with a note)
    clv = []
    for c, n in sizes.items():
        for a in np.sort(rng.integers(0, n - 3000, 25)):
            clv.append((c, int(a), int(a) + int(rng.integers(10, 2500))))
    (d / "clv.bed").write_text("".join(f"{c}\t{a}\t{b}\n" for c, a, b in clv))
    back = [x for x in clv if x[0] == "c4"] + [x for x in clv if x[0] == "c2"] + [x for x in clv if x[0] == "c5"]
    (d / "clv_unsorted.bed").write_text("".join(f"{c}\t{a}\t{b}\n" for c, a, b in back))
    return d


def _run_world(d, world, script="worker.py", out="out"):
    from finaletoolkit_amd import sharding
    env_keep = {k: os.environ.get(k) for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for k in env_keep:
        os.environ.pop(k, None)
    try:
        if world == 1:
            rc = subprocess.run([sys.executable, str(d / script)], cwd=ROOT).returncode
        else:
            rc = sharding.launch_ranks([sys.executable, str(d / script)], world, share_gpu=True)
    finally:
        for k, v in env_keep.items():
            if v is not None:
                os.environ[k] = v
    assert rc == 0
    return [pickle.load(open(d / f"{out}_w{world}_r{r}.pkl", "rb")) for r in range(world)]


def test_two_ranks_equal_one_process(dataset):
    d = dataset
    one = _run_world(d, 1)[0]
    two = _run_world(d, 2)
    assert [r["world"] for r in two] == [2, 2]
    for r in two:  # every rank returns the single-process result, bit for bit
        assert r["delfi"].equals(one["delfi"]) and r["merged"].equals(one["merged"])
        assert r["cov"] == one["cov"] and r["raw"] == one["raw"]
    assert one["delfi"]["num_frags"].sum() > 10_000 and len(one["cov"]) == 200
    # and rank 0 alone wrote the files, identical to the single-process ones
    assert open(d / "delfi_w2.tsv").read() == open(d / "delfi_w1.tsv").read()
    assert open(d / "cov_w2.bed").read() == open(d / "cov_w1.bed").read()
    # the work really was dealt out.  delfi: the bins of all contigs cut into two runs of equal cost
    # (sharding.split_counts) - each rank decoded its whole contigs and read its PART of the contig the cut falls
    # into as a region through the index (the table dropped again); no contig decoded whole by both
    a, b = set(two[0]["loaded_delfi"]), set(two[1]["loaded_delfi"])
    ra, rb = two[0]["regions"], two[1]["regions"]
    assert a and b and not (a & b), (a, b)
    assert len(ra) == 1 and len(rb) == 1 and ra[0][0] == rb[0][0] and ra[0][0] not in a | b, (ra, rb)
    assert ra[0][2] <= rb[0][1] + 20_000 and a | b | {ra[0][0]} == {"c1", "c2", "c3", "c4", "c5"}  # (the two parts meet)
    assert one["regions"] == [] and set(one["loaded"]) == {"c1", "c2", "c3", "c4", "c5"}


def test_two_ranks_write_the_single_process_files_for_every_sharded_command(dataset):
    """multi_wps, multi_cleavage_profile, frag_length_intervals, genome-wide frag_length_bins and the motif
    drivers: two ranks on GPU 0 return what one process returns and rank 0 writes byte-identical files (.bw and
    .bed.gz assembled from the ranks' compressed pieces)."""
    import gzip
    d = dataset
    one = _run_world(d, 1, "worker2.py", "out2")[0]
    two = _run_world(d, 2, "worker2.py", "out2")
    for r in two:
        for key in ("fli", "flb", "flb1", "em", "iem", "ibm", "one", "cov"):
            assert r[key] == one[key], key
    assert len(one["fli"]) == 200 and sum(x[9] for x in one["fli"] if x[9] > 0) > 1000
    for name in ("wps.bw", "clv.bw", "clv2.bw", "fli.bed", "flb.tsv", "flb1.tsv", "em.tsv", "iem.tsv", "ibm.csv", "one.wig",
                 "cov.bed"):
        a, b = open(d / f"w1_{name}", "rb").read(), open(d / f"w2_{name}", "rb").read()
        assert a == b and len(a) > 100, name
    for name in ("wps.bed.gz", "clv.bed.gz"):
        a, b = gzip.open(d / f"w1_{name}").read(), gzip.open(d / f"w2_{name}").read()
        assert a == b and a.count(b"\n") > 10_000, name
        assert open(d / f"w1_{name}", "rb").read() == open(d / f"w2_{name}", "rb").read(), name  # members too
    # the bigWigs hold what the kernels computed (the reader is the product's own, validated against pyBigWig files)
    from finaletoolkit_amd.bigwig import BigWigFile
    with BigWigFile(d / "w2_clv2.bw") as bw:
        assert bw.intervals("c4", 0, 350_000) is not None and bw.intervals("c5", 0, 130_000) is not None
        assert bw.intervals("c2", 0, 700_000) is None  # c2 came back after c4: skipped, as pyBigWig's addEntries raises
    # ONE partition for every sharded command (sharding.IntervalPlan / frag/_runs.py: equal-cost consecutive shares):
    # a contig is decoded whole by at most one rank, the contig the cut falls into is read by BOTH ranks as a region
    # through the index - each its own part - and a single process never reads a region
    everything = {"c1", "c2", "c3", "c4", "c5"}
    for cmd in ("wps.bw", "wps.bed.gz", "clv.bw", "clv.bed.gz", "fli", "iem", "ibm", "cov"):  # (em: one 1 Mb window per contig here)
        assert one["trail"][cmd][1] == [], cmd
        (w0, r0), (w1, r1) = two[0]["trail"][cmd], two[1]["trail"][cmd]
        assert not (set(w0) & set(w1)), (cmd, w0, w1)
        assert len(r0) == 1 and len(r1) == 1 and r0[0][0] == r1[0][0] and r0[0][0] not in set(w0) | set(w1), (cmd, r0, r1)
        assert r0[0][1:] != r1[0][1:] and set(w0) | set(w1) | {r0[0][0]} == everything, (cmd, w0, w1, r0, r1)
    # whole-file commands (every fragment counts once) stay dealt by whole contigs: no region, nothing decoded twice
    (w0, r0), (w1, r1) = two[0]["trail"]["flb"], two[1]["trail"]["flb"]
    assert r0 == [] and r1 == [] and not (set(w0) & set(w1)) and set(w0) | set(w1) == everything


def test_cli_refuses_gpus_on_commands_that_do_not_shard(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "gaps.bed"
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.cli", "--gpus", "2", "gap-bed", "hg19", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 2 and "does not shard" in r.stderr and not out.exists()
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.cli", "adjust-wps", "x.bw", "y.bed", "z.sizes", "-o",
                        str(tmp_path / "o.bw")], cwd=ROOT, env=dict(env, WORLD_SIZE="2", RANK="1", LOCAL_RANK="1"),
                       capture_output=True, text=True)
    assert r.returncode == 2 and "does not shard" in r.stderr


def test_cli_gpus_2_wps_and_frag_length_intervals(dataset, tmp_path):
    d = dataset
    for cmd, tail, name in (("wps", [str(d / "sites.bed"), "--chrom-sizes", str(d / "cs.genome"), "-i", "2000"], "w.bw"),
                            ("frag-length-intervals", [str(d / "iv.bed")], "f.bed")):
        outs = {}
        for world in (1, 2):
            out = tmp_path / f"w{world}_{name}"
            env = dict(os.environ, FTK_SHARE_GPU="1")
            for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
                env.pop(k, None)
            r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.cli", "--gpus", str(world), cmd,
                                str(d / "g.frag.gz")] + tail + ["-o", str(out)], cwd=ROOT, env=env, capture_output=True,
                               text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[world] = open(out, "rb").read()
        assert outs[1] == outs[2] and len(outs[1]) > 1000, cmd


def test_cli_gpus_2_writes_the_single_process_file(dataset, tmp_path):
    d = dataset
    outs = {}
    for world in (1, 2):
        out = tmp_path / f"cli_w{world}.tsv"
        env = dict(os.environ, FTK_SHARE_GPU="1")
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.cli", "--gpus", str(world), "delfi",
                            str(d / "g.frag.gz"), str(d / "cs.genome"), str(d / "ref.fa"), str(d / "bins.txt"),
                            "-b", str(d / "bl.bed"), "-g", str(d / "gaps.bed"), "--no-gc-correct", "--no-remove-nocov", "--no-merge-bins",
                            "-o", str(out)],
                           cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[world] = open(out).read()
    assert outs[1] == outs[2] and outs[1].count("\n") > 5


def test_bench_gpus_n_never_runs_fewer_ranks(tmp_path):
    """`python bench.py --gpus N` on a box with fewer than N devices exits non-zero with a clear message; a
    launcher that started a different number of ranks than --gpus is refused too."""
    import torch
    have = torch.cuda.device_count()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", str(have + 1), "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       env=env, capture_output=True, text=True)
    assert r.returncode != 0 and f"needs {have + 1} visible" in r.stderr and not r.stdout.strip()
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True)
    assert r.returncode != 0 and "must agree" in r.stderr


def test_bench_plain_run_is_the_headline_alone():
    """Without --full, bench.py prints the headline line (with the last timed step's roofline and the checks of its
    results) and runs nothing else: no CPU baseline, no kernel rows, no file -> result legs."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--contigs", "21,22"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "windows/s" and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"]
    assert line["n_gpus"] == 1 and line["checks"] and all(line["checks"].values()), line["checks"]
    assert line["roofline"]["achieved"] > 0 and "bam_kernels" not in line["roofline"]
    assert line["cpu_baseline"] is None and line["next_rows"] is None and line["end_to_end"] is None


def test_bench_two_ranks_share_the_gpu():
    """bench.py's own N-rank path (unit split, per-rank launches, all-gather of the DELFI vector) with two ranks
    on GPU 0: one JSON line from rank 0, n_gpus 2, every check true."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(FTK_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--contigs",
                        "20,21,22", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["checks"] and all(line["checks"].values()), line["checks"]
    assert "gloo" in line["exchange"] and "2 ranks" in line["exchange"]
    # the N-rank file leg: ONE indexed file -> frag.delfi on both ranks (each decodes its own contigs), same frame
    leg = line["end_to_end"]["genome_frag_delfi_api_ranks"]
    assert leg["ranks"] == 2 and leg["results_ok"] and leg["merged_rows"] > 10, line["end_to_end"]
    # three contigs, two equal-cost runs of bins: a whole contig and a region of the middle one for each rank
    assert sorted(r["contigs_decoded"] for r in leg["per_rank"]) == [1, 1]
    assert [len(r["regions_read"]) for r in leg["per_rank"]] == [1, 1] and \
        leg["per_rank"][0]["regions_read"][0][0] == leg["per_rank"][1]["regions_read"][0][0]
    assert all(r["decoder_threads"] >= 1 and r["stages_s"]["total"] > 0 for r in leg["per_rank"])


def test_bench_eight_ranks_share_the_gpu():
    """The whole `bench.py --gpus 8` path - the world size the product is sized for - with eight ranks on GPU 0 (gloo
    exchange): unit split of eight contigs (17-22, X, Y) into eight equal-cost runs, per-rank launches, the all-gather
    of the DELFI vector, and the N-rank file leg (ONE indexed file, eight `frag.delfi` ranks, every cut contig read as
    regions through the index by the ranks that share it).  What a first run on a real 8-GPU node must not discover."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(FTK_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--steps", "2", "--warmup", "1", "--contigs",
                        "17,18,19,20,21,22,X,Y", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=2400)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 8 and line["checks"] and all(line["checks"].values()), line["checks"]
    assert "gloo" in line["exchange"] and "8 ranks" in line["exchange"]
    leg = line["end_to_end"]["genome_frag_delfi_api_ranks"]
    assert leg["ranks"] == 8 and leg["results_ok"] and leg["merged_rows"] > 50, line["end_to_end"]
    per = leg["per_rank"]
    assert len(per) == 8 and sorted(x["rank"] for x in per) == list(range(8))
    # eight contigs, eight equal-cost runs: every rank reads at least one region (a cut falls into almost every
    # contig), a contig is decoded whole by at most one rank, and every region read names one of the run's contigs
    assert all(len(x["regions_read"]) >= 1 for x in per)
    assert sum(x["contigs_decoded"] for x in per) + len({r[0] for x in per for r in x["regions_read"]}) == 8
    assert all(x["decoder_threads"] >= 1 and x["stages_s"]["total"] > 0 for x in per)


# ---- the same fan-outs on a BAM (BASELINE config 5's input; reference io/alignment.py:242-268) -------------------------------
WORKER3 = r"""
import os, pickle, sys, warnings
sys.path.insert(0, {root!r})
os.environ["FTK_SHARD_OVERHEAD_BASES"] = "0"
os.environ["FTK_UNIT_BASES"] = "20000"
from finaletoolkit_amd import frag, sharding, source
rank, world = sharding.init_from_env()
d = {tmp!r}
o = d + f"/b{{world}}_"
trail = {{}}
def ran(name, call):
    source.close_all()
    del source.REGION_READS[:]
    out = call()
    trail[name] = (sorted(k.split(":", 1)[1] for k in source.get_engine().contigs if "@" not in k),
                   [tuple(r[1:]) for r in source.REGION_READS])
    return out
bam = d + "/p.bam"
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    df = ran("delfi", lambda: frag.delfi(bam, d + "/cs.genome", d + "/bins.txt", d + "/ref.fa", blacklist_file=d + "/bl.bed",
                                         gap_file=d + "/gaps.bed", no_gc_correct=True, remove_nocov=False, merge_bins=False,
                                         output_file=o + "delfi.tsv"))
    cov = ran("cov", lambda: frag.coverage(bam, d + "/iv.bed", o + "cov.bed", normalize=True, scale_factor=1e6))
    ran("wps.bw", lambda: frag.multi_wps(bam, d + "/sites.bed", d + "/cs.genome", o + "wps.bw", interval_size=3000))
    ran("clv.bed.gz", lambda: frag.multi_cleavage_profile(bam, d + "/clv.bed", d + "/cs.genome", left=20, right=30,
                                                          output_file=o + "clv.bed.gz"))
    fli = ran("fli", lambda: frag.frag_length_intervals(bam, d + "/iv.bed", o + "fli.bed", min_length=50, max_length=400))
    iem = ran("iem", lambda: frag.interval_end_motifs(bam, d + "/ref.fa", d + "/iv.bed", k=2, output_file=o + "iem.tsv"))
pickle.dump(dict(rank=rank, world=world, delfi=df, cov=[tuple(c) for c in cov], fli=[tuple(x) for x in fli],
                 iem=[(iv, dict(f)) for iv, f in iem], trail=trail), open(d + f"/out3_w{{world}}_r{{rank}}.pkl", "wb"))
sharding.finalize()
"""


@pytest.fixture(scope="module")
def bam_dataset(tmp_path_factory):
    from finaletoolkit_amd import synth
    d = tmp_path_factory.mktemp("two_ranks_bam")
    contigs = [("c1", 900_000), ("c2", 700_000), ("c3", 420_000), ("c4", 130_000)]
    sizes = dict(contigs)
    # 50 bp reads: a fragment's read1 lies up to 950 bp from its other end - the BAM window rule (read1 must overlap)
    # and the region reads (every fragment whose read1 overlaps) are both exercised; 16 kb linear index per contig
    synth.write_paired_bam_contigs(str(d / "p.bam"), contigs, 12.0, 321, read_len=50, step=1 << 18)
    (d / "cs.genome").write_text("".join(f"{c}\t{n}\n" for c, n in contigs))
    (d / "bins.txt").write_text("".join(f"{c}\t{a}\t{min(a + 9_999, n)}\n" for c, n in contigs for a in range(0, n, 10_000)))
    rng = np.random.default_rng(14)
    seqs = {c: np.frombuffer(b"ACGTNacgt", np.uint8)[rng.integers(0, 9, n)].tobytes().decode() for c, n in contigs}
    H.write_fasta(d / "ref.fa", seqs)
    (d / "gaps.bed").write_text("".join(
        f"{c}\t0\t10000\ttelomere\n{c}\t{n // 2 // 10000 * 10000}\t{n // 2 // 10000 * 10000 + 30000}\tcentromere\n"
        f"{c}\t{n - 10000}\t{n}\ttelomere\n" for c, n in contigs))
    (d / "bl.bed").write_text("".join(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(100, 2500))}\n"
                                      for c, n in contigs for a in rng.integers(0, n - 3000, 20)))
    iv = [f"{c}\t{int(a)}\t{int(a) + int(rng.integers(1, 5000))}\t{c}_{k}\n" for c, n in contigs
          for k, a in enumerate(rng.integers(0, n - 5000, 40))]
    rng.shuffle(iv)
    (d / "iv.bed").write_text("".join(iv))
    (d / "sites.bed").write_text("".join(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(1, 1500))}\n" for c, n in contigs
                                         for a in np.sort(rng.integers(0, n - 2000, 30))))
    (d / "clv.bed").write_text("".join(f"{c}\t{int(a)}\t{int(a) + int(rng.integers(10, 2500))}\n" for c, n in contigs
                                       for a in np.sort(rng.integers(0, n - 3000, 25))))
    (d / "worker3.py").write_text(WORKER3.format(root=ROOT, tmp=str(d)))
    return d, sizes


def test_two_ranks_on_a_bam_equal_one_process(bam_dataset):
    """BASELINE config 5's input under the rank fan-out: `frag.delfi`, `coverage(normalize=True)`, `multi_wps`,
    `multi_cleavage_profile`, `frag_length_intervals` and `interval_end_motifs` on a coordinate-sorted paired-end BAM with
    two ranks on GPU 0 return what one process returns and write byte-identical files; the contig a cut falls into is
    read by both ranks as a region through the BAI's linear index (every fragment whose READ1 overlaps the region - the
    reference's window rule for BAM input)."""
    import gzip
    d, sizes = bam_dataset
    one = _run_world(d, 1, "worker3.py", "out3")[0]
    two = _run_world(d, 2, "worker3.py", "out3")
    for r in two:
        assert r["delfi"].equals(one["delfi"])
        for key in ("cov", "fli", "iem"):
            assert r[key] == one[key], key
    assert one["delfi"]["num_frags"].sum() > 10_000 and len(one["cov"]) == 160 and sum(x[9] for x in one["fli"] if x[9] > 0) > 500
    for name in ("delfi.tsv", "cov.bed", "wps.bw", "fli.bed", "iem.tsv"):
        a, b = open(d / f"b1_{name}", "rb").read(), open(d / f"b2_{name}", "rb").read()
        assert a == b and len(a) > 100, name
    assert open(d / "b1_clv.bed.gz", "rb").read() == open(d / "b2_clv.bed.gz", "rb").read()
    assert gzip.open(d / "b1_clv.bed.gz").read().count(b"\n") > 10_000
    everything = set(sizes)
    for cmd in ("delfi", "wps.bw", "clv.bed.gz", "fli", "iem"):
        assert one["trail"][cmd][1] == [], cmd
        (w0, r0), (w1, r1) = two[0]["trail"][cmd], two[1]["trail"][cmd]
        assert not (set(w0) & set(w1)), (cmd, w0, w1)
        assert len(r0) == 1 and len(r1) == 1 and r0[0][0] == r1[0][0] and r0[0][0] not in set(w0) | set(w1), (cmd, r0, r1)
        assert set(w0) | set(w1) | {r0[0][0]} == everything, (cmd, w0, w1, r0, r1)


WORKER_EDGE = """
import os, pickle, sys, warnings
sys.path.insert(0, {root!r})
warnings.simplefilter("ignore")
from finaletoolkit_amd import frag, sharding
rank, world = sharding.init_from_env()
G = {gold!r}
bam, iv = os.path.join(G, "edge.bam"), os.path.join(G, "edge_intervals.bed")
out = dict(world=world)
out["cov"] = [list(r) for r in frag.coverage(bam, iv, {tmp!r} + f"/e{{world}}_cov.bed")]
out["cov_any"] = [list(r) for r in frag.coverage(bam, iv, None, intersect_policy="any", quality_threshold=0)]
out["fli"] = [tuple(r) for r in frag.frag_length_intervals(bam, iv)]
frag.multi_wps(bam, os.path.join(G, "edge_sites.bed"), None, {tmp!r} + f"/e{{world}}_wps.bed.gz", interval_size=2000)
pickle.dump(out, open({tmp!r} + f"/edge_w{{world}}_r{{rank}}.pkl", "wb"))
sharding.finalize()
"""


def test_two_ranks_on_the_multi_op_cigar_bam_give_the_reference_rows(tmp_path):
    """The edge BAM of tests/golden (soft clips, I / D / N ops, CIGAR-less records, read1 poking out of its fragment ...)
    under the rank fan-out: two ranks on GPU 0 return - and write - what the REFERENCE returned for it in BAM mode
    (tests/golden/bam.json.gz, produced by the imported reference over oracle/bamstub.py), not merely what one process
    of this package returns."""
    import gzip
    from tests.helpers import GOLDEN
    from tests.test_oracle_golden_bam import bam_golden
    G = bam_golden()["edge"]
    A = np.load(os.path.join(GOLDEN, "bam.npz"))
    d = tmp_path
    (d / "worker_edge.py").write_text(WORKER_EDGE.format(root=ROOT, gold=GOLDEN, tmp=str(d)))
    one = _run_world(d, 1, "worker_edge.py", "edge")[0]
    two = _run_world(d, 2, "worker_edge.py", "edge")
    for r in [one] + two:
        assert r["cov"] == G["coverage_default"] and r["cov_any"] == G["coverage_any_q0"]
        for got, want in zip(r["fli"], G["frag_length_intervals"], strict=True):
            assert list(got[:4]) == list(want[:4]) and got[9] == want[9] and list(got[7:9]) == list(want[7:9])
            assert got[4] == pytest.approx(want[4], rel=1e-12) and got[5] == want[5] and got[6] == pytest.approx(want[6], rel=1e-9)
    assert open(d / "e1_cov.bed").read() == open(d / "e2_cov.bed").read()
    for w in (1, 2):
        rows = [ln.split("\t") for ln in gzip.open(d / f"e{w}_wps.bed.gz", "rt").read().splitlines()]
        assert np.array_equal(np.array([int(x[1]) for x in rows]), A["edge_multi_wps_pos"])
        assert np.array_equal(np.array([int(x[3]) for x in rows]), A["edge_multi_wps_val"])


def test_bench_under_torch_distributed_run():
    """The driver's own launch form for N > 1 - `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
    --gpus N` - with two ranks on GPU 0.  (Round 4 found it hanging on a shared box: LOCAL_RANK is the rank under that
    launcher, the product's engine of rank 1 looked for GPU 1, failed alone inside the file leg and left rank 0 in
    the leg's first collective.)"""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(FTK_BENCH_SHARE_GPU="1", FTK_BENCH_WATCHDOG="500")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--contigs", "21,22", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.strip().splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["checks"] and all(line["checks"].values()), line["checks"]
    leg = line["end_to_end"]["genome_frag_delfi_api_ranks"]
    assert leg["ranks"] == 2 and leg["results_ok"], line["end_to_end"]
