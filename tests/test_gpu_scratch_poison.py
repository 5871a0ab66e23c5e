"""
GPU: every device-side entry point of the C ABI gives the same answer on a poisoned scratch block.

The calls carve their temporaries, and the device stand-ins of host outputs, out of one scratch block per context that is
never cleared between calls ("What a call may assume about the scratch: nothing"): each buffer has to be
initialised by a memset, a copy or a kernel that writes every cell before any is read - which nothing else checks, since
the block normally holds zeros or the leftovers of the same call.  Here every entry point of
``tests/scratch_poison_calls.py`` (the world, the table, the procedure) runs once as found and once on a block filled
with each of 0x00, 0xFF and 0x7F through ``Engine.scratch_fill`` - filled again in front of every library call of an
entry that makes several, and once more under 0xFF with device outputs where the call takes them: the block keeps its
size, every output of every run is the same bits, and the first run equals the restatement the call's own test module
uses.  The window features and the
batch / merged calls run the same procedure once more in a child process with ``FTK_FEAT_BLOCK=1`` (the block-per-window
kernels and the merged feature + WPS launch).  The last test ties the table to ``_lib.EXPORTS``.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from finaletoolkit_amd import _lib as L
from tests import scratch_poison_calls as P
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return P.World(str(tmp_path_factory.mktemp("poison")))


@pytest.fixture(scope="module")
def own_engine(world):
    """An Engine of this module's own, not the session's: the block's size then does not depend on what ran earlier."""
    eng = P.open_engine(world)
    yield eng
    eng.close()


def test_the_world_holds_what_the_calls_need(world):
    W = world
    assert 10_000 <= W.n <= 20_000 and W.n % 4 and np.all(np.diff(W.s) >= 0)
    s, e = W.s.astype(np.int64), W.e.astype(np.int64)
    a, b = P.QUIET  # no fragment starts or ends in it, and it holds three whole tiles of every 4096-base grid in use
    assert not ((s >= a) & (s < b)).any() and not ((e > a) & (e <= b)).any()
    assert b // P.TILE - -(-a // P.TILE) >= 3 and (b - P.A0) // P.TILE - -(-(a - P.A0) // P.TILE) >= 3
    assert len(W.ws) % 4 and len(W.ws) % 64 and W.we[5] == W.ws[5] and len(W.centres) == 53 and 10 < W.flip.sum() < 43
    assert a <= W.ws[66] and W.we[66] <= b and a <= 157_000 < b
    # candidates of a window as the planner counts them (window_candidates: whole 512-base index bins from ws - lmax to
    # we): the long window goes to the chunk walker - cells zeroed by the plan, added to with atomics -, the others do not
    cand = np.array([np.searchsorted(s, (int(w1) // 512 + 1) * 512) - np.searchsorted(s, max(int(w0) - 1_000, 0) // 512 * 512)
                     for w0, w1 in zip(W.ws, W.we)])
    assert cand[20] > P.SMALL_MAX + 100 and np.delete(cand, 20).max() < P.SMALL_MAX - 100 and int((e - s).max()) == 1_000
    lens = P.IV_STOP - P.IV_START
    assert P.IV_START[0] % P.TILE and lens[0] % P.TILE and lens[1] == 0 and a <= P.IV_START[2] and P.IV_STOP[2] <= b
    assert (P.B0 - P.A0) % P.TILE and P.A0 % P.TILE and P.SIZE % P.FASTA_WIDTH
    assert np.all(W.r1s >= W.s) and np.all(W.r1e <= W.e) and np.all(W.r1s < W.r1e)
    assert "N" in W.seq[:137] and W.seq[150_000] == "N" and any(ch.islower() for ch in W.seq)


def test_scratch_fill_arguments(own_engine):
    """The hook itself: the size query fills nothing and allocates nothing, a byte out of range is refused."""
    eng = own_engine
    eng.window_counts("pt", [0], [1000])
    size = eng.scratch_fill(None)
    assert size > 0 and eng.scratch_fill(0x5A) == size and eng.scratch_fill(None) == size
    for bad in (-2, 256, 1 << 20):
        with pytest.raises(L.FtkError) as ei:
            eng.scratch_fill(bad)
        assert ei.value.code == L.FTK_ERR_INVALID
    assert eng.lib.ftk_ctx_scratch_fill(eng.ctx, 0, None) == L.FTK_OK  # (bytes_out may be NULL)
    assert np.array_equal(eng.window_counts("pt", [0], [P.SIZE], 0), [world_count(eng)])


def world_count(eng):
    return eng.info("pt")[0]


@pytest.mark.parametrize("name", list(P.CALLS))
def test_same_answer_on_a_poisoned_scratch(own_engine, world, name):
    R, S, runs, sizes = P.procedure(own_engine, world, name)
    assert S > 0
    assert list(runs) == [tag for tag, _, _ in P.fill_runs(name)] and len(runs) == 3 + P.CALLS[name][2]
    grew = {tag: sizes[tag] for tag in runs if sizes[tag] != S}
    assert not grew, (name, S, grew)  # a call that grew the block would have escaped the poison
    differ = {tag: P.differing(R, runs[tag]) for tag in runs if not P.same_bits(R, runs[tag])}
    assert not differ, (name, differ)  # run: the outputs that are not the bits of the first run
    P.CALLS[name][1](world, R, own_engine)


@pytest.fixture(scope="module")
def block_path(tmp_path_factory):
    """ONE child process with FTK_FEAT_BLOCK=1 runs the whole procedure for CHILD_CALLS."""
    tmp = str(tmp_path_factory.mktemp("poison_child"))
    path = os.path.join(tmp, "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("FTK_PACKED", "FTK_FEAT_FAST")}
    env["FTK_FEAT_BLOCK"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scratch_poison_calls.py"), tmp, path], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", P.CHILD_CALLS)
def test_same_answer_on_the_block_path(block_path, world, own_engine, name):
    got = {}
    for key, v in block_path.items():
        if key.startswith(name + "/") and not key.endswith("/S"):
            _, tag, k = key.split("/")
            got.setdefault(tag, {})[k] = v
    sizes = block_path[name + "/S"]
    assert sizes[0] > 0 and np.all(sizes == sizes[0]), (name, sizes)
    tags = [tag for tag, _, _ in P.fill_runs(name)]
    assert sorted(got) == sorted(["R"] + tags) and len(sizes) == 1 + len(tags)
    differ = {tag: P.differing(got["R"], got[tag]) for tag in tags if not P.same_bits(got["R"], got[tag])}
    assert not differ, (name, differ)
    P.CALLS[name][1](world, got["R"], own_engine)


# Exported symbols that place nothing in the context's scratch block, each group with its reason.
EXEMPT = {
    # no device work at all: versions, errors, counters, constants of the kernels
    "host only": ["ftk_version", "ftk_device_count", "ftk_last_error", "ftk_frags_name", "ftk_frags_info", "ftk_frags_packed",
                  "ftk_mask_lds_intervals", "ftk_end_context_lds_classes"],
    # the context itself, its stream, its timers - and the hook this module drives
    "context": ["ftk_ctx_create", "ftk_ctx_destroy", "ftk_ctx_set_stream", "ftk_ctx_sync", "ftk_ctx_scratch_fill", "ftk_timer_start",
                "ftk_timer_stop", "ftk_event_record", "ftk_event_elapsed_ms"],
    # residency: columns, weights and reference images live in allocations of their own (hipMalloc per contig / image, the
    # summary word block ctx->d_stats), never in the scratch
    "residency": ["ftk_frags_from_host", "ftk_frags_from_device", "ftk_frags_from_table", "ftk_frags_set_read1", "ftk_frags_set_order",
                  "ftk_frags_release", "ftk_frags_set_weights", "ftk_ref_upload", "ftk_ref_upload_file", "ftk_ref_release",
                  "ftk_ref_set_layout"],
    # ftk_frags_weights alone is a copy out of the contig's column; it is run behind ftk_frags_set_gc_weights in the table
    # the asynchronous WPS writes into the context's two result buffers (ctx->abuf), not the scratch
    "async results": ["ftk_wps_async", "ftk_result_wait"],
    # the stream decoders and the file loads built on them keep device buffers per stream (ftk_stream_*.inc, ftk_decode.cpp
    # hold no reference to ctx->scratch); their tables go to the GPU through ftk_frags_from_table
    "streams": ["ftk_fragfile_decode", "ftk_bam_decode", "ftk_fragfile_index_contigs", "ftk_fragstream_open", "ftk_fragstream_open_device",
                "ftk_fragstream_open_region", "ftk_fragstream_next", "ftk_fragstream_n_refs", "ftk_fragstream_ref_name",
                "ftk_fragstream_ref_length", "ftk_fragstream_close", "ftk_fragstream_stage_ms", "ftk_fragstream_skipped",
                "ftk_fragtable_is_device", "ftk_fragtable_ready_event", "ftk_fragtable_columns_to_host", "ftk_fragtable_read1_to_host",
                "ftk_fragtable_skipped", "ftk_fragtable_error", "ftk_fragtable_is_bed6", "ftk_fragtable_n_contigs",
                "ftk_fragtable_contig_name", "ftk_fragtable_contig_length", "ftk_fragtable_contig_rows", "ftk_fragtable_columns",
                "ftk_fragtable_order", "ftk_fragtable_is_pinned", "ftk_fragtable_free", "ftk_frags_load_fraggz", "ftk_frags_load_bam"],
    # host memory and host formatters / writers (csrc/ftk_writers.cpp): no device
    "host buffers and writers": ["ftk_host_alloc", "ftk_host_alloc_pageable", "ftk_host_free", "ftk_cache_trim", "ftk_buffer_free",
                                 "ftk_format_wig_i64", "ftk_format_bedgraph_i64", "ftk_format_bedgraph_f64", "ftk_format_bedgraph_runs",
                                 "ftk_file_write", "ftk_gzip_members", "ftk_bigwig_fixedstep_sections", "ftk_format_frag_rows",
                                 "ftk_bgzf_write", "ftk_synth_bam_contig", "ftk_fill_wps_records"],
    # the communicator works on the caller's device arrays and its own staging
    "comm": ["ftk_comm_unique_id", "ftk_comm_create", "ftk_comm_size", "ftk_allgather_i64", "ftk_allreduce_sum_i64", "ftk_comm_send",
             "ftk_comm_recv", "ftk_comm_join", "ftk_comm_destroy"],
}


def test_every_export_is_in_the_table_or_exempt():
    """A later entry point cannot be added without a decision: in the table of calls, or exempt with a reason."""
    covered = [sym for name in P.CALLS for sym in name.split("+")]
    exempt = [sym for group in EXEMPT.values() for sym in group]
    assert len(set(covered)) == len(covered) and len(set(exempt)) == len(exempt)
    assert not set(covered) & set(exempt)
    assert sorted(covered + exempt) == sorted(L.EXPORTS), (sorted(set(L.EXPORTS) - set(covered) - set(exempt)),
                                                          sorted((set(covered) | set(exempt)) - set(L.EXPORTS)))
    assert set(P.CHILD_CALLS) <= set(P.CALLS)
