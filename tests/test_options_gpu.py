"""ps_set_option / ps_get_option on a live context: the glue between the table of pypore_amd/csrc/ctx_options.hpp (checked on the CPU,
tests/test_ctx_options_host.py) and the context -- every row of the product reaches its value through the library, a refused value
raises with the library's message and changes nothing, and the options that act on the context still do.  The rows are what
tests/native/ctx_options_check.cpp prints.  The swept values are set on a private context that never segments with them; a context
made afterwards, with nothing set, segments the first golden event to its recorded bounds."""
import numpy as np
import pytest
import torch

from golden_util import cases, input_pa, npz
from pypore_amd import _lib, engine, synth
from test_ctx_options_host import build, table_rows

TIMING_KEYS = {"spine_ms", "tree_ms", "gather_ms", "total_ms", "stitch_ms", "bridge_ms", "blocksum_ms", "seq_ms", "windows", "candidates", "tiles",
               "tree_jobs", "repairs", "exact_rescans", "full_exact_scans", "wide_redo", "windows_spine", "windows_bridge", "windows_tree",
               "near_ties", "helper_chunks_published", "helper_chunks_taken", "tree_deferred", "windows_screen", "lookahead_skipped",
               "upload_skipped", "seams_resumed"}
I64 = (-(1 << 63), (1 << 63) - 1)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """the product's rows"""
    return [r for r in table_rows(build(tmp_path_factory.mktemp("ctx_options_gpu"), "check", [])) if not r["diag"]]


def stored(row, value):
    """what the library keeps of a value it takes"""
    return int(value != 0) if row["norm"] == "bool" else min(max(value, row["lo"]), row["hi"])


@pytest.mark.gpu
def test_every_option_round_trips_through_the_library(rows):
    assert len(rows) >= 40
    start = {r["name"]: engine.DEFAULT_OPTIONS.get(r["name"], r["default"]) for r in rows}      # (a suite started with PORESEG_* set pins some)
    ctx = engine.Context(0)
    try:
        probe = ctx.get_option("k0_unaligned")                  # what the device's probe granted at ps_create
        assert probe in (0, 1)
        for r in rows:
            if r["name"] != "k0_unaligned":
                assert ctx.get_option(r["name"]) == start[r["name"]], r["name"]
        for r in rows:
            name = r["name"]
            planned = {k: ctx.get_option(k) for k in ("k0_waves", "k0_admit", "lat_help") if k != name}
            for value in (r["lo"], r["hi"]):
                ctx.set_option(name, value)
                want = stored(r, value)
                assert ctx.get_option(name) == (want and probe if name == "k0_unaligned" else want), (name, value)
            if r["norm"] == "given":
                bad = r["lo"] - 1 if r["lo"] > I64[0] else r["hi"] + 1
                assert I64[0] <= bad <= I64[1], name
                kept = ctx.get_option(name)
                with pytest.raises(ValueError, match="unknown option or value: %s" % name):
                    ctx.set_option(name, bad)
                assert ctx.get_option(name) == kept, name
            if name != "shared_device":
                assert {k: ctx.get_option(k) for k in planned} == planned, name                     # no option writes another's value
        with pytest.raises(ValueError, match="unknown option or value: no_such_option"):
            ctx.set_option("no_such_option", 1)
        with pytest.raises(ValueError, match="unknown option or value: dbg_phase"):                # the diagnostic library's
            ctx.set_option("dbg_phase", 1)
        with pytest.raises(ValueError):
            ctx.get_option("dbg_phase")
        # the options that act on the context
        ctx.set_option("k0_unaligned", 0)
        assert ctx.get_option("k0_unaligned") == 0
        ctx.set_option("k0_unaligned", 1)
        assert ctx.get_option("k0_unaligned") == probe
        ctx.set_option("hw_queues", 0)
        ctx.set_option("shared_device", 16)
        plan = _lib.pool_plan(16, _lib.hw_queues())
        assert {k: ctx.get_option(k) for k in ("k0_waves", "k0_admit", "lat_help")} == {k: plan[k] for k in ("k0_waves", "k0_admit", "lat_help")}
        assert ctx.get_option("shared_device") == 16
    finally:
        ctx.close()
    # a context made afterwards knows nothing of all that
    case = cases("parse")[0]
    x = torch.from_numpy(input_pa(case, np.float32)).cuda()
    fresh = engine.Context(0)
    try:
        assert {r["name"]: fresh.get_option(r["name"]) for r in rows if r["name"] != "k0_unaligned"} == \
               {n: v for n, v in start.items() if n != "k0_unaligned"}
        b, off, _ = fresh.segment_batch(x, np.array([0, x.numel()], dtype=np.int64), _lib.split_params(**case["params"]), synth.QUANTUM)
        np.testing.assert_array_equal(b.cpu().numpy()[:int(off[1])], npz()[case["name"] + "/bounds"])
        t = fresh.timings()
        assert set(t) == TIMING_KEYS and len(t) == 27 and t["tiles"] >= 1
    finally:
        fresh.close()
