"""The device route's tile plan as the library applies it (pypore_amd/csrc/seg_plan.hpp: plan_device_tiles): one small batch --
empty events, events of 1, 7, 8 and 9 samples, events of 383 / 384 / 385 samples around 1.5 tile lengths, one of 2 000 -- on a lone
context with tiles of 4 W = 256 samples (W = 64, min_width 8).  The call's tile count is the one the stand-alone program of
tests/test_seg_plan_host.py plans for the same layout, and the boundaries are the CPU oracle's."""
import numpy as np
import pytest

from test_seg_plan_host import GPU_CASE, build, planned_tiles
from test_short_chain import against_oracle, random_steps
from test_tree_screen import P, Q, plain_suite, tensor


@pytest.mark.gpu
def test_tiles_as_planned_and_boundaries_as_the_oracle(tmp_path):
    from pypore_amd import engine
    mw, W, lens = GPU_CASE["mw"], GPU_CASE["W"], GPU_CASE["lens"]
    want = planned_tiles(build(tmp_path, "check", []), mw, W, GPU_CASE["tile_len"], lens)
    assert want == GPU_CASE["tiles"]
    ev_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = random_steps(int(ev_off[-1]), 91, 20, 160)
    ctx = engine.Context(0)
    try:
        ctx.set_tiling(GPU_CASE["tile_len"], 0)
        for dtype in ("int16", "float32"):
            r = ctx.segment_batch(tensor(c, dtype), ev_off, P(min_width=mw, window_width=W), Q)
            tm = ctx.timings()
            print("%s: tiles %d (planned %d), repairs %d, boundaries %d" % (dtype, tm["tiles"], want, tm["repairs"], r[0].numel()))
            if plain_suite():
                assert tm["tiles"] == want and tm["repairs"] < 1000000
            b, off = r[0].cpu().numpy(), np.array(r[1])
            assert off[-1] == b.size and b.size > 20
            against_oracle((b, off), c, ev_off, min_width=mw, window_width=W)
    finally:
        ctx.close()
