"""Pooled calls planned for the hardware queues of the process (option "shared_device" with "hw_queues", ps_pool_plan; the K0
gate of "k0_admit", ps_gate_stats).  The plan changes how a call is scheduled and nothing it returns: every case compares
boundaries and offsets with a lone context's and with the oracle's.

Shapes: a 2e5-sample step trace, W = 1 000, min_width 50: tiles are 4 W long, so the call has fifty of them, and K0's last wave
block is ragged (2e5 samples are 97.7 wave blocks of 2 048).  The gate runs on a 1e5-sample trace."""
import numpy as np
import pytest

import oracle
from pypore_amd import _lib, synth
from test_short_chain import SKIPPED, WORK, random_steps
from test_tree_screen import plain_suite, tensor

Q = synth.QUANTUM
W, MW = 1000, 50
N = 200000
HWQ = (1, 4, 16)
SHARED = (1, 4, 16)
PLANNED = ("k0_waves", "k0_admit", "lat_help")


def P():
    return _lib.split_params(min_width=MW, max_width=1000000, window_width=W, prior_segments_per_second=10.)


@pytest.fixture(scope="module")
def trace():
    """counts, the oracle's boundaries -- computed once, never written to"""
    c = random_steps(N, 91, 150, 3000)
    ref = oracle.parse(synth.counts_to_pa(c, np.float64), min_width=MW, max_width=1000000, window_width=W, prior_segments_per_second=10.)
    ref.setflags(write=False)
    return c, ref


@pytest.fixture()
def ctx():
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def call(cx, t):
    b, off, _ = cx.segment_batch(t, np.array([0, t.numel()], dtype=np.int64), P(), Q)
    return b.cpu().numpy(), np.array(off)


def pinned():
    """options the suite was started with (tests/conftest.py) stay in force over what shared_device plans"""
    from pypore_amd import engine
    return {k: engine.DEFAULT_OPTIONS[k] for k in PLANNED if k in engine.DEFAULT_OPTIONS}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_every_plan_returns_the_lone_result(ctx, trace, dtype):
    c, ref = trace
    t = tensor(c, dtype)
    lone = call(ctx, t)
    np.testing.assert_array_equal(lone[0], ref)
    assert ctx.timings()["tiles"] >= 50
    for q in HWQ:
        ctx.set_option("hw_queues", q)
        for n in SHARED:
            ctx.set_option("shared_device", n)
            plan = _lib.pool_plan(n, q)
            assert plan["n_eff"] == min(n, q)
            assert {k: ctx.get_option(k) for k in PLANNED} == {k: plan[k] for k in PLANNED}, (q, n)
            assert ctx.get_option("shared_device") == n and ctx.get_option("hw_queues") == q
            got = call(ctx, t)
            np.testing.assert_array_equal(got[0], lone[0], err_msg="hw_queues %d shared_device %d" % (q, n))
            np.testing.assert_array_equal(got[1], lone[1])
    # hw_queues 0: the process's own
    ctx.set_option("hw_queues", 0)
    ctx.set_option("shared_device", 16)
    plan = _lib.pool_plan(16, _lib.hw_queues())
    assert {k: ctx.get_option(k) for k in PLANNED} == {k: plan[k] for k in PLANNED}
    np.testing.assert_array_equal(call(ctx, t)[0], ref)


@pytest.mark.gpu
def test_explicit_options_win_and_one_restores(ctx, trace):
    c, ref = trace
    t = tensor(c, "float32")
    ctx.set_option("hw_queues", 4)
    ctx.set_option("shared_device", 16)
    ctx.set_option("k0_waves", 2)
    ctx.set_option("k0_admit", 1)
    assert (ctx.get_option("k0_waves"), ctx.get_option("k0_admit"), ctx.get_option("lat_help")) == (2, 1, 0)
    before = _lib.gate_stats(0)["tickets"]
    np.testing.assert_array_equal(call(ctx, t)[0], ref)
    assert _lib.gate_stats(0)["tickets"] == before + 1          # the call went through the gate: k0_admit 1 was in force
    ctx.set_option("shared_device", 1)
    assert (ctx.get_option("k0_waves"), ctx.get_option("k0_admit"), ctx.get_option("lat_help")) == (0, 0, 1)
    np.testing.assert_array_equal(call(ctx, t)[0], ref)
    g = _lib.gate_stats(0)
    assert g["tickets"] == before + 1 and g["open"] == 0        # a lone context takes no ticket
    # ... and through the pool's overrides (engine.POOL_OVERRIDES), on top of what shared_device planned
    from pypore_amd import engine
    pool = engine.StreamPool(0, 2, overrides={"k0_waves": 3, "k0_admit": 2})
    try:
        seen = pool.run(2, lambda cx, k, t_: (cx.get_option("k0_waves"), cx.get_option("k0_admit"), cx.get_option("shared_device")))
    finally:
        pool.close()
    want = pinned()
    assert seen == [(want.get("k0_waves", 3), want.get("k0_admit", 2), 2)] * 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_short_chain_counters_do_not_depend_on_the_queues(ctx, trace, dtype):
    c, ref = trace
    t = tensor(c, dtype)
    seen = {}
    for q in HWQ:
        ctx.set_option("hw_queues", q)
        ctx.set_option("shared_device", 16)
        np.testing.assert_array_equal(call(ctx, t)[0], ref)
        call(ctx, t)                                            # (the repeated layout: no upload on the short route)
        tm = ctx.timings()
        seen[q] = {k: tm[k] for k in SKIPPED + WORK + ("repairs",)}
        ctx.set_option("shared_device", 1)
    print(seen)
    assert seen[1] == seen[4] == seen[16]
    if plain_suite():
        # a pooled call whatever the queues: no look-ahead launch, no seam left to the second round
        assert seen[16]["lookahead_skipped"] == 1 and seen[16]["seams_resumed"] == 0 and seen[16]["repairs"] == 0


@pytest.mark.gpu
def test_four_threads_on_four_queues(trace):
    from pypore_amd import engine
    c, ref = trace
    ts = [tensor(c, "float32"), tensor(c, "int16")]
    single = [call(engine.context(0), t) for t in ts]
    for s in single:
        np.testing.assert_array_equal(s[0], ref)
    pool = engine.StreamPool(0, 4)
    try:
        for cx in pool.contexts:
            cx.set_option("hw_queues", 4)
        planned = []

        def job(cx, k, t_):
            planned.append(tuple(cx.get_option(k_) for k_ in PLANNED))
            return call(cx, ts[k % 2])
        got = pool.run(16, job)
    finally:
        for cx in pool.contexts:
            cx.set_option("hw_queues", 0)
        pool.close()
    plan = dict(_lib.pool_plan(4, 4), **pinned())
    assert set(planned) == {tuple(plan[k] for k in PLANNED)}
    for k, g in enumerate(got):
        np.testing.assert_array_equal(g[0], single[k % 2][0])
        np.testing.assert_array_equal(g[1], single[k % 2][1])


@pytest.mark.gpu
def test_gate_admits_no_more_than_m():
    """k0_admit 1, four threads racing through twenty calls each: equal results, and never more than one call between the gate
    and the record behind its K0 -- a call whose predecessor's ticket is taken but not yet recorded waits for the record."""
    from pypore_amd import engine
    c = random_steps(100000, 93, 150, 3000)
    t = tensor(c, "float32")
    ref = call(engine.context(0), t)
    np.testing.assert_array_equal(ref[0], oracle.parse(synth.counts_to_pa(c, np.float64), min_width=MW, max_width=1000000, window_width=W,
                                                      prior_segments_per_second=10.))
    m = pinned().get("k0_admit", 1)
    pool = engine.StreamPool(0, 4, overrides={"k0_admit": 1})
    try:
        start = _lib.gate_stats(0, reset=True)
        got = pool.run(80, lambda cx, k, t_: call(cx, t))      # job k on context k % 4: twenty calls a thread
        g = _lib.gate_stats(0)
    finally:
        pool.close()
    print(start, g)
    for r in got:
        np.testing.assert_array_equal(r[0], ref[0])
        np.testing.assert_array_equal(r[1], ref[1])
    assert g["tickets"] - start["tickets"] == (80 if m > 0 else 0)
    assert g["open"] == 0 and g["gave_up"] == 0
    assert g["open_max"] <= max(m, 0) and (g["open_max"] == 1 or m != 1)
