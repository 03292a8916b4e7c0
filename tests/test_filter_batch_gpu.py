"""ps_filter_bessel_batch (engine.Context.filter_bessel_batch) and the two entries rewired onto its kernels.

The oracle is Context.filter_bessel per event: existing code, itself pinned to scipy's goldens (test_filter.py,
test_filter_edges.py).  The batch hands every workgroup (thread) the (event, unit) it would have had in the per-event launch,
so the comparison is torch.equal: no tolerance anywhere in this file.

One seeded trace of 70 001 samples (the order-n cases need one event of 70 000) as int16 counts, float32 on the 2^-5 pA grid and
float64 off every grid.  The event set (event_set): lengths 7, 8, T - 13, T - 12, T - 11, 2 T - 12, 2 T - 11, 3 T + 5 with T from
the rule (filter_exact.order1_geometry), two pairs of events that touch, two that overlap, one starting at sample 0, one ending
on the last sample, odd starts, given in descending order of start."""
import contextlib
import ctypes

import numpy as np
import pytest

import filter_exact as fx
from launch_geometry import options
from pypore_amd import _lib, synth

pytestmark = pytest.mark.gpu

N = 70_001
Q = synth.QUANTUM
SECOND = fx.SECOND
OFF_GRID = r"status -6"
BAD_ARG = r"status -1"
I16_OFFSET = 37                          # offset_counts of the int16 form: the batch hands it on like the single call
SCRATCH_DEFAULT = 256 << 20


def context():
    from pypore_amd import engine
    return engine.context(0)


@contextlib.contextmanager
def scratch_cap(ctx, nbytes):
    try:
        ctx.set_option("filt_batch_scratch", int(nbytes))
        yield ctx
    finally:
        ctx.set_option("filt_batch_scratch", SCRATCH_DEFAULT)


_TRACES = {}


def trace(dtype):
    """The trace as a CUDA tensor (built once per form and left unchanged): dwells of 200 .. 3000 samples at 30 .. 110 pA
    with 1 pA of noise, in counts of 2^-5 pA; the float64 form is moved off every grid by an irrational ripple."""
    import torch
    if dtype not in _TRACES:
        rng = np.random.default_rng(20240611)
        k = np.empty(N, dtype=np.int64)
        at = 0
        while at < N:
            n = int(rng.integers(200, 3000))
            k[at:at + n] = int(rng.integers(960, 3520))
            at += n
        k += np.rint(rng.normal(0.0, 32.0, N)).astype(np.int64)
        assert np.abs(k).max() + I16_OFFSET < 2 ** 15
        if dtype == "i16":
            t = torch.from_numpy((k - I16_OFFSET).astype(np.int16))
        elif dtype == "f32":
            t = torch.from_numpy((k * Q).astype(np.float32))
        else:
            t = torch.from_numpy(k * Q + np.sin(np.arange(N) * np.sqrt(2.0)) * (Q / np.pi))
        _TRACES[dtype] = t.cuda()
    return _TRACES[dtype]


def call_kw(dtype, cutoff, order=1):
    return dict(cutoff=cutoff, sampling_freq=SECOND, order=order, offset_counts=I16_OFFSET if dtype == "i16" else 0)


_SINGLE = {}


def single(ctx, dtype, s, n, cutoff, order=1, fused=1):
    """Context.filter_bessel on the stretch alone (computed once per stretch and filter, kept on the device)."""
    key = (dtype, int(s), int(n), cutoff, order, fused)
    if key not in _SINGLE:
        with options(ctx, filter_fused=fused):
            _SINGLE[key] = ctx.filter_bessel(trace(dtype)[int(s):int(s) + int(n)], Q, **call_kw(dtype, cutoff, order))
    return _SINGLE[key]


def assert_batch_equals_singles(ctx, dtype, st, ln, cutoff, order=1, fused=1, what=""):
    import torch
    with options(ctx, filter_fused=fused):
        y, off = ctx.filter_bessel_batch(trace(dtype), st, ln, Q, **call_kw(dtype, cutoff, order))
    assert y.dtype == torch.float64 and y.numel() == int(np.sum(ln)) == off[-1] and len(off) == len(ln) + 1
    for e in range(len(ln)):
        assert torch.equal(y[off[e]:off[e + 1]], single(ctx, dtype, st[e], ln[e], cutoff, order, fused)), \
            "%s: event %d (start %d, length %d) of %d differs from the single call" % (what, e, st[e], ln[e], len(ln))
    return y, off


def event_set(T):
    """(starts, lengths) int64: see the module's docstring.  T: the unit of the route (the fused tile, the scan's chunk)."""
    ev = [(0, T - 12),                                   # starts at sample 0
          (N - (2 * T - 11), 2 * T - 11),                # ends on the last sample
          (1001, 7), (1008, 8),                          # touch: a wrong reflection of either reads the other
          (20001, T - 13), (20001 + T - 13, 2 * T - 12),  # touch, across tiles
          (30001, T - 11), (30001 + 100, T - 12),        # overlap
          (7777, 3 * T + 5), (7777 + T, 7),              # odd starts; a short event inside a long one
          (41113, T - 13)]
    ev.sort(key=lambda p: -p[0])                         # descending starts: the packed order is not the trace's
    st, ln = np.array([p[0] for p in ev], dtype=np.int64), np.array([p[1] for p in ev], dtype=np.int64)
    assert set(ln) == {7, 8, T - 13, T - 12, T - 11, 2 * T - 12, 2 * T - 11, 3 * T + 5}
    assert st.min() == 0 and (st + ln).max() == N and np.any(st % 2 == 1) and np.all(st + ln <= N) and np.all(np.diff(st) <= 0)
    return st, ln


# ---- order 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", fx.DTYPES)
@pytest.mark.parametrize("cutoff", [2000., 650., 20000., 600.])
def test_order1_event_set(cutoff, dtype):
    """2 000 Hz (H 384), 650 Hz (H 1 024, the last fused cutoff), 20 kHz (H 64): one fused launch.  600 Hz: the scan route, the
    per-event fallback inside the batch."""
    g = fx.order1_geometry(50_000, cutoff, SECOND, 1)
    assert g["route"] == ("scan" if cutoff == 600. else "fused")
    T = g["T"] if g["route"] == "fused" else fx.CHUNK
    st, ln = event_set(T)
    if g["route"] == "fused":                            # the lengths sit where they claim: 1, 1, 2, 2, 3, 4 tiles
        tiles = {int(n): fx.order1_geometry(int(n), cutoff, SECOND, 1)["tiles"] for n in ln}
        assert [tiles[n] for n in (7, T - 13, T - 12, T - 11, 2 * T - 12, 2 * T - 11, 3 * T + 5)] == [1, 1, 1, 2, 2, 3, 4]
    assert_batch_equals_singles(context(), dtype, st, ln, cutoff, what="%g Hz %s" % (cutoff, dtype))


@pytest.mark.parametrize("dtype", fx.DTYPES)
def test_order1_fused_switch_off(dtype):
    """filter_fused = 0: the default filter takes the scan route per event inside the batch, like the single call."""
    st, ln = event_set(fx.CHUNK)
    assert_batch_equals_singles(context(), dtype, st, ln, 2000., fused=0, what="fused off %s" % dtype)


@pytest.mark.parametrize("n_ev", [1, 2, 63, 64, 65])
def test_event_counts(n_ev):
    rng = np.random.default_rng(n_ev)
    ln = rng.integers(7, 9000, n_ev).astype(np.int64)
    st = rng.integers(0, N - 9000, n_ev).astype(np.int64)
    assert_batch_equals_singles(context(), "i16", st, ln, 2000., what="%d events" % n_ev)


def test_three_thousand_short_events():
    """The tables at scale: 3 000 events of 7 .. 40 samples, one tile each."""
    rng = np.random.default_rng(3000)
    ln = rng.integers(7, 41, 3000).astype(np.int64)
    ln[:2] = 7, 40
    st = rng.integers(0, N - 40, 3000).astype(np.int64)
    assert_batch_equals_singles(context(), "i16", st, ln, 2000., what="3000 events")


# ---- orders 2 .. 8 ------------------------------------------------------------------------------------------------------------
def order_n_events(order, cutoff):
    g = fx.halo_geometry(70_000, order, cutoff, SECOND)
    S, pad = g["S"], g["pad"]
    assert g["H"] > 0 and g["nseg"] > 64                 # the long event: more than one workgroup of 64 threads
    ln = [S - 2 * pad - 1, S - 2 * pad, S - 2 * pad + 1, 2 * S - 2 * pad, 2 * S - 2 * pad + 1, pad + 1, 70_000, 3 * S + 5]
    st = [1, 3001, 0, 5001, N - ln[4], 333, 1, 40_001]
    segs = [fx.halo_geometry(n, order, cutoff, SECOND)["nseg"] for n in ln]
    assert segs[:6] == [1, 1, 2, 2, 3, 1]
    order_ = np.argsort(-np.array(st), kind="stable")
    return np.array(st, dtype=np.int64)[order_], np.array(ln, dtype=np.int64)[order_], np.array(segs)[order_], (S + g["H"]) * 8


def planned_groups(segs, rows_max):
    """filt_plan.hpp's greedy cut, restated: events in order, a group closes when the next event's rows would not fit."""
    groups, rows = 0, 0
    for k in segs:
        if groups == 0 or rows + k > rows_max:
            groups, rows = groups + 1, 0
        rows += k
    return groups


@pytest.mark.parametrize("dtype", fx.DTYPES)
@pytest.mark.parametrize("order,cutoff", [(2, 5000.), (8, 10000.)])
def test_order_n_in_one_two_and_many_groups(order, cutoff, dtype):
    """Lengths around S - 2 pad and 2 S - 2 pad, padlen + 1, and 70 000 samples (69 segments: two workgroups); the same batch
    under the default scratch cap (one launch), a cap that cuts it in two, and a cap of one byte (a launch per event)."""
    import torch
    ctx = context()
    st, ln, segs, row = order_n_events(order, cutoff)
    two = next(r for r in range(int(segs.max()), int(segs.sum()) + 1) if planned_groups(segs, r) == 2)
    assert planned_groups(segs, SCRATCH_DEFAULT // row) == 1 and planned_groups(segs, 1) == len(ln)
    y1, _ = assert_batch_equals_singles(ctx, dtype, st, ln, cutoff, order, what="order %d %s" % (order, dtype))
    for cap in (two * row, 1):
        with scratch_cap(ctx, cap):
            y, _ = ctx.filter_bessel_batch(trace(dtype), st, ln, Q, **call_kw(dtype, cutoff, order))
        assert torch.equal(y, y1), "cap %d" % cap


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_no_events():
    y, off = context().filter_bessel_batch(trace("i16"), [], [], Q)
    assert y.numel() == 0 and off.tolist() == [0]


def raw_batch(ctx, t, st, ln, out, order=1, cutoff=2000.):
    st, ln = np.ascontiguousarray(st, dtype=np.int64), np.ascontiguousarray(ln, dtype=np.int64)
    P64 = ctypes.POINTER(ctypes.c_int64)
    fmt = _lib.SampleFormat(_lib.PS_DTYPE_I16, 0, Q)
    with ctx.lock:
        rc = ctx.L.ps_filter_bessel_batch(ctx.handle, ctypes.c_void_p(t.data_ptr()), ctypes.byref(fmt), st.ctypes.data_as(P64), ln.ctypes.data_as(P64),
                                          st.size, order, cutoff, SECOND, ctypes.c_void_p(out.data_ptr()))
        msg = ctx.L.ps_last_error(ctx.handle)
    return rc, (msg.decode() if msg else "")


@pytest.mark.parametrize("order", [1, 2])
def test_short_event_is_named_and_nothing_is_written(order):
    import torch
    ctx = context()
    pad = 3 * (order + 1)
    out = torch.full((4096,), -7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc, msg = raw_batch(ctx, trace("i16"), [10, 500, 900, 1500], [100, 200, pad, pad - 1], out, order=order)
    assert rc == _lib.PS_ERR_ARG and "event 2" in msg and "padlen, which is %d" % pad in msg
    rc, msg = raw_batch(ctx, trace("i16"), [10, -1], [100, 50], out, order=order)
    assert rc == _lib.PS_ERR_ARG and "event 1" in msg
    rc, msg = raw_batch(ctx, trace("i16"), [10, 20], [0, 50], out, order=order)
    assert rc == _lib.PS_ERR_ARG and "event 0" in msg
    assert raw_batch(ctx, trace("i16"), [10], [100], out, order=9)[0] == _lib.PS_ERR_ARG
    rc, msg = raw_batch(ctx, trace("i16"), [10], [100], out, order=order, cutoff=5.e4)
    assert rc == _lib.PS_ERR_ARG and "Nyquist" in msg
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    with pytest.raises(ValueError, match=BAD_ARG):
        ctx.filter_bessel_batch(trace("i16"), [10, 500], [100, pad], Q, order=order)
    with pytest.raises(ValueError, match="outside"):
        ctx.filter_bessel_batch(trace("i16"), [N - 50], [51], Q, order=order)


@pytest.mark.parametrize("order,cutoff", [(1, 2000.), (1, 600.), (2, 5000.)])
def test_off_grid_sample_in_one_event(order, cutoff):
    """A float32 sample off the grid inside one event: the batch raises what the single call raises, and the next batch on
    the same context is clean."""
    ctx = context()
    st, ln = np.array([100, 5000, 9001]), np.array([3000, 3501, 700])
    dirty = trace("f32").clone()
    dirty[5000 + 1700] += np.float32(Q / 2)
    with pytest.raises(ValueError, match=OFF_GRID):
        ctx.filter_bessel(dirty[5000:8501], Q, cutoff=cutoff, sampling_freq=SECOND, order=order)
    with pytest.raises(ValueError, match=OFF_GRID):
        ctx.filter_bessel_batch(dirty, st, ln, Q, cutoff=cutoff, sampling_freq=SECOND, order=order)
    assert_batch_equals_singles(ctx, "f32", st, ln, cutoff, order, what="after the refusal")


# ---- the rewired entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", fx.DTYPES)
@pytest.mark.parametrize("order,cutoff", [(1, 2000.), (2, 5000.)])
def test_filter_requantise_batch_on_the_event_set(order, cutoff, dtype):
    import torch
    ctx = context()
    if order == 1:
        st, ln = event_set(fx.order1_geometry(50_000, cutoff, SECOND, 1)["T"])
    else:
        st, ln = order_n_events(order, cutoff)[:2]
    filt, rnd, off, centre, step = ctx.filter_requantise_batch(trace(dtype), st, ln, Q, **call_kw(dtype, cutoff, order))
    for e in range(len(ln)):
        y = single(ctx, dtype, st[e], ln[e], cutoff, order)
        z, c, s = ctx.requantise(y)
        assert torch.equal(filt[off[e]:off[e + 1]], y) and torch.equal(rnd[off[e]:off[e + 1]], z), "event %d" % e
        assert (centre[e], step[e]) == (c, s), "event %d" % e


@pytest.mark.parametrize("cutoff", [2000., 600.])
def test_filter_derivative_on_the_event_set(cutoff):
    """prefiltered = 0 on the float64 trace against prefiltered = 1 on the per-event filtered currents, packed."""
    import torch
    ctx = context()
    g = fx.order1_geometry(50_000, cutoff, SECOND, 1)
    st, ln = event_set(g["T"] if g["route"] == "fused" else fx.CHUNK)
    par = lambda pre: _lib.FilterDerivativeParams(0.05, 2.0, cutoff, SECOND, pre)
    spans, off = ctx.filter_derivative_f64(trace("f64"), st, ln, par(0))
    packed = torch.cat([single(ctx, "f64", st[e], ln[e], cutoff) for e in range(len(ln))])
    want, want_off = ctx.filter_derivative_f64(packed, np.concatenate(([0], np.cumsum(ln)))[:-1], ln, par(1))
    print("%d spans of %d events" % (off[-1], len(ln)))
    assert np.array_equal(off, want_off) and torch.equal(spans, want) and off[-1] >= len(ln)
