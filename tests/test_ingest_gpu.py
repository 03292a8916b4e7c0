"""Grid recovery on the MI355X (csrc/seg_ingest.hpp: grid_check_kernel, grid_counts_kernel, narrow_f64_kernel behind
ps_grid_check_f64 / ps_grid_counts_f64 / ps_narrow_f64) and the roads that reach it: grid.affine_grid_device,
engine.to_device_with_counts for float64 CUDA tensors and long numpy float64 arrays, FastStatSplit.parse_batch's off_grid
policy for tensors, lambda_event_parser.  The oracle of every decision is the host code on the same values
(grid.affine_grid, the numpy roads of engine.to_device_with_counts); test_ingest_host.py holds that code to the counts the
arrays were built from.  Lengths: the seams of a wave (64), a workgroup (256) and a workgroup pass (engine.INGEST_PASS =
ING_T, one pass per workgroup up to engine.INGEST_GRID_MAX workgroups), and the lengths at which the subset's stride becomes
2 and 3; the grid-stride step itself needs more than INGEST_GRID_MAX * INGEST_PASS samples and has tests of its own
(STRIDED)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ingest_host as ic  # noqa: E402  (the currents built from known counts are defined there)
import oracle  # noqa: E402
from pypore_amd import engine, grid, synth  # noqa: E402
from pypore_amd.parsers import SpeedyStatSplit, lambda_event_parser  # noqa: E402

pytestmark = pytest.mark.gpu
T = engine.INGEST_PASS
LENGTHS = (3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 5, 140001, 200000)
G = engine.INGEST_GRID_MAX
# beyond G * T samples the launch is G workgroups and each strides: a second trip that is full for workgroup 0 and ragged for
# workgroup 1; two full trips for every workgroup and a ragged third for workgroup 0
STRIDED = (G * T + T + 5, 2 * G * T + 65)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same_as_host(x, t=None):
    """affine_grid_device on the tensor == affine_grid on the array: quantum and offset to the bit, the counts exactly;
    ValueError where it raises.  Returns the device result (None: both refused)."""
    t = _dev(x) if t is None else t
    try:
        with np.errstate(all="ignore"):
            want = grid.affine_grid(x)
    except ValueError:
        with pytest.raises(ValueError, match="not on an ADC grid"):
            grid.affine_grid_device(t)
        return None
    q, o, k = grid.affine_grid_device(t)
    assert (q, o) == want[:2]
    assert k.dtype == torch.int16 and k.is_cuda and k.shape == t.shape
    np.testing.assert_array_equal(k.cpu().numpy(), want[2])
    return q, o, k


@pytest.mark.parametrize("offset", ic.OFFSETS)
@pytest.mark.parametrize("n", LENGTHS)
def test_grid_recovery_equals_affine_grid_and_the_counts(n, offset):
    counts = ic.noisy_counts(n, seed=n)
    x = ic.current_of(counts, ic.Q, offset)
    got = _same_as_host(x)
    if n >= 63:                                              # (neighbouring counts occur: the construction itself)
        np.testing.assert_array_equal(got[2].cpu().numpy(), ic.recentred(counts))
    # the same samples 8 bytes off a 16-byte boundary: one head sample, the counts go out unpaired
    t = _dev(np.concatenate(([0.0], x)))[1:]
    assert t.data_ptr() % 16 == 8
    _same_as_host(x, t)


def test_grid_recovery_on_the_shortest_arrays():
    q, o, k = grid.affine_grid_device(torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert (q, o, k.numel(), k.dtype) == (1.0, 0.0, 0, torch.int16)
    for offset in ic.OFFSETS:
        for c in ([7], [7, 7], [5, 9], [4, 5, 7]):
            assert _same_as_host(ic.current_of(c, ic.Q, offset)) is not None


def test_grid_recovery_recentres_a_trace_on_both_rails():
    counts = ic.rails_counts()
    for offset in ic.OFFSETS:
        q, o, k = _same_as_host(ic.current_of(counts, ic.Q, offset))
        np.testing.assert_array_equal(k.cpu().numpy(), counts)


def test_grid_recovery_refines_a_candidate_that_is_twice_the_spacing():
    counts = ic.refinement_counts()
    q, o, k = _same_as_host(ic.current_of(counts, ic.Q, 12.25))
    np.testing.assert_array_equal(k.cpu().numpy(), ic.recentred(counts))


@pytest.mark.parametrize("d", ic.TOLERANCE_D)
def test_grid_recovery_at_the_tolerance(d):
    _same_as_host(ic.tolerance_current(d))


def test_grid_check_reports_what_numpy_computes():
    """The report itself, on a grid that fits (fractions of rounding size) and on one that does not (twice the spacing)."""
    ctx = engine.context()
    for n in (1, 65, T + 1, 2 * T + 5, 140001):
        x = ic.current_of(ic.noisy_counts(n, n, -300, 300), ic.Q, -3.7)
        for q in (ic.Q, 2 * ic.Q, 0.7 * ic.Q):
            r = ctx.grid_check(_dev(x), float(x.min()), q, ic.TOL)
            want = ic.check_on_host(x, float(x.min()), q)
            assert (r.max_frac, r.min_frac_above, r.min_count, r.max_count, r.n_nonfinite, r.n_undefined) == want


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_grid_recovery_refuses_samples_that_are_not_finite(bad):
    n = 2 * T + 5
    for at in (0, T, n - 1):
        x = ic.current_of(ic.noisy_counts(n, 3), ic.Q, 12.25)
        x[at] = bad
        assert _same_as_host(x) is None
        assert engine.context().grid_check(_dev(x), 0.0, ic.Q).n_nonfinite == 1
        with pytest.raises(ValueError):
            engine.to_device(_dev(x))


def test_grid_recovery_refuses_counts_beyond_int16():
    x = ic.current_of(np.arange(70000), ic.Q, 12.25)
    with pytest.raises(ValueError, match="ADC counts beyond int16 on a grid that is not a power of two"):
        grid.affine_grid_device(_dev(x))
    with pytest.raises(ValueError, match="ADC counts beyond int16 on a grid that is not a power of two"):
        engine.to_device(x)                                  # (the host road: _int_counts_tensor's own refusal)
    with pytest.raises(ValueError, match="ADC counts beyond int16 on a grid that is not a power of two"):
        engine.to_device(_dev(x))


@pytest.mark.parametrize("where", ("first", "last", "last partial wave", "none"))
def test_narrow_f64_equals_astype_and_counts_what_it_changed(where, monkeypatch):
    n = 2 * T + 5 + 64 + 7                                   # three workgroups (one pass each): two full, then a wave and a partial one
    x = synth.counts_to_pa(ic.noisy_counts(n, 11, 1200, 1800), np.float64)
    if where != "none":
        x[{"first": 0, "last": n - 1, "last partial wave": n - 5}[where]] += 2.0 ** -40
    a32 = x.astype(np.float32)
    for t in (_dev(x), _dev(np.concatenate(([0.0], x)))[1:]):
        out, bad = engine.context().narrow_f64(t)
        assert bad == int(np.sum(a32.astype(np.float64) != x)) == (0 if where == "none" else 1)
        assert out.dtype == torch.float32
        np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), a32.view(np.int32))
    _staged_equals_host(x, monkeypatch)                      # the refusal (and what follows it) is the host road's


# ---- the grid-stride step: more samples than one pass of the whole launch ----------------------------------------------------
@pytest.fixture(scope="module", params=STRIDED)
def strided(request):
    """(counts, their current on the header scale, affine_grid of it) at a length that makes workgroups stride."""
    n = request.param
    counts = ic.noisy_counts(n, seed=n % 1000)
    x = ic.current_of(counts, ic.Q, 12.25)
    return counts, x, grid.affine_grid(x)


def test_strided_grid_recovery_equals_affine_grid(strided):
    counts, x, want = strided
    n = x.size
    assert n > G * T and grid.subset_step(n) >= 64
    padded = _dev(np.concatenate(([0.0], x)))
    for t in (_dev(x), padded[1:]):                          # aligned, and 8 bytes off a 16-byte boundary
        q, o, k = grid.affine_grid_device(t)
        assert (q, o) == want[:2]
        k = k.cpu().numpy()
        np.testing.assert_array_equal(k, want[2])
        np.testing.assert_array_equal(k, ic.recentred(counts))
        # the report of a grid that does not fit, against numpy: every trip of every workgroup is in these numbers
        r = engine.context().grid_check(t, float(x.min()), 0.7 * ic.Q, ic.TOL)
        assert (r.max_frac, r.min_frac_above, r.min_count, r.max_count, r.n_nonfinite, r.n_undefined) == \
            ic.check_on_host(x, float(x.min()), 0.7 * ic.Q)
    del padded


def test_strided_grid_recovery_sees_one_sample_of_a_later_trip(strided):
    """One sample that only a second (or third) trip reads -- off the subset -- moved off the grid, and made non-finite."""
    _, x, want = strided
    n, step = x.size, grid.subset_step(x.size)
    for at in (G * T + 3, n - 2):                            # workgroup 0's second trip; the last, ragged trip
        assert at % step and at >= G * T
        y = x.copy()
        y[at] += 2e-6 * ic.Q
        for t in (_dev(y), _dev(np.concatenate(([0.0], y)))[1:]):
            r = engine.context().grid_check(t, float(y.min()), want[0], ic.TOL)
            assert r.max_frac > ic.TOL and r.min_frac_above == r.max_frac and r.n_nonfinite == 0
            assert r.max_frac == ic.check_on_host(y, float(y.min()), want[0])[0]
            with pytest.raises(ValueError, match="not on an ADC grid"):
                grid.affine_grid_device(t)
        y[at] = np.nan
        assert engine.context().grid_check(_dev(y), float(x.min()), want[0]).n_nonfinite == 1
        with pytest.raises(ValueError, match="not on an ADC grid"):
            grid.affine_grid_device(_dev(y))


@pytest.mark.parametrize("n", STRIDED)
def test_strided_narrow_f64_equals_astype(n):
    x = synth.counts_to_pa(ic.noisy_counts(n, 11, 1200, 1800), np.float64)
    bad_at = (G * T + 3, n - 2)                              # both beyond the first trip
    for at in bad_at:
        x[at] += 2.0 ** -40
    a32 = x.astype(np.float32)
    assert int(np.sum(a32.astype(np.float64) != x)) == len(bad_at)
    for t in (_dev(x), _dev(np.concatenate(([0.0], x)))[1:]):
        out, bad = engine.context().narrow_f64(t)
        assert bad == len(bad_at)
        assert torch.equal(out.view(torch.int32), _dev(a32.view(np.int32)))
    x[list(bad_at)] = a32[list(bad_at)]
    out, bad = engine.context().narrow_f64(_dev(x))
    assert bad == 0 and torch.equal(out.view(torch.int32), _dev(a32.view(np.int32)))


# ---- roads ---------------------------------------------------------------------------------------------------------------------
def _staged_equals_host(x, monkeypatch):
    """to_device_with_counts through the staged float64 upload == through the host passes."""
    monkeypatch.setattr(engine, "_STAGE_F64_MIN", None)
    try:
        want = engine.to_device_with_counts(x)
    except ValueError:
        want = None
    monkeypatch.setattr(engine, "_STAGE_MIN", 1024)
    monkeypatch.setattr(engine, "_STAGE_F64_MIN", 1024)
    monkeypatch.setattr(engine, "_STAGE_CHUNK_F64", 4096)
    if want is None:
        with pytest.raises(ValueError):
            engine.to_device_with_counts(x)
        return None
    (s, k), (hs, hk) = engine.to_device_with_counts(x), want
    assert s.tensor.dtype == hs.tensor.dtype and (s.quantum, s.offset) == (hs.quantum, hs.offset)
    assert torch.equal(s.tensor.view(torch.int16), hs.tensor.view(torch.int16))      # bit for bit
    assert (k is None) == (hk is None)
    if k is not None:
        assert k.dtype == hk.dtype == np.int64
        np.testing.assert_array_equal(k, hk)
    assert engine.to_device(x).tensor.dtype == hs.tensor.dtype
    return s


def test_staged_numpy_road_equals_the_host_road(monkeypatch):
    counts = synth.random_dwell_counts(20001, 5)
    s = _staged_equals_host(synth.counts_to_pa(counts, np.float64), monkeypatch)          # several chunks and a ragged tail
    assert s.tensor.dtype == torch.float32 and s.quantum == synth.QUANTUM
    monkeypatch.undo()
    s = _staged_equals_host(ic.current_of(counts, ic.Q, 12.25), monkeypatch)
    assert s.tensor.dtype == torch.int16
    monkeypatch.undo()
    assert _staged_equals_host(100.0 + np.random.default_rng(2).normal(size=20001), monkeypatch) is None


@pytest.fixture(scope="module")
def step_trace():
    """A 3e5-sample step trace on the header scale with an offset: the values, its oracle boundaries and statistics."""
    x = ic.current_of(synth.random_dwell_counts(300000, 5), ic.Q, 12.25)
    ref = oracle.parse(x, prior_segments_per_second=10.)
    return x, ref, oracle.segment_stats(x, ref)


def test_speedystatsplit_takes_a_float64_device_tensor_on_the_header_scale(step_trace):
    x, ref, st = step_trace
    t = _dev(x)
    with pytest.raises(ValueError):                          # (what made this input a ValueError: it is not float32)
        engine.to_device_samples(t)
    segs = SpeedyStatSplit(prior_segments_per_second=10.).parse(t)
    host = SpeedyStatSplit(prior_segments_per_second=10.).parse(x)
    got = np.array([s.start for s in segs[1:]], dtype=np.int32)
    np.testing.assert_array_equal(got, [s.start for s in host[1:]])
    np.testing.assert_array_equal(got, ref)
    assert len(ref) >= 10
    assert [(s.start, s.end, s.duration) for s in segs] == [(s.start, s.end, s.duration) for s in host]
    np.testing.assert_allclose([s.mean for s in segs], st[:, 0], rtol=1e-5)
    np.testing.assert_allclose([s.std for s in segs], st[:, 1], rtol=1e-5)
    assert torch.equal(segs[1].current, t[segs[1].start:segs[1].end])           # slices of the caller's tensor
    s = engine.to_device(t)
    assert s.tensor.dtype == torch.int16 and (s.quantum, s.offset) == grid.affine_grid(x)[:2]


def _events(p, cur):
    return [(e.start, e.duration, np.asarray(e.current)) for e in p.parse(cur)]


def _same_events(p, x):
    got, want = _events(p, _dev(x)), _events(p, x)
    assert [(a, n) for a, n, _ in got] == [(a, n) for a, n, _ in want]
    for (_, _, c), (_, _, w) in zip(got, want):
        np.testing.assert_array_equal(c, w)                  # the caller's own values, not count * quantum + offset
    return want


def test_event_detector_takes_a_float64_device_tensor_on_the_header_scale(step_trace):
    c, _ = synth.file_trace_counts(600000, 41, gap=30011, ev_lo=60000, ev_hi=200000)
    x = ic.current_of(c, ic.Q, 12.25)
    between = x[(x > 70.0) & (x < 118.0)]
    on_a_sample = float(between.max()) if between.size else float(np.median(x))
    for threshold in (on_a_sample, on_a_sample + 0.5 * ic.Q, 100.0):
        p = lambda_event_parser(threshold=threshold)
        p.MIN_DURATION = 1000
        want = _same_events(p, x)
        rs, rl = oracle.lambda_events(x, threshold=threshold, min_duration=1000)
        assert [(a, n) for a, n, _ in want] == list(zip(rs.tolist(), rl.tolist())) and len(want) >= 2
    # the step trace itself: cut at its largest value, and whole under a threshold between two counts above it
    xs = step_trace[0]
    for threshold, n_min in ((float(xs.max()), 0), (float(xs.max()) + 0.5 * ic.Q, 1)):
        assert len(_same_events(lambda_event_parser(threshold=threshold), xs)) >= n_min


def test_off_grid_policy_takes_a_float64_device_tensor():
    x = synth.offgrid_trace(60000, 3)
    x = np.asarray(x[0] if isinstance(x, tuple) else x, dtype=np.float64)
    t = _dev(x)
    with pytest.raises(ValueError) as dev_err:
        SpeedyStatSplit(prior_segments_per_second=10.).parse(t)
    with pytest.raises(ValueError) as host_err:
        SpeedyStatSplit(prior_segments_per_second=10.).parse(x)
    assert str(dev_err.value) == str(host_err.value)
    for mode in ("requantise", "exact", "exact_on_near_tie"):
        p = SpeedyStatSplit(prior_segments_per_second=10., off_grid=mode)
        segs, host = p.parse(t), p.parse(x)
        assert [(s.start, s.end) for s in segs] == [(s.start, s.end) for s in host] and len(segs) >= 3
        assert torch.equal(segs[1].current, t[segs[1].start:segs[1].end])
        np.testing.assert_allclose([s.mean for s in segs], [s.mean for s in host], rtol=1e-12)


def test_a_float32_exact_float64_tensor_goes_up_as_before():
    x = synth.counts_to_pa(synth.random_dwell_counts(50000, 7), np.float64)
    s, k = engine.to_device_with_counts(_dev(x))
    assert k is None and s.tensor.dtype == torch.float32 and (s.quantum, s.offset) == (synth.QUANTUM, 0.0)
    assert torch.equal(s.tensor, _dev(x.astype(np.float32)))
    t, q = engine.to_device_samples(_dev(x))
    assert q == synth.QUANTUM and torch.equal(t, s.tensor)
    segs = SpeedyStatSplit(prior_segments_per_second=10.).parse(_dev(x))
    np.testing.assert_array_equal([s_.start for s_ in segs[1:]], oracle.parse(x, prior_segments_per_second=10.))
