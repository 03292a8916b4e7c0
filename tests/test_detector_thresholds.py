"""The thresholds the event detector's kernels receive (engine.detector_thresholds).  The kernels test
double(k) * quantum < threshold and > min_current on the counts k; the reference tests x < threshold and x > min_current on
the pA values x the caller holds.  Stub contexts record what lambda_event_parser.parse, File.parse and
pipeline.segment_file_trace hand to the library, and the two predicates are compared on every sample (no GPU)."""
import os

import numpy as np
import pytest
import torch

from pypore_amd import abf, engine, pipeline, synth
from pypore_amd.grid import Deferred, GridArray
from pypore_amd.parsers import lambda_event_parser

MIN_CURRENT = lambda_event_parser.MIN_CURRENT


class _Recorder:
    """Stands in for engine.Context: records (samples, quantum, threshold, min_current, offset_counts) of every detector
    call and finds no events."""

    def __init__(self):
        self.calls = []

    def detect_events(self, samples, quantum, threshold=90.0, min_duration=100000, min_current=-0.5, offset_counts=0):
        self.calls.append((samples, quantum, threshold, min_current, offset_counts))
        return np.zeros(0, np.int64), np.zeros(0, np.int64)

    def detect_segment_trace(self, samples, quantum, params, threshold=90.0, min_duration=100000, min_current=-0.5,
                             offset_counts=0, want_stats=False):
        self.calls.append((samples, quantum, threshold, min_current, offset_counts))
        return np.zeros(0, np.int64), np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int32), np.zeros(1, np.int64), None

    def segment_events(self, samples, st, ln, params, quantum, offset_counts=0, want_stats=False):
        return torch.zeros(0, dtype=torch.int32), np.zeros(len(st) + 1, np.int64), None


@pytest.fixture
def rec(monkeypatch):
    """A recorder behind engine.context, and host tensors where the parsers would upload."""
    r = _Recorder()
    monkeypatch.setattr(engine, "context", lambda device=None: r)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(engine, "_int_counts_tensor", lambda counts, dev: torch.from_numpy(np.asarray(counts).astype(np.int16)))

    def samples(current, quantum=None, device=None, full_detect=False):
        a = np.asarray(current)
        if a.dtype == np.int16:
            return torch.from_numpy(a.copy()), (1.0 if quantum is None else quantum)
        q = engine.detect_quantum(a, full=full_detect) if quantum is None else quantum
        a32 = a.astype(np.float32)
        if not np.array_equal(a32.astype(np.float64), a):
            raise ValueError("samples are not exactly representable in float32")
        return torch.from_numpy(a32), q
    monkeypatch.setattr(engine, "to_device_samples", samples)
    return r


def _kernel_counts(call):
    """The counts k the kernels test (seg_device.hpp load_count: int16 + offset_counts, float32 value / quantum)."""
    t, q, _, _, oc = call
    a = t.numpy()
    if a.dtype == np.int16:
        return a.astype(np.int64) + oc
    k = a.astype(np.float64) / q
    assert np.array_equal(k, np.rint(k))
    return k.astype(np.int64)


def _assert_same_predicates(call, x, threshold, min_current=MIN_CURRENT):
    """double(k) * q < threshold' is x < threshold and double(k) * q > min_current' is x > min_current, sample by sample."""
    kq = _kernel_counts(call).astype(np.float64) * call[1]
    x = np.asarray(x, dtype=np.float64)
    assert kq.shape == x.shape
    bad = np.flatnonzero((kq < call[2]) != (x < threshold))
    assert bad.size == 0, "threshold %r -> %r: %d samples judged otherwise, first x = %r" % (threshold, call[2], bad.size, x[bad[0]])
    bad = np.flatnonzero((kq > call[3]) != (x > min_current))
    assert bad.size == 0, "min_current %r -> %r: %d samples judged otherwise, first x = %r" % (min_current, call[3], bad.size, x[bad[0]])


def _decimal_trace(step, seed=11):
    """float64 currents at `step` pA resolution (no power-of-two grid): open channel at 110 pA, a 150 000-sample blockade at
    45 pA over [100000, 250000), samples of exactly 90.0 and -0.5 inside the blockade and where it ends."""
    rng = np.random.default_rng(seed)
    n = 300000
    x = 110.0 + rng.normal(0, 1.5, n)
    x[100000:250000] = 45.0 + rng.normal(0, 1.5, 150000)
    x = np.round(x / step) * step
    x[250000] = 90.0
    x[120000:120010] = 90.0
    x[130000] = -0.5
    x[130001] = -0.5 + step
    return x


@pytest.mark.parametrize("step", [0.1, 0.05, 0.01])
def test_decimal_resolution_float64(rec, step):
    x = _decimal_trace(step)
    assert np.count_nonzero(x == 90.0) == 11 and np.count_nonzero(x == -0.5) == 1
    lambda_event_parser(threshold=90).parse(x, device=0)
    (call,) = rec.calls
    assert call[0].dtype == torch.int16                     # (the affine-grid route: counts of a recovered grid)
    _assert_same_predicates(call, x, 90)


def _repro_trace():
    rng = np.random.default_rng(0)
    x = np.round(110 + rng.normal(0, 1.5, 300000), 1)
    x[100000:250000] = np.round(45 + rng.normal(0, 1.5, 150000), 1)
    x[250000] = 90.0
    return x


def test_decimal_resolution_repro_of_the_issue(rec):
    """x = round(110 + N(0, 1.5), 1) with a blockade at round(45 + N(0, 1.5), 1) over [100000, 250000) and x[250000] = 90.0:
    the sample at the threshold is not below it."""
    x = _repro_trace()
    lambda_event_parser(threshold=90).parse(x, device=0)
    (call,) = rec.calls
    _assert_same_predicates(call, x, 90)
    k = _kernel_counts(call)
    assert not float(k[250000]) * call[1] < call[2]


def test_a_grid_that_is_not_monotone_at_the_threshold_is_detected_on_the_host(rec):
    """Counts of the recovered grid that fall on both sides of the rule: no count-space threshold exists, so the default rules
    run on the host -- the same events as custom rules that restate them."""
    x = _repro_trace()
    s = engine.to_device(x, None, None, 0)
    q, o = s.quantum, s.offset
    k = _kernel_counts((s.tensor, q, 0, 0, 0))
    kt = int(k[250000])
    # a value of count kt just below 90 beside the 90.0 of the same count: still on the grid to within its tolerance
    y = x.copy()
    y[250001] = np.nextafter(90.0, -np.inf)
    assert np.rint((y[250001] - o) / q) == kt
    assert engine.detector_thresholds(q, 90, MIN_CURRENT, values=y, counts=k) is None
    p = lambda_event_parser(threshold=90)
    got = p.parse(y, device=0)
    assert rec.calls == []
    rules = lambda_event_parser(threshold=90, rules=[lambda e: e.duration > p.MIN_DURATION, lambda e: e.min > p.MIN_CURRENT,
                                                    lambda e: e.max < 90])
    want = rules.parse(y)
    assert [(e.start, e.duration) for e in got] == [(e.start, e.duration) for e in want] == [(100000, 150000)]


def _abf_grid():
    """Scale and offset as an .abf header gives them: fp32 header floats, a scale on no power-of-two grid."""
    scale = float(np.float32(10.0)) / float(np.float32(0.0005)) / float(np.float32(20.0)) / 32768
    return scale, 1.75


def _hard_thresholds(q, o, k):
    """Sample values (and their float64 neighbours) at which x < t on x = fl(fl(k q) + o) and the old count-space test
    fl(k q) < t - o disagree for some count of `k` -- searched, not hard-wired."""
    ks = np.unique(k)
    x = GridArray.from_counts(ks, q, o)
    cands = np.unique(np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]))
    kq = ks.astype(np.float64) * q
    hard = [t for t in cands if np.any((kq < t - o) != (np.asarray(x) < t))]
    return hard, cands


def _abf_counts(seed=3, n=300000):
    rng = np.random.default_rng(seed)
    scale, _ = _abf_grid()
    k = np.rint((110 + rng.normal(0, 1.5, n)) / scale)
    k[100000:250000] = np.rint((45 + rng.normal(0, 1.5, 150000)) / scale)
    # every count from 62 to 68 pA and from 126 to 131 pA, short ramps in the open channel: x = fl(fl(k q) + o) crosses a
    # power of two there while k q does not yet, which is where the two roundings part
    for at, lo, hi in ((1000, 62.0, 68.0), (2000, 126.0, 131.0)):
        r = np.arange(np.rint(lo / scale), np.rint(hi / scale))
        k[at:at + r.size] = r
    return k.astype(np.int16)


@pytest.mark.parametrize("kind", ["GridArray", "Deferred"])
def test_file_grid_with_inexact_scale_and_offset(rec, kind):
    q, o = _abf_grid()
    k = _abf_counts()
    hard, cands = _hard_thresholds(q, o, k)
    assert len(hard) >= 3, "no threshold found at which the old test fails: the case covers nothing"
    x = np.asarray(GridArray.from_counts(k, q, o))
    sel = hard[:: max(1, len(hard) // 24)] + [90, 90.0, cands[len(cands) // 2]]
    for t in sel:
        cur = GridArray.from_counts(k, q, o) if kind == "GridArray" else Deferred.from_counts(k, q, o)
        rec.calls.clear()
        lambda_event_parser(threshold=t).parse(cur, device=0)
        (call,) = rec.calls
        assert call[0].dtype == torch.int16
        _assert_same_predicates(call, x, t)
        if kind == "Deferred":
            assert not cur.built                                  # (no float64 array was written out for the thresholds)


def test_file_parse_on_an_abf_with_inexact_scale_and_offset(rec, tmp_path):
    from pypore_amd.DataTypes import File
    k = _abf_counts(seed=4)
    path = abf.write_abf(os.path.join(str(tmp_path), "t.abf"), k, adc_range=10.0, adc_resolution=32768,
                         instrument_scale=0.0005, signal_gain=20.0, instrument_offset=1.75)
    _, _, scale, offset = abf.read_abf_counts(path)
    assert (scale, offset) == _abf_grid()
    x = np.asarray(GridArray.from_counts(k, scale, offset))
    hard, _ = _hard_thresholds(scale, offset, k)
    assert hard
    for t in hard[:4] + [90]:
        rec.calls.clear()
        File(path).parse(lambda_event_parser(threshold=t))
        (call,) = rec.calls
        _assert_same_predicates(call, x, t)


@pytest.mark.parametrize("single_pass", [True, False])
@pytest.mark.parametrize("offset_counts", [0, 1234, -1234])
def test_segment_file_trace_on_an_inexact_grid(rec, single_pass, offset_counts):
    """pipeline.segment_file_trace (and parse_abf through it): pA = fl(fl(k q) + offset) of the counts the kernels read."""
    q, o = _abf_grid()
    raw = (_abf_counts(seed=5).astype(np.int64) - offset_counts).astype(np.int16)
    k = raw.astype(np.int64) + offset_counts
    x = np.asarray(GridArray.from_counts(k, q, o))
    hard, _ = _hard_thresholds(q, o, k)
    assert hard
    for t in hard[:6] + [90.0]:
        rec.calls.clear()
        pipeline.segment_file_trace(torch.from_numpy(raw), q, threshold=t, offset_counts=offset_counts, offset=o, ctx=rec,
                                    single_pass=single_pass)
        (call,) = rec.calls
        _assert_same_predicates(call, x, t)


def test_power_of_two_float64_with_an_explicit_offset(rec):
    q, o = synth.QUANTUM, 2.375
    c = synth.file_trace_counts(300000, 7, gap=30011, ev_lo=60000, ev_hi=200000)[0]
    x = c.astype(np.float64) * q + o
    for t in (90.0, float(x[1000]), float(np.nextafter(x[1000], np.inf)), float(np.nextafter(x[1000], -np.inf)),
              o + 90.0 - q / 3):
        rec.calls.clear()
        lambda_event_parser(threshold=t).parse(x, quantum=q, offset=o, device=0)
        (call,) = rec.calls
        assert call[0].dtype == torch.float32
        _assert_same_predicates(call, x, t)


@pytest.mark.parametrize("quantum,offset", [(None, None), (0.030517578125, None), (_abf_grid()[0], _abf_grid()[1])])
def test_int16_numpy(rec, quantum, offset):
    k = _abf_counts(seed=6)
    q = 1.0 if quantum is None else quantum
    x = np.asarray(GridArray.from_counts(k, q, 0.0 if offset is None else offset))
    ts = [90, float(x[5]), float(np.nextafter(x[5], -np.inf)), float(x[150000])]
    if quantum is None:
        ts += [3600, 3600.5]
    for t in ts:
        rec.calls.clear()
        lambda_event_parser(threshold=t).parse(k, quantum=quantum, offset=offset, device=0)
        (call,) = rec.calls
        _assert_same_predicates(call, x, t)


def test_zero_offset_is_passed_through_bit_for_bit(rec):
    """Power-of-two grid, no offset (bench, synth): the thresholds reach the library as the caller gave them."""
    c = synth.file_trace_counts(300000, 8, gap=30011, ev_lo=60000, ev_hi=200000)[0]
    x = synth.counts_to_pa(c, np.float64)
    for t in (90, 90.0, 87.3, float(x[17])):
        rec.calls.clear()
        lambda_event_parser(threshold=t).parse(x, device=0)
        (call,) = rec.calls
        assert float(call[2]).hex() == float(t).hex() and float(call[3]).hex() == MIN_CURRENT.hex()
        _assert_same_predicates(call, x, t)
    for single_pass in (True, False):
        rec.calls.clear()
        pipeline.segment_file_trace(torch.from_numpy(c.astype(np.int16)), synth.QUANTUM, threshold=90.0, ctx=rec,
                                    single_pass=single_pass)
        (call,) = rec.calls
        assert float(call[2]).hex() == (90.0).hex() and float(call[3]).hex() == MIN_CURRENT.hex()
    # a GridArray of zero offset on an inexact scale: the kernel's product fl(k q) is the caller's value itself
    q, _ = _abf_grid()
    k = _abf_counts(seed=9)
    rec.calls.clear()
    lambda_event_parser(threshold=90).parse(GridArray.from_counts(k, q, 0.0), device=0)
    (call,) = rec.calls
    assert (call[2], call[3]) == (90.0, MIN_CURRENT)


def test_each_threshold_on_its_own_at_extremes():
    """Every pair of thresholds -- finite, at a sample value, huge, infinite (min_current=-inf: the rule off), NaN -- over every
    int16 count: each threshold is decided on its own, a finite one beside an infinite one included."""
    q, o = _abf_grid()
    k = np.arange(-32768, 32768, dtype=np.int64)
    x = np.asarray(GridArray.from_counts(k, q, o))
    kq = k.astype(np.float64) * q
    hard, _ = _hard_thresholds(q, o, _abf_counts())
    ts = [90.0, hard[0], hard[-1], -0.5, 1e9, -1e9, 1e307, -1e307, 1.7e308, float("inf"), -float("inf"), float("nan")]
    for t in ts:
        for mc in ts:
            thr, mcd = engine.detector_thresholds(q, t, mc, offset=o)
            assert np.array_equal(kq < thr, x < t), (t, mc)
            assert np.array_equal(kq > mcd, x > mc), (t, mc)
    # no count to find (quantum not positive): the offset moves to the other side, as ever
    assert engine.detector_thresholds(-q, 90.0, -0.5, offset=o) == (90.0 - o, -0.5 - o)
    ks = np.arange(-40, 40)
    xs = ks * 0.1 + 3.0
    for t in (-10.0, 10.0, xs[0], xs[-1], float("inf"), -float("inf")):
        thr, mc = engine.detector_thresholds(0.1, t, t, values=xs, counts=ks)
        assert np.array_equal(ks * 0.1 < thr, xs < t) and np.array_equal(ks * 0.1 > mc, xs > t)


class _NoMinCurrent(lambda_event_parser):
    MIN_CURRENT = -float("inf")                            # the min-current rule switched off


@pytest.mark.parametrize("single_pass", [True, False])
def test_min_current_off_with_an_offset_on_segment_file_trace(rec, single_pass):
    """min_current=-inf beside a finite threshold on a grid with an offset: the threshold still moves to count space."""
    q, o = _abf_grid()
    k = _abf_counts(seed=10)
    x = np.asarray(GridArray.from_counts(k, q, o))
    hard, _ = _hard_thresholds(q, o, k)
    for t in hard[:4] + [90.0]:
        rec.calls.clear()
        pipeline.segment_file_trace(torch.from_numpy(k), q, threshold=t, min_current=-np.inf, offset=o, ctx=rec,
                                    single_pass=single_pass)
        (call,) = rec.calls
        assert call[3] == -np.inf
        _assert_same_predicates(call, x, t, min_current=-np.inf)
        if t == 90.0:
            assert abs(call[2] - (90.0 - o)) < q                  # (not 90 itself: 1.75 pA, some 57 counts, away)


@pytest.mark.parametrize("kind", ["GridArray", "Deferred", "float64"])
def test_min_current_off_with_an_offset_through_the_parser(rec, kind):
    q, o = _abf_grid()
    k = _abf_counts(seed=11)
    x = np.asarray(GridArray.from_counts(k, q, o))
    hard, _ = _hard_thresholds(q, o, k)
    for t in hard[:3] + [90.0]:
        cur = dict(GridArray=lambda: GridArray.from_counts(k, q, o), Deferred=lambda: Deferred.from_counts(k, q, o),
                   float64=lambda: x.copy())[kind]()
        rec.calls.clear()
        _NoMinCurrent(threshold=t).parse(cur, device=0)
        (call,) = rec.calls
        if kind != "float64":                                  # (float64: read off the data, below every count)
            assert call[3] == -np.inf
        _assert_same_predicates(call, x, t, min_current=-np.inf)


def test_a_grid_array_with_an_explicit_quantum_is_judged_on_its_values(rec):
    """quantum= given: to_device rebuilds the counts from the caller's grid instead of the array's own, and the thresholds
    come from the values the array holds and those counts."""
    q, o = _abf_grid()
    k = _abf_counts(seed=12)
    g = GridArray.from_counts(k, q, o)
    s, counts = engine.to_device_with_counts(g, q, o, 0)
    assert counts is not None and np.array_equal(counts, k)
    hard, _ = _hard_thresholds(q, o, k)
    for t in hard[:4] + [90.0]:
        rec.calls.clear()
        lambda_event_parser(threshold=t).parse(g, quantum=q, offset=o, device=0)
        (call,) = rec.calls
        _assert_same_predicates(call, np.asarray(g), t)


def test_to_device_reports_the_counts_of_recovered_grids_only(rec):
    """to_device_with_counts: None where the values are fl(fl(k q) + o) by construction, the host counts where float samples
    went up as the counts of a grid they only lie on to within rounding (no copy back from the device)."""
    q, o = _abf_grid()
    k = _abf_counts(seed=13)
    assert engine.to_device_with_counts(GridArray.from_counts(k, q, o), device=0)[1] is None
    assert engine.to_device_with_counts(Deferred.from_counts(k, q, o), device=0)[1] is None
    assert engine.to_device_with_counts(k, q, o, device=0)[1] is None
    c = synth.file_trace_counts(30000, 7, gap=3011, ev_lo=6000, ev_hi=20000)[0]
    assert engine.to_device_with_counts(synth.counts_to_pa(c, np.float64), device=0)[1] is None
    s, got = engine.to_device_with_counts(c * synth.QUANTUM + 2.375, None, 2.375, 0)
    assert s.tensor.dtype == torch.float32 and np.array_equal(got, c)
    x = _repro_trace()
    s, got = engine.to_device_with_counts(x, device=0)
    assert s.tensor.dtype == torch.int16 and np.array_equal(got, s.tensor.numpy())
