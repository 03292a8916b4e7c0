"""StatSplit on the GPU against the goldens recorded from the reference (tests/golden/make_golden_statsplit.py).

use_log=False runs -- both splitters -- are compared bit for bit on every case: the arithmetic is the reference's, operation
for operation, and nothing but IEEE additions, products and divisions lies between the samples and a decision.  use_log=True
runs are compared where the recorded decision margin is at least 1e-9 (a device logarithm differs from the host's in its
last bit: ~1e-14 of a gain at these sizes); the generator asserts that this leaves at least 9 runs in 10.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import statsplit_cases as SC  # noqa: E402
import statsplit_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pypore_amd import _lib, engine, synth  # noqa: E402
from pypore_amd.parsers import SpeedyStatSplit, StatSplit  # noqa: E402

MARGIN_MIN = 1e-9


def _bounds(segs):
    return np.array([s.start for s in segs[1:]], dtype=np.int32)


def _decided(run):
    case, splitter, use_log = run
    return not use_log or SC.golden()[1][SC.key(case, splitter, use_log)] >= MARGIN_MIN


RUNS = [r for r in SC.runs() if _decided(r)]


@pytest.mark.parametrize("run", RUNS, ids=[SC.key(*r) for r in RUNS])
def test_golden(run):
    case, splitter, use_log = run
    x = SC.build(case)
    segs = StatSplit(use_log=use_log, splitter=splitter, **case["par"]).parse(x, case.get("start", 0), case.get("end", -1))
    want = SC.golden()[0][SC.key(case, splitter, use_log)]
    assert np.array_equal(_bounds(segs), want)
    # Segments: absolute start and duration, in samples, tiling [start, end); their current is a view of the input
    start, end = SC.normalised(case)
    edges = [start] + want.tolist() + [end]
    assert [(s.start, s.duration) for s in segs] == [(a, b - a) for a, b in zip(edges, edges[1:])]
    assert all(np.shares_memory(s.current, x) and s.current.shape[0] == s.duration for s in segs)


def test_every_variance_run_is_compared():
    assert sum(1 for _, _, lg in RUNS if not lg) == sum(1 for _, _, lg in SC.runs() if not lg)
    assert 10 * (len(SC.runs()) - len(RUNS)) <= sum(1 for _, _, lg in SC.runs() if lg)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_prefix_sums_are_numpys(n):
    # centred on a level so that samples of both signs occur (x[0] * 0 is a signed zero)
    x = synth.counts_to_pa(synth.step_counts(n, 300, 50 + n), np.float64) - 47.0
    ctx = engine.context(None)
    c, c2, ct = ctx.statsplit_prefix_f64(torch.from_numpy(x).cuda())
    for got, want in ((c, np.cumsum(x)), (c2, np.cumsum(np.multiply(x, x))),
                      (ct, np.cumsum(np.multiply(x, np.linspace(0, n, num=n, endpoint=False))))):
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))
    c, c2, ct = ctx.statsplit_prefix_f64(torch.from_numpy(x).cuda(), want_ct=False)
    assert ct is None and np.array_equal(c2.cpu().numpy().view(np.int64), np.cumsum(x * x).view(np.int64))


def test_window_of_exactly_two_min_widths():
    """W = 2 mw: every window has one candidate and StatSplit takes it; SpeedyStatSplit's guard (cparsers.pyx:164, '<=')
    never scans such a window, with the matching threshold (its own is doubled) or any other."""
    case = SC.BY_NAME["w_eq_2mw"]
    x, par = SC.build(case), case["par"]
    got = _bounds(StatSplit(use_log=True, splitter="stepwise", **par).parse(x))
    assert got.size == 4 and np.array_equal(got, SC.golden()[0]["w_eq_2mw/stepwise/log"])
    speedy = SpeedyStatSplit(min_width=par["min_width"], max_width=par["max_width"], window_width=par["window_width"],
                             min_gain_per_sample=par["min_gain_per_sample"] / 2, off_grid="exact")
    assert len(speedy.parse_exact(np.array(x))) == 1


@pytest.mark.parametrize("splitter", ["stepwise", "slanted"])
def test_short_and_empty_events(splitter):
    p = StatSplit(min_width=50, window_width=100, use_log=False, splitter=splitter)
    x = SC.build(SC.BY_NAME["steps"])
    for n in (0, 1, 49, 99, 100):           # empty; shorter than 2 mw; 2 mw - 1 and 2 mw samples: no window is scanned
        segs = p.parse(np.array(x[:n]))
        assert [(s.start, s.duration) for s in segs] == [(0, n)]
    # one sample more and the single candidate is scanned (and taken: a step sits on it)
    assert _bounds(p.parse(np.array(SC.build(SC.BY_NAME["short_2mw_p1"])))).tolist() == [50]


def _batch_events():
    """Events of unequal lengths cut from the cases, with empty and boundary-free ones between the others."""
    flat = SC.build(SC.BY_NAME["flat_after"])
    names = ["dwell_odd", None, "steps", "flat", None, "dwell", "short", "dwell_maxw"]
    evs = []
    for nm in names:
        if nm is None:
            evs.append(np.zeros(0))
        elif nm == "flat":
            evs.append(np.array(flat[:250]))
        elif nm == "short":
            evs.append(np.array(flat[:33]))
        else:
            evs.append(np.array(SC.build(SC.BY_NAME[nm])))
    return evs


@pytest.mark.parametrize("splitter", ["stepwise", "slanted"])
def test_batch_of_unequal_events(splitter):
    evs = _batch_events()
    par = dict(min_width=17, max_width=100000, window_width=173, min_gain_per_sample=0.5, use_log=False, splitter=splitter)
    got = StatSplit(**par).parse_batch(evs)
    assert len(got) == len(evs)
    for x, segs in zip(evs, got):
        want = statsplit_oracle.segment(x, **par)
        assert np.array_equal(_bounds(segs), want)
        assert sum(s.duration for s in segs) == len(x)
    assert [len(s) for s in got][1] == 1 and len(got[3]) == 1 and len(got[6]) == 1 and len(got[0]) > 1


def test_more_events_than_workgroups():
    n_ev, n = 1100, 300
    x = synth.counts_to_pa(synth.random_dwell_counts(n_ev * n, 61, 60, 250), np.float64)
    par = dict(min_width=40, max_width=100000, window_width=120, min_gain_per_sample=0.5, use_log=False, splitter="stepwise")
    got = StatSplit(**par).parse_batch([x[e * n:(e + 1) * n] for e in range(n_ev)])
    total = 0
    for e in range(n_ev):
        want = statsplit_oracle.segment(x[e * n:(e + 1) * n], **par)
        assert np.array_equal(_bounds(got[e]), want), e
        total += want.size
    assert total > n_ev


def test_capacity_one_short_reports_the_need():
    evs = _batch_events()
    lens = np.array([len(e) for e in evs], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lens)))[:-1]
    cur = torch.from_numpy(np.concatenate(evs)).cuda()
    p = StatSplit(min_width=17, max_width=100000, window_width=173, min_gain_per_sample=0.5, use_log=False)
    ctx = engine.context(None)
    full, off = ctx.statsplit_f64(cur, starts, lens, p._params())
    need = int(off[-1])
    assert need > 0
    with pytest.raises(engine.CapacityError) as err:
        ctx.statsplit_f64(cur, starts, lens, p._params(), cap=need - 1)
    assert err.value.required == need
    again, off2 = ctx.statsplit_f64(cur, starts, lens, p._params(), cap=need)
    assert torch.equal(again, full) and np.array_equal(off, off2)


def test_abi_refusals():
    ctx = engine.context(None)
    cur = torch.zeros(100, dtype=torch.float64, device="cuda")
    one, ln = np.zeros(1, dtype=np.int64), np.full(1, 100, dtype=np.int64)

    def par(mw, maxw, W, splitter=0):
        return _lib.StatSplitParams(mw, maxw, W, 1.0, 0, splitter)
    with pytest.raises(AssertionError):
        ctx.statsplit_f64(cur, one, ln, par(10, 9, 100))
    with pytest.raises(AssertionError):
        ctx.statsplit_f64(cur, one, ln, par(10, 100, 19))
    with pytest.raises(ValueError):
        ctx.statsplit_f64(cur, one, ln, par(0, 100, 19))
    with pytest.raises(ValueError):
        ctx.statsplit_f64(cur, one, ln, par(10, 100, 20, splitter=2))
    with pytest.raises(ValueError):
        ctx.statsplit_f64(cur, one, ln, par(10, 100, 20), hi=np.full(1, 101))
    with pytest.raises(ValueError):                          # longer than 2**30 samples: refused before anything is read
        ctx.statsplit_f64(cur, one, np.full(1, (1 << 30) + 1, dtype=np.int64), par(10, 100, 20))


def test_deviations_from_the_reference():
    x = np.array(SC.build(SC.BY_NAME["steps_ramp"]))
    par = SC.BY_NAME["steps_ramp"]["par"]
    p = StatSplit(use_log=False, splitter="slanted", **par)
    first = _bounds(p.parse(x))
    assert p.splitter == "slanted" and np.array_equal(_bounds(p.parse(x)), first)       # a second parse stays slanted
    assert np.array_equal(first, SC.golden()[0]["steps_ramp/slanted/var"])
    assert not np.array_equal(first, SC.golden()[0]["steps_ramp/stepwise/var"])
    with pytest.raises(ValueError):
        p.parse(x, 0, len(x) - 1)                           # slanted needs end == len(current)
    with pytest.raises(NotImplementedError):
        StatSplit(splitter=lambda a, b: None, **par).parse(x)


def test_tensor_input_and_event_parse():
    from pypore_amd.DataTypes import Event, File
    case = SC.BY_NAME["dwell"]
    x = np.array(SC.build(case))
    p = StatSplit(use_log=False, splitter="stepwise", **case["par"])
    want = SC.golden()[0]["dwell/stepwise/var"]
    assert np.array_equal(_bounds(p.parse(torch.from_numpy(x).cuda())), want)
    assert np.array_equal(_bounds(p.parse(x.astype(np.float32))), want)          # (the 2**-5 grid is exact in float32)
    f = File(current=x, timestep=1000. / 1e5)
    ev = Event(current=x, start=0., end=len(x) / 1e5, duration=len(x) / 1e5, second=1e5, file=f)
    ev.parse(parser=p)
    assert [int(round(s.start * 1e5)) for s in ev.segments[1:]] == want.tolist()


@pytest.mark.parametrize("splitter", ["slanted", "stepwise"])
def test_large_t(splitter):
    """2**24 + 3000 samples, segmented from 2**24 on: sample indices (and their squares) that no float32 holds."""
    x = SC.build(SC.BIG)
    segs = StatSplit(use_log=False, splitter=splitter, **SC.BIG["par"]).parse(x, SC.BIG_HEAD)
    want = SC.golden()[0][SC.key(SC.BIG, splitter, False)]
    assert want.size > 2 and want.min() > SC.BIG_HEAD
    assert np.array_equal(_bounds(segs), want)
    assert segs[0].start == SC.BIG_HEAD and sum(s.duration for s in segs) == 3000
