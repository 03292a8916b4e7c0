"""The state parsers on the GPU against the goldens recorded from the reference (tests/golden/make_golden_state_parsers.py).

snakebase: `==` on every case -- one subtraction and one comparison lie between a sample and a decision.
filter-derivative, prefiltered = 1 (the decision kernels alone): `==` against the restatement on scipy's y for every case,
and against the reference's own decisions on the constructed y of the fdy cases.
filter-derivative, the full route: `==` against the goldens wherever the case's smallest decision margin is at least
1e-9 * max|current| (100 x the device filter's distance from scipy); a case below that is skipped by name, from the manifest.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_parser_cases as PC  # noqa: E402
import state_parser_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pypore_amd import _lib, engine  # noqa: E402
from pypore_amd.DataTypes import File  # noqa: E402
from pypore_amd.parsers import FilterDerivativeSegmenter, snakebase_parser  # noqa: E402


def _ids(cases):
    return [c["name"] for c in cases]


def _spans(segs):
    return np.array([[s.start, s.start + len(s.current)] for s in segs], dtype=np.int32).reshape(-1, 2)


def _params(par, prefiltered):
    return _lib.FilterDerivativeParams(par["low_threshold"], par["high_threshold"], par["cutoff_freq"], par["sampling_freq"],
                                       1 if prefiltered else 0)


def _from_y(y, par):
    """Spans of one filtered current on the prefiltered route."""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).cuda()
    spans, off = engine.context(None).filter_derivative_f64(t, [0], [y.size], _params(par, True))
    assert off.tolist() == [0, spans.shape[0]]
    return spans.cpu().numpy()


# ---- snakebase ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.SNAKE_CASES, ids=_ids(PC.SNAKE_CASES))
def test_snakebase_golden(case):
    x = PC.snake_build(case)
    segs = snakebase_parser().parse(x)
    want = PC.golden()[0]["snake/" + case["name"]]
    assert np.array_equal(_spans(segs), want)
    # the reference's keywords: current and start; the current is a view of the input
    assert all(set(vars(s)) == {"current", "start"} and isinstance(s.start, int) for s in segs)
    assert all(np.shares_memory(s.current, x) for s in segs)


def test_snakebase_tensor_input_and_threshold():
    x = PC.snake_build(PC.SNAKE_BY_NAME["coarse_long"])
    want = PC.golden()[0]["snake/coarse_long"]
    for threshold in (1.5, 0.0, 1e9):
        assert np.array_equal(_spans(snakebase_parser(threshold).parse(torch.from_numpy(x).cuda())), want)


def test_snakebase_batch_of_300_equals_lone_runs():
    events = PC.snake_batch()
    assert len(events) == 300 and any(e.size == 0 for e in events)
    p = snakebase_parser()
    batch = p.parse_batch(events)
    want = [PO.snakebase_spans(e) for e in events]
    assert sum(w.shape[0] for w in want) > 1000
    for e in range(300):
        assert np.array_equal(_spans(batch[e]), want[e]), e
    for e in range(0, 300, 13):                                 # lone device runs of a sample of them
        assert np.array_equal(_spans(p.parse(events[e])), want[e]), e


def test_snakebase_events_inside_one_array():
    """Events as sub-ranges of one device array, out of order and overlapping: every event reads its own range only."""
    x = PC.snake_build(PC.SNAKE_BY_NAME["coarse_long"])
    t = torch.from_numpy(x).cuda()
    starts, lens = [4000, 0, 4096, 100, 8190, 8192], [4192, 4097, 0, 2049, 2, 0]
    spans, off = engine.context(None).snakebase_f64(t, starts, lens)
    sp = spans.cpu().numpy()
    for e, (a, n) in enumerate(zip(starts, lens)):
        assert np.array_equal(sp[off[e]:off[e + 1]], PO.snakebase_spans(x[a:a + n])), e


# ---- filter-derivative ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.FDY_CASES, ids=_ids(PC.FDY_CASES))
def test_filter_derivative_decisions_on_constructed_y(case):
    y, par = PC.fdy_build(case), case["par"]
    got = _from_y(y, par)
    assert np.array_equal(got, PO.filter_derivative_spans_from_y(y, par["low_threshold"], par["high_threshold"]))
    if y.size:
        assert np.array_equal(got, PC.golden()[0]["fdy/" + case["name"]])


@pytest.mark.parametrize("case", PC.FD_CASES, ids=_ids(PC.FD_CASES))
def test_filter_derivative_prefiltered_on_scipys_y(case):
    par = case["par"]
    y = PO.bessel_filtfilt(PC.fd_build(case), par["cutoff_freq"], par["sampling_freq"])
    got = _from_y(y, par)
    assert np.array_equal(got, PO.filter_derivative_spans_from_y(y, par["low_threshold"], par["high_threshold"]))
    assert np.array_equal(got, PC.golden()[0]["fd/" + case["name"]])


@pytest.mark.parametrize("case", PC.FD_CASES, ids=_ids(PC.FD_CASES))
def test_filter_derivative_full_route_golden(case):
    npz, man = PC.golden()
    if "fd/" + case["name"] in man["below_margin"]:
        pytest.skip("decision margin below 1e-9 * max|current| (manifest_state_parsers.json: below_margin)")
    x = PC.fd_build(case)
    segs = FilterDerivativeSegmenter(**case["par"]).parse(x)
    assert np.array_equal(_spans(segs), npz["fd/" + case["name"]])
    assert all(set(vars(s)) == {"current", "start"} and np.shares_memory(s.current, x) for s in segs)
    # the spans tile what the kept pairs leave: first at 0, last at n
    assert segs[0].start == 0 and segs[-1].start + len(segs[-1].current) == x.size


def test_filter_derivative_batch_equals_lone_runs():
    cases = [c for c in PC.FD_CASES if c["par"]["cutoff_freq"] == 1000. and c["par"]["sampling_freq"] == 1.e5 and
             c["par"]["low_threshold"] == 0.05 and c["par"]["high_threshold"] == 2]
    assert len(cases) >= 5
    p = FilterDerivativeSegmenter(**cases[0]["par"])
    batch = p.parse_batch([PC.fd_build(c) for c in cases] + [torch.from_numpy(PC.fd_build(cases[0])).cuda()])
    for c, segs in zip(cases + [cases[0]], batch):
        assert np.array_equal(_spans(segs), PC.golden()[0]["fd/" + c["name"]]), c["name"]


def test_filter_derivative_prefiltered_batch_with_empty_events():
    cases = PC.FDY_CASES
    ys = [PC.fdy_build(c) for c in cases if c["par"]["low_threshold"] == 1.0 and c["par"]["high_threshold"] == 2]
    ys = ys + [np.zeros(0)] + ys[::-1]
    lens = [y.size for y in ys]
    starts = np.concatenate(([0], np.cumsum(lens)))[:-1]
    par = dict(low_threshold=1.0, high_threshold=2, cutoff_freq=1000., sampling_freq=1.e5)
    spans, off = engine.context(None).filter_derivative_f64(torch.from_numpy(np.concatenate(ys)).cuda(), starts, lens, _params(par, True))
    sp = spans.cpu().numpy()
    for e, y in enumerate(ys):
        assert np.array_equal(sp[off[e]:off[e + 1]], PO.filter_derivative_spans_from_y(y, 1.0, 2)), e


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_capacity_then_retry():
    ctx = engine.context(None)
    x = PC.snake_build(PC.SNAKE_BY_NAME["coarse_long"])
    want = PC.golden()[0]["snake/coarse_long"]
    t = torch.from_numpy(x).cuda()
    with pytest.raises(engine.CapacityError) as err:
        ctx.snakebase_f64(t, [0], [x.size], cap=want.shape[0] - 1)
    assert err.value.required == want.shape[0]
    spans, off = ctx.snakebase_f64(t, [0], [x.size], cap=err.value.required)
    assert np.array_equal(spans.cpu().numpy(), want) and off.tolist() == [0, want.shape[0]]
    case = PC.FDY_BY_NAME["many_pairs_300"]
    y, want = torch.from_numpy(PC.fdy_build(case)).cuda(), PC.golden()[0]["fdy/many_pairs_300"]
    with pytest.raises(engine.CapacityError) as err:
        ctx.filter_derivative_f64(y, [0], [y.numel()], _params(case["par"], True), cap=0)
    assert err.value.required == want.shape[0]
    spans, _ = ctx.filter_derivative_f64(y, [0], [y.numel()], _params(case["par"], True), cap=err.value.required)
    assert np.array_equal(spans.cpu().numpy(), want)
    # a first call that is too small is repeated by the wrapper when no cap is given (a span per 64 samples is the guess)
    case = PC.FDY_BY_NAME["pairs_every_other_sample"]
    y = torch.from_numpy(PC.fdy_build(case)).cuda()
    spans, _ = ctx.filter_derivative_f64(y, [0], [y.numel()], _params(case["par"], True))
    assert np.array_equal(spans.cpu().numpy(), PC.golden()[0]["fdy/pairs_every_other_sample"])


def _raw(fn, t, starts, lens, *mid):
    """A raw call of a C entry with a one-span output: (status, message)."""
    ctx = engine.context(None)
    P64 = ctypes.POINTER(ctypes.c_int64)
    st, ln = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    out, off = torch.zeros(2, dtype=torch.int32, device="cuda"), np.zeros(st.size + 1, dtype=np.int64)
    with ctx.lock:
        rc = fn(ctx.handle, ctypes.c_void_p(t.data_ptr()), st.ctypes.data_as(P64), ln.ctypes.data_as(P64), st.size, *mid,
                ctypes.c_void_p(out.data_ptr()), 1, off.ctypes.data_as(P64))
        msg = ctx.L.ps_last_error(ctx.handle)
    return rc, (msg.decode() if msg else "")


def test_argument_errors():
    L = engine.context(None).L
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    par = dict(low_threshold=1.0, high_threshold=2.0, cutoff_freq=1000., sampling_freq=1.e5)

    def fd(lens, prefiltered=False, **kw):
        return _raw(L.ps_filter_derivative_f64, t, [0] * len(lens), lens, ctypes.byref(_params(dict(par, **kw), prefiltered)))

    for n in (0, 6):
        rc, msg = fd([20, n])
        assert rc == _lib.PS_ERR_ARG and "event 1" in msg and "padlen, which is 6" in msg
    assert fd([7])[0] == _lib.PS_OK and fd([6], prefiltered=True)[0] == _lib.PS_OK
    for kw in (dict(cutoff_freq=0.0), dict(cutoff_freq=-5.0), dict(cutoff_freq=5.e4), dict(cutoff_freq=float("nan")),
               dict(sampling_freq=0.0)):
        rc, msg = fd([20], **kw)
        assert rc == _lib.PS_ERR_ARG and "Nyquist" in msg, kw
    assert fd([20], prefiltered=True, cutoff_freq=0.0)[0] == _lib.PS_OK            # (no filter: the cutoff is not read)
    for kw in (dict(low_threshold=float("nan")), dict(high_threshold=float("nan"))):
        rc, msg = fd([20], **kw)
        assert rc == _lib.PS_ERR_ARG and "NaN" in msg
    for fn, mid in ((L.ps_snakebase_f64, ()), (L.ps_filter_derivative_f64, (ctypes.byref(_params(par, True)),))):
        rc, msg = _raw(fn, t, [0], [(1 << 30) + 1], *mid)
        assert rc == _lib.PS_ERR_ARG and "2^30" in msg
        rc, msg = _raw(fn, t, [0, 0], [10, -1], *mid)
        assert rc == _lib.PS_ERR_ARG and "event 1" in msg and "negative" in msg
        rc, msg = _raw(fn, t, [-1], [10], *mid)
        assert rc == _lib.PS_ERR_ARG and "negative" in msg
    with pytest.raises(ValueError, match="padlen"):
        engine.context(None).filter_derivative_f64(t, [0], [5], _params(par, False))


# ---- the callers ------------------------------------------------------------------------------------------------------------
def _file():
    """A synthetic file: open channel at 110 pA, three blockades (coarse grid: equal neighbours are common)."""
    from pypore_amd import synth
    parts, bounds, at = [], [], 0
    for e, n in enumerate((3000, 5000, 2100)):
        gap = np.full(500, 110.0)
        ev = (synth.random_dwell_counts(n, 400 + e, 150, 600) // 16) * (synth.QUANTUM * 16)
        parts += [gap, np.asarray(ev, dtype=np.float64)]
        bounds.append((at + 500, at + 500 + n))
        at += 500 + n
    return np.concatenate(parts + [np.full(500, 110.0)]), bounds


@pytest.mark.parametrize("make", [lambda: snakebase_parser(), lambda: FilterDerivativeSegmenter(low_threshold=0.05)],
                         ids=["snakebase", "filter_derivative"])
def test_event_parse_and_file_parse_events(make):
    from pypore_amd.parsers import MemoryParse
    x, bounds = _file()
    oracle = (PO.snakebase_spans if isinstance(make(), snakebase_parser) else
              lambda c: PO.filter_derivative_spans(c, low_threshold=0.05))
    f = File(current=x, timestep=0.01)                       # 100 kHz
    f.parse(MemoryParse([a for a, _ in bounds], [b for _, b in bounds]))
    assert len(f.events) == 3
    f.parse_events(parser=make())
    rate = f.second
    for ev, (a, b) in zip(f.events, bounds):
        want = oracle(x[a:b])
        assert want.shape[0] > 1 and type(ev.state_parser) is type(make())
        assert np.array_equal(np.rint([s.start * rate for s in ev.segments]).astype(np.int64), want[:, 0])
        assert [len(s.current) for s in ev.segments] == (want[:, 1] - want[:, 0]).tolist()
        assert all(s.event is ev for s in ev.segments)
    lone = f.events[1]
    batched = [(s.start, len(s.current)) for s in lone.segments]
    lone.parse(parser=make())
    assert [(s.start, len(s.current)) for s in lone.segments] == batched
