"""Near-tie sites per event (ps_get_near_ties, engine.Context.near_tie_sites, engine.consistent_sites, Event.near_ties) and
the per-event exact redo of off_grid="exact_on_near_tie"."""
import ctypes
import os
import re

import numpy as np
import pytest

from pypore_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_BS = os.environ.get("PORESEG_SCAN_BS", "1") != "0"


def _sites(rows):
    return np.array(rows, dtype=engine.NEAR_TIE_DTYPE)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_ps_near_tie_struct_matches_the_header():
    """ps_near_tie of include/poreseg.h: four int32 in the order event, window_start, window_end, split (16 bytes)."""
    from pypore_amd import _lib
    with open(os.path.join(HERE, "..", "include", "poreseg.h")) as f:
        h = f.read()
    m = re.search(r"typedef struct ps_near_tie \{\s*int32_t ([^;]*);", h)
    assert m, "ps_near_tie not declared"
    assert [s.strip() for s in m.group(1).split(",")] == ["event", "window_start", "window_end", "split"]
    assert ctypes.sizeof(_lib.NearTie) == 16
    assert [f[0] for f in _lib.NearTie._fields_] == ["event", "window_start", "window_end", "split"]
    assert engine.NEAR_TIE_DTYPE.itemsize == 16 and list(engine.NEAR_TIE_DTYPE.names) == [f[0] for f in _lib.NearTie._fields_]
    assert "ps_get_near_ties" in _lib.EXPORTS
    assert re.search(r"#define PS_NT_NOT_COUNTED\s+-1", h) and re.search(r"#define PS_NT_INCOMPLETE\s+-2", h)


def test_filter_keeps_the_windows_of_the_final_recursion():
    # one event of 30 000 samples, W = 10 000, boundaries 12 000 and 20 000:
    # rec(0, 30000) scans [0, 10000) (no split), [5000, 15000) -> 12000; rec(0, 12000): [0, 10000), [5000, 12000) ...
    W, n, b = 10000, 30000, [12000, 20000]
    sites = _sites([(0, 5000, 15000, 12000), (0, 0, 10000, -1), (0, 5000, 12000, -1), (0, 12000, 22000, 20000),
                    (0, 20000, 30000, -1)])
    got = engine.consistent_sites(sites, np.array(b), np.array([0, 2]), [n], W)
    assert got.tolist() == sites.tolist()


def test_filter_drops_tile_starts_and_splits_that_are_not_boundaries():
    W, n, b = 10000, 100000, [12000, 20000]
    sites = _sites([(0, 41000, 51000, -1),          # a tile's spine from 41 000: not on the grid of any range start
                    (0, 43000, 53000, 45000),        # ... nor this one
                    (0, 5000, 15000, 13000),         # window of the recursion, but its split is not a returned boundary
                    (0, 5000, 14000, -1),            # ends neither at start + W nor at a boundary
                    (0, 25000, 35000, -1)])          # 25 000 = 20 000 + W / 2: kept
    got = engine.consistent_sites(sites, np.array(b), np.array([0, 2]), [n], W)
    assert got.tolist() == [(0, 25000, 35000, -1)]


def test_filter_short_events_and_forced_splits():
    # n < W: the one window is [0, n)
    got = engine.consistent_sites(_sites([(0, 0, 700, 300), (0, 0, 700, -1), (0, 0, 10000, -1)]), np.array([300]),
                                  np.array([0, 1]), [700], 10000)
    assert got.tolist() == [(0, 0, 700, 300), (0, 0, 700, -1)]
    # max_width forced split at 3000 (no split found in [0, 3000 + ...)): the right range starts at the forced boundary
    W, n, b = 1000, 7000, [3000]
    sites = _sites([(0, 3000, 4000, -1), (0, 3500, 4500, -1), (0, 6500, 7000, -1), (0, 2500, 3000, -1), (0, 3200, 4200, -1)])
    got = engine.consistent_sites(sites, np.array(b), np.array([0, 1]), [n], W)
    assert got.tolist() == [(0, 3000, 4000, -1), (0, 3500, 4500, -1), (0, 6500, 7000, -1), (0, 2500, 3000, -1)]
    # several events: each is filtered against its own boundaries
    got = engine.consistent_sites(_sites([(0, 0, 500, 200), (1, 0, 500, 200), (1, 0, 500, 250)]), np.array([200, 250]),
                                  np.array([0, 1, 2]), [500, 500], 1000)
    assert got.tolist() == [(0, 0, 500, 200), (1, 0, 500, 250)]
    assert engine.consistent_sites(None, np.array([]), np.array([0]), [], 1000) is None


def test_redo_selection():
    assert engine.events_to_redo(_sites([(5, 0, 700, 300), (5, 100, 700, -1), (2, 0, 10, -1)]), 8) == [2, 5]
    assert engine.events_to_redo(_sites([]), 8) == []
    assert engine.events_to_redo(None, 3) == [0, 1, 2]


def test_redo_selection_and_warning_flag_in_parse_filtered_batch_with_a_stub_context(monkeypatch):
    """parse_filtered_batch sends only the flagged events to the exact route; None sends the whole group; the
    NEAR_TIE_WARNING switch plays no part; the fast call it acts on is made with segment_batch(near_tie_warning=False)."""
    import torch
    from pypore_amd import cparsers
    from pypore_amd.grid import Deferred
    lens = [900, 700, 800]
    currents = [np.full(n, 100.0 + 0.125 * k) for k, n in enumerate(lens)]

    class Ctx:
        def __init__(self, sites):
            self.sites, self.exact, self.warn = sites, [], []

        def filter_bessel(self, t, q, cutoff, sampling_freq, order):
            return t.double() * q

        def requantise(self, y):
            return y.float(), 0.0, 1.0

        def segment_batch(self, samples, ev_off, params, step, want_stats=False, offset_counts=0, near_tie_warning=True):
            self.warn.append(near_tie_warning)
            n_ev = len(ev_off) - 1
            return torch.tensor([300] * n_ev, dtype=torch.int32), np.arange(n_ev + 1, dtype=np.int64), None

        def near_tie_sites(self):
            return self.sites

        def segment_exact_f64(self, allt, starts, lens_, params):
            self.exact.append(len(lens_))
            return torch.tensor([100] * len(lens_), dtype=torch.int32), np.arange(len(lens_) + 1, dtype=np.int64)

    class Stream:
        tensor, offset = None, 0.0

    def to_device(cur, quantum, offset, device):
        s = Stream()
        s.tensor, s.quantum, s.offset = torch.from_numpy(np.asarray(cur)), 1.0, 0.0
        return s

    monkeypatch.setattr(cparsers.engine, "to_device", to_device)
    monkeypatch.setattr(cparsers, "segments_from_edges", lambda cur, edges: edges)
    class Filtered:
        def __init__(self, y, off):
            self.tensor, self.offset = y, off

    monkeypatch.setattr(Deferred, "from_tensor", staticmethod(Filtered))
    fs = cparsers.FastStatSplit(min_width=50, window_width=1000, off_grid="exact_on_near_tie")
    for warn in (True, False):
        monkeypatch.setattr(engine, "NEAR_TIE_WARNING", warn)
        for sites, n_exact, firsts in ((_sites([(1, 0, 700, 300)]), [1], [300, 100, 300]),
                                       (None, [3], [100, 100, 100]),
                                       (_sites([]), [], [300, 300, 300])):
            c = Ctx(sites)
            monkeypatch.setattr(cparsers.engine, "context", lambda device=None, c=c: c)
            nt = []
            out = fs.parse_filtered_batch(currents, near_ties_out=nt)
            assert c.exact == n_exact
            assert c.warn == [False]                   # (the result is acted upon: no NearTieWarning from the fast call)
            assert [edges[1] for _, edges in out] == firsts
            if sites is None:
                assert nt == [None] * 3
            else:
                assert nt == [[(0, 700, 300)] if e in sites["event"].tolist() else [] for e in range(3)]


class _StubCtx:
    """A context that records the calls the policy makes: segment_batch returns one boundary at 300, the exact route one at
    100 per event."""
    device = 0

    def __init__(self, sites):
        self.sites, self.calls = sites, []

    def requantise(self, y):
        self.calls.append(("requantise", int(y.numel())))
        return y.float(), 0.0, 1.0

    def segment_batch(self, samples, ev_off, params, q, want_stats=True, offset_counts=0, near_tie_warning=True):
        import torch
        n_ev = len(ev_off) - 1
        self.calls.append(("batch", n_ev, near_tie_warning))
        stats = torch.zeros((2 * n_ev, 4), dtype=torch.float64) if want_stats else None
        return torch.tensor([300] * n_ev, dtype=torch.int32), np.arange(n_ev + 1, dtype=np.int64), stats

    def near_tie_sites(self):
        self.calls.append(("sites",))
        return self.sites

    def segment_exact_f64(self, allt, starts, lens, params):
        import torch
        self.calls.append(("exact", [int(n) for n in lens]))
        return torch.tensor([100] * len(lens), dtype=torch.int32), np.arange(len(lens) + 1, dtype=np.int64)


def _use(monkeypatch, c):
    from pypore_amd import cparsers
    monkeypatch.setattr(cparsers.engine, "context", lambda device=None: c)


def test_parse_batch_with_exact_from_under_every_mode(monkeypatch):
    """parse_batch(rounded, levels, exact_from=...): the off_grid policy applies to events the caller rounded itself --
    which calls it makes, with which warning flag, on which events, and the sites it reports."""
    import torch
    import warnings
    from pypore_amd import cparsers
    lens = [900, 700, 800]
    rounded = [np.full(n, 100.0 + 0.125 * k) for k, n in enumerate(lens)]
    exact_from = [torch.from_numpy(r + 1e-7) for r in rounded]

    class Samples:
        offset = 0.0

    def to_device(cur, quantum, offset, device, full_detect=False):
        s = Samples()
        s.tensor, s.quantum = torch.from_numpy(np.asarray(cur, dtype=np.float32)), 0.125
        return s

    monkeypatch.setattr(cparsers.engine, "to_device", to_device)
    one = _sites([(1, 0, 700, 300)])
    fast_sites = [[], [(0, 700, 300)], []]
    expect = {   # mode -> (calls, first boundary per event, near_ties)
        "raise": ([("batch", 3, True), ("sites",)], [300, 300, 300], fast_sites),
        "requantise": ([("batch", 3, True), ("sites",)], [300, 300, 300], fast_sites),
        "exact": ([("exact", lens)], [100, 100, 100], [None] * 3),
        "exact_on_near_tie": ([("batch", 3, False), ("sites",), ("exact", [700])], [300, 100, 300], fast_sites),
    }
    for mode, (calls, firsts, near) in expect.items():
        c = _StubCtx(one)
        _use(monkeypatch, c)
        nt = []
        before, saved = warnings.filters, list(warnings.filters)
        out = cparsers.FastStatSplit(min_width=50, window_width=1000, off_grid=mode).parse_batch(
            rounded, [100.0] * 3, near_ties_out=nt, exact_from=exact_from)
        assert warnings.filters is before and warnings.filters == saved
        assert c.calls == calls, mode
        assert [segs[1].start for segs in out] == firsts, mode
        assert nt == near, mode
        assert all(segs[0].current.base is r or segs[0].current is r or np.shares_memory(segs[0].current, r)
                   for segs, r in zip(out, rounded))
    # sites not counted: the whole call goes to the exact route
    c = _StubCtx(None)
    _use(monkeypatch, c)
    nt = []
    out = cparsers.FastStatSplit(min_width=50, window_width=1000, off_grid="exact_on_near_tie").parse_batch(
        rounded, [100.0] * 3, near_ties_out=nt, exact_from=exact_from)
    assert c.calls == [("batch", 3, False), ("sites",), ("exact", lens)]
    assert [segs[1].start for segs in out] == [100] * 3 and nt == [None] * 3
    # without exact_from, input on a grid is segmented as it is, whatever the mode: warning on, no redo, no sites unasked
    c = _StubCtx(None)
    _use(monkeypatch, c)
    out = cparsers.FastStatSplit(min_width=50, window_width=1000, off_grid="exact_on_near_tie").parse_batch(rounded)
    assert c.calls == [("batch", 3, True)] and [segs[1].start for segs in out] == [300] * 3


def test_off_grid_parse_batch_route_under_exact_on_near_tie(monkeypatch):
    """Float input on no grid: the device requantises it, one fast call without the warning, the sites, and the exact
    route only when a site was logged or the sites were not counted.  The sites are reported (Event.near_ties); the
    segments are views of the caller's array."""
    import torch
    import warnings
    from pypore_amd import cparsers

    def off_grid(*a, **kw):
        raise ValueError("no grid")

    monkeypatch.setattr(cparsers.engine, "to_device", off_grid)
    cpu = torch.device("cpu")
    monkeypatch.setattr(torch, "device", lambda *a, **kw: cpu)      # (no GPU here: the stub takes host tensors)
    x = 100.0 + np.random.default_rng(3).normal(size=900)
    fs = cparsers.FastStatSplit(min_width=50, window_width=1000, device=0, off_grid="exact_on_near_tie")
    for sites, exact, first, near in ((None, [("exact", [900])], 100, None),
                                      (_sites([]), [], 300, []),
                                      (_sites([(0, 0, 900, 300)]), [("exact", [900])], 100, [(0, 900, 300)])):
        c = _StubCtx(sites)
        _use(monkeypatch, c)
        nt = []
        before, saved = warnings.filters, list(warnings.filters)
        segs = fs.parse_batch([x], near_ties_out=nt)[0]
        assert warnings.filters is before and warnings.filters == saved
        assert c.calls == [("requantise", 900), ("batch", 1, False), ("sites",)] + exact
        assert segs[1].start == first and nt == [near]
        assert np.shares_memory(segs[0].current, x)
    # "requantise": the warning stays on, and nobody asked for the sites
    c = _StubCtx(_sites([(0, 0, 900, 300)]))
    _use(monkeypatch, c)
    cparsers.FastStatSplit(min_width=50, window_width=1000, device=0, off_grid="requantise").parse(x)
    assert c.calls == [("requantise", 900), ("batch", 1, True)]


def _filtered_events(amplitudes):
    from pypore_amd.DataTypes import Event, File
    rng = np.random.default_rng(5)
    xs = [60.0 + a * np.sin(np.linspace(0, 9, 1500 + 100 * k)) + rng.normal(0, 0.01, 1500 + 100 * k)
          for k, a in enumerate(amplitudes)]
    f = File(current=np.concatenate(xs), timestep=0.01)
    f.events = []
    for x in xs:
        ev = Event(current=x, start=0., end=len(x) / f.second, duration=len(x) / f.second, second=f.second, file=f)
        ev.filtered = True
        f.events.append(ev)
    return f


@pytest.mark.parametrize("mode", ["raise", "requantise", "exact", "exact_on_near_tie"])
def test_event_and_file_segment_filtered_events_through_the_same_calls(monkeypatch, mode):
    """Event._parse_filtered and File._parse_events share one helper: for the same filtered events they make the same
    parse_batch calls (rounded currents, their levels, the unrounded currents for the exact route) -- one per grid step
    -- and, when the policy makes no fast call, one exact call with the unrounded currents.  No warning filter is touched."""
    import warnings
    from pypore_amd import cparsers
    from pypore_amd.core import Segment
    from pypore_amd.parsers import SpeedyStatSplit
    log = []

    class Spy(SpeedyStatSplit):
        def parse_batch(self, currents, levels=None, near_ties_out=None, exact_from=None):
            if len(currents):
                log.append(("parse_batch", [len(c) for c in currents], [float(v) for v in levels],
                            [np.asarray(x).tolist() for x in exact_from]))
            if near_ties_out is not None:
                near_ties_out[:] = [[(0, len(c), 40)] for c in currents]
            return [[Segment(current=c[:40], start=0, duration=40, end=40),
                     Segment(current=c[40:], start=40, duration=len(c) - 40, end=len(c))] for c in currents]

    def exact(self, currents):
        log.append(("exact", [np.asarray(x).tolist() for x in currents]))
        return [[Segment(current=c, start=0, duration=len(c), end=len(c))] for c in currents]

    monkeypatch.setattr(cparsers.FastStatSplit, "parse_exact_batch", exact)
    f = _filtered_events([2.0, 2.0, 30.0])                          # two grid steps
    steps = {ev._on_fine_grid()[1] for ev in f.events}
    assert len(steps) == 2
    parser = Spy(min_width=20, window_width=200, off_grid=mode)
    before, saved = warnings.filters, list(warnings.filters)
    one_by_one = []
    for ev in f.events:
        log.clear()
        segs = ev._parse_filtered(parser)
        one_by_one.append(list(log))
        assert all(np.shares_memory(s.current, ev.current) for s in segs)
    log.clear()
    f._parse_events(parser, None)
    whole = list(log)
    assert warnings.filters is before and warnings.filters == saved
    values = [np.asarray(ev.current, dtype=np.float64).tolist() for ev in f.events]
    if mode == "exact":
        assert one_by_one == [[("exact", [v])] for v in values]
        assert whole == [("exact", values)]                           # one call for the file
        assert all(ev.near_ties is None for ev in f.events)
        return
    for ev, calls in zip(f.events, one_by_one):
        rounded, _, centre = ev._on_fine_grid()
        assert calls == [("parse_batch", [len(rounded)], [centre], [np.asarray(ev.current).tolist()])]
    assert len(whole) == 2                                           # one per grid step, same events, same arguments
    assert sorted(k for _, lens, _, _ in whole for k in lens) == sorted(len(v) for v in values)
    merged = {}
    for _, lens, levels, ex in whole:
        for n, level, e in zip(lens, levels, ex):
            merged[tuple(e)] = (n, level)
    for calls in one_by_one:
        _, (n,), (level,), (e,) = calls[0]
        assert merged[tuple(e)] == (n, level)
    for ev in f.events:
        assert ev.near_ties == [(0, len(ev.current), 40)]
        assert [s.start * f.second for s in ev.segments] == [0, 40]
        assert all(np.shares_memory(s.current, ev.current) for s in ev.segments)


# ---- GPU ------------------------------------------------------------------------------------------------------------

def _tie_case():
    from golden_util import offgrid_cases
    (case,) = offgrid_cases("tie")
    return case


@pytest.mark.gpu
def test_palindrome_tie_site_and_log_reset():
    import oracle
    from pypore_amd import synth
    from pypore_amd.parsers import SpeedyStatSplit
    case = _tie_case()
    a, n = case["gen"]["a"], case["gen"]["n"]
    x = synth.counts_to_pa(synth.palindrome_counts(**case["gen"]), np.float64)
    p = SpeedyStatSplit(quantum=synth.QUANTUM, **case["params"])
    segs = p.parse(x)
    ctx = engine.context()
    got = np.array([s_.start for s_ in segs[1:]], dtype=np.int64)
    np.testing.assert_array_equal(got, oracle.parse(x, **case["params"]))
    raw = ctx.near_tie_sites()
    if not SCAN_BS:
        assert raw is None
        return
    sites = engine.consistent_sites(raw, got, np.array([0, got.size]), [n], case["params"].get("window_width", 10000))
    assert len(sites) >= 1 and ctx.near_ties() >= len(sites)
    hit = [s for s in sites.tolist() if s[3] == a]
    assert hit, sites
    _, ws, we, _ = hit[0]
    assert ws <= a and n - a < we                      # the window holds both steps
    _, g = oracle.score_window(x[ws:we], case["params"]["min_width"])
    assert g[a - ws] == g[n - a - ws]                 # the reference's own gains: the two steps tie
    assert p.parse(synth.config1()) is not None
    empty = ctx.near_tie_sites()
    assert empty is not None and len(empty) == 0      # the log is reset by the next call


@pytest.mark.gpu
def test_tie_inside_a_batch_is_attributed_to_its_event():
    import oracle
    from pypore_amd import synth
    from pypore_amd.parsers import SpeedyStatSplit
    case = _tie_case()
    W = case["params"].get("window_width", 10000)
    tie = synth.counts_to_pa(synth.palindrome_counts(**case["gen"]), np.float64)
    ev = [synth.counts_to_pa(synth.random_dwell_counts(6000 + 500 * k, 100 + k), np.float64) for k in range(8)]
    ev[5] = tie
    p = SpeedyStatSplit(quantum=synth.QUANTUM, **case["params"])
    segs = p.parse_batch(ev)
    ctx = engine.context()
    raw = ctx.near_tie_sites()
    b = [np.array([s_.start for s_ in sg[1:]], dtype=np.int64) for sg in segs]
    for k in range(8):
        np.testing.assert_array_equal(b[k], oracle.parse(ev[k], **case["params"]))
    if not SCAN_BS:
        assert raw is None
        return
    boff = np.concatenate(([0], np.cumsum([x.size for x in b])))
    sites = engine.consistent_sites(raw, np.concatenate(b), boff, [x.size for x in ev], W)
    assert set(sites["event"].tolist()) == {5}
    p.parse(tie)
    alone = engine.consistent_sites(ctx.near_tie_sites(), b[5], np.array([0, b[5].size]), [tie.size], W)
    assert sorted(map(tuple, sites[["window_start", "window_end", "split"]].tolist())) == \
        sorted(map(tuple, alone[["window_start", "window_end", "split"]].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("single_pass", [1, 0])
def test_single_pass_route_attributes_the_site_to_the_detected_event(single_pass):
    import torch
    import oracle
    from pypore_amd import _lib, synth
    case = _tie_case()
    a, n = case["gen"]["a"], case["gen"]["n"]
    tie = synth.palindrome_counts(**case["gen"])                 # counts around LEVEL_COUNTS (below the threshold)
    gap = np.full(5003, int(np.max(tie)) + 4000, dtype=np.int32)  # open pore, well above
    trace = np.concatenate((gap, tie, gap)).astype(np.int16)
    thr = float((int(np.max(tie)) + 2000) * synth.QUANTUM)
    ctx = engine.context()
    ctx.set_option("single_pass", single_pass)
    try:
        params = _lib.split_params(**case["params"])
        st, ln, bounds, boff, _ = ctx.detect_segment_trace(torch.from_numpy(trace).cuda(), synth.QUANTUM, params,
                                                             threshold=thr, min_duration=1000)
        assert st.tolist() == [gap.size] and ln.tolist() == [n]
        b = bounds.cpu().numpy()
        x = synth.counts_to_pa(tie, np.float64)
        np.testing.assert_array_equal(b, oracle.parse(x, **case["params"]))
        raw = ctx.near_tie_sites()
        if not SCAN_BS:
            assert raw is None
            return
        sites = engine.consistent_sites(raw, b, boff, ln, case["params"].get("window_width", 10000))
        assert set(sites["event"].tolist()) == {0}
        assert any(s[3] == a and s[1] <= a and n - a < s[2] for s in sites.tolist()), sites
    finally:
        ctx.set_option("single_pass", 1)


@pytest.mark.gpu
def test_overflow_and_not_counted():
    import oracle
    from pypore_amd import synth
    from pypore_amd.parsers import SpeedyStatSplit
    case = _tie_case()
    tie = synth.counts_to_pa(synth.palindrome_counts(**case["gen"]), np.float64)
    ctx = engine.context()
    p = SpeedyStatSplit(quantum=synth.QUANTUM, **case["params"])
    if SCAN_BS:
        p.parse_batch([tie, tie, tie])
        assert ctx.near_ties() >= 2
        assert len(ctx.near_tie_sites()) >= 2
        ctx.set_option("near_tie_log", 1)
        try:
            p.parse_batch([tie, tie, tie])
            assert ctx.near_ties() >= 2 and ctx.near_tie_sites() is None        # incomplete: counted on, stored one
        finally:
            ctx.set_option("near_tie_log", 65536)
        ctx.set_option("near_tie_log", 0)
        try:
            p.parse(tie)
            assert ctx.near_tie_sites() is None                                  # off: not counted
        finally:
            ctx.set_option("near_tie_log", 65536)
    params = dict(case["params"], min_width=4)
    segs = SpeedyStatSplit(quantum=synth.QUANTUM, **params).parse(tie)
    np.testing.assert_array_equal([s_.start for s_ in segs[1:]], oracle.parse(tie, **params))
    assert ctx.near_tie_sites() is None                                          # LDS-window kernels: not counted


@pytest.mark.gpu
def test_site_of_a_window_that_starts_inside_the_event():
    """The tie window starts past sample 0 (a first step at L0 is found first, then rec(L0, n) scans the palindrome as one
    window): window and split come back as indices of the event."""
    import oracle
    from pypore_amd import synth
    from pypore_amd.parsers import SpeedyStatSplit
    case = _tie_case()
    a, npal = case["gen"]["a"], case["gen"]["n"]
    L0 = 3000
    head = (synth.LEVEL_COUNTS[0] - 1200) + synth.noise_counts(77, 0, L0)
    x = synth.counts_to_pa(np.concatenate((head, synth.palindrome_counts(**case["gen"]))), np.float64)
    ref = oracle.parse(x, **case["params"])
    assert list(ref) == [L0, L0 + a, L0 + npal - a]
    segs = SpeedyStatSplit(quantum=synth.QUANTUM, **case["params"]).parse(x)
    got = np.array([s_.start for s_ in segs[1:]], dtype=np.int64)
    np.testing.assert_array_equal(got, ref)
    raw = engine.context().near_tie_sites()
    if not SCAN_BS:
        assert raw is None
        return
    sites = engine.consistent_sites(raw, got, np.array([0, got.size]), [x.size], case["params"].get("window_width", 10000))
    assert (0, L0, L0 + npal, L0 + a) in sites.tolist(), raw
    for _, ws, we, sp in raw.tolist():
        assert sp == -1 or ws < sp < we


@pytest.mark.gpu
def test_filtered_golden_sample_sites():
    """The 52 filtered events of the golden sample segmented without cutoff_freq: filtered on the device and
    re-quantised as Event.parse does, then segmented by grid step in one call per step at the group's largest level.  Every
    record lies in its event; every event the reference differs on (KNOWN_DIFFERING) has a site; each event's sites equal
    those it has alone at the same level."""
    import torch
    from pypore_amd import cparsers
    from pypore_amd.DataTypes import Event, File
    from test_parity_sample import KNOWN_DIFFERING, MAN, SECOND, _event_current, _seg_params
    from pypore_amd import _lib
    cases = [c for c in MAN["cases"] if c["op"] == "filtered" and not c.get("seg_cutoff")]
    assert len(cases) == 52
    params = _lib.split_params(**_seg_params(cases[0]))
    W = params.window_width
    ctx = engine.context()
    by_step = {}
    for c in cases:
        assert _seg_params(c) == _seg_params(cases[0])
        x = _event_current(c)
        ev = Event(current=x, start=0., end=len(x) / SECOND, duration=len(x) / SECOND, second=SECOND,
                   file=File(current=x, timestep=1000. / SECOND))
        ev.filter(order=c["order"], cutoff=c["cutoff"])
        rounded, step, centre = ev._on_fine_grid()
        by_step.setdefault(step, []).append((c["name"], torch.from_numpy(rounded.astype(np.float32)).cuda(), centre))
    flagged, logged = set(), set()
    for step, group in by_step.items():
        dc = cparsers._dc_counts(max((g[2] for g in group), key=abs), step)
        lens = np.array([g[1].numel() for g in group], dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(lens)))
        bounds, boff, _ = ctx.segment_batch(torch.cat([g[1] for g in group]), off, params, step, want_stats=False, offset_counts=dc)
        b = bounds.cpu().numpy()
        raw = ctx.near_tie_sites()
        if not SCAN_BS:
            assert raw is None
            return
        for e, ws, we, sp in raw.tolist():
            assert 0 <= ws < we <= lens[e] and we - ws <= W and (sp == -1 or ws < sp < we), (e, ws, we, sp)
        sites = engine.consistent_sites(raw, b, boff, lens, W)
        logged |= {group[e][0] for e in raw["event"].tolist()}
        for e, (name, t, _) in enumerate(group):
            mine = sorted(map(tuple, sites[sites["event"] == e][["window_start", "window_end", "split"]].tolist()))
            if mine:
                flagged.add(name)
            bb, bo, _ = ctx.segment_batch(t, np.array([0, t.numel()]), params, step, want_stats=False, offset_counts=dc)
            np.testing.assert_array_equal(bb.cpu().numpy(), b[boff[e]:boff[e + 1]])
            alone = engine.consistent_sites(ctx.near_tie_sites(), bb.cpu().numpy(), bo, [t.numel()], W)
            assert sorted(map(tuple, alone[["window_start", "window_end", "split"]].tolist())) == mine, name
    assert KNOWN_DIFFERING["filtered"] <= logged
    assert KNOWN_DIFFERING["filtered"] <= flagged, sorted(KNOWN_DIFFERING["filtered"] - flagged)


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff", [None, 2000.])
def test_exact_redo_is_per_event(tmp_path, monkeypatch, cutoff):
    """Experiment.parse with off_grid="exact_on_near_tie": every event equals the oracle on its filtered current, and only
    events with sites (all of a group whose sites are not counted) go to the exact route -- with or without the warning."""
    import oracle
    from pypore_amd import abf, synth
    from pypore_amd.DataTypes import Experiment
    from pypore_amd.parsers import SpeedyStatSplit
    counts, _ = synth.file_trace_counts(1_200_000, 52)
    path = str(tmp_path / "t.abf")
    abf.write_abf(path, counts.astype(np.int16), adc_range=10.0, adc_resolution=32768, instrument_scale=0.0005,
                  signal_gain=20.0, instrument_offset=1.25, signal_offset=0.5)
    sent, trail = [], []
    orig_exact, orig_batch, orig_sites = engine.Context.segment_exact_f64, engine.Context.segment_batch, engine.Context.near_tie_sites

    def spy(self, current, ev_start, ev_len, params):
        sent.append(len(ev_start))
        trail.append(("exact", len(ev_start)))
        return orig_exact(self, current, ev_start, ev_len, params)

    def spy_batch(self, samples, ev_off, *a, **kw):
        trail.append(("batch", len(ev_off) - 1))
        return orig_batch(self, samples, ev_off, *a, **kw)

    def spy_sites(self):
        r = orig_sites(self)
        trail.append(("sites", r))
        return r

    monkeypatch.setattr(engine.Context, "segment_exact_f64", spy)
    monkeypatch.setattr(engine.Context, "segment_batch", spy_batch)
    monkeypatch.setattr(engine.Context, "near_tie_sites", spy_sites)
    for warn in (True, False):
        monkeypatch.setattr(engine, "NEAR_TIE_WARNING", warn)
        sent.clear()
        trail.clear()
        kw = dict(prior_segments_per_second=10.) if cutoff is None else dict(prior_segments_per_second=10., cutoff_freq=cutoff)
        seg = SpeedyStatSplit(off_grid="exact_on_near_tie", **kw)
        e = Experiment([path])
        e.parse(segmenter=seg, verbose=False)
        events = [ev for f in e.files for ev in f.events]
        assert events
        for ev in events:
            ref = oracle.parse(np.asarray(ev.current, dtype=np.float64), **kw)
            got = [int(round(s_.start * e.files[0].second)) for s_ in ev.segments[1:]]
            np.testing.assert_array_equal(got, ref)
        # after every fast call: exactly the events with a record went to the exact route (the whole group when not counted)
        checked = 0
        for k, (kind, v) in enumerate(trail):
            if kind != "sites" or k == 0 or trail[k - 1][0] != "batch":
                continue
            n_ev = trail[k - 1][1]
            want = n_ev if v is None else len(set(v["event"].tolist()))
            nxt = trail[k + 1] if k + 1 < len(trail) and trail[k + 1][0] == "exact" else ("exact", 0)
            assert nxt[1] == want, (n_ev, v)
            checked += 1
        assert checked >= 1
        if SCAN_BS:
            assert all(ev.near_ties is not None for ev in events)
            if cutoff is not None:
                assert sum(sent) < len(events)         # per event: not every group went whole
        e.delete()
