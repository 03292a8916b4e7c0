"""HMM-guided segmentation of a whole file in one go: File.parse_events(parser, hmm=model) against the per-event route,
`event.parse(parser, hmm=model)` in a loop, on a second copy of the same file.

The file is synthetic: int16 counts behind a current that has not been written out (grid.Deferred.from_counts, what File(filename)
holds), six events of at most 4 000 samples -- dwells of 300 .. 480 samples at four levels 10 pA apart with 0.75 pA of noise,
one event of a single level, one with a dwell at 20 pA that a model of uniform states cannot emit.  The model has four levels, a
silent state, and two states that share a name.  Boundaries, starts and hidden states are compared with ==; the statistics of
the merged segments come from ps_range_stats on the batched route and from numpy on the float64 current in the loop, and are
compared within the 1e-5 relative the suite applies to device segment statistics against numpy everywhere."""
import numpy as np
import pytest

from pypore_amd import synth
from pypore_amd.core import raw_current
from pypore_amd.DataTypes import File
from pypore_amd.hmm import Model, MultivariateDistribution, NormalDistribution, State, UniformDistribution
from pypore_amd.parsers import SpeedyStatSplit, lambda_event_parser

pytestmark = pytest.mark.gpu

Q = synth.QUANTUM
OFFSET = 0.5                                             # pA at count 0: the device statistics are those of count * quantum
LEVELS = (1280, 1600, 1920, 2240)                        # 40, 50, 60, 70 pA
DEEP = 640                                               # 20 pA: outside every state of uniform_model()
EVENTS = ([0, 1, 2, 3, 1, 0, 2], [3, 1, 2, 0, 3], [1], [0, 2, 0, 2, 0, 2, 0, 2], [2, 1, 3], [0, DEEP, 3, 1])
SINGLE, IMPOSSIBLE = 2, 5
RTOL = 1e-5

_CACHE = {}


def trace_counts():
    if "counts" not in _CACHE:
        rng = np.random.default_rng(20241021)
        parts = [np.full(1500, synth.OPEN_COUNTS)]
        for ev in EVENTS:
            for lv in ev:
                parts.append(np.full(int(rng.integers(300, 481)), lv if lv >= 100 else LEVELS[lv]))
            parts.append(np.full(1500, synth.OPEN_COUNTS))
        k = np.concatenate(parts)
        k = k + np.rint(rng.normal(0.0, 24.0, k.size)).astype(np.int64)
        _CACHE["counts"] = k.astype(np.int16)
    return _CACHE["counts"]


def new_file():
    """The file with its six events detected, its current still unwritten."""
    from pypore_amd.grid import Deferred
    f = File(current=Deferred.from_counts(trace_counts(), Q, OFFSET), timestep=0.01)
    detector = lambda_event_parser(threshold=90)
    detector.MIN_DURATION = 200
    f.parse(detector)
    assert f.n == len(EVENTS) and max(len(raw_current(ev)) for ev in f.events) <= 4000
    return f


def segmenter():
    return SpeedyStatSplit(min_width=50, max_width=100000, window_width=600, prior_segments_per_second=100., sampling_freq=1.e5)


def _wire(m, emit, silent):
    for s in emit:
        m.add_transition(m.start, s, 1.0)
        for t in emit:
            m.add_transition(s, t, 0.6 if s is t else 0.1)
        m.add_transition(s, silent, 0.05)
        m.add_transition(s, m.end, 0.05)
    m.add_transition(silent, emit[0], 0.5)
    m.add_transition(silent, emit[-1], 0.5)
    m.bake()
    return m


def level_model():
    """Four levels; the two middle ones share the name "mid"; a silent state between any level and the outer two."""
    m = Model("levels")
    emit = [State(NormalDistribution(lv * Q + OFFSET, 3.0), name) for lv, name in zip(LEVELS, ("low", "mid", "mid", "high"))]
    return _wire(m, emit, State(None, "quiet"))


def uniform_model():
    m = Model("uniform levels")
    emit = [State(UniformDistribution(lv * Q + OFFSET - 5.0, lv * Q + OFFSET + 5.0), name)
            for lv, name in zip(LEVELS, ("low", "mid", "mid", "high"))]
    return _wire(m, emit, State(None, "quiet"))


def vector_model():
    m = Model("vector levels")
    emit = [State(MultivariateDistribution([NormalDistribution(lv * Q + OFFSET, 3.0), UniformDistribution(0.0, 50.0),
                                            UniformDistribution(0.0, 1.0)]), name)
            for lv, name in zip(LEVELS, ("low", "mid", "mid", "high"))]
    return _wire(m, emit, State(None, "quiet"))


def compare(batched, looped, exact_stats):
    """Event by event: count, start, duration, hidden_state with ==; the statistics with == or within RTOL.  Returns the
    largest relative error seen."""
    worst = 0.0
    assert batched.n == looped.n
    for ev_a, ev_b in zip(batched.events, looped.events):
        assert len(ev_a.segments) == len(ev_b.segments)
        for sa, sb in zip(ev_a.segments, ev_b.segments):
            assert sa.start == sb.start and sa.n == sb.n and sa.hidden_state == sb.hidden_state
            assert getattr(sa, "duration", None) == getattr(sb, "duration", None)
            assert sa.event is ev_a and sa.second == sb.second
            for name in ("mean", "std", "min", "max"):
                a, b = float(getattr(sa, name)), float(getattr(sb, name))
                if exact_stats:
                    assert a == b, (name, a, b)
                else:
                    err = abs(a - b) / max(abs(b), 1e-300)
                    worst = max(worst, err)
                    assert err <= RTOL, (name, a, b)
    return worst


def test_parse_events_with_hmm_equals_the_loop():
    from pypore_amd.grid import Deferred
    model = level_model()
    fa, fb = new_file(), new_file()
    fa.parse_events(segmenter(), hmm=model)
    for ev in fb.events:
        ev.parse(segmenter(), hmm=model)
    worst = compare(fa, fb, exact_stats=False)
    print("largest relative error of a merged segment's device statistics against numpy: %.3g" % worst)
    assert sum(ev.n for ev in fa.events) >= 8 and len({s.hidden_state for ev in fa.events for s in ev.segments}) >= 3
    # the event of a single level has one segment and ends with none
    assert fa.events[SINGLE].segments == [] and fb.events[SINGLE].segments == []
    # the batched route never wrote the file's float64 current out; its merged segments hold deferred stretches and device rows
    assert isinstance(raw_current(fa), Deferred) and not raw_current(fa).built
    for ev in fa.events:
        assert isinstance(raw_current(ev), Deferred) and not raw_current(ev).built
        for seg in ev.segments:
            assert isinstance(raw_current(seg), Deferred) and "_gpu_stats" in seg.__dict__
    assert raw_current(fb).built
    # a stretch built later holds the samples the statistics were taken of
    seg = fa.events[0].segments[0]
    assert seg.mean == pytest.approx(float(np.mean(np.asarray(seg.current))), rel=RTOL)


def test_filtered_events_merge_as_in_the_loop():
    model = level_model()
    fa, fb = new_file(), new_file()
    fa.parse_events(segmenter(), filter_params=(1, 2000.), hmm=model)
    for ev in fb.events:
        ev.filter(1, 2000.)
        ev.parse(segmenter(), hmm=model)
    assert all(ev.filtered for ev in fa.events) and sum(ev.n for ev in fa.events) >= 4
    compare(fa, fb, exact_stats=True)
    for ev in fa.events:
        for seg in ev.segments:
            assert "_gpu_stats" not in seg.__dict__ and np.shares_memory(seg.current, ev.current)


def test_features_with_a_vector_model():
    model = vector_model()
    features = ("mean", "std", "duration")
    fa, fb = new_file(), new_file()
    fa.parse_events(segmenter(), hmm=model, features=features)
    for ev in fb.events:
        ev.parse(segmenter(), hmm=model, features=features)
    compare(fa, fb, exact_stats=False)
    assert sum(ev.n for ev in fa.events) >= 8
    with pytest.raises(ValueError):
        new_file().parse_events(segmenter(), hmm=model)              # a vector model without features


def test_an_impossible_event_raises_and_nothing_is_merged():
    model = uniform_model()
    f, plain = new_file(), new_file()
    plain.parse_events(segmenter())
    with pytest.raises(ValueError, match="event %d" % IMPOSSIBLE):
        f.parse_events(segmenter(), hmm=model)
    for ev, ev_plain in zip(f.events, plain.events):
        assert [(s.start, s.end) for s in ev.segments] == [(s.start, s.end) for s in ev_plain.segments] and ev.n >= 1
        assert all("hidden_state" not in s.__dict__ for s in ev.segments)
    assert f.events[IMPOSSIBLE].n >= 2
