"""HMM-guided segmentation for many events at once, the host side (DataTypes.merge_ranges, merge_by_hmm, the hmm= keyword of
File.parse_events and Experiment.parse) -- no GPU.

The vectorised merge is compared with hmm_oracle.merge_loop, the reference's loop restated on plain tuples, with == : random
paths over models that have repeated state names and silent states, events of 0, 1, 2, 3 and 40 segments, segment starts whose
round trip through seconds truncates (7, 13, 14 samples at 1e5 samples per second) and one whose does not (8), a path that never
changes name and one that changes at every step.  merge_by_hmm is run with duck-typed models (a stub `viterbi`, with and without
`viterbi_batch` and `states`) on events whose currents are host arrays, against Event._merge_by_hmm on a second copy."""
import inspect

import numpy as np
import pytest

import hmm_oracle
from pypore_amd import DataTypes
from pypore_amd.core import Segment
from pypore_amd.DataTypes import Event, Experiment, File, MetaEvent, merge_by_hmm, merge_ranges, state_name_ids
from pypore_amd.hmm import Model, NormalDistribution, State


def model_with_shared_names(seed):
    """Emitting states a, a, b, c, c, d and silent states s, s, t: two pairs of emitting states and one of silent states share
    a name."""
    rng = np.random.default_rng(seed)
    m = Model("shared")
    emit = [State(NormalDistribution(float(3 * k), 1.0), name) for k, name in enumerate("aabccd")]
    silent = [State(None, name) for name in "sst"]
    for s in emit:
        m.add_transition(m.start, s, 1.0)
        for t in emit:
            m.add_transition(s, t, float(rng.uniform(0.1, 1)))
        m.add_transition(s, silent[0], 0.1)
        m.add_transition(s, m.end, 0.1)
    m.add_transition(silent[0], silent[1], 0.5)
    m.add_transition(silent[1], silent[2], 0.5)
    m.add_transition(silent[2], emit[0], 1.0)
    m.bake()
    return m


def segments_at(edges, second):
    """[(start in seconds, n)] of the segments between consecutive edges, as Segment.scale leaves them."""
    return [(a / second, z - a) for a, z in zip(edges[:-1], edges[1:])]


def both(segments, path, model, second):
    ids, names = state_name_ids(model.states)
    want = hmm_oracle.merge_loop(segments, [(int(i), model.states[i]) for i in path], second)
    s, e, hid = merge_ranges([a for a, _ in segments], [n for _, n in segments], path, ids, second)
    assert s.dtype == np.int64 and e.dtype == np.int64
    return list(zip(s.tolist(), e.tolist(), [names[h] for h in hid])), want


def test_name_ids_share_an_id_between_equal_names():
    m = model_with_shared_names(0)
    ids, names = state_name_ids(m.states)
    assert len(names) == len(set(names)) == len({s.name for s in m.states})
    assert [names[i] for i in ids] == [s.name for s in m.states]
    assert len(names) < len(m.states)


@pytest.mark.parametrize("second", [1e5, 5e4, 2e5])
@pytest.mark.parametrize("n_seg", [0, 1, 2, 3, 40])
def test_merge_equals_the_loop_on_random_paths(n_seg, second):
    rng = np.random.default_rng(1000 * n_seg + int(second) % 977)
    for trial in range(40):
        m = model_with_shared_names(trial % 3)
        edges = np.concatenate(([0], np.cumsum(rng.integers(1, 400, n_seg)))).tolist()
        # (few distinct states in a row: runs of one name, runs of two states of one name, single steps)
        path = rng.choice(len(m.states), size=n_seg + 1 + int(rng.integers(0, 5)), p=None)
        if trial % 2:
            path = np.repeat(path, 3)[:path.size]
        got, want = both(segments_at(edges, second), path.tolist(), m, second)
        assert got == want
        assert (len(got) == 0) == (n_seg < 2)


def test_merge_keeps_the_truncating_round_trip():
    second = 1e5
    # (the measured quirk itself: the round trip of these indices through seconds falls just below them)
    assert [int((a / second) * second) for a in (7, 8, 13, 14)] == [6, 8, 12, 13]
    m = model_with_shared_names(1)
    names = [s.name for s in m.states]
    a, b, c = names.index("a"), names.index("b"), names.index("c")
    edges = [0, 7, 8, 13, 14, 30, 50, 70]
    segs = segments_at(edges, second)
    # a group closes at every step (group k starts with the segment that closed group k - 1): the merged segments start at the
    # truncated indices, and end at int(start * second + n) -- 6.99.. + 1 = 7, 12.99.. + 1 = 13
    got, want = both(segs, [m.states.index(m.start), a, b, c, b, a, b, c], m, second)
    assert got == want
    assert [s for s, _, _ in got] == [0, 0, 6, 8, 12, 13]
    assert [e for _, e, _ in got][:4] == [7, 7, 13, 13]
    got, want = both(segs, [m.states.index(m.start), a, a, b, b, c, c, a], m, second)
    assert got == want and len(got) >= 2
    # consecutive merged segments share their boundary segment: they overlap
    assert all(got[k + 1][0] < got[k][1] for k in range(len(got) - 1))


@pytest.mark.parametrize("n_seg", [2, 3, 40])
def test_merge_on_constant_and_alternating_paths(n_seg):
    second = 1e5
    m = model_with_shared_names(2)
    names = [s.name for s in m.states]
    edges = np.arange(0, 13 * (n_seg + 1), 13).tolist()
    segs = segments_at(edges, second)
    first_a, second_a = [k for k, nm in enumerate(names) if nm == "a"]
    # never changes name: the two states called "a" in turn -- one group, closed by i == n - 2
    const = [first_a if k % 2 else second_a for k in range(n_seg + 1)]
    got, want = both(segs, const, m, second)
    assert got == want and len(got) == 1 and got[0][2] == "a"
    assert got[0][0] == int(segs[0][0] * second) and got[0][1] == int(segs[-1][0] * second + segs[-1][1])
    # changes name at every step
    alt = [names.index("b") if k % 2 else names.index("d") for k in range(n_seg + 1)]
    got, want = both(segs, alt, m, second)
    assert got == want and len(got) == n_seg - 1


# ---- merge_by_hmm on host-array events, duck-typed models ------------------------------------------------------------------
class _S(object):
    def __init__(self, name):
        self.name = name


class StubModel(object):
    """viterbi by thresholds: an observation's state is its level's bucket; two buckets share the name "mid"; a silent state
    is visited after every third observation; an observation above 1000 makes the sequence impossible."""

    def __init__(self):
        self.table = [_S("stub-start"), _S("low"), _S("mid"), _S("mid"), _S("high"), _S("quiet")]
        self.calls = 0

    def viterbi(self, obs):
        self.calls += 1
        obs = np.asarray(obs, dtype=np.float64)
        if obs.ndim == 2:
            obs = obs[:, 0]
        if obs.size and obs.max() > 1000:
            return -np.inf, None
        path = [(0, self.table[0])]
        for k, x in enumerate(obs):
            i = 1 + int(np.searchsorted([20.0, 40.0, 60.0], x))
            path.append((i, self.table[i]))
            if k % 3 == 2:
                path.append((5, self.table[5]))
        return -1.0, path


class BatchStub(StubModel):
    """The same model with a state list and viterbi_batch: one call for all events."""

    def __init__(self):
        StubModel.__init__(self)
        self.states = self.table
        self.batches = 0

    def viterbi_batch(self, sequences):
        self.batches += 1
        return [StubModel.viterbi(self, s) for s in sequences]


LEVELS = [[10, 30, 50, 50, 70, 10, 10, 30], [30, 50], [70], [], [10, 10, 10, 10], [10, 70, 10, 70, 10, 70, 30]]


def host_file(levels=LEVELS, spoil=None):
    """A File on a float64 host array: one event per level list, its segments the levels' plateaus (7, 13, 14 .. samples long),
    segmented already -- `start`, `end`, `duration` in seconds, as Event.parse leaves them.  spoil: the event whose first
    plateau is raised above every state of the stub."""
    rng = np.random.default_rng(5)
    f = File(current=np.zeros(1), timestep=0.01)
    rate = f.second
    pieces, at = [], 100
    for k, lv in enumerate(levels):
        lens = [7 + 6 * (q % 3) + q for q in range(len(lv))]
        x = np.concatenate([np.full(n, float(v)) for v, n in zip(lv, lens)] + [np.zeros(0)]) + rng.normal(0, 0.5, int(sum(lens)))
        if spoil == k:
            x[:lens[0]] += 5000.0
        pieces.append((at, x, lens))
        at += x.size + 50
    cur = np.zeros(at)
    for a, x, _ in pieces:
        cur[a:a + x.size] = x
    f.current = cur
    for a, x, lens in pieces:
        ev = Event(current=f.current[a:a + x.size], start=a / rate, end=(a + x.size) / rate, duration=x.size / rate, second=rate, file=f)
        edges = np.concatenate(([0], np.cumsum(lens))).astype(int).tolist()
        ev.segments = [Segment(current=ev.current[p:q], start=p, duration=q - p, end=q) for p, q in zip(edges[:-1], edges[1:])]
        for seg in ev.segments:
            seg.event = ev
            seg.scale(rate)
        f.events.append(ev)
    return f


def same_segments(ev_a, ev_b):
    assert len(ev_a.segments) == len(ev_b.segments)
    for sa, sb in zip(ev_a.segments, ev_b.segments):
        assert type(sa) is Segment and set(sa.__dict__) == set(sb.__dict__)
        assert sa.start == sb.start and type(sa.start) is type(sb.start) and sa.n == sb.n
        assert getattr(sa, "duration", None) == getattr(sb, "duration", None)
        assert sa.hidden_state == sb.hidden_state and sa.second == sb.second
        assert sa.event is ev_a and sb.event is ev_b
        assert np.array_equal(sa.current, sb.current) and np.shares_memory(sa.current, ev_a.current)
        assert (sa.mean, sa.std, sa.min, sa.max) == (sb.mean, sb.std, sb.min, sb.max)


@pytest.mark.parametrize("stub", [StubModel, BatchStub])
def test_merge_by_hmm_leaves_events_as_the_loop_does(stub):
    fa, fb = host_file(), host_file()
    model_a, model_b = stub(), stub()
    merge_by_hmm(fa.events, model_a)
    for ev in fb.events:
        ev.segments = ev._merge_by_hmm(model_b)
    assert [ev.n for ev in fb.events] == [ev.n for ev in fa.events]
    assert sum(ev.n for ev in fa.events) > 6 and fa.events[2].segments == [] and fa.events[3].segments == []
    for ev_a, ev_b in zip(fa.events, fb.events):
        same_segments(ev_a, ev_b)
    if stub is BatchStub:
        assert model_a.batches == 1
    # with features: the stub reads the first column
    fa, fb = host_file(), host_file()
    merge_by_hmm(fa.events, stub(), features=("mean", "std"))
    for ev in fb.events:
        ev.segments = ev._merge_by_hmm(stub(), ("mean", "std"))
    for ev_a, ev_b in zip(fa.events, fb.events):
        same_segments(ev_a, ev_b)


@pytest.mark.parametrize("stub", [StubModel, BatchStub])
def test_an_impossible_event_raises_before_anything_changes(stub):
    f = host_file(spoil=4)
    before = [list(ev.segments) for ev in f.events]
    with pytest.raises(ValueError, match="event 4"):
        merge_by_hmm(f.events, stub())
    for ev, segs in zip(f.events, before):
        assert len(ev.segments) == len(segs) and all(a is b for a, b in zip(ev.segments, segs))
        assert all("hidden_state" not in s.__dict__ for s in ev.segments)
    # an impossible event of fewer than two segments ends with none, as in the loop
    f = host_file(spoil=2)
    merge_by_hmm(f.events, stub())
    assert f.events[2].segments == [] and f.events[0].n > 0


def test_type_errors_come_first():
    f = host_file()
    before = [list(ev.segments) for ev in f.events]
    with pytest.raises(TypeError):
        merge_by_hmm(f.events, object())
    with pytest.raises(TypeError):
        merge_by_hmm(f.events, None)
    meta = MetaEvent(start=0.0, duration=1.0, segments=[])
    model = StubModel()
    with pytest.raises(TypeError):
        merge_by_hmm(f.events[:2] + [meta], model)
    assert model.calls == 0
    assert all(a is b for ev, segs in zip(f.events, before) for a, b in zip(ev.segments, segs))
    with pytest.raises(TypeError):
        f.parse_events(FixedParser(), hmm=object())


class FixedParser(object):
    """A user's parser without parse_batch: a boundary every 9 samples."""

    def parse(self, current):
        edges = list(range(0, len(current), 9)) + [len(current)]
        return [Segment(current=current[a:z], start=a, duration=z - a, end=z) for a, z in zip(edges[:-1], edges[1:]) if z > a]


def test_the_new_keywords_default_to_todays_behaviour():
    for fn in (File.parse_events, Experiment.parse):
        p = inspect.signature(fn).parameters
        assert p["hmm"].default is None and p["features"].default is None
    assert list(inspect.signature(File.parse_events).parameters)[:3] == ["self", "parser", "filter_params"]
    assert list(inspect.signature(Experiment.parse).parameters)[:7] == ["self", "event_detector", "segmenter", "filter_params", "verbose",
                                                                        "meta", "workers"]
    fa, fb, fc = host_file(), host_file(), host_file()
    fa.parse_events(FixedParser())
    for ev in fb.events:
        ev.parse(FixedParser())
    fc.parse_events(FixedParser(), None, None, None)
    for ev_a, ev_b, ev_c in zip(fa.events, fb.events, fc.events):
        for other in (ev_b, ev_c):
            assert [(s.start, s.duration, s.end) for s in ev_a.segments] == [(s.start, s.duration, s.end) for s in other.segments]
        assert all("hidden_state" not in s.__dict__ for s in ev_a.segments) and ev_a.state_parser is not None


def test_parse_events_with_hmm_equals_the_per_event_route():
    fa, fb = host_file(), host_file()
    model = BatchStub()
    fa.parse_events(FixedParser(), hmm=model)
    for ev in fb.events:
        ev.parse(FixedParser(), hmm=BatchStub())
    assert model.batches == 1 and sum(ev.n for ev in fa.events) > 0
    for ev_a, ev_b in zip(fa.events, fb.events):
        same_segments(ev_a, ev_b)
        assert isinstance(ev_a.state_parser, FixedParser)
    # Experiment.parse hands the keywords on (File objects are taken as they are)
    fc = host_file()
    ex = Experiment([fc])

    class Detector(object):
        def parse(self, current):
            return [Segment(current=ev.current, start=int(round(ev.start * fc.second)), duration=len(ev.current)) for ev in host_file().events]

    ex.parse(event_detector=Detector(), segmenter=FixedParser(), filter_params=None, verbose=False, hmm=BatchStub())
    assert len(ex.files) == 1 and len(ex.events) == len(fb.events)
    for ev_c, ev_b in zip(ex.events, fb.events):
        assert [(s.start, s.hidden_state) for s in ev_c.segments] == [(s.start, s.hidden_state) for s in ev_b.segments]
    assert DataTypes.merge_by_hmm is merge_by_hmm
