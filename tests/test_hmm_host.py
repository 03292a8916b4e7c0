"""pypore_amd.hmm on the host: bake (normalisation, state order, pruning, silent cycles, add_model of a board), the test
oracle against brute force, and the callers in DataTypes (apply_hmm, parse(hmm=...), Experiment.apply_hmm) with
duck-typed models.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402

from pypore_amd.hmm import Model, NormalDistribution, State, UniformDistribution  # noqa: E402
from pypore_amd.DataTypes import Event, Experiment, File, MetaEvent  # noqa: E402
from pypore_amd.core import Segment, MetaSegment  # noqa: E402


def _names(model):
    return [s.name for s in model.states]


def test_bake_normalises_orders_and_prunes():
    m = Model("m")
    b = State(NormalDistribution(1, 1), "b")
    a = State(NormalDistribution(2, 1), "a")
    a2 = State(UniformDistribution(0, 5), "a")            # same name as `a`: stable order keeps a before a2
    d = State(None, "d")
    lost = State(NormalDistribution(0, 1), "lost")        # never reached from start
    m.add_states([b, a, a2, d, lost])
    m.add_transition(m.start, b, 2.0)
    m.add_transition(m.start, d, 6.0)
    m.add_transition(d, a, 1.0)
    m.add_transition(d, a2, 1.0)
    m.add_transition(b, m.end, 0.3)
    m.add_transition(a, m.end, 1.0)
    m.add_transition(a2, m.end, 1.0)
    m.add_transition(lost, a, 1.0)
    m.bake()
    assert _names(m) == ["a", "a", "b", "m-start", "m-end", "d"]     # end: level 0 (no silent predecessor), d: level 1
    assert m.states[0] is a and m.states[1] is a2 and lost not in m.states
    ix = {id(s): i for i, s in enumerate(m.states)}
    p = {(i, j): w for i, j, w in m.edges}
    assert p[(ix[id(m.start)], ix[id(b)])] == pytest.approx(0.25) and p[(ix[id(m.start)], ix[id(d)])] == pytest.approx(0.75)
    assert p[(ix[id(b)], ix[id(m.end)])] == pytest.approx(1.0)
    for i in range(len(m.states)):
        out = [w for (a_, _), w in p.items() if a_ == i]
        assert not out or sum(out) == pytest.approx(1.0)
    assert m.finite
    f = m.flat
    assert f["n_states"] == 6 and f["n_emit"] == 3 and f["level_ptr"][0] == 3 and f["level_ptr"][-1] == 6
    # in-edges: sources ascending per target
    for k in range(6):
        src = f["in_src"][f["in_ptr"][k]:f["in_ptr"][k + 1]]
        assert list(src) == sorted(src)


def test_bake_keeps_end_and_is_infinite_without_edges_into_it():
    m = Model("inf")
    a = State(NormalDistribution(0, 1), "a")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, a, 1.0)
    m.bake()
    assert not m.finite and m.end in m.states and len(m.states) == 3


def test_silent_cycle_raises():
    m = Model("cyc")
    x, y = State(None, "x"), State(None, "y")
    m.add_transition(m.start, x, 1.0)
    m.add_transition(x, y, 0.5)
    m.add_transition(y, x, 0.5)
    m.add_transition(y, m.end, 0.5)
    with pytest.raises(ValueError):
        m.bake()
    m2 = Model("self")
    z = State(None, "z")
    m2.add_transition(m2.start, z, 1.0)
    m2.add_transition(z, z, 0.5)
    m2.add_transition(z, m2.end, 0.5)
    with pytest.raises(ValueError):
        m2.bake()


class Board(Model):
    """A subclass in the style of the reference's HMMBoard: n lanes, each with a silent start and end."""

    def __init__(self, n, name=None):
        super(Board, self).__init__(name="Board {}".format(name))
        self.n = n
        for i in range(1, n + 1):
            s, e = State(None, name="b{}s{}".format(name, i)), State(None, name="b{}e{}".format(name, i))
            setattr(self, "s%d" % i, s)
            setattr(self, "e%d" % i, e)
            self.add_state(s)
            self.add_state(e)


def test_add_model_of_a_board():
    model = Model("profile")
    board = Board(2, name=0)
    match = State(NormalDistribution(5, 1), "M:0")
    board.add_transition(board.s1, board.e1, 1.0)
    board.add_transition(board.s2, match, 1.0)
    board.add_transition(match, board.e2, 1.0)
    model.add_model(board)
    assert board.start in model._added and board.end in model._added       # the board's start/end join as silent states
    model.add_transition(model.start, board.s1, 0.5)
    model.add_transition(model.start, board.s2, 0.5)
    model.add_transition(board.e1, model.end, 1.0)
    model.add_transition(board.e2, model.end, 1.0)
    model.bake()
    names = _names(model)
    assert names[0] == "M:0" and "Board 0-start" not in names          # unreachable board start / end are dropped
    c = O.Compiled(model)
    lp, path, _ = O.viterbi(c, [5.0])
    assert [model.states[k].name for k in path] == ["profile-start", "b0s2", "M:0", "b0e2", "profile-end"]
    assert lp == pytest.approx(math.log(0.5) + O.emission(match, 5.0))
    assert O.log_probability(c, []) == pytest.approx(math.log(0.5))


@pytest.mark.parametrize("seed", range(40))
def test_oracle_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    model = O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0)
    c = O.Compiled(model)
    assert c.S - 2 <= 4
    for n in range(0, 7):
        seq = rng.normal(size=n)
        F_bf, logp_bf, best_bf, path_bf = O.brute_force(c, seq)
        F = O.forward(c, seq)
        assert np.array_equal(np.isneginf(F), np.isneginf(F_bf))
        fin = np.isfinite(F)
        assert np.allclose(F[fin], F_bf[fin], rtol=1e-12, atol=1e-12)
        logp = O.log_probability(c, seq)
        B = O.backward(c, seq)
        v_lp, v_path, _ = O.viterbi(c, seq)
        if path_bf is None:
            assert logp == -np.inf and v_lp == -np.inf and v_path is None and B[0, c.start] == -np.inf
            continue
        assert logp == pytest.approx(logp_bf, rel=1e-12, abs=1e-12)
        assert B[0, c.start] == pytest.approx(logp_bf, rel=1e-10, abs=1e-10)
        assert v_lp == pytest.approx(best_bf, rel=1e-12, abs=1e-12)
        assert O.path_score(c, seq, v_path) == pytest.approx(best_bf, rel=1e-12, abs=1e-12)
        assert v_path == path_bf


def test_uniform_makes_sequences_impossible():
    m = Model("u")
    a = State(UniformDistribution(0, 1), "a")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, a, 0.5)
    m.add_transition(a, m.end, 0.5)
    m.bake()
    c = O.Compiled(m)
    assert O.viterbi(c, [0.5, 2.0])[:2] == (-np.inf, None)
    assert O.log_probability(c, [0.5, 0.2]) == pytest.approx(2 * math.log(0.5))


# ---- callers in DataTypes -------------------------------------------------------------------------------------------
class FakeHMM(object):
    """Duck-typed model: records the means it was given, returns fixed answers."""

    def __init__(self, names):
        self.states = [(i, State(None, nm)) for i, nm in enumerate(names)]
        self.calls = []

    def viterbi(self, seq):
        self.calls.append(np.asarray(seq))
        return -1.5, self.states

    def forward(self, seq):
        self.calls.append(np.asarray(seq))
        return np.zeros((len(seq) + 1, 2))


def _event(n_samples=100, second=1000.0):
    f = File(current=np.arange(n_samples, dtype=np.float64), timestep=1000.0 / second)
    return Event(current=np.arange(n_samples, dtype=np.float64), start=0, end=n_samples / second,
                 duration=n_samples / second, second=second, file=f)


def test_apply_hmm_on_event_and_metaevent():
    ev = _event()
    ev.segments = [Segment(current=np.full(5, v)) for v in (1.0, 2.0, 4.0)]
    hmm = FakeHMM(["s", "a"])
    assert ev.apply_hmm(hmm) == (-1.5, hmm.states)
    assert np.array_equal(hmm.calls[-1], [1.0, 2.0, 4.0])
    assert ev.apply_hmm(hmm, algorithm="forward").shape == (4, 2)
    me = MetaEvent(mean=1.0, start=0.0, duration=1.0)
    me.segments = [MetaSegment(mean=m, start=0.0, duration=1.0) for m in (3.0, 7.0)]
    assert me.apply_hmm(hmm) == (-1.5, hmm.states)
    assert np.array_equal(hmm.calls[-1], [3.0, 7.0])


class StubParser(object):
    """Cuts the current at fixed sample boundaries."""

    def __init__(self, bounds):
        self.bounds = bounds

    def parse(self, current):
        edges = [0] + list(self.bounds) + [len(current)]
        return [Segment(current=current[a:b], start=a, end=b, duration=b - a) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("bounds,names", [
    ([], ["start", "x"]),                                              # n = 1: no segments
    ([40], ["start", "x", "x"]),                                       # n = 2
    ([30, 60], ["start", "x", "y", "y"]),                             # n = 3
    ([10, 20, 30, 45, 50, 70, 80, 95], ["start", "a", "a", "b", "b", "b", "c", "a", "a", "end"]),
])
def test_parse_with_hmm_merges_like_the_reference(bounds, names):
    second = 1000.0
    ev = _event(100, second)
    hmm = FakeHMM(names)
    ev.parse(StubParser(bounds), hmm=hmm)
    plain = StubParser(bounds).parse(np.arange(100, dtype=np.float64))
    want = O.merge_loop([(s.start / second, s.n) for s in plain], hmm.states, second)
    got = [(seg.start, seg.start + seg.n, seg.hidden_state) for seg in ev.segments]
    want = [(s, min(e, 100), h) for s, e, h in want]
    assert got == want
    assert all(seg.event is ev for seg in ev.segments)
    if len(plain) < 2:
        assert ev.segments == []
    assert np.array_equal(hmm.calls[-1], [s.mean for s in plain])
    if bounds == [10, 20, 30, 45, 50, 70, 80, 95]:
        # the quirks, spelled out: shared boundary segments, start in samples, hidden state of path entry j+1
        assert got == [(0, 10, "a"), (0, 30, "a"), (20, 70, "b"), (50, 80, "c"), (70, 100, "a")]


def test_parse_rejects_an_object_without_viterbi():
    with pytest.raises(TypeError):
        _event().parse(StubParser([50]), hmm=object())


def test_experiment_apply_hmm_one_batch_call():
    exp = Experiment([])
    f = File(current=np.zeros(10), timestep=1.0)
    evs = []
    for k in range(4):
        ev = _event()
        ev.segments = [Segment(current=np.full(3, float(k + j))) for j in range(2)]
        evs.append(ev)
    f.events = evs
    exp.files = [f]

    class Batched(FakeHMM):
        def viterbi_batch(self, seqs):
            self.batches = [list(map(list, seqs))]
            return [(0.0, [(q, State(None, "q%d" % q))]) if q != 2 else (-np.inf, None) for q in range(len(seqs))]

    hmm = Batched(["s"])
    out = exp.apply_hmm(hmm, filter=lambda e: e is not evs[3], indices=[3, 0, 1, 2])
    assert hmm.batches == [[[0.0, 1.0], [1.0, 2.0], [2.0, 3.0]]] and hmm.calls == []
    assert [i for i, _ in out] == [0, 1]
    with pytest.raises(NotImplementedError):
        exp.apply_hmm(None)
    with pytest.raises(NotImplementedError):
        exp.apply_hmm(object())
    plain = FakeHMM(["s", "t"])
    assert len(exp.apply_hmm(plain)) == 8 and len(plain.calls) == 4
