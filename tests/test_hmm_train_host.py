"""Model.train on the host (no GPU): the numpy E-step of the test oracle against brute-force path enumeration, the
M-step's rules on hand-made statistics, pseudocounts, Viterbi training's counting, the stop loop with the E-step stubbed,
and argument errors."""
import copy
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import hmm_train_oracle as T  # noqa: E402

from pypore_amd.hmm import Expectations, Model, NormalDistribution, State, UniformDistribution  # noqa: E402


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.size == 0 or err.max() <= tol, err.max()


def small_model(name="m"):
    """start -> a | b | d (silent) ; a -> a | b | end ; b -> b | end ; d -> b ; u (uniform) -> end; start -> u."""
    m = Model(name)
    a = State(NormalDistribution(1.0, 1.0), "a")
    b = State(NormalDistribution(4.0, 2.0), "b")
    u = State(UniformDistribution(0.0, 10.0), "u")
    d = State(None, "d")
    m.add_transition(m.start, a, 0.5, pseudocount=2.0)
    m.add_transition(m.start, b, 0.2)
    m.add_transition(m.start, d, 0.2)
    m.add_transition(m.start, u, 0.1)
    m.add_transition(a, a, 0.6)
    m.add_transition(a, b, 0.3)
    m.add_transition(a, m.end, 0.1)
    m.add_transition(b, b, 0.5)
    m.add_transition(b, m.end, 0.5)
    m.add_transition(d, b, 1.0)
    m.add_transition(u, m.end, 1.0)
    m.bake()
    return m


def edge_p(m, a, b):
    ix = {id(s): i for i, s in enumerate(m.states)}
    return {(i, j): p for i, j, p in m.edges}[(ix[id(a)], ix[id(b)])]


def by_name(m, name):
    return [s for s in m.states if s.name == name][0]


@pytest.mark.parametrize("seed", range(10))
def test_numpy_estep_equals_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    model = O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=True)
    for n in range(6):
        x = rng.normal(size=n)
        c1, s1, l1 = T.estep_one(model, x)
        c2, s2, l2 = T.estep_brute_force(model, x)
        if not l2 > -np.inf:
            assert not l1 > -np.inf and not c1.any() and not s1.any()
            continue
        close([l1], [l2], 1e-12)
        close(c1, c2, 1e-12)
        close(s1, s2, 1e-12)


def test_expected_counts_sum_to_path_lengths():
    """Every observation is consumed by exactly one emitting state: sum W = n; the edges into emitting states are used n
    times in all."""
    model, means = O.profile_model(6, seed=2)
    x = O.profile_events(means, 1, lo=8, hi=8, seed=3)[0]
    counts, stats, _ = T.estep_one(model, x)
    NE = T.n_emit(model)
    into_emit = sum(cn for (i, j, _), cn in zip(model.edges, counts) if j < NE)
    assert stats[:, 0].sum() == pytest.approx(x.size, rel=1e-12)
    assert into_emit == pytest.approx(x.size, rel=1e-12)


def test_m_step_transitions():
    m = small_model()
    a, b, d, u = (by_name(m, s) for s in "abdu")
    E = len(m.edges)
    counts = np.zeros(E)
    ix = {id(s): i for i, s in enumerate(m.states)}
    pos = {(i, j): e for e, (i, j, _) in enumerate(m.edges)}

    def put(x, y, v):
        counts[pos[(ix[id(x)], ix[id(y)])]] = v

    put(m.start, a, 3.0)
    put(m.start, b, 1.0)
    put(a, a, 2.0)
    put(a, b, 2.0)                 # a -> end stays 0: the edge keeps its place with probability 0
    stats = np.zeros((T.n_emit(m), 3))
    old = copy.deepcopy(m.edges)
    m._m_step(counts, stats)
    assert edge_p(m, m.start, a) == pytest.approx(0.75) and edge_p(m, m.start, b) == pytest.approx(0.25)
    assert edge_p(m, m.start, d) == 0.0 and edge_p(m, m.start, u) == 0.0
    assert edge_p(m, a, a) == 0.5 and edge_p(m, a, m.end) == 0.0
    assert edge_p(m, b, b) == 0.5 and edge_p(m, b, m.end) == 0.5        # zero-sum row: old probabilities
    assert [(i, j) for i, j, _ in m.edges] == [(i, j) for i, j, _ in old]
    assert m._edges[(a, m.end)] == 0.0 and m._edges[(m.start, a)] == pytest.approx(0.75)
    f = m.flat
    assert np.isneginf(f["out_lp"]).sum() == 3 and np.isneginf(f["in_lp"]).sum() == 3
    # a later bake drops the zero edges (and with them d and u, which start no longer reaches)
    m.bake()
    assert all(p > 0 for _, _, p in m.edges) and d not in m.states and u not in m.states
    assert len(m.edges) == len(old) - 5


def test_m_step_pseudocounts_and_inertia_against_oracle():
    rng = np.random.default_rng(5)
    for kw in (dict(use_pseudocount=True), dict(transition_pseudocount=0.5), dict(edge_inertia=0.3),
               dict(use_pseudocount=True, transition_pseudocount=1.0, edge_inertia=0.9, distribution_inertia=0.4),
               dict(distribution_inertia=1.0), dict(min_std=5.0)):
        m = small_model()
        counts = rng.uniform(0, 3, len(m.edges))
        counts[rng.random(counts.size) < 0.3] = 0.0
        stats = np.zeros((T.n_emit(m), 3))
        for k in range(stats.shape[0]):
            W = rng.uniform(0.5, 4)
            A = W * rng.normal()
            stats[k] = (W, A, A * A / W + W * rng.uniform(0.1, 2))
        want = copy.deepcopy(m)
        T.m_step(want, counts, stats, pseudocounts=T.pseudocounts_of(want), **kw)
        m._m_step(counts, stats, **kw)
        close([p for _, _, p in m.edges], [p for _, _, p in want.edges], 1e-15)
        for s, w in zip(m.states, want.states):
            if not s.is_silent():
                close(s.distribution.parameters, w.distribution.parameters, 1e-14)


def test_m_step_distribution_rules():
    m = small_model()
    a, b, u = by_name(m, "a"), by_name(m, "b"), by_name(m, "u")
    k = {id(s): i for i, s in enumerate(m.states)}
    stats = np.zeros((T.n_emit(m), 3))
    stats[k[id(a)]] = (4.0, 2.0, 5.0)          # mean 1 + 0.5, var 5/4 - 0.25 = 1
    stats[k[id(u)]] = (3.0, 1.0, 9.0)          # uniform: never trained
    b.distribution.freeze()
    stats[k[id(b)]] = (2.0, 2.0, 8.0)          # frozen
    m._m_step(np.zeros(len(m.edges)), stats, distribution_inertia=0.25)
    assert a.distribution.parameters == pytest.approx([0.25 * 1 + 0.75 * 1.5, 0.25 * 1 + 0.75 * 1.0])
    assert u.distribution.parameters == [0.0, 10.0] and b.distribution.parameters == [4.0, 2.0]
    b.distribution.thaw()
    assert not b.distribution.frozen
    # W = 0 leaves the parameters; var <= 0 gives min_std
    stats[:] = 0
    stats[k[id(b)]] = (2.0, 2.0, 2.0)          # var 1 - 1 = 0
    m._m_step(np.zeros(len(m.edges)), stats, min_std=0.2)
    assert b.distribution.parameters == pytest.approx([5.0, 0.2])
    assert a.distribution.parameters == pytest.approx([1.375, 1.0])
    # the flat arrays follow
    f = m.flat
    assert f["param"][3 * k[id(b)]] == pytest.approx(5.0)
    assert f["param"][3 * k[id(b)] + 1] == pytest.approx(1 / (2 * 0.04))


def test_m_step_shared_distribution_pools_statistics():
    m = Model("shared")
    dist = NormalDistribution(0.0, 1.0)
    a, b = State(dist, "a"), State(dist, "b")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, b, 1.0)
    m.add_transition(b, m.end, 1.0)
    m.bake()
    m._m_step(np.zeros(len(m.edges)), np.array([[1.0, 1.0, 1.0], [1.0, 3.0, 9.0]]))
    assert dist.parameters == pytest.approx([2.0, 1.0])


def test_recompiled_model_equals_fresh_bake():
    m = small_model()
    rng = np.random.default_rng(1)
    stats = np.abs(rng.normal(size=(T.n_emit(m), 3))) + 1
    m._m_step(rng.uniform(0.1, 2, len(m.edges)), stats)
    f = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in m.flat.items()}
    m.bake()
    g = m.flat
    for key in f:
        if isinstance(f[key], np.ndarray):
            np.testing.assert_allclose(f[key], g[key], rtol=1e-14, atol=0)
        else:
            assert f[key] == g[key]


def test_pseudocount_defaults_and_add_model():
    m = Model("m")
    a, b = State(NormalDistribution(0, 1), "a"), State(NormalDistribution(1, 1), "b")
    m.add_transition(m.start, a, 2.0)
    m.add_transition(a, b, 0.5, pseudocount=7.0)
    m.add_transition(b, m.end, 1.0, 0.0)
    assert m._pseudo[(m.start, a)] == 2.0 and m._pseudo[(a, b)] == 7.0 and m._pseudo[(b, m.end)] == 0.0
    assert m._edges[(m.start, a)] == 2.0                   # three-argument calls as before
    with pytest.raises(ValueError):
        m.add_transition(a, b, 0.5, pseudocount=-1)
    outer = Model("outer")
    outer.add_model(m)
    outer.add_transition(outer.start, m.start, 1.0)
    outer.add_transition(m.end, outer.end, 1.0)
    assert outer._pseudo[(a, b)] == 7.0 and outer._pseudo[(m.start, a)] == 2.0
    outer.bake()
    pc = T.pseudocounts_of(outer)
    assert sorted(pc) == sorted([2.0, 7.0, 0.0, 1.0, 1.0])


def test_viterbi_counts_from_given_paths(monkeypatch):
    m = small_model()
    a, b, d = by_name(m, "a"), by_name(m, "b"), by_name(m, "d")
    ix = {id(s): i for i, s in enumerate(m.states)}
    p1 = [m.start, a, a, b, m.end]
    p2 = [m.start, d, b, m.end]
    paths = [(-3.0, [(ix[id(s)], s) for s in p1]), (-np.inf, None), (-2.0, [(ix[id(s)], s) for s in p2])]
    monkeypatch.setattr(m, "viterbi_batch", lambda seqs, device=None: paths)
    seqs = [np.array([0.5, 2.0, 5.0]), np.array([1.0]), np.array([3.0])]
    est = m._viterbi_counts(seqs)
    want = np.zeros(len(m.edges))
    pos = {(i, j): e for e, (i, j, _) in enumerate(m.edges)}
    for p in (p1, p2):
        for s, t in zip(p[:-1], p[1:]):
            want[pos[(ix[id(s)], ix[id(t)])]] += 1
    assert np.array_equal(est.counts, want)
    assert est.skipped == 1 and list(est.logp) == [-3.0, -np.inf, -2.0]
    ka, kb = ix[id(a)], ix[id(b)]
    close(est.stats[ka], [2, (0.5 - 1) + (2 - 1), 0.25 + 1], 1e-15)
    close(est.stats[kb], [2, (5 - 4) + (3 - 4), 1 + 1], 1e-15)


class Stub(object):
    """A scripted E-step: logp sums per pass, and a record of which passes asked for statistics."""

    def __init__(self, model, sums):
        self.sums, self.calls = list(sums), []
        self.model = model

    def __call__(self, seqs, algorithm, want_stats, device):
        k = len(self.calls)
        self.calls.append(want_stats)
        logp = np.full(len(seqs), self.sums[k] / max(1, len(seqs)))
        est = Expectations(np.zeros(len(self.model.edges)), np.zeros((T.n_emit(self.model), 3)), logp, 0)
        return logp, est if want_stats else None


@pytest.mark.parametrize("kw,sums,steps,stats_calls", [
    (dict(max_iterations=3), [-100, -60, -50, -45, -44], [40, 10, 5], [True, True, True, False]),
    (dict(max_iterations=10), [-100, -60, -60, -55], [40, 0], [True, True, True]),
    (dict(max_iterations=10, stop_threshold=8), [-100, -60, -55, -50], [40, 5], [True, True, True]),
    (dict(max_iterations=10, stop_threshold=8, min_iterations=3), [-100, -60, -55, -50, -49], [40, 5, 5], [True] * 4),
    (dict(max_iterations=0), [-100], [], [False]),
    (dict(), [-100, -90, -95], [10, -5], [True, True, True]),
])
def test_stop_loop_and_printed_lines(monkeypatch, capsys, kw, sums, steps, stats_calls):
    m = small_model()
    stub = Stub(m, sums)
    monkeypatch.setattr(m, "_estep", stub)
    total = m.train([np.zeros(3), np.ones(2)], **kw)
    out = capsys.readouterr().out.strip().splitlines()
    assert out == ["Training improvement: {}".format(float(s)) for s in steps] + \
        ["Total Training Improvement: {}".format(float(sum(steps)))]
    assert total == float(sum(steps))
    assert stub.calls == stats_calls
    monkeypatch.setattr(m, "_estep", Stub(m, [-7.0]))
    assert m.train([np.zeros(3)], max_iterations=0, verbose=False) == 0.0
    assert capsys.readouterr().out == ""


def test_impossible_sequences_are_left_out(monkeypatch):
    m = small_model()
    seen = []

    def estep(seqs, algorithm, want_stats, device):
        seen.append(len(seqs))
        logp = np.array([-np.inf if s.size == 0 else -1.0 for s in seqs])
        return logp, Expectations(np.zeros(len(m.edges)), np.zeros((T.n_emit(m), 3)), logp, int(np.isinf(logp).sum()))

    monkeypatch.setattr(m, "_estep", estep)
    assert m.train([np.zeros(0), np.ones(2), np.ones(1)], max_iterations=2, verbose=False) == 0.0
    assert seen == [3, 2]


def test_argument_errors():
    m = small_model()
    seqs = [np.zeros(2)]
    for kw in (dict(algorithm="em"), dict(max_iterations=-1), dict(max_iterations=1.5), dict(min_iterations=-2),
               dict(edge_inertia=1.5), dict(distribution_inertia=-0.1), dict(transition_pseudocount=-1),
               dict(min_std=0.0)):
        with pytest.raises(ValueError):
            m.train(seqs, verbose=False, **kw)
    with pytest.raises(ValueError, match="list of sequences"):
        m.train(np.zeros(4), verbose=False)
    with pytest.raises(ValueError, match="1-D"):
        m.train([np.zeros((2, 2))], verbose=False)
    with pytest.raises(ValueError, match="not baked"):
        Model("raw").train(seqs, verbose=False)
    with pytest.raises(ValueError, match="statistics"):
        m._m_step(np.zeros(1), np.zeros((T.n_emit(m), 3)))
    assert not NormalDistribution(0, 1).frozen and not UniformDistribution(0, 1).frozen
    assert math.isfinite(m.train([], max_iterations=0, verbose=False))
