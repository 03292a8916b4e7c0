"""Vector models of pypore_amd.hmm on the host (no GPU): the three new distributions against long-double formulas, their
argument errors, what bake() compiles (n_dim, the component tables entry by entry, a univariate model's arrays as they
were with the new ones empty), the oracle of tests/multivariate_oracle.py against brute-force path enumeration and its
flat-array Viterbi against its dynamic programme, the M-step from hand-made statistics, features= on Event, MetaEvent and
Experiment with a stub model, and the oracle's near-tie report on every log-normal input the GPU tests decode.

yahmm is not available to compare against; nothing here is compared with it."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import multivariate_oracle as MV  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution, Model,  # noqa: E402
                            MultivariateDistribution, NormalDistribution, State, UniformDistribution)

LSQ = 0.5 * math.log(2 * math.pi)


def rel(got, want):
    return abs(got - float(want)) / max(1.0, abs(float(want)))


# ---- the distributions ------------------------------------------------------------------------------------------------
def test_log_probability_against_long_double():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(200):
        ln = LogNormalDistribution(float(rng.normal(0, 2)), float(rng.uniform(0.05, 3)))
        ex = ExponentialDistribution(float(rng.uniform(0.01, 50)))
        no = NormalDistribution(float(rng.normal(0, 5)), float(rng.uniform(0.1, 4)))
        x = float(rng.lognormal(0, 2))
        for d in (ln, ex):
            worst = max(worst, rel(d.log_probability(x), MV.component_ld(d, x)))
            assert d.log_probability(x) == MV.component(d, x) or rel(d.log_probability(x), MV.component(d, x)) <= 1e-14
        w = [float(v) for v in rng.uniform(0.2, 3, 3)]
        mv = MultivariateDistribution([no, ln, ex], w)
        row = [float(rng.normal(0, 5)), x, float(rng.exponential(2))]
        want = MV.emission(mv, row, MV.component_ld)
        worst = max(worst, rel(mv.log_probability(row), want))
        assert mv.log_probability(tuple(row)) == mv.log_probability(np.array(row))
    print("largest error against long double %.3g" % worst)
    assert worst <= 1e-14


def test_supports_and_single_component_bits():
    ln, ex = LogNormalDistribution(0.3, 0.7), ExponentialDistribution(2.5)
    assert ln.log_probability(0.0) == -np.inf and ln.log_probability(-1.0) == -np.inf and ln.log_probability(1e-300) > -np.inf
    assert ex.log_probability(-1e-300) == -np.inf and ex.log_probability(0.0) == math.log(2.5)
    assert ln.parameters == [0.3, 0.7] and ex.parameters == [2.5]
    no = NormalDistribution(1.25, 0.8)
    one = MultivariateDistribution([no])
    assert one.parameters == [[no], [1.0]] and one.parameters[0][0] is no
    for x in (0.1, -3.7, 12.0):
        assert one.log_probability([x]) == no.log_probability(x)              # bit for bit: 1.0 * l, no 0.0 + ...
    # an impossible component gives -inf, never NaN, whatever the others say
    mv = MultivariateDistribution([UniformDistribution(0, 1), ex, ln], [0.5, 2.0, 3.0])
    assert mv.log_probability([2.0, 1.0, 1.0]) == -np.inf
    assert mv.log_probability([0.5, -1.0, 0.0]) == -np.inf
    assert mv.log_probability([0.5, 1.0, 2.0]) == 0.5 * 0.0 + 2.0 * ex.log_probability(1.0) + 3.0 * ln.log_probability(2.0)
    # compiled triples (include/poreseg.h comp_param)
    assert ln.compiled() == (0.3, 1.0 / (2.0 * 0.7 * 0.7), -(math.log(0.7) + LSQ))
    assert ex.compiled() == (0.0, 2.5, math.log(2.5))


def test_argument_errors():
    for bad in (dict(mu=0, sigma=0), dict(mu=0, sigma=-1), dict(mu=0, sigma=np.inf), dict(mu=np.nan, sigma=1)):
        with pytest.raises(ValueError):
            LogNormalDistribution(**bad)
    for rate in (0, -1, np.inf, np.nan):
        with pytest.raises(ValueError):
            ExponentialDistribution(rate)
    n = NormalDistribution(0, 1)
    with pytest.raises(ValueError, match="at least one"):
        MultivariateDistribution([])
    with pytest.raises(ValueError, match="GaussianKernelDensity"):
        MultivariateDistribution([n, GaussianKernelDensity([1.0, 2.0])])
    with pytest.raises(ValueError, match="component of another"):
        MultivariateDistribution([n, MultivariateDistribution([n])])
    with pytest.raises(ValueError):
        MultivariateDistribution([n, "normal"])
    with pytest.raises(ValueError, match="weights"):
        MultivariateDistribution([n, n], [1.0])
    for w in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="weights"):
            MultivariateDistribution([n, n], [1.0, w])
    with pytest.raises(ValueError):
        MultivariateDistribution([n, n]).log_probability([1.0])


# ---- bake -------------------------------------------------------------------------------------------------------------
def two_state(da, db, name="m"):
    m = Model(name)
    a, b = State(da, "a"), State(db, "b")
    m.add_transition(m.start, a, 0.6)
    m.add_transition(m.start, b, 0.4)
    m.add_transition(a, a, 0.5)
    m.add_transition(a, b, 0.3)
    m.add_transition(a, m.end, 0.2)
    m.add_transition(b, a, 0.5)
    m.add_transition(b, m.end, 0.5)
    return m, a, b


def test_bake_errors_and_n_dim():
    n, u = NormalDistribution(0, 1), UniformDistribution(0, 1)
    m, _, _ = two_state(MultivariateDistribution([n, u]), n)
    with pytest.raises(ValueError, match="same dimension"):
        m.bake()
    m, _, _ = two_state(MultivariateDistribution([n, u]), MultivariateDistribution([n, u, n]))
    with pytest.raises(ValueError, match="same dimension"):
        m.bake()
    for other in (MultivariateDistribution([n]), LogNormalDistribution(0, 1), ExponentialDistribution(1)):
        m, _, _ = two_state(GaussianKernelDensity([1.0, 2.0]), other)
        with pytest.raises(ValueError, match="kernel-density"):
            m.bake()
    m, _, _ = two_state(MultivariateDistribution([n] * 17), MultivariateDistribution([n] * 17))
    with pytest.raises(ValueError, match="at most 16"):
        m.bake()
    assert Model("raw").n_dim is None
    for da, db, dim, vector in ((n, u, 1, False), (n, GaussianKernelDensity([1.0, 2.0]), 1, False), (n, ExponentialDistribution(2), 1, True),
                                (LogNormalDistribution(0, 1), u, 1, True), (MultivariateDistribution([n]), u, 1, True),
                                (MultivariateDistribution([n, u, n]), MultivariateDistribution([u, u, u]), 3, True)):
        m, _, _ = two_state(da, db)
        m.bake()
        f = m.flat
        assert m.n_dim == f["n_dim"] == dim
        assert bool(f["comp_kind"].size) == vector and f["comp_kind"].size == f["comp_w"].size == (2 * dim if vector else 0)
        assert f["comp_param"].size == 3 * f["comp_kind"].size
        assert list(f["kind"][:2]) == ([4, 4] if vector else [da.kind, db.kind])
        assert f["comp_kind"].dtype == np.int32 and f["comp_param"].dtype == f["comp_w"].dtype == np.float64


def test_flat_tables_entry_by_entry():
    n1, u, ln, ex = NormalDistribution(3.0, 2.0), UniformDistribution(-1.0, 4.0), LogNormalDistribution(0.5, 0.25), ExponentialDistribution(4.0)
    m, a, b = two_state(MultivariateDistribution([n1, ln, ex], [1.0, 0.5, 2.0]), MultivariateDistribution([u, n1, ln]))
    m.bake()
    f = m.flat
    assert [s.name for s in m.states[:2]] == ["a", "b"] and f["n_emit"] == 2 and f["n_dim"] == 3
    assert list(f["kind"]) == [4, 4, 0, 0]
    assert list(f["comp_kind"]) == [1, 5, 6, 2, 1, 5]
    assert list(f["comp_w"]) == [1.0, 0.5, 2.0, 1.0, 1.0, 1.0]
    tn = (3.0, 1.0 / (2.0 * 2.0 * 2.0), -(math.log(2.0) + LSQ))
    tl = (0.5, 1.0 / (2.0 * 0.25 * 0.25), -(math.log(0.25) + LSQ))
    te = (0.0, 4.0, math.log(4.0))
    tu = (-1.0, 4.0, -math.log(5.0))
    assert list(f["comp_param"]) == list(tn + tl + te + tu + tn + tl)
    assert not f["param"].any() and f["param"].size == 3 * f["n_states"]          # (not read for a vector model)
    assert f["kde_pt"].size == 0 and list(f["kde_ptr"]) == [0, 0, 0]
    # a plain state of a D = 1 vector model is one component of weight 1
    m, a, b = two_state(n1, ex)
    m.bake()
    f = m.flat
    assert list(f["comp_kind"]) == [1, 6] and list(f["comp_w"]) == [1.0, 1.0] and list(f["comp_param"]) == list(tn + te)
    # the ctypes view carries the tables
    c = m._c_model()
    assert c.n_dim == 1 and c.comp_kind == f["comp_kind"].ctypes.data and c.comp_param == f["comp_param"].ctypes.data \
        and c.comp_w == f["comp_w"].ctypes.data


def test_univariate_flat_is_unchanged():
    """A model of normal, uniform and kernel-density states: every array the parent compiled, value for value from the
    formulas, the new ones empty, n_dim 1, and no table pointer in the C view."""
    n1, u, k = NormalDistribution(3.0, 2.0), UniformDistribution(-1.0, 4.0), GaussianKernelDensity([1.0, 4.0], 0.5, [1, 3])
    m = Model("uni")
    a, b, c = State(n1, "a"), State(u, "b"), State(k, "c")
    for s, t, p in ((m.start, a, 1.0), (a, b, 0.5), (a, c, 0.5), (b, c, 1.0), (c, a, 0.25), (c, m.end, 0.75)):
        m.add_transition(s, t, p)
    m.bake()
    f = m.flat
    assert sorted(f) == sorted(["n_states", "n_emit", "n_levels", "start", "end", "finite", "n_dim", "kind", "level_ptr", "param",
                                "in_ptr", "in_src", "in_lp", "out_ptr", "out_dst", "out_lp", "kde_ptr", "kde_pt", "kde_lw",
                                "comp_kind", "comp_param", "comp_w"])
    assert (f["n_states"], f["n_emit"], f["n_levels"], f["start"], f["end"], f["finite"], f["n_dim"]) == (5, 3, 1, 3, 4, 1, 1)
    assert list(f["kind"]) == [1, 2, 3, 0, 0] and list(f["level_ptr"]) == [3, 5]
    assert list(f["param"]) == [3.0, 0.125, -(math.log(2.0) + LSQ), -1.0, 4.0, -math.log(5.0),
                                math.fsum([1.0 * 0.25, 4.0 * 0.75]), 2.0, -(math.log(0.5) + LSQ)] + [0.0] * 6
    assert list(f["kde_ptr"]) == [0, 0, 0, 2] and list(f["kde_pt"]) == [1.0, 4.0] and list(f["kde_lw"]) == [math.log(0.25), math.log(0.75)]
    assert list(f["in_ptr"]) == [0, 2, 3, 5, 5, 6] and list(f["in_src"]) == [2, 3, 0, 0, 1, 2]
    assert list(f["in_lp"]) == [math.log(0.25), 0.0, math.log(0.5), math.log(0.5), 0.0, math.log(0.75)]
    assert list(f["out_ptr"]) == [0, 2, 3, 5, 6, 6] and list(f["out_dst"]) == [1, 2, 2, 0, 4, 0]
    assert list(f["out_lp"]) == [math.log(0.5), math.log(0.5), 0.0, math.log(0.25), math.log(0.75), 0.0]
    for key in ("comp_kind", "comp_param", "comp_w"):
        assert f[key].size == 0
    cm = m._c_model()
    assert cm.n_dim == 1 and cm.comp_kind is None and cm.comp_param is None and cm.comp_w is None and cm.kde_pt == f["kde_pt"].ctypes.data


def test_sequences_shapes():
    n = NormalDistribution(0, 1)
    m3, _, _ = two_state(MultivariateDistribution([n, n, n]), MultivariateDistribution([n, n, n]))
    m3.bake()
    got = m3._sequences([[(1, 2, 3), (4, 5, 6)], [], np.zeros((0, 3)), np.ones((4, 3), np.float32)])
    assert [s.shape for s in got] == [(2, 3), (0, 3), (0, 3), (4, 3)] and all(s.dtype == np.float64 for s in got)
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((2, 3, 1)), [1.0, 2.0]):
        with pytest.raises(ValueError, match="n_dim = 3"):
            m3._sequences([bad])
    with pytest.raises(ValueError, match="n_dim = 3"):
        m3.train([np.zeros(4)], verbose=False)
    m1, _, _ = two_state(MultivariateDistribution([n]), ExponentialDistribution(1))
    m1.bake()
    assert [s.shape for s in m1._sequences([np.zeros(3), np.zeros((3, 1)), []])] == [(3,), (3,), (0,)]
    with pytest.raises(ValueError, match="1-D"):
        m1._sequences([np.zeros((3, 2))])
    plain, _, _ = two_state(n, n)
    plain.bake()
    with pytest.raises(ValueError, match="1-D"):                               # a univariate model is as strict as before
        plain._sequences([np.zeros((3, 1))])


# ---- the oracle against brute force -----------------------------------------------------------------------------------
def tiny_vector(rng, letters, finite, silent_chain):
    """hmm_oracle.random_tiny's graph with vector states of components `letters` (rotated per state)."""
    plain = O.random_tiny(rng, finite, silent_chain)
    twin = {id(plain.start): None}
    m = Model("tinyv")
    twin[id(plain.start)], twin[id(plain.end)] = m.start, m.end
    k = 0
    for s in plain._added:
        if id(s) in twin:
            continue
        d = None
        if s.distribution is not None:
            d = MV.random_state_distribution(rng, MV.cycle(letters, k))
            k += 1
        twin[id(s)] = State(d, s.name)
    for (a, b), p in plain._edges.items():
        m.add_transition(twin[id(a)], twin[id(b)], p)
    m.bake()
    return m


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= tol, err.max()


@pytest.mark.parametrize("seed", range(12))
def test_oracle_against_brute_force(seed):
    rng = np.random.default_rng(900 + seed)
    letters = ("n", "e", "l", "nu", "le", "nle", "uel", "lnu")[seed % 8]
    model = tiny_vector(rng, letters, finite=seed % 2 == 0, silent_chain=seed % 3 != 0)
    assert model.n_dim == len(letters) and model._vector
    for n in range(5):
        seq = MV.draw(rng, letters, n)
        if n == 3 and "u" not in letters:
            seq = np.array(seq)
            seq.reshape(n, -1)[1, letters.find("l") if "l" in letters else 0] *= -1.0      # may be impossible for l / e
        F, logp, best, path = MV.brute_force(model, seq)
        close(MV.forward(model, seq), F, 1e-12)
        close([MV.log_probability(model, seq)], [logp], 1e-12)
        lp, vpath, gap, ties, _ = MV.viterbi_ties(model, seq)
        close([lp], [best], 1e-12)
        if path is not None and ties == 0 and gap > 1e-9:
            assert vpath == path
        B = MV.backward(model, seq)
        close([B[0][model.flat["start"]]], [logp], 1e-12)
        if "l" not in letters:                                              # the flat-array restatement, same programme
            elp, epath, mat = MV.viterbi_exact(model, seq)
            close([elp], [lp], 1e-12)
            c = MV.Compiled(model)
            close(mat, O._forward_like(c, c.bind(seq), True)[0], 1e-12)
            if ties == 0 and gap > 1e-9:
                assert epath == vpath
    with pytest.raises(ValueError):
        MV.viterbi_exact(MV.line_model(3, "nl"), np.ones((2, 2)))


def test_estep_oracle_against_path_enumeration():
    """W and (A_d, B_d) by weighting every complete path's emissions with the path's posterior."""
    rng = np.random.default_rng(5)
    for seed, letters in enumerate(("nl", "e", "nle")):
        model = tiny_vector(np.random.default_rng(40 + seed), letters, finite=True, silent_chain=seed == 1)
        seq = MV.draw(rng, letters, 4)
        c = MV.Compiled(model)
        E, dev = MV.table(model, seq), MV.deviations(model, seq)
        paths = []

        def walk(k, t, lp, emitted):
            if t == 4 and k == c.end:
                paths.append((lp, emitted))
            for l, w in c.outs[k]:
                if l < c.NE:
                    if t < 4 and E[t, l] > -np.inf:
                        walk(l, t + 1, lp + w + E[t, l], emitted + [(t, l)])
                else:
                    walk(l, t, lp + w, emitted)

        walk(c.start, 0, 0.0, [])
        counts, stats, logp = MV.estep_one(model, seq)
        if not paths:
            assert logp == -np.inf
            continue
        total = O.lse_rows(np.array([p[0] for p in paths])[None, :])[0]
        want = np.zeros_like(stats)
        for lp, emitted in paths:
            w = math.exp(lp - total)
            for t, k in emitted:
                want[k, 0] += w
                want[k, 1::2] += w * dev[t, k]
                want[k, 2::2] += w * dev[t, k] ** 2
        close([logp], [total], 1e-12)
        close(stats, want, 1e-10)
        assert stats.shape == (c.NE, 1 + 2 * len(letters))


# ---- the M-step -------------------------------------------------------------------------------------------------------
def test_m_step_from_hand_made_statistics():
    shared = NormalDistribution(2.0, 1.0)              # in two states and two slots
    ln, ex, ex_stuck, u = LogNormalDistribution(0.5, 0.4), ExponentialDistribution(2.0), ExponentialDistribution(3.0), UniformDistribution(0, 9)
    tight = NormalDistribution(1.0, 0.5)
    da = MultivariateDistribution([shared, ln, ex])
    db = MultivariateDistribution([tight, shared, ex_stuck], [1.0, 2.0, 0.5])
    m, a, b = two_state(da, db)
    frozen_part = NormalDistribution(7.0, 1.0)
    frozen = MultivariateDistribution([frozen_part, u, LogNormalDistribution(0.0, 1.0)])
    frozen.freeze()
    c = State(frozen, "c")
    m.add_transition(b, c, 0.2)
    m.add_transition(c, m.end, 1.0)
    m.bake()
    assert [s.name for s in m.states[:3]] == ["a", "b", "c"]
    stats = np.array([[4.0, 2.0, 5.0, -0.8, 0.4, 8.0, 20.0],           # a: W, (A, B) of shared, ln, ex
                      [1.0, 0.3, 0.09, 1.0, 3.0, -1.0, 2.0],           # b: tight (variance 0 -> min_std), shared, ex_stuck (A <= 0)
                      [3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])            # c: frozen
    counts = np.ones(len(m.edges))
    before = {id(d): list(d.parameters) for d in (ex_stuck, u, frozen_part, frozen.parameters[0][2])}
    m._m_step(counts, stats, min_std=0.05)
    W, A, B = 5.0, 3.0, 8.0                                             # shared: pooled over a slot 0 and b slot 1
    assert shared.parameters == [2.0 + A / W, math.sqrt(B / W - (A / W) ** 2)]
    assert ln.parameters == [0.5 + (-0.8 / 4.0), math.sqrt(0.4 / 4.0 - (-0.8 / 4.0) ** 2)]
    assert ex.parameters == [4.0 / 8.0]
    assert tight.parameters == [1.0 + 0.3, 0.05]                        # sqrt(max(0.09 - 0.09, 0)) floored by min_std
    for d in (ex_stuck, u, frozen_part, frozen.parameters[0][2]):
        assert d.parameters == before[id(d)]
    f = m.flat                                                          # recompiled: the tables hold the new values
    assert f["comp_param"][0] == shared.parameters[0] and f["comp_param"][3 * 4] == shared.parameters[0]
    assert f["comp_param"][3 * 2 + 1] == 0.5 and f["comp_param"][3 * 2 + 2] == math.log(0.5) and f["comp_param"][3 * 2] == 0.0
    assert list(f["comp_w"]) == [1.0, 1.0, 1.0, 1.0, 2.0, 0.5, 1.0, 1.0, 1.0]
    # the oracle's M-step is the same rule, and inertia mixes old and new
    m2, _, _ = two_state(MultivariateDistribution([NormalDistribution(2.0, 1.0), ExponentialDistribution(2.0)]),
                         MultivariateDistribution([NormalDistribution(0.0, 1.0), ExponentialDistribution(1.0)]))
    m2.bake()
    st = np.array([[4.0, 2.0, 5.0, 8.0, 20.0], [2.0, -1.0, 3.0, 1.0, 2.0]])
    twin, _, _ = MV.train(m2, [], 0)
    m2._m_step(np.arange(1.0, len(m2.edges) + 1), st, distribution_inertia=0.25, edge_inertia=0.5)
    MV.m_step(twin, np.arange(1.0, len(m2.edges) + 1), st, distribution_inertia=0.25, edge_inertia=0.5)
    for s, t in zip(m2.states[:2], twin.states[:2]):
        for (d, _), (e, _) in zip(MV.parts(s.distribution), MV.parts(t.distribution)):
            assert d.parameters == pytest.approx(e.parameters, rel=1e-15)
    assert m2.states[0].distribution.parameters[0][1].parameters == [0.25 * 2.0 + 0.75 * (4.0 / 8.0)]
    assert [p for _, _, p in m2.edges] == pytest.approx([p for _, _, p in twin.edges], rel=1e-15)
    with pytest.raises(ValueError, match="statistics"):
        m2._m_step(np.zeros(len(m2.edges)), np.zeros((2, 3)))


def test_viterbi_counts_on_the_host(monkeypatch):
    """Viterbi training's statistics for a vector model: weight 1 per consumed observation, log x for a log-normal slot."""
    m, a, b = two_state(MultivariateDistribution([NormalDistribution(1.0, 1.0), LogNormalDistribution(0.5, 1.0)]),
                        MultivariateDistribution([ExponentialDistribution(2.0), NormalDistribution(4.0, 1.0)]))
    m.bake()
    ix = {id(s): i for i, s in enumerate(m.states)}
    paths = [[m.start, a, a, b, m.end], None]
    monkeypatch.setattr(m, "viterbi_batch", lambda seqs, device=None: [
        (-3.0, [(ix[id(s)], s) for s in paths[0]]), (-np.inf, None)])
    x = np.array([[0.5, 2.0], [2.0, 3.0], [5.0, 3.0]])
    est = m._viterbi_counts([x, np.ones((1, 2))])
    assert est.skipped == 1 and list(est.logp) == [-3.0, -np.inf] and est.stats.shape == (2, 5)
    la, lb = math.log(2.0) - 0.5, math.log(3.0) - 0.5
    close(est.stats[ix[id(a)]], [2, (0.5 - 1) + (2 - 1), 0.25 + 1, la + lb, la * la + lb * lb], 1e-15)
    close(est.stats[ix[id(b)]], [1, 5.0, 25.0, 3.0 - 4.0, 1.0], 1e-15)
    assert est.counts.sum() == 4


# ---- features= --------------------------------------------------------------------------------------------------------
class Recorder(object):
    """A duck-typed HMM that records what it is handed."""

    def __init__(self):
        self.seen = []

    def viterbi(self, x):
        self.seen.append(x)
        return -1.0, [(0, State(None, "s"))] * (len(x) + 1)

    forward = log_probability = viterbi


def segments(rng, n):
    from pypore_amd.core import Segment
    return [Segment(current=rng.normal(40, 1 + i, 50 + 10 * i), start=100 * i, duration=0.001 * (i + 1)) for i in range(n)]


def test_features_on_event_metaevent_and_experiment():
    from pypore_amd.DataTypes import Event, Experiment, MetaEvent
    rng = np.random.default_rng(3)
    segs = segments(rng, 5)
    ev = Event(current=np.zeros(10), segments=segs)
    meta = MetaEvent(segments=segs, duration=1.0)
    want3 = np.array([(s.mean, s.std, s.duration) for s in segs])
    for holder in (ev, meta):
        rec = Recorder()
        holder.apply_hmm(rec)
        holder.apply_hmm(rec, 'viterbi', ('mean', 'std', 'duration'))
        holder.apply_hmm(rec, algorithm='forward', features=['duration', 'mean'])
        assert rec.seen[0].shape == (5,) and np.array_equal(rec.seen[0], want3[:, 0])
        assert rec.seen[1].shape == (5, 3) and rec.seen[1].dtype == np.float64 and np.array_equal(rec.seen[1], want3)
        assert np.array_equal(rec.seen[2], want3[:, [2, 0]])
        with pytest.raises(ValueError, match="tuple"):
            holder.apply_hmm(rec, features='mean')
    n = NormalDistribution(40, 5)
    vec, _, _ = two_state(MultivariateDistribution([n, n, ExponentialDistribution(1)]), MultivariateDistribution([n, n, ExponentialDistribution(2)]))
    vec.bake()
    uni, _, _ = two_state(n, n)
    uni.bake()
    for holder in (ev, meta):
        with pytest.raises(ValueError, match="features"):
            holder.apply_hmm(vec)
        with pytest.raises(ValueError, match="n_dim = 3"):
            holder.apply_hmm(vec, features=('mean', 'std'))
        with pytest.raises(ValueError, match="n_dim = 1"):
            holder.apply_hmm(uni, features=('mean', 'std'))
    exp = Experiment([])

    class F(object):
        events = [Event(current=np.zeros(10), segments=segments(rng, k)) for k in (3, 0, 4)]
    exp.files = [F()]
    rec = Recorder()
    out = exp.apply_hmm(rec, features=('mean', 'duration'), indices=[0, 2])
    assert [x.shape for x in rec.seen] == [(3, 2), (4, 2)] and len(out) == 4 + 5
    assert np.array_equal(rec.seen[1], [(s.mean, s.duration) for s in F.events[2].segments])
    rec = Recorder()
    exp.apply_hmm(rec)
    assert [x.shape for x in rec.seen] == [(3,), (0,), (4,)]
    with pytest.raises(ValueError, match="features"):
        exp.apply_hmm(vec)
    calls = []
    vec.viterbi_batch = lambda seqs: calls.append(seqs) or [(-1.0, [(0, None)]) for _ in seqs]
    exp.apply_hmm(vec, features=('mean', 'std', 'duration'))
    assert len(calls) == 1 and [x.shape for x in calls[0]] == [(3, 3), (0, 3), (4, 3)]


def test_parse_hands_features_to_the_merge(monkeypatch):
    from pypore_amd.DataTypes import Event
    rng = np.random.default_rng(4)
    ev = Event(current=np.zeros(10), segments=segments(rng, 4))
    ev.second = 1.0
    monkeypatch.setattr(ev, "_segment", lambda parser: None)
    rec = Recorder()
    ev.parse(parser=object(), hmm=rec, features=('mean', 'std'))
    assert len(rec.seen) == 1 and rec.seen[0].shape == (4, 2)


# ---- no near ties on the log-normal inputs of the GPU tests -----------------------------------------------------------
def test_no_near_tie_on_any_log_normal_input():
    """The GPU tests compare Viterbi paths on these inputs without leaving any out; that is sound only if the oracle
    alone shows every decision on the winning path decided by more than 1e-9 relative, and no exact tie."""
    smallest, count = np.inf, 0
    for name, model, seqs in MV.lognormal_cases():
        assert 5 in model.flat["comp_kind"], name
        for q, seq in enumerate(seqs):
            lp, path, gap, ties, _ = MV.viterbi_ties(model, seq)
            count += 1
            if path is None:
                continue
            smallest = min(smallest, gap)
            assert ties == 0 and gap > 1e-9, (name, q, gap, ties)
    print("%d inputs, smallest margin %.3g" % (count, smallest))
    assert count >= 30
