"""MixtureDistribution on the host (no GPU): the constructor, the log density and the responsibilities against
tests/mixture_oracle.py, the tables Model.bake() builds beside `flat` (Model._mix) written out by hand, the refusals, the
M-step on hand-made statistics, the oracle against its own brute force on the tiny models, and the condition under which
tests/test_mixture_gpu.py demands equal Viterbi paths: the oracle alone shows that no path decision of those inputs lies
within 1e-9."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixture_oracle as MX  # noqa: E402

from pypore_amd import hmm as H  # noqa: E402
from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution,  # noqa: E402
                            MixtureDistribution, Model, MultivariateDistribution, NormalDistribution, State,
                            UniformDistribution)

NEG = float("-inf")


def close(got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= tol * np.maximum(1.0, np.abs(want[fin]))))


# ---- the distribution -------------------------------------------------------------------------------------------------
def test_constructor_errors_and_normalisation():
    n, u = NormalDistribution(0, 1), UniformDistribution(0, 1)
    assert H.KIND_MIXTURE == 7 and MixtureDistribution.kind == 7
    d = MixtureDistribution([n, u, n], [2, 0, 6])
    assert d.parameters[0] == [n, u, n] and d.parameters[1] == [0.25, 0.0, 0.75] and d.parameters[0][0] is n
    assert MixtureDistribution([n, u]).parameters[1] == [0.5, 0.5]
    assert MixtureDistribution([LogNormalDistribution(0, 1), ExponentialDistribution(2)]).parameters[1] == [0.5, 0.5]
    for bad, message in (([], "at least one"), ([GaussianKernelDensity([1.0])], "GaussianKernelDensity"),
                         ([MultivariateDistribution([n])], "MultivariateDistribution"),
                         ([MixtureDistribution([n])], "MixtureDistribution cannot be a component"), ([3.0], "component must be")):
        with pytest.raises(ValueError, match=message):
            MixtureDistribution(bad)
    for w, message in (([1.0], "1 weights for 2"), ([1.0, -1.0], ">= 0"), ([1.0, np.inf], "finite"), ([np.nan, 1.0], "finite"),
                       ([0.0, 0.0], "some weight > 0")):
        with pytest.raises(ValueError, match=message):
            MixtureDistribution([n, u], w)
    with pytest.raises(ValueError, match="MixtureDistribution cannot be a component of a MultivariateDistribution"):
        MultivariateDistribution([n, MixtureDistribution([n])])


MIX = MixtureDistribution([NormalDistribution(1.0, 0.5), UniformDistribution(0.0, 2.0), LogNormalDistribution(0.2, 0.4),
                           ExponentialDistribution(1.5), NormalDistribution(-3.0, 1.0)], [0.3, 0.2, 0.25, 0.0, 0.25])


@pytest.mark.parametrize("x", [0.5, 1.0, 2.5, 0.0, -0.5, -3.0, 40.0, -40.0, 1e-300])
def test_log_probability_and_responsibilities_against_the_oracle(x):
    """The zero-weight exponential never counts; the uniform excludes 2.5 and the negatives; the log-normal x <= 0."""
    want = MX.emission(MIX, x)
    assert math.isfinite(want) and close([MIX.log_probability(x)], [want])
    r = MIX.responsibilities(x)
    assert close(r, MX.responsibilities(MIX, x)) and r[3] == 0.0 and abs(math.fsum(r) - 1.0) <= 1e-12
    terms = MX.terms(MIX, x)
    assert (r[1] == 0.0) == (not 0.0 <= x <= 2.0) and (terms[2] == NEG) == (not x > 0) and (x > 0 or r[2] == 0.0)
    assert terms[3] == NEG and close([math.exp(t - want) if t > NEG else 0.0 for t in terms], r)


def test_every_term_impossible_gives_minus_infinity_never_nan():
    d = MixtureDistribution([UniformDistribution(0, 1), LogNormalDistribution(0, 1), ExponentialDistribution(1.0),
                             NormalDistribution(0, 1)], [1, 1, 1, 0])
    for x in (-1.0, -1e300):
        assert d.log_probability(x) == NEG == MX.emission(d, x) and d.responsibilities(x) == [0.0] * 4
    assert math.isfinite(d.log_probability(0.5)) and math.isfinite(d.log_probability(1e300))   # (far out, not impossible)


def test_one_component_of_weight_one_gives_its_own_bits():
    rng = np.random.default_rng(0)
    for c in (NormalDistribution(3.0, 1.7), UniformDistribution(-1.0, 2.0), LogNormalDistribution(0.3, 0.9), ExponentialDistribution(0.37)):
        d = MixtureDistribution([c])
        for x in rng.normal(1.0, 3.0, 50).tolist() + [0.0, -1.0, 2.0]:
            assert d.log_probability(x) == c.log_probability(x)
            assert d.responsibilities(x) == [1.0 if c.log_probability(x) > NEG else 0.0]
        two = MixtureDistribution([NormalDistribution(0, 1), c], [0, 5])
        assert all(two.log_probability(x) == c.log_probability(x) for x in (0.5, 1.5))


def test_sample_draws_from_the_components_by_weight_and_freeze():
    d = MixtureDistribution([NormalDistribution(-50.0, 1.0), UniformDistribution(10.0, 11.0), NormalDistribution(0.0, 1.0)], [1, 3, 0])
    rng = np.random.default_rng(5)
    x = np.array([d.sample(rng) for _ in range(4000)])
    assert ((x < -40) | ((x >= 10) & (x <= 11))).all() and abs(np.mean(x > 0) - 0.75) < 0.03
    assert isinstance(d.sample(), float) and not d.frozen
    d.freeze()
    assert d.frozen and [f for _, _, f in H._mixture_slots(d)] == [True] * 3 and not d.parameters[0][0].frozen
    d.thaw()
    d.parameters[0][1].freeze()
    assert [f for _, _, f in H._mixture_slots(d)] == [False, True, False]


# ---- the tables -------------------------------------------------------------------------------------------------------
def small_model():
    m = Model("small")
    a = State(MixtureDistribution([NormalDistribution(1.0, 0.5), UniformDistribution(0.0, 4.0), LogNormalDistribution(0.5, 0.25),
                                   ExponentialDistribution(2.0)], [1, 2, 1, 0]), "a")
    b = State(NormalDistribution(5.0, 2.0), "b")
    c = State(MixtureDistribution([ExponentialDistribution(0.5), NormalDistribution(2.0, 1.0), UniformDistribution(1.0, 3.0)],
                                  [0, 1, 0]), "c")
    d = State(GaussianKernelDensity([1.0, 2.0], 0.5), "d")
    for x, y, p in ((m.start, a, 0.5), (m.start, b, 0.5), (a, b, 0.5), (a, c, 0.5), (b, c, 0.5), (b, d, 0.5), (c, a, 0.5),
                    (c, m.end, 0.5), (d, a, 1.0)):
        m.add_transition(x, y, p)
    m.bake()
    return m


FLAT_KEYS = {"n_states", "n_emit", "n_levels", "start", "end", "finite", "n_dim", "kind", "level_ptr", "param", "in_ptr", "in_src",
             "in_lp", "out_ptr", "out_dst", "out_lp", "kde_ptr", "kde_pt", "kde_lw", "comp_kind", "comp_param", "comp_w"}


def test_mix_tables_written_out_by_hand():
    m = small_model()
    f, x = m.flat, m._mix
    s2pi = math.sqrt(2 * math.pi)
    assert set(f) == FLAT_KEYS and m.n_dim == 1 and not m._vector and m._n_mix == 7 and m._stat_width == 3
    assert f["kind"].tolist() == [7, 1, 7, 3, 0, 0] and f["kde_ptr"].tolist() == [0, 0, 0, 0, 2]
    assert f["param"][0:3].tolist() == [0.0, 0.0, 0.0] and f["param"][6:9].tolist() == [0.0, 0.0, 0.0] and f["param"][3] == 5.0
    assert set(x) == {"mix_ptr", "mix_kind", "mix_param", "mix_lw", "mix_cdf", "mix_draw"}
    assert x["mix_ptr"].dtype == np.int32 and x["mix_ptr"].tolist() == [0, 4, 4, 7, 7]
    assert x["mix_kind"].dtype == np.int32 and x["mix_kind"].tolist() == [1, 2, 5, 6, 6, 1, 2]
    want = [1.0, 1 / (2 * 0.25), -math.log(0.5 * s2pi), 0.0, 4.0, -math.log(4.0), 0.5, 1 / (2 * 0.0625), -math.log(0.25 * s2pi),
            0.0, 2.0, math.log(2.0), 0.0, 0.5, math.log(0.5), 2.0, 0.5, -math.log(s2pi), 1.0, 3.0, -math.log(2.0)]
    assert np.allclose(x["mix_param"], want, rtol=1e-15, atol=0) and x["mix_param"].size == 21
    assert x["mix_lw"].tolist() == [math.log(0.25), math.log(0.5), math.log(0.25), NEG, NEG, 0.0, NEG]
    # 1.0 from the last component of positive weight on: a trailing zero weight is never picked, nor a leading one
    assert x["mix_cdf"].tolist() == [0.25, 0.75, 1.0, 1.0, 0.0, 1.0, 1.0]
    assert x["mix_draw"].tolist() == [1.0, 0.5, 0.0, 4.0, 0.5, 0.25, 0.0, 2.0, 0.0, 0.5, 2.0, 1.0, 1.0, 2.0]
    c = m._c_model()
    assert c.mix_ptr == x["mix_ptr"].ctypes.data and c.mix_draw == x["mix_draw"].ctypes.data and c.mix_lw == x["mix_lw"].ctypes.data
    t = m._sample_tables()
    assert t["emit_param"].tolist() == [0.0, 0.0, 5.0, 2.0, 0.0, 0.0, 0.0, 0.5] and t["emit_param"].size == 2 * f["n_emit"]
    TB = MX.tables(m)
    assert TB["mix_cdf"] == x["mix_cdf"].tolist() and TB["mix_draw"] == x["mix_draw"].tolist() and TB["mix_ptr"] == x["mix_ptr"].tolist()
    assert TB["emit_param"] == t["emit_param"].tolist()


def test_a_model_without_mixture_states_is_as_it_was():
    import hmm_oracle as O
    m, _ = O.profile_model(5)
    assert set(m.flat) == FLAT_KEYS and m._n_mix == 0
    assert m._mix["mix_ptr"].tolist() == [0] * (m.flat["n_emit"] + 1) and all(m._mix[k].size == 0 for k in m._mix if k != "mix_ptr")
    c = m._c_model()
    assert not c.mix_ptr and not c.mix_kind and not c.mix_param and not c.mix_lw and not c.mix_cdf and not c.mix_draw


def test_bake_refuses_a_mixture_in_a_vector_model():
    for other in (MultivariateDistribution([NormalDistribution(0, 1)]), LogNormalDistribution(0, 1), ExponentialDistribution(1)):
        m = Model("v")
        a, b = State(MixtureDistribution([NormalDistribution(0, 1)]), "the-mixture"), State(other, "b")
        for x, y in ((m.start, a), (a, b), (b, m.end)):
            m.add_transition(x, y, 1.0)
        with pytest.raises(ValueError, match="the-mixture"):
            m.bake()
    # log-normal and exponential COMPONENTS do not make a vector model
    m = Model("s")
    a = State(MixtureDistribution([LogNormalDistribution(0, 1), ExponentialDistribution(1)]), "a")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, m.end, 1.0)
    m.bake()
    assert m.n_dim == 1 and not m._vector and m.flat["kind"][0] == 7 and m.flat["comp_kind"].size == 0


# ---- the M-step -------------------------------------------------------------------------------------------------------
def mstep_model():
    """s0 and s1 hold one mixture; s2's first component is s3's distribution; s4's mixture is frozen."""
    mix = MixtureDistribution([NormalDistribution(0.0, 1.0), NormalDistribution(4.0, 1.0), UniformDistribution(-9.0, 9.0)], [0.5, 0.25, 0.25])
    shared = NormalDistribution(10.0, 1.0)
    frozen = MixtureDistribution([NormalDistribution(20.0, 1.0), ExponentialDistribution(0.1)], [0.5, 0.5])
    frozen.freeze()
    ds = [mix, mix, MixtureDistribution([shared, LogNormalDistribution(2.0, 0.5), ExponentialDistribution(0.2)], [0.2, 0.3, 0.5]), shared, frozen]
    m = Model("mstep")
    st = [State(d, "s%d" % i) for i, d in enumerate(ds)]
    for s in st:
        m.add_transition(m.start, s, 1.0)
        m.add_transition(s, s, 0.5)
        m.add_transition(s, m.end, 0.5)
    m.bake()
    return m


def hand_stats(m):
    rng = np.random.default_rng(11)
    NE, n_mix = m.flat["n_emit"], m._n_mix
    stats = np.zeros((NE + n_mix, 3))
    stats[:, 0] = rng.uniform(0.5, 3.0, NE + n_mix)
    stats[:, 1] = rng.normal(0, 0.5, NE + n_mix) * stats[:, 0]
    stats[:, 2] = (rng.uniform(0.5, 2.0, NE + n_mix) + (stats[:, 1] / stats[:, 0]) ** 2) * stats[:, 0]
    return stats


def test_m_step_on_hand_made_statistics():
    m = mstep_model()
    NE, ptr = 5, m._mix["mix_ptr"].tolist()
    assert ptr == [0, 3, 6, 9, 9, 11] and m._n_mix == 11
    stats = hand_stats(m)
    stats[NE + 8, 1] = abs(stats[NE + 8, 1]) + 1.0                                  # the exponential slot: A > 0
    counts = np.ones(len(m.edges))
    rows = stats[NE:]
    mix, second, shared, frozen = (m.states[i].distribution for i in (0, 2, 3, 4))
    frozen_before = [list(d.parameters) for d in frozen.parameters[0]] + [list(frozen.parameters[1])]
    with pytest.raises(ValueError, match="statistics"):
        m._m_step(counts, stats[:NE])
    m._m_step(counts, stats, min_std=0.05)
    # weights pooled over the two states that hold the mixture
    W = rows[0:3, 0] + rows[3:6, 0]
    assert np.allclose(mix.parameters[1], W / W.sum(), rtol=1e-15) and abs(sum(mix.parameters[1]) - 1.0) < 1e-15
    # its first component, pooled over both slots: shift 0.0
    Wc, A, B = rows[0] + rows[3]
    assert np.allclose(mix.parameters[0][0].parameters, [A / Wc, math.sqrt(B / Wc - (A / Wc) ** 2)], rtol=1e-14)
    assert mix.parameters[0][2].parameters == [-9.0, 9.0]                           # uniform components stay
    # the component object shared with the plain state s3: the slot's row and the state's row, shift 10.0
    Wc, A, B = rows[6] + stats[3]
    assert np.allclose(shared.parameters, [10.0 + A / Wc, math.sqrt(B / Wc - (A / Wc) ** 2)], rtol=1e-14)
    assert second.parameters[0][0] is shared
    Wc, A, B = rows[7]                                                              # log-normal: mu and sigma of log x, shift 2.0
    assert np.allclose(second.parameters[0][1].parameters, [2.0 + A / Wc, math.sqrt(B / Wc - (A / Wc) ** 2)], rtol=1e-14)
    assert np.allclose(second.parameters[0][2].parameters, [rows[8, 0] / rows[8, 1]], rtol=1e-15)
    assert np.allclose(second.parameters[1], rows[6:9, 0] / rows[6:9, 0].sum(), rtol=1e-15)
    # a frozen mixture: neither its weights nor, in its slots, its components
    assert [list(d.parameters) for d in frozen.parameters[0]] + [list(frozen.parameters[1])] == frozen_before
    # the tables follow
    assert m._mix["mix_lw"][:3].tolist() == [math.log(w) for w in mix.parameters[1]]
    assert m._mix["mix_param"][0] == mix.parameters[0][0].parameters[0] and m.flat["param"][9] == shared.parameters[0]
    assert m._c is None and m._s is None


def test_m_step_against_the_oracle_with_inertia_and_zero_sums():
    for inertia in (0.0, 0.3):
        m, want = mstep_model(), mstep_model()
        stats = hand_stats(m)
        stats[5 + 8, 1] = abs(stats[5 + 8, 1]) + 1.0
        stats[5 + 6:5 + 9] = 0.0                                                    # sum W = 0 in s2's slots: its weights stay
        stats[5 + 1, 0] = stats[5 + 4, 0] = 0.0                                     # one pooled weight becomes 0
        stats[5 + 1, 1:] = stats[5 + 4, 1:] = 0.0
        counts = np.arange(1.0, len(m.edges) + 1)
        m._m_step(counts, stats, distribution_inertia=inertia, min_std=0.05)
        MX.m_step(want, counts, stats, distribution_inertia=inertia, min_std=0.05)
        for s, t in zip(m.states[:5], want.states[:5]):
            for (d, w), (e, v) in zip(MX.slots(s.distribution) or [(s.distribution, 1.0)], MX.slots(t.distribution) or [(t.distribution, 1.0)]):
                assert type(d) is type(e) and np.allclose(d.parameters, e.parameters, rtol=1e-14, atol=0) and abs(w - v) <= 1e-15
        assert np.allclose([p for _, _, p in m.edges], [p for _, _, p in want.edges], rtol=1e-15)
        assert m.states[2].distribution.parameters[1] == [0.2, 0.3, 0.5]
        w = m.states[0].distribution.parameters[1]
        if inertia == 0.0:                                                          # the slot stays, its log weight is -inf
            assert w[1] == 0.0 and m._mix["mix_lw"][1] == NEG and m._mix["mix_ptr"].tolist() == [0, 3, 6, 9, 9, 11]
            assert m._mix["mix_cdf"][:3].tolist() == [w[0], w[0], 1.0]
        else:
            assert abs(w[1] - 0.3 * 0.25) <= 1e-15


# ---- the oracle against its own brute force, and the Viterbi margins ---------------------------------------------------
@pytest.mark.parametrize("finite", [True, False])
def test_oracle_against_brute_force_on_the_tiny_models(finite):
    model = MX.tiny_model(finite)
    assert model.flat["n_emit"] == 3 and model._n_mix == 6
    some = 0
    for s in MX.TINY_SEQUENCES:
        F, logp, best, path = MX.brute_force(model, s)
        assert close(MX.forward(model, s), F) and close([MX.log_probability(model, s)], [logp])
        vlp, vpath = MX.viterbi_ties(model, s)[:2]
        assert close([vlp], [best]) and vpath == path
        counts, stats, lp = MX.estep_one(model, s)
        bc, bs, blp = MX.estep_brute_force(model, s)
        assert close([lp], [blp]) and close(counts, bc, 1e-11) and close(stats, bs, 1e-11)
        if lp > NEG and len(s):
            some += 1
            assert stats[3:, 0].sum() > 0
            # a mixture state's components share out its posterior: their W sum to the state's
            assert abs(stats[3:7, 0].sum() - stats[0, 0]) <= 1e-12 and abs(stats[7:9, 0].sum() - stats[2, 0]) <= 1e-12
            assert stats[3 + 2, 0] == 0.0                                            # the zero-weight slot
    assert some >= 3


@pytest.mark.parametrize("index", range(9))
def test_no_viterbi_decision_of_the_gpu_inputs_lies_within_1e_9(index):
    name, model, seqs = MX.viterbi_inputs()[index]
    possible = 0
    for s in seqs:
        lp, path, gap, ties, _ = MX.viterbi_ties(model, s)
        if path is not None:
            possible += 1
            assert ties == 0 and gap > 1e-9, (name, len(s), ties, gap)
    assert possible >= 2, name


def test_viterbi_training_shares_observations_out_by_responsibility():
    """Model._viterbi_counts' host part, on paths handed to it in place of the device's."""
    model = MX.tiny_model(True)
    seqs = [np.array(s, np.float64) for s in MX.TINY_SEQUENCES[1:5]]
    paths = [MX.viterbi_ties(model, s)[:2] for s in seqs]
    model.viterbi_batch = lambda sequences, device=None: [(lp, None if p is None else [(i, model.states[i]) for i in p]) for lp, p in paths]
    try:
        got = model._viterbi_counts(seqs)
    finally:
        del model.viterbi_batch
    counts, stats, scores, skipped = MX.viterbi_counts(model, seqs)
    assert got.stats.shape == (3 + 6, 3) and got.skipped == skipped
    assert close(got.counts, counts) and close(got.stats, stats, 1e-12) and stats[3:, 0].sum() > 0
