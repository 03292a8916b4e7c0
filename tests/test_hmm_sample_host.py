"""HMM sampling on the host (no GPU): the random stream's known answers, the sampling tables of Model._sample_tables
against their restatement in tests/sample_oracle.py, the argument errors of sample / sample_batch, and Distribution.sample
of every class against the distribution's own moments.

yahmm is not available to compare against; nothing here is compared with it."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_models as SM  # noqa: E402
import sample_oracle as SO  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution, Model,  # noqa: E402
                            MultivariateDistribution, NormalDistribution, State, UniformDistribution)

FLAT_KEYS = {"n_states", "n_emit", "n_levels", "start", "end", "finite", "n_dim", "kind", "level_ptr", "param", "in_ptr",
             "in_src", "in_lp", "out_ptr", "out_dst", "out_lp", "kde_ptr", "kde_pt", "kde_lw", "comp_kind", "comp_param", "comp_w"}


def words(text):
    return tuple(int(w, 16) for w in text.split())


@pytest.mark.parametrize("counter, key, out", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, out):
    assert SO.philox(words(counter), words(key)) == words(out)


def test_the_two_uniforms_of_a_block_by_hand():
    # r0 = 0x6627e8d5: r0 >> 5 = 0x3313f46;  r1 = 0xe169c58d: r1 >> 6 = 0x385a716
    r = words("6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    assert (r[0] >> 5, r[1] >> 6, r[2] >> 5, r[3] >> 6) == (0x3313f46, 0x385a716, 0x5e2bd62, 0x26c036f)
    u0, u1 = SO.uniforms(r)
    assert u0 == (0x3313f46 * 67108864 + 0x385a716) / 9007199254740992.0
    assert u1 == (0x5e2bd62 * 67108864 + 0x26c036f) / 9007199254740992.0
    assert 0.0 <= u0 < 1.0 and 0.0 <= u1 < 1.0
    assert SO.uniforms((0xffffffff,) * 4) == (1.0 - 2.0 ** -53,) * 2 and SO.uniforms((0, 0, 31, 63)) == (0.0, 0.0)
    # the block of (seed, Q, j): the key is the seed's halves, the counter (j, Q) in halves, low word first
    seed, Q, j = 0xa4093822 | (0x299f31d0 << 32), 0x13198a2e | (0x03707344 << 32), 0x243f6a88 | (0x85a308d3 << 32)
    assert SO.block(seed, Q, j) == SO.uniforms(words("d16cfe09 94fdcceb 5001e420 24126ea1"))


@pytest.mark.parametrize("name", ["kde", "vector3", "silent", "phi29"])
def test_sample_tables_equal_the_oracles(name):
    m = SM.MODELS[name][0]()
    keys = set(m.flat)
    got, want = m._sample_tables(), SO.tables(m)
    f = m.flat
    assert set(f) == keys == FLAT_KEYS                                        # flat has gained no key
    for k in ("out_cdf", "emit_param", "kde_cdf"):
        assert got[k].dtype == np.float64 and got[k].tolist() == want[k], k
    assert got["out_cdf"].size == f["out_lp"].size and got["kde_cdf"].size == f["kde_pt"].size
    assert got["emit_param"].size == 2 * f["n_emit"] * f["n_dim"]
    for cdf, ptr in ((got["out_cdf"], f["out_ptr"]), (got["kde_cdf"], f["kde_ptr"])):
        for k in range(ptr.size - 1):
            if ptr[k + 1] > ptr[k]:
                row = cdf[ptr[k]:ptr[k + 1]]
                assert row[-1] == 1.0 and np.all(np.diff(row[:-1]) >= 0) and np.all(row[:-1] >= 0)
    assert m._sample_tables() is got                                          # cached
    c = got["c"]
    assert (c.n_cdf, c.n_param, c.n_kde) == (got["out_cdf"].size, got["emit_param"].size, got["kde_cdf"].size)
    assert c.out_cdf == got["out_cdf"].ctypes.data and c.emit_param == got["emit_param"].ctypes.data
    assert c.kde_cdf == (got["kde_cdf"].ctypes.data if got["kde_cdf"].size else None)


def test_sample_tables_by_hand_and_after_a_change():
    m = SM.kde()
    f, t = m.flat, m._sample_tables()
    names = [s.name for s in m.states[:f["n_emit"]]]
    assert names == ["k1", "k7", "n", "un"]
    assert t["emit_param"].tolist() == [0.0, 0.7, 0.0, 0.4, -4.0, 1.0, 20.0, 10.0]
    assert f["kde_ptr"].tolist() == [0, 1, 7, 7, 7] and t["kde_cdf"][0] == 1.0 and t["kde_cdf"][6] == 1.0      # weight 0 left out
    w = np.exp(f["kde_lw"][1:7])
    assert t["kde_cdf"][1] == w[0] and t["kde_cdf"][3] == (w[0] + w[1]) + w[2]
    v = SM.vector3()
    assert v._sample_tables()["emit_param"].reshape(3, 3, 2).tolist() == [
        [[40.0, 3.0], [0.5, 2.0], [-1.0, 0.5]], [[0.0, 0.25], [1.0, 0.2], [-1.0, 2.0]], [[3.0, 0.25], [0.0, 40.0], [0.0, 10.0]]]
    # a retrained model compiles new tables (the M-step derives the flat arrays again)
    c = SM.chain4()
    before = c._sample_tables()
    c._m_step(np.ones(len(c.edges)), np.zeros((4, 3)))
    after = c._sample_tables()
    assert after is not before and after["out_cdf"].tolist() == SO.tables(c)["out_cdf"] != before["out_cdf"].tolist()


def test_argument_errors():
    raw = Model("raw")
    raw.add_transition(raw.start, State(NormalDistribution(0, 1), "a"), 1.0)
    for call in (lambda: raw.sample(), lambda: raw.sample_batch(3), lambda: raw._sample_tables()):
        with pytest.raises(ValueError, match="not baked"):
            call()
    r = SM.ring()
    with pytest.raises(ValueError, match="must specify a length"):
        r.sample()
    with pytest.raises(ValueError, match="must specify a length"):
        r.sample_batch(4, length=0)
    c = SM.chain4()
    for kw in (dict(n=-1), dict(n=2, length=-1), dict(n=2, first=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            c.sample_batch(**kw)
    with pytest.raises(ValueError, match="max_length"):
        c.sample_batch(2, max_length=0)
    with pytest.raises(ValueError, match=">= 0"):
        c.sample(length=-3)
    from pypore_amd import _lib, engine
    assert "ps_hmm_sample" in _lib.EXPORTS and callable(engine.Context.hmm_sample)


def moments(d):
    """(mean, variance, fourth central moment) of a univariate distribution, from its parameters."""
    a = d.parameters
    if isinstance(d, NormalDistribution):
        return a[0], a[1] ** 2, 3 * a[1] ** 4
    if isinstance(d, UniformDistribution):
        w = a[1] - a[0]
        return 0.5 * (a[0] + a[1]), w * w / 12, w ** 4 / 80
    if isinstance(d, ExponentialDistribution):
        return 1 / a[0], 1 / a[0] ** 2, 9 / a[0] ** 4
    if isinstance(d, LogNormalDistribution):
        raw = [math.exp(k * a[0] + 0.5 * k * k * a[1] ** 2) for k in range(5)]       # E x^k
        mu = raw[1]
        return mu, raw[2] - mu * mu, raw[4] - 4 * mu * raw[3] + 6 * mu * mu * raw[2] - 3 * mu ** 4
    points, h, w = a                                                                 # a mixture of normals N(p_i, h)
    mu = sum(wi * p for p, wi in zip(points, w))
    var = sum(wi * (h * h + (p - mu) ** 2) for p, wi in zip(points, w))
    m4 = sum(wi * (3 * h ** 4 + 6 * h * h * (p - mu) ** 2 + (p - mu) ** 4) for p, wi in zip(points, w))
    return mu, var, m4


def check_moments(x, d, n=20000):
    mu, var, m4 = moments(d)
    assert x.shape == (n,) and np.all(np.isfinite(x))
    assert abs(x.mean() - mu) <= 5 * math.sqrt(var / n), (d, x.mean(), mu)
    assert abs(x.var(ddof=1) - var) <= 5 * math.sqrt((m4 - var * var) / n), (d, x.var(ddof=1), var)


UNIVARIATE = [NormalDistribution(3.0, 4.0), UniformDistribution(-2.0, 5.5), LogNormalDistribution(0.3, 0.4),
              ExponentialDistribution(2.5), GaussianKernelDensity([1.0, 4.0, 9.0], bandwidth=0.5, weights=[1, 2, 5])]


@pytest.mark.parametrize("d", UNIVARIATE, ids=lambda d: type(d).__name__)
def test_distribution_sample_has_the_distributions_moments(d):
    rng = np.random.default_rng(20260101)
    draws = [d.sample(rng) for _ in range(20000)]
    assert all(type(v) is float for v in draws[:5])
    x = np.array(draws)
    check_moments(x, d)
    if isinstance(d, UniformDistribution):
        assert x.min() >= d.parameters[0] and x.max() <= d.parameters[1]
    if isinstance(d, GaussianKernelDensity):
        pts, h = np.array(d.parameters[0]), d.parameters[1]
        assert np.all(np.abs(x[:, None] - pts[None, :]).min(axis=1) <= 8 * h)
    if isinstance(d, (LogNormalDistribution, ExponentialDistribution)):
        assert x.min() >= 0
    assert isinstance(d.sample(), float)                                      # rng=None: a generator of its own


def test_multivariate_sample_draws_every_component_and_ignores_the_weights():
    parts = UNIVARIATE[:4]
    rng = np.random.default_rng(7)
    rows = np.array([MultivariateDistribution(parts, [0.25, 3.0, 1.5, 2.0]).sample(rng) for _ in range(20000)])
    assert rows.shape == (20000, 4)
    for c, d in enumerate(parts):
        check_moments(rows[:, c], d)
    # the weights take no part: the same generator state gives the same draws whatever they are
    a = MultivariateDistribution(parts, [0.25, 3.0, 1.5, 2.0]).sample(np.random.default_rng(11))
    b = MultivariateDistribution(parts).sample(np.random.default_rng(11))
    assert a == b and isinstance(a, list) and len(a) == 4
