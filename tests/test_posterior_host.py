"""Posterior decoding on the host (no GPU): the numpy oracle of tests/posterior_oracle.py against brute-force path
enumeration on hmm_oracle.random_tiny models (finite and infinite, with and without a silent chain, normal, uniform and
kernel-density states), the normalisation of every posterior row, the oracle's tie rule and summation order, and the
public surface that needs no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import posterior_oracle as PO  # noqa: E402
import profile_oracle as P  # noqa: E402

from pypore_amd.hmm import Model, NormalDistribution, State  # noqa: E402

TOL = 1e-12


def close(got, want, tol=TOL):
    """The measure of tests/test_hmm_gpu.py: relative to max(1, |want|), -inf exactly where the oracle has it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= tol, err.max()


def tiny(seed, kde):
    rng = np.random.default_rng(300 + seed)
    make = lambda: O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 4 < 2)      # noqa: E731
    model = P.with_kde(make, rng, share=0.6) if kde else make()
    return rng, model, P.Compiled(model)


@pytest.mark.parametrize("kde", [False, True])
@pytest.mark.parametrize("seed", range(12))
def test_oracle_equals_brute_force(seed, kde):
    """Every posterior row and every edge count to 1e-12; each row of a possible sequence sums to probability 1."""
    rng, model, c = tiny(seed, kde)
    possible = 0
    for n in range(7):
        x = rng.normal(size=n)
        got = PO.posterior(c, x)
        logp, post, counts = PO.posterior_brute_force(c, x)
        assert got.post.shape == (n, c.NE) and got.state.shape == (n,) and got.counts.shape == (len(model.edges),)
        if not logp > -np.inf:
            assert got.logp == -np.inf and np.isneginf(got.post).all() and (got.state == -1).all()
            assert got.map_logp == -np.inf and not got.counts.any()
            continue
        possible += 1
        close([got.logp], [logp])
        # brute force takes log of a sum of path posteriors: an entry it rounds to log(0) is one the recursion has at -inf
        close(got.post, post)
        close(got.counts, counts)
        close(O.lse_rows(got.post) if n else np.zeros(0), np.zeros(n))
        assert np.array_equal(got.state, [int(np.argmax(r)) for r in got.post])
        assert got.map_logp == PO.ordered_sum(got.post[t, k] for t, k in enumerate(got.state))
        # expected counts: every observation is emitted once, so the edges into emitting states carry n in all
        into_emit = [e for e, (_, l, _) in enumerate(model.edges) if l < c.NE]
        close([got.counts[into_emit].sum()], [float(n)])
    assert 1 <= possible <= 7          # (uniform states make some sequences impossible: both kinds are met)


def test_the_four_kinds_of_tiny_model_are_drawn():
    kinds = set()
    for seed in range(12):
        _, model, c = tiny(seed, False)
        kinds.add((c.finite, c.S - c.NE > 2))
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}


def mirrored_model():
    """Two emitting states that share one distribution object and have mirrored edges: their posteriors are equal bit
    for bit at every observation."""
    m = Model("mirror")
    d = NormalDistribution(0.5, 1.25)
    a, b = State(d, "a"), State(d, "b")
    m.add_transition(m.start, a, 0.5)
    m.add_transition(m.start, b, 0.5)
    for s, o in ((a, b), (b, a)):
        m.add_transition(s, s, 0.5)
        m.add_transition(s, o, 0.3)
        m.add_transition(s, m.end, 0.2)
    m.bake()
    return m


def test_lowest_index_wins_an_exact_tie():
    m = mirrored_model()
    c = O.Compiled(m)
    x = np.random.default_rng(4).normal(0.5, 1.0, 33)
    got = PO.posterior(c, x)
    assert np.array_equal(got.post[:, 0], got.post[:, 1]) and np.isfinite(got.post).all()
    assert (got.state == 0).all() and (got.gap == 0).all()
    close(got.post, np.full((33, 2), np.log(0.5)))


def test_gap_and_ordered_sum():
    post = np.array([[-1.0, -3.0, -2.0], [-np.inf, -0.5, -np.inf], [-2.0, -2.0, -5.0]])
    assert np.array_equal(PO.top_two_gap(post), [1.0, np.inf, 0.0])
    assert np.array_equal(PO.top_two_gap(np.zeros((2, 1))), [np.inf, np.inf])
    v = [1e16, 1.0, -1e16, 1.0]
    assert PO.ordered_sum(v) == ((1e16 + 1.0) - 1e16) + 1.0 and PO.ordered_sum([]) == 0.0


def test_public_surface_without_a_device():
    from pypore_amd import _lib, engine
    assert "ps_hmm_posterior" in _lib.EXPORTS
    assert callable(engine.Context.hmm_posterior)
    for name in ("maximum_a_posteriori", "maximum_a_posteriori_batch", "forward_backward", "forward_backward_batch"):
        assert callable(getattr(Model, name))
    with pytest.raises(ValueError, match="not baked"):
        Model("raw").maximum_a_posteriori([0.0])
    with pytest.raises(ValueError, match="not baked"):
        Model("raw").forward_backward_batch([[0.0]])
