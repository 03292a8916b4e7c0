"""The reference's profile HMM builders on the MI355X: the five HMM kernels (Viterbi, forward, backward, E-step, posterior;
csrc/seg_hmm.hpp) on the models of pypore_amd.hmm's ModularProfileModel, Phi29ProfileHMM and Hel308ProfileHMM -- up to 1 742
states, 293 silent levels per step, dead-end silent states, and an E-step accumulator row on either side of the 64 KiB of
LDS (96 and 97 positions, no option forced) -- and Model.expected_transitions_batch.

Bounds.
  * Viterbi: log probability and path equal hmm_oracle.viterbi_exact's, `==`: the models hold normal and uniform states
    only, so the device's Viterbi calls no libm and the oracle restates it operation by operation.
  * forward, backward, log_probability: the measure and TOL = 1e-12 of tests/test_hmm_gpu.py (relative to max(1, |oracle|),
    -inf exactly where the oracle has -inf).
  * E-step: the measure and bounds of tests/test_hmm_train_gpu.py: log probabilities to 1e-12, counts and (W, A, B) to 1e-9
    relative to max(1, |oracle|), trained edge probabilities and improvements to 1e-8.
  * Per-sequence edge counts: the bound derived in the docstring of tests/test_posterior_gpu.py, 4 TOL max(1, |logp| +
    |log C| + 80) + (n + 1) 2^-52 relative to the oracle's count C, below 1e-300 where C is 0.  (Its premise, log
    densities at most about 40 above 0, holds here with room: every density is a normal of std 1.5 or uniform on 90.)  A
    sum of counts is held to the sum of its terms' bounds.
  * expected_transitions_batch equals forward_backward_batch's dense array at model.edges bit for bit: the same device call.

train() is compared on a model whose match distributions are frozen: tests/hmm_train_oracle.py updates a distribution
state by state, so it cannot say what the four states that share a position's distribution (M:, MO:, MS:, ME:) should pool
to; the pooled update is held to hand-computed numbers in tests/test_hmm_train_host.py.  What the merged model adds to
training -- the structure that trains, and the summed pseudocounts -- is in the edges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import hmm_train_oracle as T  # noqa: E402
import modular_models as MM  # noqa: E402
import posterior_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


def assert_close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    print("max error %.3g over %d entries (bound %.3g)" % (err.max() if err.size else 0.0, err.size, tol))
    assert err.size == 0 or err.max() <= tol, err.max()


# ---- the models and their sequences, built once ---------------------------------------------------------------------------
def _seqs54():
    mu = MM.means(54)
    return [MM.walk_with_backslip(mu, 27), MM.noisy_walk(mu, 78, seed=54)]


def _seqs(n, seed):
    mu = MM.means(n)
    rng = np.random.default_rng(seed)
    return [MM.walk(mu), MM.walk_with_backslip(mu, n // 2), MM.noisy_walk(mu, 2 * n, seed), rng.uniform(0, 90, n)]


CASES = {
    "phi29-3": (lambda: MM.modular(3), lambda: [np.zeros(0), np.array([35.2]), np.array([20.0, 35.0, 20.0, 35.0, 50.0])]),
    "fork": (lambda: MM.fork_model(), lambda: [MM.FORK_SEQS["a"], MM.FORK_SEQS["b"]]),
    "phi29-54": (lambda: MM.modular(54), _seqs54),
    "phi29-54-all": (lambda: MM.modular(54, merge="all"), _seqs54),
    "nanopore-8": (lambda: MM.modular(8, "nanopore"), lambda: _seqs(8, 1)),
    "global-8": (lambda: MM.modular(8, "global"), lambda: _seqs(8, 2)),
    "linear-phi29-12": (lambda: MM.linear("phi29", 12), lambda: _seqs(12, 3)),
    "linear-hel308-12": (lambda: MM.linear("hel308", 12), lambda: _seqs(12, 4)),
}
_built = {}


def case(name):
    if name not in _built:
        make, seqs = CASES[name]
        model = make()
        _built[name] = (model, O.Compiled(model), seqs())
    return _built[name]


# ---- Viterbi, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_viterbi_bit_for_bit(name):
    model, _, seqs = case(name)
    got = model.viterbi_batch(seqs)
    for s, (lp, path) in zip(seqs, got):
        want_lp, want_path, _, _, _ = O.viterbi_exact(model, s)
        assert want_path is not None and lp == want_lp
        assert [i for i, _ in path] == want_path and all(model.states[i] is st for i, st in path)
    if name == "phi29-3":
        assert MM.emitting_names(model, [i for i, _ in got[2][1]]) == ["M:0", "M:1", "M:0", "M:1", "M:2"]
        assert MM.emitting_names(model, [i for i, _ in got[0][1]]) == []            # the delete lane, start to end
    if name == "fork":
        assert got[0][0] == got[1][0]
        for k, (_, path) in zip("ab", got):
            assert MM.emitting_names(model, [i for i, _ in path]) == ["M:0", "M:%s:2" % k, "M:%s:3" % k, "M:3"]


def test_viterbi_merged_path_is_the_unmerged_one_without_the_removed_states():
    base, _, seqs = case("phi29-54")
    merged, _, _ = case("phi29-54-all")
    kept = {s.name for s in merged.states}
    for (_, a), (_, b) in zip(base.viterbi_batch(seqs), merged.viterbi_batch(seqs)):
        assert [s.name for _, s in a if s.name in kept] == [s.name for _, s in b]


# ---- forward, backward, log_probability ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_backward_log_probability(name):
    model, c, seqs = case(name)
    assert_close(model.log_probability_batch(seqs), [O.log_probability(c, s) for s in seqs])
    for s, f in zip(seqs, model.forward_batch(seqs)):
        assert_close(f, O.forward(c, s))
    for s, b in zip(seqs, model.backward_batch(seqs)):
        assert_close(b, O.backward(c, s))


def test_merged_log_probabilities_equal_the_unmerged():
    base, _, seqs = case("phi29-54")
    merged, _, _ = case("phi29-54-all")
    assert_close(merged.log_probability_batch(seqs), base.log_probability_batch(seqs))


# ---- E-step ------------------------------------------------------------------------------------------------------------------
def check_estep(model, seqs):
    got = model.expected_counts_batch(seqs)
    counts, stats, logp, skipped = T.estep(model, seqs)
    assert_close(got.logp, logp, 1e-12)
    assert got.skipped == skipped
    assert_close(got.counts, counts, 1e-9)
    assert_close(got.stats, stats, 1e-9)
    return got


def test_estep_fork():
    model = MM.fork8_model()
    mu = MM.means(8)
    up = mu.copy()
    up[3] += 6.0                                          # branch b's level
    check_estep(model, [MM.walk(mu), MM.walk(up), MM.walk_with_backslip(mu, 4), np.zeros(0), MM.noisy_walk(mu, 16, 8)])


def test_estep_54_positions():
    model, _, seqs = case("phi29-54")
    check_estep(model, seqs)
    check_estep(case("phi29-54-all")[0], seqs)


@pytest.mark.parametrize("n,in_lds", [(96, True), (97, False)])
def test_estep_on_both_sides_of_the_lds_limit(n, in_lds):
    """The accumulator row beside the two score rows, 16 S + 8 (E + 3 NE + 1) bytes: 65 144 at 96 positions (LDS), 65 824
    at 97 (global memory)."""
    model = MM.modular(n)
    S, NE, levels, E, _ = MM.size(model)
    assert (16 * S + 8 * (E + 3 * NE + 1) <= 64 << 10) == in_lds and levels >= 290
    mu = MM.means(n)
    rng = np.random.default_rng(n)
    seqs = [mu[np.sort(rng.choice(n, 20, replace=False))] + rng.normal(0, 1.0, 20) for _ in range(3)]
    got = check_estep(model, seqs)
    assert got.skipped == 0


def test_train_one_iteration_on_a_merged_model():
    model = MM.modular(3, merge="all")
    for s in model.states[:model.flat["n_emit"]]:
        s.distribution.freeze()                            # (module docstring)
    mu = MM.means(3)
    seqs = [MM.walk(mu), MM.walk(mu, -0.4), np.array([20.0, 35.0, 20.0, 35.0, 50.0]), np.array([21.0, 21.5, 49.0]),
            np.array([20.5, 70.0, 36.0, 50.5])]
    pseudo = T.pseudocounts_of(model)
    assert any(abs(p - 0.98) < 1e-12 for p in pseudo)      # the last match's 0.01 and 0.97 into e1 and e2: one edge into `end`
    want, steps, total = T.train(model, seqs, 1, use_pseudocount=True)
    got = model.train(seqs, max_iterations=1, use_pseudocount=True, verbose=False)
    assert_close([got], [total], 1e-8)
    assert_close([p for _, _, p in model.edges], [p for _, _, p in want.edges], 1e-8)
    assert [s.distribution.parameters for s in model.states if not s.is_silent()] \
        == [s.distribution.parameters for s in want.states if not s.is_silent()]


# ---- posterior edge counts -----------------------------------------------------------------------------------------------------
def count_bounds(want, n):
    """Per edge: the absolute error allowed against the oracle's count (tests/test_posterior_gpu.py, module docstring)."""
    with np.errstate(divide="ignore"):
        size = np.where(want.counts > 0, np.abs(np.log(want.counts)), 0.0)
    rel = 4 * TOL * np.maximum(1.0, abs(want.logp) + size + 80.0) + (n + 1) * 2.0 ** -52
    return rel * want.counts + 1e-300


@pytest.mark.parametrize("name", ["phi29-3", "fork", "phi29-54", "phi29-54-all", "nanopore-8", "linear-hel308-12"])
def test_expected_transitions(name):
    model, c, seqs = case(name)
    got = model.expected_transitions_batch(seqs)
    assert got.dtype == np.float64 and got.shape == (len(seqs), len(model.edges))
    for q, s in enumerate(seqs):
        want = PO.posterior(c, s)
        assert want.logp > -np.inf
        err = np.abs(got[q] - want.counts)
        bound = count_bounds(want, len(s))
        print("counts: max error / bound %.3g" % (err / bound).max())
        assert (err <= bound).all()
    assert np.array_equal(model.expected_transitions(seqs[-1]), got[-1])
    src = [e[0] for e in model.edges]
    dst = [e[1] for e in model.edges]
    for q, (transitions, _) in enumerate(model.forward_backward_batch(seqs)):
        assert np.array_equal(transitions[src, dst], got[q])                        # bit for bit: the same device call
        assert np.count_nonzero(transitions) == np.count_nonzero(got[q])             # and 0 off the edges


def test_fork_branch_shares():
    """The expected flow out of board 0 into each branch's first board (the '>' lanes 1, 2 and 4): the sequence at a
    branch's levels puts more than 0.99 of it into that branch."""
    model, c, _ = case("fork")
    into = {k: [e for e, (i, j, _) in enumerate(model.edges)
                if model.states[i].name.startswith("b0e") and model.states[j].name.startswith("b%s:2s" % k)] for k in "ab"}
    assert [len(into[k]) for k in "ab"] == [3, 3]
    seqs = [MM.FORK_SEQS["a"], MM.FORK_SEQS["b"]]
    got = model.expected_transitions_batch(seqs)
    for q, taken in enumerate("ab"):
        want = PO.posterior(c, seqs[q])
        bound = count_bounds(want, len(seqs[q]))
        flow = {k: want.counts[into[k]].sum() for k in "ab"}
        share = flow[taken] / (flow["a"] + flow["b"])
        print("branch %s: oracle share %.6f" % (taken, share))
        assert share > 0.99
        for k in "ab":
            assert abs(got[q][into[k]].sum() - flow[k]) <= bound[into[k]].sum()
        assert got[q][into[taken]].sum() / (got[q][into["a"]].sum() + got[q][into["b"]].sum()) > 0.99


def test_an_impossible_sequence_has_a_zero_row():
    """1e200 is outside every insert's [0, 90], and every normal's log density of it is -inf, so no path holds it."""
    model, c, _ = case("phi29-3")
    seqs = [np.array([20.0, 35.0, 50.0]), np.array([20.0, 1e200, 50.0]), np.array([20.3, 35.3, 50.3])]
    assert not O.log_probability(c, seqs[1]) > -np.inf
    got = model.expected_transitions_batch(seqs)
    assert not got[1].any() and got[0].any() and got[2].any()
    assert np.array_equal(got[0], model.expected_transitions(seqs[0]))
    assert model.expected_transitions_batch([]).shape == (0, len(model.edges))
