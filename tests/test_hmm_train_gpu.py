"""Model.train on the MI355X: the Baum-Welch E-step (ps_hmm_expect, csrc/seg_hmm.hpp hmm_expect_kernel) against the
numpy oracle (tests/hmm_train_oracle.py) on brute-forceable models, random models with long silent chains, the
54-position profile, infinite models, impossible and empty sequences and a ragged batch; launch splitting, determinism and
the global-memory accumulator route; many sequences per workgroup and a model at the state cap; train() against the
oracle's loop for both algorithms; decoding after training; the reference tutorial's flow.

Tolerances: counts and (W, A, B) to 1e-9 relative to max(|oracle|, 1); log probabilities to 1e-12; trained parameters and
improvements to 1e-8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import hmm_train_oracle as T  # noqa: E402
import launch_geometry as LG  # noqa: E402

from pypore_amd.hmm import Model, NormalDistribution, State, UniformDistribution  # noqa: E402

pytestmark = pytest.mark.gpu


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= tol, err.max()


def check_estep(model, seqs):
    got = model.expected_counts_batch(seqs)
    counts, stats, logp, skipped = T.estep(model, seqs)
    close(got.logp, logp, 1e-12)
    assert got.skipped == skipped
    close(got.counts, counts, 1e-9)
    close(got.stats, stats, 1e-9)
    return got


@pytest.mark.parametrize("seed", range(8))
def test_estep_tiny_models_against_brute_force(seed):
    rng = np.random.default_rng(300 + seed)
    model = O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0)
    seqs = [rng.normal(size=n) for n in range(6)]
    got = check_estep(model, seqs)
    counts = np.zeros(len(model.edges))
    stats = np.zeros((T.n_emit(model), 3))
    for s in seqs:
        c, st, lp = T.estep_brute_force(model, s)
        counts += c
        stats += st
    close(got.counts, counts, 1e-9)
    close(got.stats, stats, 1e-9)


def test_estep_random_models_with_long_silent_chains():
    rng = np.random.default_rng(77)
    for k in range(24):
        model = O.random_model(rng, max_states=200, max_chain=60, finite=k % 4 != 3)
        seqs = [rng.normal(0, 2, int(rng.integers(0, 10))) for _ in range(3)]
        check_estep(model, seqs)


def test_estep_profile_and_ragged_batch():
    model, means = O.profile_model(54)
    seqs = O.profile_events(means, 8, lo=50, hi=400)
    seqs[2] = np.zeros(0)                                  # empty: its silent edges at t = 0 only
    seqs[5] = np.full(3, 1e300)                            # every normal density underflows, no insert holds it: impossible
    got = check_estep(model, seqs)
    assert got.skipped == 1 and np.isneginf(got.logp[5])


def test_estep_infinite_and_impossible():
    m = Model("u")
    a = State(UniformDistribution(0, 1), "a")
    b = State(NormalDistribution(0.5, 0.3), "b")
    m.add_transition(m.start, a, 0.7)
    m.add_transition(m.start, b, 0.3)
    m.add_transition(a, a, 0.5)
    m.add_transition(a, b, 0.5)
    m.add_transition(b, a, 0.2)
    m.add_transition(b, b, 0.8)
    m.bake()
    assert not m.finite
    seqs = [np.array([0.2, 0.9, 3.0]), np.array([3.0, 0.1]), np.zeros(0), np.array([0.4]), np.array([-1.0, 2.0])]
    got = check_estep(m, seqs)
    assert got.skipped == 0
    only_a = Model("a")
    a2 = State(UniformDistribution(0, 1), "a")
    only_a.add_transition(only_a.start, a2, 1.0)
    only_a.add_transition(a2, a2, 0.5)
    only_a.add_transition(a2, only_a.end, 0.5)
    only_a.bake()
    got = check_estep(only_a, [np.array([0.5, 3.0]), np.array([0.2]), np.array([2.0])])
    assert got.skipped == 2
    got = only_a.expected_counts_batch([])
    assert got.skipped == 0 and not got.counts.any() and not got.stats.any() and got.logp.size == 0


def test_launch_splitting_and_determinism():
    from pypore_amd import engine
    model, means = O.profile_model(54, seed=3)
    seqs = O.profile_events(means, 60, lo=20, hi=150, seed=5)
    whole = model.expected_counts_batch(seqs)
    again = model.expected_counts_batch(seqs)
    for x, y in zip(whole[:3], again[:3]):
        assert np.array_equal(x, y)
    ctx = engine.context()
    ctx.set_option("hmm_fb_budget", 165 * 8 * 160 * 3)      # about three sequences per launch
    try:
        split = model.expected_counts_batch(seqs)
    finally:
        ctx.set_option("hmm_fb_budget", 4 << 30)
    close(split.counts, whole.counts, 1e-12)
    close(split.stats, whole.stats, 1e-12)
    assert np.array_equal(split.logp, whole.logp)
    counts, stats, logp, _ = T.estep(model, seqs[:12])
    part = model.expected_counts_batch(seqs[:12])
    close(part.counts, counts, 1e-9)
    close(part.stats, stats, 1e-9)


def test_accumulators_in_global_memory():
    from pypore_amd import engine
    # forced: the same model on both routes
    model, means = O.profile_model(30, seed=8)
    seqs = O.profile_events(means, 20, lo=10, hi=80, seed=9)
    lds = model.expected_counts_batch(seqs)
    ctx = engine.context()
    ctx.set_option("hmm_expect_lds", 0)
    try:
        glob = model.expected_counts_batch(seqs)
    finally:
        ctx.set_option("hmm_expect_lds", 1)
    close(glob.counts, lds.counts, 1e-12)
    close(glob.stats, lds.stats, 1e-12)
    # a model whose 8 E + 24 NE + 16 S bytes exceed 64 KiB takes the global route by itself
    rng = np.random.default_rng(4)
    big = Model("dense")
    st = [State(NormalDistribution(float(rng.normal(0, 2)), float(rng.uniform(0.5, 2))), "e%03d" % i) for i in range(100)]
    for s in st:
        big.add_transition(big.start, s, float(rng.uniform(0.1, 1)))
        for t in st:
            big.add_transition(s, t, float(rng.uniform(0.01, 1)))
        big.add_transition(s, big.end, 0.05)
    big.bake()
    assert 8 * len(big.edges) + 24 * 100 + 16 * len(big.states) > 64 << 10
    check_estep(big, [rng.normal(0, 2, n) for n in (0, 1, 7, 30)])


def _params(model):
    return [p for _, _, p in model.edges], [s.distribution.parameters for s in model.states if not s.is_silent()]


@pytest.mark.parametrize("kw", [dict(), dict(use_pseudocount=True),
                                dict(transition_pseudocount=0.3, edge_inertia=0.2, distribution_inertia=0.4)])
def test_train_against_oracle(kw, capsys):
    model, means = O.profile_model(12, seed=11)
    seqs = O.profile_events(means, 30, lo=15, hi=60, seed=12)
    want, steps, total = T.train(model, seqs, 5, **kw)
    got = model.train(seqs, max_iterations=5, **kw)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 6 and lines[-1].startswith("Total Training Improvement: ")
    close([float(l.split(": ")[1]) for l in lines[:-1]], steps, 1e-8)
    close([got], [total], 1e-8)
    gp, gd = _params(model)
    wp, wd = _params(want)
    close(gp, wp, 1e-8)
    close(gd, wd, 1e-8)
    if not kw:
        assert all(s >= -1e-8 * abs(total) for s in steps)        # Baum-Welch never lowers the likelihood


def test_train_viterbi_against_oracle(capsys):
    model, means = O.profile_model(12, seed=13)
    seqs = O.profile_events(means, 30, lo=15, hi=60, seed=14)
    want, steps, total = T.train(model, seqs, 3, algorithm="viterbi")
    got = model.train(seqs, max_iterations=3, algorithm="viterbi", verbose=False)
    close([got], [total], 1e-8)
    gp, gd = _params(model)
    wp, wd = _params(want)
    close(gp, wp, 1e-8)
    close(gd, wd, 1e-8)


def test_decoding_after_training_with_zero_edges():
    model, means = O.profile_model(12, seed=15)
    seqs = O.profile_events(means, 20, lo=15, hi=40, seed=16)
    ix = {id(s): i for i, s in enumerate(model.states)}
    i0 = ix[id(model.start)]
    # start -> I:0 never used by a sequence that cannot start there: give it no count by training on a start-free path
    model.train(seqs, max_iterations=2, verbose=False)
    model._m_step(np.where([i == i0 and model.states[j].name == "I:0" for i, j, _ in model.edges], 0.0, 1.0),
                  np.zeros((T.n_emit(model), 3)))
    assert any(p == 0.0 for _, _, p in model.edges)
    c = O.Compiled(T.View(model))
    close(model.log_probability_batch(seqs), [O.log_probability(c, s) for s in seqs], 1e-12)
    for s, f in zip(seqs[:4], model.forward_batch(seqs[:4])):
        close(f, O.forward(c, s), 1e-12)
    for s, (lp, path) in zip(seqs, model.viterbi_batch(seqs)):
        wlp, wpath, margin = O.viterbi(c, s)
        close([lp], [wlp], 1e-12)
        if margin > 1e-9:
            assert [i for i, _ in path] == wpath
    check_estep(model, seqs[:6])


def test_tutorial_flow_end_to_end(capsys):
    from pypore_amd.DataTypes import Experiment
    model, means = O.profile_model(54, seed=17)
    events = O.profile_events(means, 40, lo=50, hi=200, seed=18)
    total = model.train(events, max_iterations=10, use_pseudocount=True)
    lines = capsys.readouterr().out.strip().splitlines()
    steps = [float(l.split(": ")[1]) for l in lines if l.startswith("Training improvement: ")]
    assert isinstance(total, float) and 1 <= len(steps) <= 10
    assert lines[-1] == "Total Training Improvement: {}".format(total)
    assert abs(sum(steps) - total) <= 1e-9 * max(1.0, abs(total))
    # classify with the trained model through Experiment.apply_hmm (duck-typed events carrying segment means)
    from pypore_amd.core import Segment

    class Ev(object):
        def __init__(self, means):
            self.segments = [Segment(current=np.full(4, m), mean=m) for m in means]

    exp = Experiment([])

    class F(object):
        pass

    f = F()
    f.events = [Ev(e[:60]) for e in events[:5]]
    exp.files = [f]
    out = exp.apply_hmm(model)
    c = O.Compiled(T.View(model))
    want = []
    for e in events[:5]:
        want += O.viterbi(c, np.array([s.mean for s in Ev(e[:60]).segments]))[1]
    assert [i for i, _ in out] == want


# ---- launch shapes of ps_hmm_expect -----------------------------------------------------------------------------------

def _launch_cuts(lengths, S, budget):
    """The first sequence of every launch after the first (hmm_expect_run: forward matrices within the budget, at least
    one sequence per launch)."""
    cuts, q0, n = [], 0, len(lengths)
    while q0 < n:
        b, q1 = (lengths[q0] + 1) * S * 8, q0 + 1
        while q1 < n and b + (lengths[q1] + 1) * S * 8 <= budget:
            b += (lengths[q1] + 1) * S * 8
            q1 += 1
        if q1 < n:
            cuts.append(q1)
        q0 = q1
    return cuts


_MANY = {}


def _many_sequences():
    """480 short sequences through a 12-position profile and the oracle's E-step of them (computed once)."""
    if not _MANY:
        model, means = O.profile_model(12, seed=31)
        seqs = O.profile_events(means, 480, lo=4, hi=24, seed=32)
        _MANY["case"] = model, seqs, T.estep(model, seqs)
    return _MANY["case"]


@pytest.mark.parametrize("acc_lds", [1, 0])
def test_estep_many_sequences_per_workgroup(acc_lds, capfd, record_property):
    """slots_pct 1 shrinks the E-step grid G to a handful of workgroups, so each one carries its score rows and its
    accumulator row from sequence to sequence (both accumulator routes), and an hmm_fb_budget cuts the batch into launches
    whose first sequences are not multiples of G (the `qs` start of hmm_expect_kernel).  Counts, (W, A, B) and logp match
    the oracle, lie within 1e-12 of the default grid's, and two runs at the same options agree bit for bit."""
    from pypore_amd import engine
    model, seqs, (counts, stats, logp, skipped) = _many_sequences()
    S, E, NE = len(model.states), len(model.edges), T.n_emit(model)
    lds = (2 * S + (E + 3 * NE + 1 if acc_lds else 0)) * 8
    ctx = engine.context()
    with LG.options(ctx, hmm_expect_lds=acc_lds):
        ref = model.expected_counts_batch(seqs)
    capfd.readouterr()
    with LG.options(ctx, hmm_expect_lds=acc_lds, slots_pct=1, debug=1):
        small = model.expected_counts_batch(seqs)
    (slots, pct), = LG.printed_slots(capfd.readouterr().err, lds)
    G = min(len(seqs), slots)
    assert pct == 1 and 2 <= G and len(seqs) >= 4 * G, G
    lengths = [len(s) for s in seqs]
    total = sum((n + 1) * S * 8 for n in lengths)
    budget = next(b for b in (total // d for d in range(5, 40))
                  if len(_launch_cuts(lengths, S, b)) >= 3 and any(q % G for q in _launch_cuts(lengths, S, b)))
    record_property("geometry", {"G": G, "cuts": _launch_cuts(lengths, S, budget)})
    with LG.options(ctx, hmm_expect_lds=acc_lds, slots_pct=1, hmm_fb_budget=budget):
        cut = model.expected_counts_batch(seqs)
        again = model.expected_counts_batch(seqs)
    for got in (small, cut):
        close(got.logp, logp, 1e-12)
        assert got.skipped == skipped == 0
        close(got.counts, counts, 1e-9)
        close(got.stats, stats, 1e-9)
        close(got.counts, ref.counts, 1e-12)
        close(got.stats, ref.stats, 1e-12)
        assert np.array_equal(got.logp, ref.logp)
    for x, y in zip(cut[:3], again[:3]):
        assert np.array_equal(x, y)


def test_estep_at_the_state_cap():
    """4096 states: two score rows fill 64 KiB, so the accumulators take the global-memory route."""
    model = O.line_model(4096)
    assert len(model.states) == 4096
    assert (2 * 4096 + len(model.edges) + 3 * T.n_emit(model) + 1) * 8 > 64 << 10
    rng = np.random.default_rng(6)
    got = check_estep(model, [rng.normal(0, 3, n) for n in (0, 1, 2, 5, 3)])
    assert got.skipped == 1                                # the empty sequence: start reaches end only through a state
