"""pypore_amd.hmm on the MI355X (ps_hmm_batch, csrc/seg_hmm.hpp) against the numpy oracle (tests/hmm_oracle.py):
Viterbi, forward, backward and log_probability on brute-forceable models, random models with long silent chains and a
54-position profile HMM; edge cases; a ragged batch against single calls; the DataTypes callers end to end; launch
shapes: in-degrees on both sides of the 8-bit backpointer width, paths longer than their slots, a model at the state cap.

Tolerances: log probabilities and matrix entries to 1e-12 relative (to max(|oracle|, 1), so that entries near log 1 are
not judged by their rounding noise); -inf exactly where the oracle has -inf.  Viterbi paths are identical wherever the
oracle's winning margin exceeds 1e-9 relative; elsewhere the device path's own score must be within 1e-9 of the best."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402

from pypore_amd.hmm import Model, NormalDistribution, State  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


def assert_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= TOL, err.max()


def check_viterbi(c, seq, got):
    lp, path, margin = O.viterbi(c, seq)
    glp, gpath = got
    if path is None:
        assert glp == -np.inf and gpath is None
        return
    assert_close([glp], [lp])
    idx = [i for i, _ in gpath]
    assert all(c.states[i] is s for i, s in gpath)
    if margin > 1e-9:
        assert idx == path
    else:
        score = O.path_score(c, seq, idx)
        assert score is not None and abs(score - lp) <= 1e-9 * max(1.0, abs(lp))


def check_all(model, seqs, matrices=True):
    c = O.Compiled(model)
    vit = model.viterbi_batch(seqs)
    for s, v in zip(seqs, vit):
        check_viterbi(c, s, v)
    assert_close(model.log_probability_batch(seqs), [O.log_probability(c, s) for s in seqs])
    if matrices:
        for s, f in zip(seqs, model.forward_batch(seqs)):
            assert_close(f, O.forward(c, s))
        for s, b in zip(seqs, model.backward_batch(seqs)):
            assert_close(b, O.backward(c, s))


@pytest.mark.parametrize("seed", range(12))
def test_tiny_models_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    model = O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0)
    c = O.Compiled(model)
    seqs = [rng.normal(size=n) for n in range(7)]
    check_all(model, seqs)
    for s, (lp, path) in zip(seqs, model.viterbi_batch(seqs)):
        _, logp_bf, best_bf, path_bf = O.brute_force(c, s)
        if path_bf is None:
            assert lp == -np.inf and path is None
        else:
            assert abs(lp - best_bf) <= 1e-12 * max(1, abs(best_bf)) and [i for i, _ in path] == path_bf
            assert abs(model.log_probability(s) - logp_bf) <= 1e-12 * max(1, abs(logp_bf))


def test_random_models_with_long_silent_chains():
    rng = np.random.default_rng(2024)
    for k in range(200):
        model = O.random_model(rng, max_states=300, max_chain=60, finite=k % 4 != 3)
        seqs = [rng.normal(0, 2, int(rng.integers(0, 12))) for _ in range(2)]
        check_all(model, seqs, matrices=k % 5 == 0)


def test_profile_hmm():
    model, means = O.profile_model(54)
    assert len(model.states) == 165
    seqs = O.profile_events(means, 12, lo=50, hi=400)
    check_all(model, seqs)


def test_edge_cases():
    model, means = O.profile_model(10)
    c = O.Compiled(model)
    # the empty sequence: silent paths only (here start -> D:1 .. D:10 -> end)
    lp, path = model.viterbi([])
    assert [s.name for _, s in path] == ["profile-start"] + ["D:%d" % i for i in range(1, 11)] + ["profile-end"]
    assert_close([lp], [O.viterbi(c, [])[0]])
    assert_close(model.forward([]), O.forward(c, []))
    # impossible: a value outside every insert's support and far from every match is still possible (normal), so use
    # a model whose only emitting state is uniform
    from pypore_amd.hmm import UniformDistribution
    u = Model("u")
    a = State(UniformDistribution(0, 1), "a")
    u.add_transition(u.start, a, 1.0)
    u.add_transition(a, a, 0.5)
    u.add_transition(a, u.end, 0.5)
    u.bake()
    assert u.viterbi([0.5, 3.0]) == (-np.inf, None)
    assert u.log_probability([0.5, 3.0]) == -np.inf
    assert np.isneginf(u.backward([0.5, 3.0])[0][u.states.index(u.start)])
    assert u.viterbi_batch([[0.2], [2.0], []])[1] == (-np.inf, None)
    # too large for the kernel
    big = Model("big")
    prev = big.start
    for i in range(4100):
        s = State(NormalDistribution(0, 1), "s%05d" % i)
        big.add_transition(prev, s, 1.0)
        prev = s
    big.add_transition(prev, big.end, 1.0)
    big.bake()
    with pytest.raises(ValueError, match="4096"):
        big.viterbi([0.0])


def test_batch_split_across_launches():
    from pypore_amd import engine
    model, means = O.profile_model(54, seed=3)
    seqs = O.profile_events(means, 40, lo=50, hi=120, seed=5)
    whole = model.viterbi_batch(seqs)
    ctx = engine.context()
    ctx.set_option("hmm_bp_budget", 165 * 130 * 3)          # about three sequences per launch
    try:
        split = model.viterbi_batch(seqs)
    finally:
        ctx.set_option("hmm_bp_budget", 512 << 20)
    for (a, pa), (b, pb) in zip(whole, split):
        assert a == b and [i for i, _ in pa] == [i for i, _ in pb]
    c = O.Compiled(model)
    for s, v in zip(seqs[:5], split[:5]):
        check_viterbi(c, s, v)


def test_ragged_batch_equals_single_calls():
    model, means = O.profile_model(54, seed=7)
    rng = np.random.default_rng(9)
    seqs = O.profile_events(means, 2000, lo=1, hi=120, seed=11)
    seqs[5] = np.zeros(0)
    vit = model.viterbi_batch(seqs)
    lps = model.log_probability_batch(seqs)
    for q in rng.permutation(2000):
        lp, path = model.viterbi(seqs[q])
        assert lp == vit[q][0] and [i for i, _ in path] == [i for i, _ in vit[q][1]]
        assert model.log_probability(seqs[q]) == lps[q]


def _level_model(levels):
    """A left-to-right model over the given current levels (one match state each, self-loops), finite."""
    m = Model("levels")
    st = [State(NormalDistribution(float(v), 1.5), "L%d" % i) for i, v in enumerate(levels)]
    m.add_transition(m.start, st[0], 1.0)
    for i, s in enumerate(st):
        m.add_transition(s, s, 0.6)
        if i + 1 < len(st):
            m.add_transition(s, st[i + 1], 0.4)
    m.add_transition(st[-1], m.end, 0.4)
    m.bake()
    return m


def _synthetic_event(rng, levels, second=1.0e5):
    from pypore_amd.DataTypes import Event, File
    x = np.concatenate([np.full(int(rng.integers(2000, 6000)), v) + rng.normal(0, 0.6, 1) for v in levels
                        for _ in range(int(rng.integers(1, 3)))])
    x = np.round((x + rng.normal(0, 0.3, x.size)) * 32) / 32
    f = File(current=x, timestep=1000.0 / second)
    return Event(current=x, start=0, end=x.size / second, duration=x.size / second, second=second, file=f)


def test_parse_with_hmm_and_experiment_apply_hmm_end_to_end():
    from pypore_amd.DataTypes import Experiment
    from pypore_amd.parsers import SpeedyStatSplit
    rng = np.random.default_rng(21)
    levels = [30.0, 45.0, 25.0, 50.0, 35.0]
    model = _level_model(levels)
    c = O.Compiled(model)
    events = []
    for k in range(4):
        ev = _synthetic_event(rng, levels)
        plain = np.copy(ev.current)
        ev.parse(SpeedyStatSplit(prior_segments_per_second=10))
        segs = [(s.start, s.n) for s in ev.segments]
        means = np.array([s.mean for s in ev.segments])
        assert len(segs) >= 2
        lp, path, _ = O.viterbi(c, means)
        want = O.merge_loop(segs, [(i, model.states[i]) for i in path], ev.second)
        want = [(a, min(b, plain.size), h) for a, b, h in want]
        ev.parse(SpeedyStatSplit(prior_segments_per_second=10), hmm=model)
        assert [(s.start, s.start + s.n, s.hidden_state) for s in ev.segments] == want
        ev.parse(SpeedyStatSplit(prior_segments_per_second=10))
        events.append(ev)
    exp = Experiment([])
    exp.files = [events[0].file]
    exp.files[0].events = events
    out = exp.apply_hmm(model, filter=lambda e: e is not events[1])
    want = []
    for ev in (events[0], events[2], events[3]):
        _, path, _ = O.viterbi(c, np.array([s.mean for s in ev.segments]))
        want += path
    assert [i for i, _ in out] == want


# ---- launch shapes of ps_hmm_batch ----------------------------------------------------------------------------------


_hub_model = O.hub_model                  # (model, h, [e states]); shared with tests/viterbi_ties.py


def _hub_seqs(rng, es, winners):
    """Sequences that pass through h from the given e states (ordinals into h's in-edges), plus random ones."""
    seqs = []
    for w in winners:
        v = int(rng.integers(len(es)))
        seqs.append(np.array([3.0 * w, -50.0, -49.5, 3.0 * v, -50.5, 3.0 * (len(es) - 1 - w)]) + rng.normal(0, 0.05, 6))
    for _ in range(6):                                  # e, then h one or more times, ...
        x = []
        for _ in range(int(rng.integers(0, 4))):
            x += [3.0 * int(rng.integers(len(es)))] + [-50.0] * int(rng.integers(1, 3))
        seqs.append(np.array(x) + rng.normal(0, 0.3, len(x)))
    return seqs


@pytest.mark.parametrize("n_in", [255, 256, 257, 600])
def test_in_degree_across_the_backpointer_width(n_in):
    """In-degree 255 takes the 8-bit Viterbi backpointers, 256 and more the 16-bit ones.  From 257 up the winning in-edge
    into h has ordinal >= 256 (the emission makes it unambiguous), so a backpointer cut to 8 bits gives a wrong path."""
    model, h, es = _hub_model(n_in)
    ix = {id(s): i for i, s in enumerate(model.states)}
    ins = {}
    for i, j, _ in model.edges:
        ins.setdefault(j, []).append(i)
    assert len(ins[ix[id(h)]]) == n_in and len(ins[ix[id(model.end)]]) == n_in
    assert max(len(v) for v in ins.values()) == n_in
    rng = np.random.default_rng(n_in)
    winners = [0, min(254, n_in - 2), n_in - 2] + ([256, 300 % (n_in - 1), n_in - 3] if n_in > 257 else [])
    seqs = _hub_seqs(rng, es, winners)
    check_all(model, seqs)
    c = O.Compiled(model)
    used = []                                           # in-edge ordinals on the oracle's paths
    for q, s in enumerate(seqs):
        lp, path, margin = O.viterbi(c, s)
        if path is None:
            continue
        used += [sorted(ins[k]).index(i) for i, k in zip(path[:-1], path[1:])]
        if q < len(winners):
            into_h = path[path.index(ix[id(h)]) - 1]
            assert into_h == ix[id(es[winners[q]])] and margin > 1e-3
            assert sorted(ins[ix[id(h)]]).index(into_h) == winners[q]
    if n_in > 256:                                      # (h's self-loop is its last in-edge, ordinal n_in - 1)
        assert max(used) >= 256


def test_in_degree_600_under_a_small_backpointer_budget():
    """The 16-bit route with launches cut by hmm_bp_budget, one sequence alone exceeding the budget (the at-least-one
    branch)."""
    from pypore_amd import engine
    model, h, es = _hub_model(600)
    rng = np.random.default_rng(5)
    seqs = _hub_seqs(rng, es, [256, 598, 400, 3])
    alt = np.stack([3.0 * rng.integers(599, size=20), np.full(20, -50.0)], axis=1).ravel()     # e, h, e, h, ...
    seqs.insert(3, alt + rng.normal(0, 0.1, 40))
    S = len(model.states)
    budget = 9 * S * 2                                  # rows of 16-bit backpointers: 9 (n + 1 <= 9 for the short ones)
    assert (len(seqs[3]) + 1) * S * 2 > budget
    whole = model.viterbi_batch(seqs)
    with LG.options(engine.context(), hmm_bp_budget=budget):
        split = model.viterbi_batch(seqs)
    c = O.Compiled(model)
    for s, a, b in zip(seqs, whole, split):                  # (an empty sequence is impossible here: path None)
        assert a[0] == b[0] and [i for i, _ in a[1] or []] == [i for i, _ in b[1] or []]
        check_viterbi(c, s, b)


_chain_model = O.chain_model


def test_viterbi_path_longer_than_its_slot():
    """Paths of ~50 observations through a 20-state silent loop are about eight times longer than the default slot
    2 (n + 1) + silent states + 1: the call reruns with slots of the exact lengths (PS_ERR_CAPACITY, hmm_trace_kernel's flag bit 0).
    Short sequences in the same batch fit their slots.  The same with the backpointers split across launches."""
    from pypore_amd import engine
    model = _chain_model(20)
    S, NE = len(model.states), sum(1 for s in model.states if not s.is_silent())
    rng = np.random.default_rng(8)
    seqs = [rng.normal(0, 0.5, n) for n in (50, 1, 2, 48, 0, 1, 55, 2)] + [np.array([2.0, 2.1, 1.9, 0.0])]
    slot = [2 * (len(s) + 1) + (S - NE) + 1 for s in seqs]
    c = O.Compiled(model)
    for opts in ({}, {"hmm_bp_budget": 60 * S}):
        with LG.options(engine.context(), **opts):
            got = model.viterbi_batch(seqs)
        lens = [len(p) if p is not None else 0 for _, p in got]
        assert any(n > 5 * sl for n, sl in zip(lens, slot)) and any(0 < n <= sl for n, sl in zip(lens, slot))
        for s, v in zip(seqs, got):
            check_viterbi(c, s, v)


def test_model_at_the_state_cap():
    """Exactly HMM_S_MAX = 4096 states (64 KiB of LDS score rows): Viterbi, forward, backward and log_probability; one
    state more is refused, naming the cap."""
    model = O.line_model(4096)
    assert len(model.states) == 4096
    rng = np.random.default_rng(3)
    check_all(model, [rng.normal(0, 3, n) for n in (0, 1, 3, 6)])
    over = O.line_model(4097)
    assert len(over.states) == 4097
    with pytest.raises(ValueError, match="4096"):
        over.viterbi([0.0])
    with pytest.raises(ValueError, match="4096"):
        over.log_probability_batch([[0.0]])
