"""Posterior decoding on the MI355X (ps_hmm_posterior, csrc/seg_hmm.hpp hmm_posterior_kernel; Model.forward_backward,
Model.maximum_a_posteriori) against the numpy oracle of tests/posterior_oracle.py, which tests/test_posterior_host.py holds
to brute-force path enumeration.

Tolerances.  Log probabilities and log posteriors: the measure and TOL = 1e-12 of tests/test_hmm_gpu.py (relative to
max(1, |oracle|), -inf exactly where the oracle has -inf).  MAP states: equal to the oracle's at every observation whose
top-two posterior gap in the oracle is at least 1e-9; the observations left out are capped at 1 per 1000 per case, and
for every seed used here the oracle alone leaves out none (checked on the CPU with the oracle only; every case asserts it
again), the exact-tie model apart, where the lower index must be returned.  The MAP log probability is, bit for bit, the
sum in ascending t of the entries of d_post that d_map_state names.

Edge counts against the oracle (a bound the issue leaves open, so derived here, not observed).  A count C is a sum of at
most n + 1 positive terms exp(a), where the device's a = (f - logp) + (b' + lp) combines f, logp and b, each of which the
checks here and tests/test_hmm_gpu.py hold to TOL max(1, |value|) of the oracle's, plus roundings no larger.  f and b' are
at most about 40 above 0 on these models (log densities) and f + b' + lp = logp + a, so |f|, |b'| <= |logp| + |a| + 40.
Terms with a < log C - 40 add less than e^-40 of C in all; the others have |a| <= |log C| + 40.  So C is within
4 TOL max(1, |logp| + |log C| + 80) relative, plus (n + 1) 2^-52 for the order of the sum; where the oracle's count is 0
or underflows the device's must be below 1e-300.

Agreement with ps_hmm_expect: the two kernels form the same terms with the same arithmetic, so only the order of the sums
differs.  A sum of N positive terms differs between any two orders by at most 2 (N - 1) 2^-53 relative; the counts below
sum at most 40 * 61 terms and the statistics 40 * 60, so at most 5.5e-13, below a tenth of the 1e-10 the check uses; the
same two orders taken on the oracle's terms of that batch on the CPU differ by 2.2e-15 (counts) and 1.4e-15 (weights)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import posterior_oracle as PO  # noqa: E402
import profile_oracle as P  # noqa: E402
from test_posterior_host import mirrored_model  # noqa: E402

from pypore_amd.hmm import GaussianKernelDensity, Model, NormalDistribution, State  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
GAP = 1e-9
LENGTHS = (0, 1, 2, 65, 400)


def assert_close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    print("max error %.3g over %d entries" % (err.max() if err.size else 0.0, err.size))
    assert err.size == 0 or err.max() <= tol, err.max()


class Raw(object):
    """One ps_hmm_posterior call with every output asked for, as numpy arrays split per sequence."""

    def __init__(self, model, seqs):
        ctx, off, obs = model._upload(seqs, None)
        logp, post, state, map_logp, counts = ctx.hmm_posterior(model._c_model(), obs, off, want_post=True, want_map=True,
                                                                 want_counts=True)
        self.off = off
        self.logp, self.map_logp = logp.cpu().numpy(), map_logp.cpu().numpy()
        self.post_all, self.state_all, self.counts = post.cpu().numpy(), state.cpu().numpy(), counts.cpu().numpy()
        assert self.post_all.shape == (off[-1], model.flat["n_emit"]) and self.state_all.shape == (off[-1],)
        assert self.counts.shape == (len(seqs), len(model.edges)) and self.logp.shape == self.map_logp.shape == (len(seqs),)

    def post(self, q):
        return self.post_all[self.off[q]:self.off[q + 1]]

    def state(self, q):
        return self.state_all[self.off[q]:self.off[q + 1]]

    def same_bits(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k), equal_nan=True)
                   for k in ("logp", "map_logp", "post_all", "state_all", "counts"))


def check_sequence(want, raw, q, seq):
    """Sequence q of a Raw against the oracle's Posterior; returns the number of observations below the gap."""
    n = len(seq)
    post, state = raw.post(q), raw.state(q)
    assert_close([raw.logp[q]], [want.logp])
    assert_close(post, want.post)
    if not want.logp > -np.inf:
        assert (state == -1).all() and raw.map_logp[q] == -np.inf and not raw.counts[q].any()
        return 0
    clear = want.gap >= GAP
    assert np.array_equal(state[clear], want.state[clear])
    assert ((state >= 0) & (state < post.shape[1])).all()
    assert raw.map_logp[q] == PO.ordered_sum(post[t, k] for t, k in enumerate(state))          # bit for bit
    assert_close([raw.map_logp[q]], [want.map_logp], tol=TOL * max(1, n))                       # (n entries, each to TOL)
    with np.errstate(divide="ignore"):
        size = np.where(want.counts > 0, np.abs(np.log(want.counts)), 0.0)
    rel = 4 * TOL * np.maximum(1.0, abs(want.logp) + size + 80.0) + (n + 1) * 2.0 ** -52        # (module docstring)
    err = np.abs(raw.counts[q] - want.counts)
    print("counts: max error / bound %.3g" % ((err / (rel * want.counts + 1e-300)).max() if err.size else 0.0))
    assert (err <= rel * want.counts + 1e-300).all()
    return int(n - clear.sum())


def check_case(model, seqs, c=None, raw=None):
    """Every sequence against the oracle, and the case's cap on observations below the gap (none for the seeds here)."""
    c = P.Compiled(model) if c is None else c
    raw = Raw(model, seqs) if raw is None else raw
    total = sum(len(s) for s in seqs)
    unclear = sum(check_sequence(PO.posterior(c, s), raw, q, s) for q, s in enumerate(seqs))
    assert unclear <= total // 1000 and unclear == 0, (unclear, total)
    return raw


# ---- shapes that cross lane-stride and level seams ------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 66, 67, 129])
def test_line_models_across_the_lane_stride(S):
    """line_model(S) has max(S - 2, 0) emitting states: 61 .. 65 lie around one state per lane, 127 takes two strides; S = 1
    and 2 have no emitting state at all.  Lengths 0, 1, 2, 65 and 400."""
    model = O.line_model(S)
    rng = np.random.default_rng(1000 + S)
    seqs = [rng.normal(0, 3, n) for n in LENGTHS]
    raw = check_case(model, seqs)
    if S > 2:           # a finite model whose every path emits: the empty sequence is impossible, every other possible
        assert raw.map_logp[0] == -np.inf and (raw.logp[1:] > -np.inf).all()
    else:               # start and end alone, no edge: infinite, and only the empty sequence is possible
        assert raw.logp[0] == 0.0 and raw.map_logp[0] == 0.0 and (raw.logp[1:] == -np.inf).all()


RANDOM_SEEDS = [(11, True), (12, False), (13, True), (14, False), (15, True), (16, True)]      # (seed, finite)


@pytest.mark.parametrize("seed,finite", RANDOM_SEEDS)
def test_random_models_with_silent_chains(seed, finite):
    """hmm_oracle.random_model: silent chains of 7 to 39 levels, loose silent states, normal and uniform states, finite
    and infinite; lengths 0, 1, 2, 65, 400 and four between 3 and 30."""
    rng = np.random.default_rng(seed)
    model = O.random_model(rng, max_states=200, max_chain=40, finite=finite)
    assert model.finite == finite and model.flat["n_levels"] >= 7
    seqs = [rng.normal(0, 2, n) for n in LENGTHS] + [rng.normal(0, 2, int(rng.integers(3, 30))) for _ in range(4)]
    check_case(model, seqs)


def profile_with(points, count=32, lo=4, hi=40):
    """The 165-state profile HMM and `count` events; points > 0: its match states as kernel densities of that many points
    around the mean."""
    model, means = O.profile_model(54)
    if points:
        rng = np.random.default_rng(points)
        for s in model._added:
            if not s.is_silent() and type(s.distribution).__name__ == "NormalDistribution":
                mean, std = s.distribution.parameters
                pts = [mean] if points == 1 else list(mean + rng.normal(0, 1.0, points))
                s.distribution = GaussianKernelDensity(pts, std)
        model.bake()
    assert len(model.states) == 165 and model.flat["n_levels"] == 56
    return model, O.profile_events(means, count=count, lo=lo, hi=hi)


@pytest.mark.parametrize("points", [0, 1, 8])
def test_profile_hmm_normal_and_kernel_density(points):
    """56 silent levels, 32 events; with 1 and 8 points per match state the HmmDevK instantiation runs.  The events have 4
    to 40 observations (the oracle takes 5 ms per observation on this model); a long one is the next test's."""
    model, seqs = profile_with(points)
    assert bool(model.flat["kde_pt"].size) == bool(points) and len(seqs) == 32
    check_case(model, seqs)


def test_profile_hmm_one_long_event():
    model, seqs = profile_with(0, count=1, lo=400, hi=400)
    assert len(seqs[0]) == 400
    check_case(model, seqs)


# ---- batch and launch shapes ------------------------------------------------------------------------------------------
def batch_case(count):
    model, means = O.profile_model(8, seed=3)
    seqs = O.profile_events(means, count, lo=1, hi=12, seed=count)
    if count > 2:
        seqs[count // 2] = np.array([30.0, np.inf, 31.0])          # every density is 0 at inf: an impossible sequence
        seqs[count // 2 + 1] = np.zeros(0)
    return model, seqs


def test_batch_of_one():
    model, seqs = batch_case(1)
    raw = check_case(model, seqs)
    assert raw.logp[0] > -np.inf


@pytest.fixture(scope="module")
def batch_300():
    model, seqs = batch_case(300)
    return model, seqs, Raw(model, seqs)


def test_batch_of_300_with_an_impossible_and_an_empty_sequence(batch_300):
    model, seqs, raw = batch_300
    check_case(model, seqs, raw=raw)
    assert raw.logp[150] == -np.inf and raw.map_logp[150] == -np.inf and (raw.state(150) == -1).all()
    assert np.isneginf(raw.post(150)).all() and raw.post(150).shape == (3, model.flat["n_emit"])
    assert raw.map_logp[151] == 0.0 and raw.post(151).shape[0] == 0 and raw.logp[151] > -np.inf
    # the empty sequence walks the delete states: start -> D:1 -> ... -> D:8 -> end, each edge once
    names = {(model.states[i].name, model.states[j].name): e for e, (i, j, _) in enumerate(model.edges)}
    walk = ["profile-start"] + ["D:%d" % i for i in range(1, 9)] + ["profile-end"]
    want = np.zeros(len(model.edges))
    want[[names[p] for p in zip(walk[:-1], walk[1:])]] = 1.0
    assert_close(raw.counts[151], want)


def test_one_sequence_per_launch_gives_the_same_bits(batch_300, capfd):
    from pypore_amd import engine
    model, seqs, raw = batch_300
    capfd.readouterr()
    with LG.options(engine.context(), hmm_fb_budget=1, debug=1):
        cut = Raw(model, seqs)
    launches = [ln for ln in capfd.readouterr().err.splitlines() if "posterior launch" in ln]
    assert len(launches) == 300
    assert raw.same_bits(cut)


def planned_launches(off, row_bytes, budget):
    """The launches of a batch by the rule the library states: from q0, as many sequences as keep (n + 1) * row_bytes
    within the budget, at least one.  Returns [(q0, q1, bytes)]."""
    out, q0, n_seq = [], 0, len(off) - 1
    while q0 < n_seq:
        q1, total = q0 + 1, (int(off[q0 + 1] - off[q0]) + 1) * row_bytes
        while q1 < n_seq and total + (int(off[q1 + 1] - off[q1]) + 1) * row_bytes <= budget:
            total += (int(off[q1 + 1] - off[q1]) + 1) * row_bytes
            q1 += 1
        out.append((q0, q1, total))
        q0 = q1
    return out


@pytest.mark.parametrize("case", ["exactly_three", "one_byte_less", "first_alone_over_budget"])
def test_launches_at_the_edges_of_the_budget(batch_300, capfd, case):
    """A budget that holds exactly the first three forward matrices puts three sequences in the first launch, one byte
    less two, and a sequence larger than the budget goes alone; every launch is the stated rule's, and the bits are those
    of the uncut call."""
    import re
    from pypore_amd import engine
    model, seqs, raw = batch_300
    seqs, row = seqs[:12], 8 * len(model.states)
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs])))
    sizes = [(len(s) + 1) * row for s in seqs]
    budget, first = {"exactly_three": (sum(sizes[:3]), 3), "one_byte_less": (sum(sizes[:3]) - 1, 2),
                     "first_alone_over_budget": (sizes[0] - 1, 1)}[case]
    whole = Raw(model, seqs)
    capfd.readouterr()
    with LG.options(engine.context(), hmm_fb_budget=budget, debug=1):
        cut = Raw(model, seqs)
    got = [tuple(int(g) for g in m.groups()) for m in
           re.finditer(r"posterior launch: sequences (\d+)\.\.(\d+), (\d+) bytes of forward matrix", capfd.readouterr().err)]
    assert got == planned_launches(off, row, budget) and got[0] == (0, first, sum(sizes[:first]))
    assert whole.same_bits(cut)


def test_counts_row_in_global_memory_gives_the_same_bits(batch_300):
    """Option hmm_expect_lds 0 keeps the sequence's counts row in global memory (the route a model takes by itself when
    the row does not fit LDS beside the score rows): the same additions in the same order."""
    from pypore_amd import engine
    model, seqs, raw = batch_300
    with LG.options(engine.context(), hmm_expect_lds=0):
        glob = Raw(model, seqs)
    assert raw.same_bits(glob)


def test_outputs_are_optional_and_calls_repeat(batch_300):
    model, seqs, raw = batch_300
    ctx, off, obs = model._upload(seqs, None)
    lp, post, state, mlp, counts = ctx.hmm_posterior(model._c_model(), obs, off, want_post=False, want_map=True)
    assert post is None and counts is None
    assert np.array_equal(state.cpu().numpy(), raw.state_all) and np.array_equal(mlp.cpu().numpy(), raw.map_logp)
    lp, post, state, mlp, counts = ctx.hmm_posterior(model._c_model(), obs, off, want_post=True, want_map=False)
    assert state is None and mlp is None and counts is None
    assert np.array_equal(post.cpu().numpy(), raw.post_all) and np.array_equal(lp.cpu().numpy(), raw.logp)
    lp, post, state, mlp, counts = ctx.hmm_posterior(model._c_model(), obs, off, want_post=False, want_map=False, want_counts=True)
    assert np.array_equal(counts.cpu().numpy(), raw.counts)


# ---- exact tie ----------------------------------------------------------------------------------------------------------
def test_exact_tie_goes_to_the_lower_index():
    """Two emitting states sharing one distribution object, mirrored edges: both posteriors of every row are bit-equal
    maxima, and the lower index is returned at every step."""
    model = mirrored_model()
    rng = np.random.default_rng(4)
    seqs = [rng.normal(0.5, 1.0, n) for n in (33, 1, 130)]
    raw = Raw(model, seqs)
    c = O.Compiled(model)
    for q, s in enumerate(seqs):
        want = PO.posterior(c, s)
        assert (want.gap == 0).all()
        post = raw.post(q)
        assert np.isfinite(post).all() and np.array_equal(post[:, 0], post[:, 1])
        assert (raw.state(q) == 0).all()
        assert_close(post, want.post)
        assert raw.map_logp[q] == PO.ordered_sum(post[:, 0])
    path = model.maximum_a_posteriori(seqs[0])[1]
    assert [i for i, _ in path] == [0] * 33 and all(s is model.states[0] for _, s in path)


# ---- agreement with the E-step --------------------------------------------------------------------------------------------
def test_agrees_with_expected_counts_batch():
    model, means = O.profile_model(20, seed=3)
    seqs = O.profile_events(means, 40, lo=5, hi=60, seed=8)
    est = model.expected_counts_batch(seqs)
    fb = model.forward_backward_batch(seqs)
    src = [e[0] for e in model.edges]
    dst = [e[1] for e in model.edges]
    counts = np.sum([t[src, dst] for t, _ in fb], axis=0, dtype=np.float64)
    weight = np.sum([np.exp(em).sum(axis=0) for _, em in fb], axis=0, dtype=np.float64)
    assert est.skipped == 0 and counts.shape == est.counts.shape and weight.shape == est.stats[:, 0].shape
    for got, want in ((counts, est.counts), (weight, est.stats[:, 0])):
        err = np.abs(got - want) / np.where(want > 0, want, 1.0)
        print("max relative difference %.3g" % err.max())
        assert (err <= 1e-10).all()
    # every transitions array is dense over `states` and zero off the model's edges
    off_edges = np.ones((len(model.states),) * 2, bool)
    off_edges[src, dst] = False
    assert all(t.shape == off_edges.shape and not t[off_edges].any() for t, _ in fb)


# ---- public surface -------------------------------------------------------------------------------------------------------
def test_apply_hmm_and_return_shapes():
    from pypore_amd.parsers import SpeedyStatSplit
    from test_hmm_gpu import _level_model, _synthetic_event
    rng = np.random.default_rng(21)
    levels = [30.0, 45.0, 25.0, 50.0, 35.0]
    model = _level_model(levels)
    ev = _synthetic_event(rng, levels)
    ev.parse(SpeedyStatSplit(prior_segments_per_second=10))
    means = np.array([s.mean for s in ev.segments])
    assert means.size >= 2
    logp, path = ev.apply_hmm(model, algorithm='maximum_a_posteriori')
    want_logp, want_path = model.maximum_a_posteriori(means)
    assert logp == want_logp and [i for i, _ in path] == [i for i, _ in want_path] and len(path) == means.size
    assert all(s is model.states[i] and not s.is_silent() for i, s in path)
    check = PO.posterior(O.Compiled(model), means)
    clear = check.gap >= GAP
    assert (~clear).sum() <= means.size // 1000
    assert np.array_equal(np.array([i for i, _ in path])[clear], check.state[clear])
    assert_close([logp], [check.map_logp], tol=TOL * means.size)
    transitions, emissions = ev.apply_hmm(model, algorithm='forward_backward')
    S, NE = len(model.states), model.flat["n_emit"]
    assert transitions.shape == (S, S) and transitions.dtype == np.float64
    assert emissions.shape == (means.size, NE) and emissions.dtype == np.float64
    assert_close(emissions, check.post)
    both = model.forward_backward_batch([means, means[:3], []])
    assert [e.shape for _, e in both] == [(means.size, NE), (3, NE), (0, NE)] and np.array_equal(both[0][1], emissions)
    assert model.forward_backward([])[0].shape == (S, S)


def test_impossible_empty_and_too_large():
    from pypore_amd.hmm import UniformDistribution
    u = Model("u")
    a = State(UniformDistribution(0, 1), "a")
    b = State(NormalDistribution(0.5, 1.0), "b")
    u.add_transition(u.start, a, 0.6)
    u.add_transition(u.start, b, 0.2)
    u.add_transition(u.start, u.end, 0.2)
    u.add_transition(a, a, 0.5)
    u.add_transition(a, u.end, 0.5)
    u.add_transition(b, u.end, 1.0)
    u.bake()
    assert u.maximum_a_posteriori([0.5, 3.0]) == (-np.inf, None)
    assert u.maximum_a_posteriori([]) == (0.0, [])
    res = u.maximum_a_posteriori_batch([[0.2], [2.0, 2.0], [], [0.3, 0.4]])
    assert res[1] == (-np.inf, None) and res[2] == (0.0, [])
    assert [i for i, _ in res[3][1]] == [0, 0] and abs(res[3][0]) <= 2 * TOL   # only a can emit twice: log posterior log 1
    transitions, emissions = u.forward_backward([2.0, 2.0])
    assert not transitions.any() and emissions.shape == (2, 2) and np.isneginf(emissions).all()
    assert u.maximum_a_posteriori_batch([]) == [] and u.forward_backward_batch([]) == []
    over = O.line_model(4097)
    assert len(over.states) == 4097
    with pytest.raises(ValueError, match="4096"):
        over.maximum_a_posteriori([0.0])
    with pytest.raises(ValueError, match="4096"):
        over.forward_backward_batch([[0.0]])
