"""Mixture states (MixtureDistribution, kind 7) on the MI355X: the HmmDevM instantiations of the HMM kernels
(csrc/seg_hmm.hpp) against tests/mixture_oracle.py, which tests/test_mixture_host.py holds to brute-force path enumeration.

Bits.  A model of normal and uniform states whose every distribution is wrapped in a one-component mixture of weight 1
gives the bits of the plain model in every output (compared with ==), and its E-step's component rows are the plain
model's state rows.

Tolerances where bits cannot be asked for (the device's log, exp and log1p are not numpy's), the project's own from
tests/test_multivariate_gpu.py and tests/test_hmm_train_gpu.py: log values -- log probabilities, forward and backward
matrices, log posteriors -- TOL = 1e-12 relative to max(1, |oracle|), -inf exactly where the oracle has -inf; per-sequence
edge counts by the bound derived in tests/test_posterior_gpu.py (it does not look at the emission); batch counts and
statistics, the component rows included, and trained parameters STAT_TOL = 1e-9 relative to max(1, |oracle|).  A component
row multiplies the state's posterior by a responsibility exp(v_i - e) of two log values that are each within TOL of the
oracle's, which is inside what the 1e-9 already allows the posterior itself.  Viterbi paths are compared on every input;
tests/test_mixture_host.py asserts with the oracle alone that none of them has a decision within 1e-9.
Every comparison prints its largest error before it asserts.  Measured on one MI355X: log values within 2.3e-13 of the
oracle; component rows within 2.3e-13 on the 2 495-component model of the LDS test and within 4.6e-15 everywhere else, the
brute-force enumeration on the tiny models included; trained parameters 3.9e-16; sampled values 2.2e-16.

yahmm is not available to compare against; nothing here is compared with it."""
import ctypes
import math
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import mixture_oracle as MX  # noqa: E402
import posterior_oracle as PO  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution,  # noqa: E402
                            MixtureDistribution, Model, NormalDistribution, State, UniformDistribution)

pytestmark = pytest.mark.gpu
TOL = 1e-12
STAT_TOL = 1e-9


def assert_close(got, want, tol=TOL, what="values"):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin])), what
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    print("%s: max error %.3g over %d entries (bound %.3g)" % (what, err.max() if err.size else 0.0, err.size, tol))
    assert err.size == 0 or err.max() <= tol, (what, err.max())


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


class Decoded(object):
    """Every output of the library for one batch, as numpy arrays: what two routes must agree on bit for bit."""

    def __init__(self, model, seqs):
        from pypore_amd import _lib
        ctx, off, obs = model._upload(seqs, None)
        cm = model._c_model()
        self.off = off
        logp, mat, (path, path_off, path_len) = ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, obs, off, True)
        self.v_logp, self.v_mat = logp.cpu().numpy(), mat.cpu().numpy()
        path, path_len = path.cpu().numpy(), path_len.cpu().numpy()
        self.paths = [path[path_off[q]:path_off[q] + path_len[q]].tolist() if self.v_logp[q] > -np.inf else None
                      for q in range(len(seqs))]
        logp, mat, _ = ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off, True)
        self.f_logp, self.f_mat = logp.cpu().numpy(), mat.cpu().numpy()
        logp, mat, _ = ctx.hmm_batch(cm, _lib.PS_HMM_BACKWARD, obs, off, True)
        self.b_logp, self.b_mat = logp.cpu().numpy(), mat.cpu().numpy()
        self.logp = ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off, False)[0].cpu().numpy()
        plogp, post, state, map_logp, counts = ctx.hmm_posterior(cm, obs, off, want_post=True, want_map=True, want_counts=True)
        self.p_logp, self.post, self.state = plogp.cpu().numpy(), post.cpu().numpy(), state.cpu().numpy()
        self.map_logp, self.seq_counts = map_logp.cpu().numpy(), counts.cpu().numpy()
        elogp, ecounts, stats, self.skipped = ctx.hmm_expect(cm, obs, off, 3, mix_rows=model._n_mix)
        self.e_logp, self.e_counts, self.stats = elogp.cpu().numpy(), ecounts.cpu().numpy(), stats.cpu().numpy()
        self.fields = ["v_logp", "v_mat", "paths", "f_logp", "f_mat", "b_logp", "b_mat", "logp", "p_logp", "post", "state",
                       "map_logp", "seq_counts", "e_logp", "e_counts", "stats", "skipped"]

    def rows(self, mat, q):
        return mat[self.off[q] + q:self.off[q + 1] + q + 1]

    def differing(self, other, fields=None):
        return [k for k in (fields or self.fields)
                if not (getattr(self, k) == getattr(other, k) if k in ("paths", "skipped") else same(getattr(self, k), getattr(other, k)))]


# ---- 1. bit equality with the plain kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,finite", [(1, True), (2, False), (3, True)])
def test_wrapped_model_gives_the_plain_bits(seed, finite):
    rng = np.random.default_rng(9000 + seed)
    plain = O.random_model(rng, max_states=140, max_chain=20, finite=finite)
    mix = MX.wrapped(plain)
    NE = plain.flat["n_emit"]
    assert (mix.flat["kind"][:NE] == 7).all() and mix._n_mix == NE and plain._n_mix == 0 and mix.flat["n_levels"] == plain.flat["n_levels"]
    assert [s.name for s in plain.states] == [s.name for s in mix.states]
    assert plain.edges == mix.edges and same(plain.flat["in_lp"], mix.flat["in_lp"]) and not mix.flat["param"].any()
    seqs = [rng.normal(0, 2, n) for n in (0, 1, 2, 65, 7, 30)] + [np.full(3, 1e300)]
    a, b = Decoded(plain, seqs), Decoded(mix, seqs)
    assert a.stats.shape == (NE, 3) and b.stats.shape == (2 * NE, 3)
    assert a.differing(b, [k for k in a.fields if k != "stats"]) == []
    assert same(b.stats[NE:], a.stats)                                               # the component rows: the plain states' rows
    assert same(b.stats[:NE, 0], a.stats[:, 0]) and np.isfinite(a.logp).any() and a.stats[:, 0].sum() > 1


# ---- 2. every pass against the oracle ---------------------------------------------------------------------------------
CASES = {}


def case(name):
    if not CASES:
        for n, model, seqs in MX.viterbi_inputs():
            CASES[n] = (model, seqs)
    return CASES[name]


def check_counts_per_sequence(got, want_counts, logp, n, what):
    with np.errstate(divide="ignore"):
        size = np.where(want_counts > 0, np.abs(np.log(np.where(want_counts > 0, want_counts, 1.0))), 0.0)
    rel = 4 * TOL * np.maximum(1.0, abs(logp) + size + 80.0) + (n + 1) * 2.0 ** -52      # (tests/test_posterior_gpu.py)
    err = np.abs(got - want_counts)
    print("%s: max error / bound %.3g" % (what, (err / (rel * want_counts + 1e-300)).max() if err.size else 0.0))
    assert (err <= rel * want_counts + 1e-300).all(), what


def check_every_pass(name, model, seqs, brute=False):
    got = Decoded(model, seqs)
    results = model.viterbi_batch(seqs)
    NE, n_mix = model.flat["n_emit"], model._n_mix
    tot_counts, tot_stats, skipped = np.zeros(len(model.edges)), np.zeros((NE + n_mix, 3)), 0
    assert got.stats.shape == (NE + n_mix, 3) and n_mix > 0
    for q, s in enumerate(seqs):
        n, tag = len(s), "%s[%d]" % (name, q)
        lp, path, gap, ties, _ = MX.viterbi_ties(model, s)
        assert_close([got.v_logp[q]], [lp], TOL, tag + " viterbi logp")
        if path is None:
            assert got.paths[q] is None and results[q] == (-np.inf, None)
        else:
            assert ties == 0 and gap > 1e-9                                          # (the host test's condition)
            assert got.paths[q] == path and [i for i, _ in results[q][1]] == path, tag
        want = MX.posterior(model, s)
        assert_close(got.rows(got.f_mat, q), MX.forward(model, s), TOL, tag + " forward")
        assert_close(got.rows(got.b_mat, q), MX.backward(model, s), TOL, tag + " backward")
        for k in ("f_logp", "b_logp", "logp", "p_logp", "e_logp"):
            assert_close([getattr(got, k)[q]], [want.logp], TOL, tag + " " + k)
        assert got.f_logp[q] == got.logp[q] == got.p_logp[q] == got.e_logp[q]
        post, state = got.post[got.off[q]:got.off[q + 1]], got.state[got.off[q]:got.off[q + 1]]
        assert_close(post, want.post, TOL, tag + " log posteriors")
        if not want.logp > -np.inf:
            skipped += 1
            assert (state == -1).all() and got.map_logp[q] == -np.inf and not got.seq_counts[q].any()
            continue
        clear = want.gap >= 1e-9
        assert np.array_equal(state[clear], want.state[clear]) and clear.sum() >= n - n // 1000
        assert got.map_logp[q] == PO.ordered_sum(post[t, k] for t, k in enumerate(state))
        assert_close([got.map_logp[q]], [want.map_logp], TOL * max(1, n), tag + " MAP logp")
        check_counts_per_sequence(got.seq_counts[q], want.counts, want.logp, n, tag + " counts")
        cc, st, elp = MX.estep_one(model, s)
        assert elp == want.logp
        if brute:
            F, blp, best, bpath = MX.brute_force(model, s)
            bc, bs, _ = MX.estep_brute_force(model, s)
            assert_close(got.rows(got.f_mat, q), F, TOL, tag + " forward, brute force")
            assert_close([got.logp[q], got.v_logp[q]], [blp, best], TOL, tag + " logp, brute force")
            assert got.paths[q] == bpath
            one = model.expected_counts_batch([s])
            assert_close(one.counts, bc, STAT_TOL, tag + " counts, brute force")
            assert_close(one.stats, bs, STAT_TOL, tag + " statistics with component rows, brute force")
        tot_counts += cc
        tot_stats += st
    assert got.skipped == skipped
    assert_close(got.e_counts, tot_counts, STAT_TOL, name + " batch counts")
    assert_close(got.stats[:NE], tot_stats[:NE], STAT_TOL, name + " state rows")
    assert_close(got.stats[NE:], tot_stats[NE:], STAT_TOL, name + " component rows")
    assert tot_stats[NE:, 0].sum() > 0
    # the public methods return the same numbers in their own shapes
    q = len(seqs) - 1 if np.isfinite(got.logp[len(seqs) - 1]) else int(np.flatnonzero(np.isfinite(got.logp))[-1])
    s = seqs[q]
    assert model.log_probability(s) == got.logp[q] and same(model.forward(s), got.rows(got.f_mat, q))
    assert same(model.backward(s), got.rows(got.b_mat, q))
    transitions, emissions = model.forward_backward(s)
    assert same(emissions, got.post[got.off[q]:got.off[q + 1]]) and same(model.expected_transitions(s), got.seq_counts[q])
    mlp, mpath = model.maximum_a_posteriori(s)
    assert mlp == got.map_logp[q] and [i for i, _ in mpath] == got.state[got.off[q]:got.off[q + 1]].tolist()
    est = model.expected_counts_batch(seqs)
    assert same(est.counts, got.e_counts) and same(est.stats, got.stats) and est.stats.shape == (NE + n_mix, 3)
    return got


@pytest.mark.parametrize("n_emit", [63, 64, 65, 130])
def test_line_models_every_pass_against_the_oracle(n_emit):
    model, seqs = case("line%d" % n_emit)
    kinds = model.flat["kind"][:n_emit]
    assert np.flatnonzero(kinds == 7).tolist() == [i for i in MX.MIX_LANES if i < n_emit]
    sizes = np.diff(model._mix["mix_ptr"])[kinds == 7].tolist()
    assert sizes == [1, 2, 7, 1, 2, 7, 1, 2][:len(sizes)] and len(sizes) >= 3 and np.isneginf(model._mix["mix_lw"]).any()
    assert [len(s) for s in seqs] == [0, 1, 2, 65, 3] and len(set(model._mix["mix_kind"].tolist())) >= 3
    got = check_every_pass("line%d" % n_emit, model, seqs)
    assert got.logp[0] == -np.inf and np.isfinite(got.logp[1:4]).all()


@pytest.mark.parametrize("finite", [True, False])
def test_silent_levels_and_a_kernel_density_beside_mixtures(finite):
    model, seqs = case("silent-%s" % ("finite" if finite else "infinite"))
    assert model.flat["n_levels"] >= 5 and model.finite == finite and sorted(set(model.flat["kind"][:6].tolist())) == [1, 2, 3, 7]
    got = check_every_pass("silent", model, seqs)
    assert np.isfinite(got.logp[1:]).all()


@pytest.mark.parametrize("finite", [True, False])
def test_tiny_models_against_brute_force_component_rows_included(finite):
    model, seqs = case("tiny-%s" % ("finite" if finite else "infinite"))
    assert model.flat["n_emit"] == 3 and max(len(s) for s in seqs) == 5
    check_every_pass("tiny", model, seqs, brute=True)


# ---- 3. a mixture of equal normals is a kernel density ----------------------------------------------------------------
def test_mixture_of_equal_std_normals_agrees_with_the_kernel_density():
    rng = np.random.default_rng(33)
    points, weights, h = rng.uniform(20, 60, 9), rng.uniform(0.1, 1.0, 9), 1.3
    weights[4] = 0.0

    def build(d):
        m = Model("dens")
        a, b = State(d, "a"), State(NormalDistribution(40.0, 8.0), "b")
        for x, y, p in ((m.start, a, 0.6), (m.start, b, 0.4), (a, a, 0.5), (a, b, 0.4), (a, m.end, 0.1), (b, a, 0.5), (b, b, 0.4), (b, m.end, 0.1)):
            m.add_transition(x, y, p)
        m.bake()
        return m
    kde = build(GaussianKernelDensity(points, h, weights))
    mix = build(MixtureDistribution([NormalDistribution(float(p), h) for p in points], weights))
    seqs = [rng.uniform(10, 70, n) for n in (1, 2, 17, 65)] + [np.array([500.0, -400.0])]      # the last: far from every point
    a, b = kde.log_probability_batch(seqs), mix.log_probability_batch(seqs)
    assert np.isfinite(a).all()
    assert_close(b, a, TOL, "mixture against kernel density")
    assert_close(b, [MX.log_probability(mix, s) for s in seqs], TOL, "mixture against the oracle")


# ---- 4. the E-step's LDS limit ----------------------------------------------------------------------------------------
def lds_model(J):
    """A chain of 100 emitting states, E = 201 edges; states 0 and 64 are mixtures of 2000 and J - 2000 components."""
    rng = np.random.default_rng(J)
    m = Model("lds")

    def comps(n, level):
        out = []
        for j in range(n):
            c = level + float(rng.normal(0, 3))
            out.append((NormalDistribution(c, 1.0), UniformDistribution(c - 6, c + 6), LogNormalDistribution(math.log(c), 0.1))[j % 3])
        return MixtureDistribution(out, rng.uniform(0.1, 1.0, n))
    st = [State(comps(2000, 30.0) if i == 0 else comps(J - 2000, 40.0) if i == 64 else NormalDistribution(30.0 + 0.2 * i, 2.0),
                "s%03d" % i) for i in range(100)]
    m.add_transition(m.start, st[0], 1.0)
    for i, s in enumerate(st):
        m.add_transition(s, s, 0.5)
        m.add_transition(s, st[i + 1] if i + 1 < 100 else m.end, 0.5)
    m.bake()
    return m


def expect_lds_bytes(model):
    S, E, NE = len(model.states), len(model.edges), model.flat["n_emit"]
    return 16 * S + 8 * (E + 3 * (NE + model._n_mix) + 1)


@pytest.mark.parametrize("J,in_lds", [(2495, True), (2496, False)])
def test_estep_on_both_sides_of_its_lds_limit(J, in_lds, capfd):
    """16 S + 8 n_acc <= 64 KiB with S = 102 and n_acc = E + 3 (n_emit + n_mix) + 1 = 201 + 3 (100 + J) + 1:
    5648 + 24 J <= 65536 holds up to J = 2495 (65528 bytes) and fails from J = 2496 (65552): n_mix carries n_acc across."""
    from pypore_amd import engine
    model = lds_model(J)
    assert model._n_mix == J and expect_lds_bytes(model) == 5648 + 24 * J and (expect_lds_bytes(model) <= 65536) == in_lds
    rng = np.random.default_rng(J)
    seqs = [30.0 + 0.2 * np.minimum(np.cumsum(rng.integers(0, 2, n)), 99) + rng.normal(0, 2, n) for n in (100, 120, 150)]
    seqs += [np.zeros(0), 30.0 + 0.2 * np.arange(99) + rng.normal(0, 2, 99)]         # empty, and too short to reach end: skipped
    ctx = engine.context()
    capfd.readouterr()
    with LG.options(ctx, debug=1):
        got = model.expected_counts_batch(seqs)
    lds = expect_lds_bytes(model) if in_lds else 16 * len(model.states)
    assert LG.printed_slots(capfd.readouterr().err, lds), "no E-step launch with %d bytes of dynamic LDS" % lds
    again = model.expected_counts_batch(seqs)
    assert same(again.counts, got.counts) and same(again.stats, got.stats) and same(again.logp, got.logp)
    counts, stats, logp, skipped = MX.estep(model, seqs[:1] + seqs[3:])
    part = model.expected_counts_batch(seqs[:1] + seqs[3:])
    assert_close(part.logp, logp, TOL, "logp")
    assert part.skipped == skipped == 2 and got.skipped == 2
    assert_close(part.counts, counts, STAT_TOL, "counts")
    assert_close(part.stats, stats, STAT_TOL, "statistics")
    assert part.stats[100:2100, 0].sum() > 0.5 and part.stats[2100:, 0].sum() > 0.5
    if in_lds:
        with LG.options(ctx, hmm_expect_lds=0):
            glob = model.expected_counts_batch(seqs)
        assert same(glob.logp, got.logp)
        assert_close(glob.counts, got.counts, 1e-12, "counts, accumulators in global memory")
        assert_close(glob.stats, got.stats, 1e-12, "statistics, accumulators in global memory")


# ---- 5. batch cutting -------------------------------------------------------------------------------------------------
def test_cut_batches_small_grid_and_a_batch_of_300():
    from pypore_amd import engine
    model, _ = case("silent-infinite")
    levels = np.array([20.0, 28.0, 36.0, 44.0, 52.0, 60.0])
    rng = np.random.default_rng(12)
    seqs = [levels[rng.integers(0, 6, n)] + rng.normal(0, 1.5, n) for n in rng.integers(1, 40, 300)]
    seqs[17] = np.zeros(0)
    seqs[231] = np.full(4, -1e300)                                                   # impossible in every state
    ctx = engine.context()
    whole = Decoded(model, seqs)
    assert whole.v_logp[231] == -np.inf and whole.logp[231] == -np.inf and whole.skipped == 1 and np.isfinite(whole.logp[17])
    S = len(model.states)
    per_seq = [k for k in whole.fields if k not in ("e_counts", "stats")]
    with LG.options(ctx, hmm_fb_budget=8 * S * 45, hmm_bp_budget=S * 45):            # two or three sequences per launch
        cut = Decoded(model, seqs)
    assert whole.differing(cut, per_seq) == []
    assert_close(cut.e_counts, whole.e_counts, 1e-12, "counts, cut batch")
    assert_close(cut.stats, whole.stats, 1e-12, "statistics, cut batch")
    with LG.options(ctx, slots_pct=1):
        small = Decoded(model, seqs)
    assert whole.differing(small, per_seq) == []
    assert_close(small.e_counts, whole.e_counts, 1e-12, "counts, slots_pct 1")
    assert_close(small.stats, whole.stats, 1e-12, "statistics, slots_pct 1")
    for q in (0, 17, 150, 231, 299):
        assert_close([whole.logp[q]], [MX.log_probability(model, seqs[q])], TOL, "logp[%d]" % q)
        assert_close([whole.v_logp[q]], [MX.viterbi_ties(model, seqs[q])[0]], TOL, "viterbi logp[%d]" % q)
    counts, stats, logp, skipped = MX.estep(model, seqs[:40])
    part = model.expected_counts_batch(seqs[:40])
    assert_close(part.counts, counts, STAT_TOL, "counts of 40")
    assert_close(part.stats, stats, STAT_TOL, "statistics of 40")


# ---- 6. the upload cache ----------------------------------------------------------------------------------------------
def test_upload_cache_sees_weight_parameter_kind_and_split():
    def build(weight=0.5, mean=24.0, second=NormalDistribution, split=2, d=None, e=None):
        comps = [NormalDistribution(mean, 2.0), second(3.4, 0.2) if second is LogNormalDistribution else second(30.0, 0.2),
                 NormalDistribution(36.0, 2.0), UniformDistribution(10.0, 60.0)]
        w = [weight, 1.0 - weight, 0.5, 0.5]
        m = Model("pair")
        a = State(d or MixtureDistribution(comps[:split], [x / sum(w[:split]) for x in w[:split]]), "a")
        b = State(e or MixtureDistribution(comps[split:], [x / sum(w[split:]) for x in w[split:]]), "b")
        for s, t, p in ((m.start, a, 0.5), (m.start, b, 0.5), (a, a, 0.5), (a, b, 0.5), (b, a, 0.5), (b, b, 0.3), (b, m.end, 0.2)):
            m.add_transition(s, t, p)
        m.bake()
        return m
    base, weight, param, kind = build(), build(weight=0.625), build(mean=25.0), build(second=LogNormalDistribution)
    split = build(weight=0.5, split=1)
    tables = ("mix_ptr", "mix_kind", "mix_param", "mix_lw")
    for other, changed in ((weight, {"mix_lw"}), (param, {"mix_param"}), (kind, {"mix_kind", "mix_param"})):
        assert {k for k in tables if not same(base._mix[k], other._mix[k])} == changed
        assert all(same(v, other.flat[k]) for k, v in base.flat.items() if isinstance(v, np.ndarray))
    assert same(base._mix["mix_kind"], split._mix["mix_kind"]) and same(base._mix["mix_param"], split._mix["mix_param"])
    assert base._mix["mix_ptr"].tolist() == [0, 2, 4] and split._mix["mix_ptr"].tolist() == [0, 1, 4]
    plain = build(d=NormalDistribution(24.0, 2.0), e=NormalDistribution(36.0, 2.0))
    kde = build(d=GaussianKernelDensity([24.0, 30.0], 2.0), e=NormalDistribution(36.0, 2.0))
    rng = np.random.default_rng(8)
    seqs = [rng.uniform(18, 42, n) for n in (5, 9)]
    models = (base, weight, param, kind, split)
    want = {id(m): [MX.log_probability(m, s) for s in seqs] for m in models}
    c = O.Compiled(plain)
    want[id(plain)] = [O.log_probability(c, s) for s in seqs]
    want[id(kde)] = [MX.log_probability(kde, s) for s in seqs]
    first = {}
    for m in (base, weight, base, param, kind, base, split, weight, split, kind, param,
              base, plain, base, kde, split, plain, kde, weight):
        lp, vit = m.log_probability_batch(seqs), m.viterbi_batch(seqs)
        est = m.expected_counts_batch(seqs)
        assert_close(lp, want[id(m)], TOL, "logp")
        assert same(est.logp, lp) and est.stats.shape == (2 + m._n_mix, 3)
        if id(m) in first:
            assert same(lp, first[id(m)][0]) and [v[0] for v in vit] == first[id(m)][1] and same(est.stats, first[id(m)][2])
        first[id(m)] = (lp, [v[0] for v in vit], est.stats)
    for m in models[1:]:
        assert not same(first[id(base)][0], first[id(m)][0])
    counts, stats, _, _ = MX.estep(split, seqs)
    assert_close(first[id(split)][2], stats, STAT_TOL, "statistics of the split model")


# ---- 7. the ABI -------------------------------------------------------------------------------------------------------
def copy_of(cm):
    from pypore_amd import _lib
    m = _lib.HmmModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(cm), ctypes.sizeof(m))
    return m


MIX_FIELDS = ("mix_ptr", "mix_kind", "mix_param", "mix_lw", "mix_cdf", "mix_draw")


def test_appended_fields_are_ignored_without_kind_7():
    from pypore_amd import _lib
    model, means = O.profile_model(20, seed=9)
    other, _ = case("line64")
    seqs = O.profile_events(means, 6, lo=10, hi=60, seed=3)
    ctx, off, obs = model._upload(seqs, None)
    base = model._c_model()
    assert not any(getattr(base, k) for k in MIX_FIELDS)                              # NULL, as an older caller leaves them
    alt, junk = copy_of(base), copy_of(base)
    for k in MIX_FIELDS:
        setattr(alt, k, other._mix[k].ctypes.data)
        setattr(junk, k, 8)                                                          # no address of anything
    tables = model._sample_tables()["c"]
    for cm in (alt, junk):
        for mode in (_lib.PS_HMM_VITERBI, _lib.PS_HMM_FORWARD, _lib.PS_HMM_BACKWARD):
            la, ma, pa = ctx.hmm_batch(base, mode, obs, off, True)
            lb, mb, pb = ctx.hmm_batch(cm, mode, obs, off, True)
            assert same(la.cpu().numpy(), lb.cpu().numpy()) and same(ma.cpu().numpy(), mb.cpu().numpy())
            if mode == _lib.PS_HMM_VITERBI:
                (xa, oa, na), (xb, ob, nb) = [(p[0].cpu().numpy(), p[1], p[2].cpu().numpy()) for p in (pa, pb)]
                assert same(na, nb) and same(oa, ob) and (na > 0).any()
                assert all(same(xa[oa[q]:oa[q] + na[q]], xb[ob[q]:ob[q] + nb[q]]) for q in range(len(seqs)))
        ea, eb = ctx.hmm_expect(base, obs, off), ctx.hmm_expect(cm, obs, off)
        assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(ea[:3], eb[:3])) and ea[3] == eb[3]
        pa, pb = ctx.hmm_posterior(base, obs, off, True, True, True), ctx.hmm_posterior(cm, obs, off, True, True, True)
        assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(pa, pb))
        sa, sb = ctx.hmm_sample(base, tables, 5, 0, 20), ctx.hmm_sample(cm, tables, 5, 0, 20)
        assert same(sa[3].cpu().numpy(), sb[3].cpu().numpy()) and same(sa[2], sb[2])
        la, lb = sa[3].cpu().numpy(), sb[3].cpu().numpy()
        xa, xb = sa[1].cpu().numpy().reshape(-1), sb[1].cpu().numpy().reshape(-1)
        assert all(same(xa[sa[2][q]:sa[2][q] + la[q]], xb[sb[2][q]:sb[2][q] + lb[q]]) for q in range(20)) and la.sum() > 0
    c = O.Compiled(model)
    assert_close(ctx.hmm_batch(base, _lib.PS_HMM_FORWARD, obs, off, False)[0].cpu().numpy(), [O.log_probability(c, s) for s in seqs])


def test_bad_mixture_structs_are_refused_with_their_messages():
    from pypore_amd import _lib
    model, seqs = case("tiny-finite")
    seqs = [seqs[4]]
    ctx, off, obs = model._upload(seqs, None)
    base, f, x = model._c_model(), model.flat, model._mix
    tables = model._sample_tables()["c"]
    assert f["kind"][:3].tolist() == [7, 1, 7] and x["mix_ptr"].tolist() == [0, 4, 4, 6]
    keep = []

    def with_array(field, arr):
        keep.append(arr)
        m = copy_of(base)
        setattr(m, field, arr.ctypes.data)
        return m

    def changed(field, index, value):
        arr = (f[field] if field in f else x[field]).copy()
        arr[index] = value
        return with_array(field, arr)

    def null(field):
        m = copy_of(base)
        setattr(m, field, None)
        return m

    needs = "mix_ptr, mix_kind, mix_param and mix_lw"
    bad = [(changed("kind", 1, 4), "cannot be mixed"),
           (null("mix_ptr"), needs), (null("mix_kind"), needs), (null("mix_param"), needs), (null("mix_lw"), needs),
           (changed("mix_ptr", 0, 1), "mix_ptr must start at 0"),
           (with_array("mix_ptr", np.array([0, 4, 3, 6], np.int32)), "descending mix_ptr at state 1"),
           (with_array("mix_ptr", np.array([0, 4, 5, 6], np.int32)), "state 1: a mixture state has at least one component, any other state none"),
           (with_array("mix_ptr", np.array([0, 4, 4, 4], np.int32)), "state 2: a mixture state has at least one component"),
           (with_array("mix_ptr", np.array([0, 4, 4, (1 << 24) + 1], np.int32)), "16777217 mixture components"),
           (changed("mix_kind", 0, 3), "mixture component 0: unknown component kind 3"),
           (changed("mix_kind", 5, 7), "mixture component 5: unknown component kind 7"),
           (changed("mix_kind", 2, 0), "unknown component kind 0"), (changed("mix_kind", 1, 4), "unknown component kind 4"),
           (changed("mix_lw", 0, np.nan), "mixture component 0: a log weight must be <= 0"),
           (changed("mix_lw", 4, 0.5), "mixture component 4: a log weight"), (changed("mix_lw", 5, np.inf), "a log weight must be <= 0")]
    for cm, message in bad:
        with pytest.raises(ValueError, match=message):
            ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off, False)
        with pytest.raises(ValueError, match=message):
            ctx.hmm_expect(cm, obs, off, 3, mix_rows=model._n_mix)
        with pytest.raises(ValueError, match=message):
            ctx.hmm_posterior(cm, obs, off)
        with pytest.raises(ValueError, match=message):
            ctx.hmm_sample(cm, tables, 1, 0, 4)
    assert_close([model.log_probability(seqs[0])], [MX.log_probability(model, seqs[0])], TOL, "the context still works")
    # mix_cdf and mix_draw are ps_hmm_sample's alone
    for field in ("mix_cdf", "mix_draw"):
        cm = null(field)
        want = [t.cpu().numpy() for t in ctx.hmm_expect(base, obs, off, 3, mix_rows=model._n_mix)[:3]]
        got = [t.cpu().numpy() for t in ctx.hmm_expect(cm, obs, off, 3, mix_rows=model._n_mix)[:3]]
        assert all(same(a, b) for a, b in zip(got, want))
        assert same(ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, obs, off, False)[0].cpu().numpy(),
                    ctx.hmm_batch(base, _lib.PS_HMM_VITERBI, obs, off, False)[0].cpu().numpy())
        assert same(ctx.hmm_posterior(cm, obs, off)[0].cpu().numpy(), want[0])
        with pytest.raises(ValueError, match="mix_cdf and mix_draw"):
            ctx.hmm_sample(cm, tables, 1, 0, 4)
    with pytest.raises(ValueError, match="mix_cdf of state 0"):
        ctx.hmm_sample(changed("mix_cdf", 3, 0.5), tables, 1, 0, 4)
    with pytest.raises(ValueError, match="mix_draw 1 is not finite"):
        ctx.hmm_sample(changed("mix_draw", 1, np.nan), tables, 1, 0, 4)
    want = MX.batch(model, 4, 1)
    got = model.sample_batch(4, seed=1)
    assert [len(g) for g in got] == [len(w.obs) for w in want]                        # the context still samples


# ---- 8. training ------------------------------------------------------------------------------------------------------
def all_parameters(model):
    out = []
    for s in model.states[:model.flat["n_emit"]]:
        for d, w in MX.slots(s.distribution) or [(s.distribution, None)]:
            out += list(d.parameters) + ([] if w is None else [w])
    return out


@pytest.mark.parametrize("algorithm", ["baum-welch", "viterbi"])
def test_one_training_iteration_against_the_oracle(algorithm):
    model, seqs = MX.training_model(), MX.training_data()
    assert case("train")[1][0].tolist() == seqs[0].tolist()                           # (the inputs the host test examined)
    want, steps, total = MX.train(model, seqs, 1, algorithm=algorithm, min_std=0.05)
    frozen = model.states[4].distribution
    frozen_before = [list(d.parameters) for d in frozen.parameters[0]] + [list(frozen.parameters[1])]
    before = all_parameters(model)
    got_total = model.train(seqs, max_iterations=1, algorithm=algorithm, min_std=0.05, verbose=False)
    print("improvement %.17g, oracle %.17g" % (got_total, total))
    assert abs(got_total - total) <= 1e-9 * max(1.0, abs(total)) and abs(total) > 1e-3
    assert_close(all_parameters(model), all_parameters(want), STAT_TOL, "trained parameters and weights")
    assert_close([p for _, _, p in model.edges], [p for _, _, p in want.edges], STAT_TOL, "trained edges")
    assert [list(d.parameters) for d in frozen.parameters[0]] + [list(frozen.parameters[1])] == frozen_before
    assert model.states[0].distribution is model.states[1].distribution
    assert model.states[2].distribution.parameters[0][0] is model.states[3].distribution
    after = all_parameters(model)
    assert sum(a != b for a, b in zip(before, after)) >= 12
    kinds = model.states[5].distribution
    assert kinds.parameters[1][2] == 0.0 and kinds.parameters[0][3].parameters == [50.0, 80.0]     # zero weight stays; uniform untouched
    lw = model._mix["mix_lw"]
    assert np.isneginf(lw[model._mix["mix_ptr"][5] + 2]) and (lw <= 0).all()


def test_baum_welch_recovers_a_bimodal_state_from_sampled_data():
    truth = MX.bimodal_model(split=4.0, weight=0.35, std=1.2)
    seqs = truth.sample_batch(200, seed=77)
    assert sum(len(s) for s in seqs) > 800
    model = MX.bimodal_model(split=2.0, weight=0.5, std=2.5)
    start = float(model.log_probability_batch(seqs).sum())
    steps = [model.train(seqs, max_iterations=1, verbose=False) for _ in range(5)]
    end = float(model.log_probability_batch(seqs).sum())
    total = sum(steps)
    print("log likelihood %.6f -> %.6f, steps %s" % (start, end, steps))
    assert all(s >= -1e-8 * abs(total) for s in steps) and end > start + 1.0          # Baum-Welch never lowers the likelihood
    assert abs((end - start) - total) <= 1e-9 * abs(start)
    d = model.states[0].distribution
    lo, hi = sorted(c.parameters[0] for c in d.parameters[0])
    assert hi - lo > 4.0 and abs(sum(d.parameters[1]) - 1.0) < 1e-12                 # the modes moved apart from 28 and 32, towards 26 and 34


# ---- 9. sampling ------------------------------------------------------------------------------------------------------
def compare_walks(m, seqs, paths, want):
    worst = 0.0
    assert len(seqs) == len(paths) == len(want)
    for q, (x, p, w) in enumerate(zip(seqs, paths, want)):
        assert x.dtype == np.float64 and x.shape == (len(w.obs),), (q, x.shape, len(w.obs))
        assert [i for i, _ in p] == w.path, (q, [i for i, _ in p], w.path)
        for t, (v, exact) in enumerate(zip(w.obs, w.exact)):
            if exact:
                assert x[t] == v, (q, t, x[t], v)
            else:
                err = abs(x[t] - v) / max(1.0, abs(v))
                assert err <= TOL, (q, t, x[t], v)
                worst = max(worst, err)
    return worst


def test_200_walks_against_the_oracle():
    from pypore_amd import _lib, engine
    model, _ = case("silent-finite")
    seed = (0x9E3779B9 << 32) | 0x7F4A7C15
    for first in (0, 2 ** 32 + 5):
        want = MX.batch(model, 200, seed, first)
        seqs, paths = model.sample_batch(200, path=True, seed=seed, first=first)
        print("first %d: largest emission error %.3g" % (first, compare_walks(model, seqs, paths, want)))
        ctx = engine.context(None)
        flags = ctx.hmm_sample(model._c_model(), model._sample_tables()["c"], seed, first, 200)[4].cpu().numpy().tolist()
        assert flags == [w.flag for w in want] == [0] * 200
        used = {i for w in want for i in w.comp if i >= 0}
        weights = np.exp(model._mix["mix_lw"])
        assert len(used) >= 5 and all(weights[i] > 0 for i in used) and any(e for w in want for e in w.exact)
    # a batch cut in two
    whole, wp = model.sample_batch(200, path=True, seed=seed)
    a, ap = model.sample_batch(70, path=True, seed=seed)
    b, bp = model.sample_batch(130, path=True, seed=seed, first=70)
    assert [v.tobytes() for v in whole] == [v.tobytes() for v in a + b]
    assert [[i for i, _ in p] for p in wp] == [[i for i, _ in p] for p in ap + bp]
    # a full slot, then the retry
    want = MX.batch(model, 65, seed)
    rc, obs, off, lens, flags, _ = ctx.hmm_sample(model._c_model(), model._sample_tables()["c"], seed, 0, 65,
                                                   obs_slots=np.ones(65, np.int64), retry=False)
    assert rc == _lib.PS_ERR_CAPACITY and lens.cpu().numpy().tolist() == [len(w.obs) for w in want]
    obs = obs.cpu().numpy().reshape(-1)
    assert all(abs(obs[off[q]] - w.obs[0]) <= TOL * max(1.0, abs(w.obs[0])) for q, w in enumerate(want))
    assert max(len(w.obs) for w in want) > 12                                        # (past sample_batch's first guess)
    seqs, paths = model.sample_batch(65, path=True, seed=seed)
    compare_walks(model, seqs, paths, want)


def test_no_walk_emits_from_a_component_of_weight_zero():
    """The zero-weight components -- first, in the middle and last in their state -- are uniform on [1000, 1001]."""
    far = lambda: UniformDistribution(1000.0, 1001.0)                               # noqa: E731
    m = Model("zero")
    a = State(MixtureDistribution([far(), NormalDistribution(1.0, 0.5), far(), UniformDistribution(2.0, 3.0), far()], [0, 1, 0, 2, 0]), "a")
    b = State(MixtureDistribution([ExponentialDistribution(1.0), far()], [1, 0]), "b")
    for x, y, p in ((m.start, a, 0.5), (m.start, b, 0.5), (a, a, 0.4), (a, b, 0.4), (a, m.end, 0.2), (b, a, 0.5), (b, b, 0.3), (b, m.end, 0.2)):
        m.add_transition(x, y, p)
    m.bake()
    assert m._mix["mix_cdf"].tolist() == [0.0, 1 / 3, 1 / 3, 1.0, 1.0, 1.0, 1.0]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        seqs = m.sample_batch(3000, seed=123)
    x = np.concatenate(seqs)
    assert x.size > 8000 and x.max() < 900.0 and ((x >= 2.0) & (x <= 3.0)).mean() > 0.2
    compare_walks(m, seqs[:50], m.sample_batch(50, path=True, seed=123)[1], MX.batch(m, 50, 123))
