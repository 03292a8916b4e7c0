"""Vector models (MultivariateDistribution, LogNormalDistribution, ExponentialDistribution) on the MI355X: the HmmDevV
instantiations of the five HMM kernels (csrc/seg_hmm.hpp) against tests/multivariate_oracle.py, which
tests/test_multivariate_host.py holds to brute-force path enumeration.

Bits.  A model of normal and uniform states gives the same bits through the vector type at D = 1 as through the univariate
kernels (every output compared with ==), and Viterbi on models without log-normal components equals the oracle's
flat-array restatement with ==: log probabilities, paths and the whole score matrix.

Tolerances where bits cannot be asked for (the device's log, exp and log1p are not numpy's).  Log values -- log
probabilities, forward and backward matrices, log posteriors -- TOL = 1e-12 relative to max(1, |oracle|), -inf exactly
where the oracle has -inf: the measure of tests/test_hmm_gpu.py.  Viterbi paths with log-normal components are compared on
every input; tests/test_multivariate_host.py asserts with the oracle alone that none of them has a decision within 1e-9.

Per-sequence edge counts (forward_backward, expected_transitions): the bound derived in tests/test_posterior_gpu.py.  A
count C is a sum of at most n + 1 positive terms exp(a), a = (f - logp) + (b' + lp), with f, logp and b' each within TOL
max(1, |value|) of the oracle's; |f|, |b'| <= |logp| + |a| + 40 and the terms that matter have |a| <= |log C| + 40, so C is
within 4 TOL max(1, |logp| + |log C| + 80) relative plus (n + 1) 2^-52 for the order of the sum.  Nothing in that
derivation looks at the emission, so it holds for vector models as it stands.

Batch statistics (expected_counts_batch: edge counts and the 1 + 2 D statistics per state): the bound of
tests/test_hmm_train_gpu.py, 1e-9 relative to max(1, |oracle|), for every column, the signed A_d included, as
`close(got.stats, stats, 1e-9)` there.  That figure is the empirical bound the existing E-step tests hold the univariate
kernels to; it is inherited here, not derived.  What the derivation above gives for these sums is looser: W = sum g is a
count of the kind above with g = exp((f - logp) + b); B_d = sum g (y_d - c_d)^2 multiplies every term by a non-negative
factor formed with three roundings (one more, the device's log, for a log-normal y); A_d = sum g (y_d - c_d) has signed
terms, so its absolute error is that relative bound times sum g |y_d - c_d| <= sqrt(W B_d).  With |logp| + |log C| + 80
< 2500 here that worst case is 1e-8 relative for W and B_d, above the bound the tests assert.  Trained parameters are
quotients of these statistics and are held to the same 1e-9; improvements to 1e-9 relative.
Every comparison prints its largest error before it asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import multivariate_oracle as MV  # noqa: E402
import posterior_oracle as PO  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, LogNormalDistribution, Model, MultivariateDistribution,  # noqa: E402
                            NormalDistribution, State)

pytestmark = pytest.mark.gpu
TOL = 1e-12
STAT_TOL = 1e-9
LENGTHS = (0, 1, 2, 65)


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

    def __init__(self, model, seqs, estep=True):
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
        self.fields = ["v_logp", "v_mat", "paths", "f_logp", "f_mat", "b_logp", "b_mat", "logp", "p_logp", "post", "state",
                       "map_logp", "seq_counts"]
        if estep:
            elogp, ecounts, stats, self.skipped = ctx.hmm_expect(cm, obs, off, model._stat_width)
            self.e_logp, self.e_counts, self.stats = elogp.cpu().numpy(), ecounts.cpu().numpy(), stats.cpu().numpy()
            self.fields += ["e_logp", "e_counts", "stats", "skipped"]

    def rows(self, mat, q):
        return mat[self.off[q] + q:self.off[q + 1] + q + 1]

    def differing(self, other, fields=None):
        return [k for k in (fields or self.fields)
                if not (getattr(self, k) == getattr(other, k) if k in ("paths", "skipped") else same(getattr(self, k), getattr(other, k)))]


# ---- bit equality with the univariate kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("seed,finite", [(1, True), (2, False), (3, True)])
def test_vector_type_at_d1_gives_the_univariate_bits(seed, finite):
    rng = np.random.default_rng(7000 + seed)
    plain = O.random_model(rng, max_states=140, max_chain=20, finite=finite)
    vec = MV.wrapped(plain)
    assert vec._vector and not plain._vector and vec.n_dim == 1 and (vec.flat["kind"][:vec.flat["n_emit"]] == 4).all()
    assert [s.name for s in plain.states] == [s.name for s in vec.states]
    assert "zz-unreachable" not in [s.name for s in vec.states]                      # (bake drops what start cannot reach)
    assert plain.edges == vec.edges and same(plain.flat["in_lp"], vec.flat["in_lp"])
    seqs = [rng.normal(0, 2, n) for n in LENGTHS + (7, 30)] + [np.full(3, 1e300)]
    a, b = Decoded(plain, seqs), Decoded(vec, seqs)
    assert a.stats.shape == b.stats.shape == (plain.flat["n_emit"], 3)
    assert a.differing(b) == []
    assert np.isfinite(a.logp).any()


# ---- Viterbi bit for bit ----------------------------------------------------------------------------------------------
def impossible_rows(letters, n=3):
    """Sequences no state of a model built from `letters` can emit: beyond every uniform component, negative under every
    exponential one (each state of the rotated models holds every letter)."""
    out = []
    if "u" in letters:
        out.append(np.full((n, len(letters)), 100.0))
    if "e" in letters:
        out.append(np.full((n, len(letters)), -1.0))
    return [x.reshape(-1) if len(letters) == 1 else x for x in out]


def check_viterbi_exact(model, seqs):
    from pypore_amd import _lib
    off, (logp, mat, (path, path_off, path_len)) = model._run(seqs, _lib.PS_HMM_VITERBI, True)
    logp, mat, path, path_len = logp.cpu().numpy(), mat.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()
    results = model.viterbi_batch(seqs)
    for q, s in enumerate(seqs):
        want_logp, want_path, want_mat = MV.viterbi_exact(model, s)
        assert logp[q] == want_logp and results[q][0] == want_logp, (q, logp[q], want_logp)
        assert same(mat[off[q] + q:off[q + 1] + q + 1], want_mat), q
        if want_path is None:
            assert results[q] == (-np.inf, None) and path_len[q] == 0
        else:
            assert path[path_off[q]:path_off[q] + path_len[q]].tolist() == want_path
            assert [i for i, _ in results[q][1]] == want_path and all(st is model.states[i] for i, st in results[q][1])
    return logp


@pytest.mark.parametrize("n_emit,letters", [(63, "e"), (64, "nu"), (65, "nue"), (127, "nuenuenuenuenuen")])
def test_viterbi_bit_for_bit_line_models(n_emit, letters):
    model = MV.line_model(n_emit, letters, seed=1)
    assert model.n_dim == len(letters) and (model.flat["comp_w"] != 1.0).any()
    rng = np.random.default_rng(100 + n_emit)
    seqs = [MV.draw(rng, letters, n) for n in LENGTHS] + impossible_rows(letters)
    logp = check_viterbi_exact(model, seqs)
    assert logp[0] == -np.inf and np.isfinite(logp[1:len(LENGTHS)]).all() and (logp[len(LENGTHS):] == -np.inf).all()
    assert model.viterbi(seqs[3])[0] == logp[3]
    if len(letters) > 1:
        assert model.viterbi([tuple(r) for r in seqs[2]])[0] == logp[2]             # a list of tuples, as in the tutorial


@pytest.mark.parametrize("finite", [True, False])
def test_viterbi_bit_for_bit_silent_levels(finite):
    model = MV.silent_model("nue", seed=11 + finite, finite=finite)
    assert model.flat["n_levels"] >= 5 and model.finite == finite
    rng = np.random.default_rng(31 + finite)
    seqs = [MV.draw(rng, "nue", n) for n in LENGTHS] + impossible_rows("nue")
    logp = check_viterbi_exact(model, seqs)
    assert np.isfinite(logp[1:len(LENGTHS)]).all() and (logp[len(LENGTHS):] == -np.inf).all()


def test_viterbi_bit_for_bit_hub_16_bit_backpointers():
    model = MV.hub_model(257, "ne")
    assert int(np.diff(model.flat["in_ptr"]).max()) == 257
    seqs = [MV.hub_sequence(257, "ne", seed) for seed in range(3)] + [np.zeros((0, 2))]
    logp = check_viterbi_exact(model, seqs)
    assert np.isfinite(logp[:3]).all()
    names = [s.name for _, s in model.viterbi(seqs[0])[1]]
    assert names[1:7] == ["e0005", "h", "e0200", "h", "h", "e0017"]


# ---- log-normal components and the forward-type passes ----------------------------------------------------------------
CASES = {}


def case(index):
    if not CASES:
        for k, c in enumerate(MV.lognormal_cases()):
            CASES[k] = c
    return CASES[index]


def check_counts_per_sequence(got, want_counts, logp, n, what):
    with np.errstate(divide="ignore"):
        size = np.where(want_counts > 0, np.abs(np.log(np.where(want_counts > 0, want_counts, 1.0))), 0.0)
    rel = 4 * TOL * np.maximum(1.0, abs(logp) + size + 80.0) + (n + 1) * 2.0 ** -52            # (module docstring)
    err = np.abs(got - want_counts)
    print("%s: max error / bound %.3g" % (what, (err / (rel * want_counts + 1e-300)).max() if err.size else 0.0))
    assert (err <= rel * want_counts + 1e-300).all(), what


def check_stats(got, want, what):
    """The batch statistics [NE, 1 + 2 D], every column at STAT_TOL relative to max(1, |oracle|)."""
    assert_close(got, want, STAT_TOL, what)


@pytest.mark.parametrize("index", range(8))
def test_log_normal_models_every_pass_against_the_oracle(index):
    name, model, seqs = case(index)
    D = model.n_dim
    assert 5 in model.flat["comp_kind"]
    # x <= 0 under a log-normal component of every state: impossible
    dead = [np.zeros((2, D)), -np.ones((2, D))]
    dead = [x.reshape(-1) if D == 1 else x for x in dead]
    every = all(5 in model.flat["comp_kind"][k * D:(k + 1) * D] for k in range(model.flat["n_emit"]))
    batch = list(seqs) + (dead if every else [])
    got = Decoded(model, batch)
    results = model.viterbi_batch(batch)
    E = model.flat["out_ptr"][-1]
    tot_counts, tot_stats, skipped = np.zeros(E), np.zeros((model.flat["n_emit"], 1 + 2 * D)), 0
    for q, s in enumerate(batch):
        n = len(s)
        tag = "%s[%d]" % (name, q)
        lp, path, gap, ties, _ = MV.viterbi_ties(model, s)
        if q >= len(seqs):
            assert lp == -np.inf and results[q] == (-np.inf, None)
        assert_close([got.v_logp[q]], [lp], TOL, tag + " viterbi logp")
        if path is None:
            assert got.paths[q] is None and results[q] == (-np.inf, None)
        else:
            assert ties == 0 and gap > 1e-9                                          # (the host test's condition)
            assert got.paths[q] == path, tag
        want = MV.posterior(model, s)
        assert_close(got.rows(got.f_mat, q), MV.forward(model, s), TOL, tag + " forward")
        assert_close(got.rows(got.b_mat, q), MV.backward(model, s), TOL, tag + " backward")
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
        cc, st, elp = MV.estep_one(model, s)
        assert elp == want.logp
        tot_counts += cc
        tot_stats += st
    assert got.skipped == skipped
    assert_close(got.e_counts, tot_counts, STAT_TOL, name + " batch counts")
    check_stats(got.stats, tot_stats, name + " batch statistics")
    # the public methods return the same numbers in their own shapes
    q = len(seqs) - 1
    s = seqs[q]
    assert model.log_probability(s) == got.logp[q] and same(model.forward(s), got.rows(got.f_mat, q))
    assert same(model.backward(s), got.rows(got.b_mat, q))
    transitions, emissions = model.forward_backward(s)
    assert same(emissions, got.post[got.off[q]:got.off[q + 1]]) and same(model.expected_transitions(s), got.seq_counts[q])
    assert transitions.shape == (len(model.states),) * 2 and same(transitions[[e[0] for e in model.edges], [e[1] for e in model.edges]], got.seq_counts[q])
    mlp, mpath = model.maximum_a_posteriori(s)
    if got.p_logp[q] > -np.inf:
        assert mlp == got.map_logp[q] and [i for i, _ in mpath] == got.state[got.off[q]:got.off[q + 1]].tolist()
    est = model.expected_counts_batch(batch)
    assert same(est.counts, got.e_counts) and same(est.stats, got.stats) and est.stats.shape == (model.flat["n_emit"], 1 + 2 * D)
    assert same(model.expected_transitions_batch(batch), got.seq_counts)


def test_there_are_eight_log_normal_cases():
    assert len(MV.lognormal_cases()) == 8 and case(7)[0] == "profile3" and len(case(7)[1].states) == 165


# ---- launch shapes and routes -----------------------------------------------------------------------------------------
def expect_lds_bytes(model):
    S, E, NE, D = len(model.states), len(model.edges), model.flat["n_emit"], model.n_dim
    return 16 * S + 8 * (E + (1 + 2 * D) * NE + 1)


@pytest.mark.parametrize("n_emit,in_lds", [(629, True), (630, False)])
def test_estep_on_both_sides_of_its_lds_limit(n_emit, in_lds, capfd):
    """16 S + 8 n_acc <= 64 KiB with n_acc = E + (1 + 2 D) NE + 1: a line model of 629 states at D = 3 is the last that
    keeps its accumulators in LDS.  The library prints the dynamic LDS of the launch it sizes (option debug)."""
    from pypore_amd import engine
    model = MV.line_model(n_emit, "nle", seed=2)
    assert (expect_lds_bytes(model) <= 65536) == in_lds and abs(expect_lds_bytes(model) - 65536) < 120
    rng = np.random.default_rng(n_emit)
    seqs = [MV.draw(rng, "nle", n) for n in (3, 0, 6, 1)] + [np.zeros((2, 3))]
    ctx = engine.context()
    capfd.readouterr()
    with LG.options(ctx, debug=1):
        got = model.expected_counts_batch(seqs)
    S = len(model.states)
    lds = expect_lds_bytes(model) if in_lds else 16 * S
    assert LG.printed_slots(capfd.readouterr().err, lds), "no E-step launch with %d bytes of dynamic LDS" % lds
    counts, stats, logp, skipped = MV.estep(model, seqs)
    assert_close(got.logp, logp, TOL, "logp")
    assert got.skipped == skipped == 2                                               # the empty one (finite model) and x = 0
    assert_close(got.counts, counts, STAT_TOL, "counts")
    check_stats(got.stats, stats, "statistics")
    if in_lds:
        with LG.options(ctx, hmm_expect_lds=0):
            glob = model.expected_counts_batch(seqs)
        assert same(glob.logp, got.logp)
        assert_close(glob.counts, got.counts, 1e-12, "counts, accumulators in global memory")
        assert_close(glob.stats, got.stats, 1e-12, "statistics, accumulators in global memory")


def test_cut_batches_small_grid_and_a_batch_of_300():
    from pypore_amd import engine
    name, model, _ = case(6)                                                          # the infinite silent model, D = 3
    rng = np.random.default_rng(12)
    seqs = [MV.draw(rng, "nle", int(rng.integers(1, 40))) for _ in range(300)]
    seqs[17] = np.zeros((0, 3))
    seqs[230] = np.column_stack([np.ones(4), np.ones(4), np.zeros(4)])               # x = 0 under the log-normal slot of some
    seqs[231] = -np.ones((4, 3))                                                     # ... and of every state: impossible
    ctx = engine.context()
    whole = Decoded(model, seqs)
    assert whole.v_logp[231] == -np.inf and whole.logp[231] == -np.inf and whole.skipped >= 1 and np.isfinite(whole.logp[17])
    S = len(model.states)
    per_seq = ["v_logp", "v_mat", "paths", "f_logp", "f_mat", "b_logp", "b_mat", "logp", "p_logp", "post", "state", "map_logp",
               "seq_counts", "e_logp", "skipped"]
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
    for q in (0, 17, 150, 230, 231, 299):
        assert_close([whole.logp[q]], [MV.log_probability(model, seqs[q])], TOL, "logp[%d]" % q)
        lp, path = MV.viterbi_ties(model, seqs[q])[:2]
        assert_close([whole.v_logp[q]], [lp], TOL, "viterbi logp[%d]" % q)
    counts, stats, logp, skipped = MV.estep(model, seqs[:40])
    part = model.expected_counts_batch(seqs[:40])
    assert_close(part.counts, counts, STAT_TOL, "counts of 40")
    check_stats(part.stats, stats, "statistics of 40")


# ---- upload and ABI ---------------------------------------------------------------------------------------------------
def test_upload_cache_sees_a_changed_weight_and_a_changed_parameter():
    def build(weight, rate):
        m = Model("pair")
        a = State(MultivariateDistribution([NormalDistribution(1.0, 1.0), ExponentialDistribution(rate)], [1.0, weight]), "a")
        b = State(MultivariateDistribution([NormalDistribution(3.0, 1.0), ExponentialDistribution(2.0)]), "b")
        for s, t, p in ((m.start, a, 0.5), (m.start, b, 0.5), (a, a, 0.5), (a, b, 0.5), (b, a, 0.5), (b, b, 0.3), (b, m.end, 0.2)):
            m.add_transition(s, t, p)
        m.bake()
        return m
    base, weight, param = build(1.0, 1.0), build(1.25, 1.0), build(1.0, 1.5)
    for other in (weight, param):
        diff = [k for k, v in base.flat.items() if isinstance(v, np.ndarray) and not same(v, other.flat[k])]
        assert diff == (["comp_w"] if other is weight else ["comp_param"])
    rng = np.random.default_rng(8)
    seqs = [MV.draw(rng, "ne", n) for n in (5, 9)]
    first = {id(m): (m.log_probability_batch(seqs), m.viterbi_batch(seqs)) for m in (base, weight, param)}
    for m in (base, weight, base, param, weight, param, base):
        lp, vit = m.log_probability_batch(seqs), m.viterbi_batch(seqs)
        assert same(lp, first[id(m)][0]) and [v[0] for v in vit] == [v[0] for v in first[id(m)][1]]
        assert_close(lp, [MV.log_probability(m, s) for s in seqs], TOL, "logp")
    assert not same(first[id(base)][0], first[id(weight)][0]) and not same(first[id(base)][0], first[id(param)][0])


def copy_of(cm):
    from pypore_amd import _lib
    m = _lib.HmmModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(cm), ctypes.sizeof(m))
    return m


def test_appended_fields_are_ignored_without_kind_4():
    from pypore_amd import _lib
    model, means = O.profile_model(20, seed=9)
    other = MV.line_model(70, "nle", seed=4)
    seqs = O.profile_events(means, 6, lo=10, hi=60, seed=3)
    ctx, off, obs = model._upload(seqs, None)
    base = model._c_model()
    assert not base.comp_kind and not base.comp_param and not base.comp_w             # NULL, as an older caller leaves them
    alt = copy_of(base)
    f = other.flat
    alt.n_dim, alt.comp_kind, alt.comp_param, alt.comp_w = 3, f["comp_kind"].ctypes.data, f["comp_param"].ctypes.data, f["comp_w"].ctypes.data
    junk = copy_of(base)
    junk.n_dim = 99
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
    c = O.Compiled(model)
    assert_close(ctx.hmm_batch(base, _lib.PS_HMM_FORWARD, obs, off, False)[0].cpu().numpy(), [O.log_probability(c, s) for s in seqs])


def test_bad_vector_models_are_refused_with_their_messages():
    from pypore_amd import _lib
    model = MV.line_model(5, "nle", seed=6)
    rng = np.random.default_rng(2)
    seqs = [MV.draw(rng, "nle", 4)]
    ctx, off, obs = model._upload(seqs, None)
    base, f = model._c_model(), model.flat
    keep = []

    def with_array(field, arr):
        keep.append(arr)
        m = copy_of(base)
        setattr(m, field, arr.ctypes.data)
        return m

    def changed(field, index, value):
        arr = f[field].copy()
        arr[index] = value
        return with_array(field, arr)

    def with_dim(d):
        m = copy_of(base)
        m.n_dim = d
        return m

    def null(field):
        m = copy_of(base)
        setattr(m, field, None)
        return m

    bad = [(changed("kind", 1, 1), "cannot be mixed"), (changed("kind", 0, 2), "cannot be mixed"), (changed("kind", 2, 3), "cannot be mixed"),
           (with_dim(0), "1..16"), (with_dim(17), "1..16"), (with_dim(-3), "1..16"),
           (changed("comp_kind", 4, 3), "unknown component kind 3"), (changed("comp_kind", 0, 0), "unknown component kind 0"),
           (changed("comp_kind", 14, 7), "unknown component kind 7"),
           (changed("comp_w", 3, 0.0), "finite and > 0"), (changed("comp_w", 0, -1.0), "finite and > 0"),
           (changed("comp_w", 14, np.inf), "finite and > 0"), (changed("comp_w", 7, np.nan), "finite and > 0"),
           (null("comp_kind"), "comp_kind, comp_param and comp_w"), (null("comp_param"), "comp_kind, comp_param and comp_w"),
           (null("comp_w"), "comp_kind, comp_param and comp_w")]
    for cm, message in bad:
        with pytest.raises(ValueError, match=message):
            ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off, False)
        with pytest.raises(ValueError, match=message):
            ctx.hmm_expect(cm, obs, off, model._stat_width)
        with pytest.raises(ValueError, match=message):
            ctx.hmm_posterior(cm, obs, off)
    assert_close([model.log_probability(seqs[0])], [MV.log_probability(model, seqs[0])], TOL, "the context still works")
    # `param` is not read for a vector model: NULL gives the bits of the zeros bake() leaves there
    want = [x.cpu().numpy() for x in ctx.hmm_expect(base, obs, off, model._stat_width)[:3]]
    got = [x.cpu().numpy() for x in ctx.hmm_expect(null("param"), obs, off, model._stat_width)[:3]]
    assert all(same(x, y) for x, y in zip(got, want)) and np.isfinite(got[0]).all()


# ---- training ---------------------------------------------------------------------------------------------------------
def training_model(seed):
    """Six D = 3 states (mean, std, duration): normal, normal, log-normal per state; the std component shared by states
    0 and 3, one exponential duration, one frozen state."""
    rng = np.random.default_rng(seed)
    shared = NormalDistribution(1.0, 0.5)
    m = Model("train3")
    st = []
    for k in range(6):
        dur = ExponentialDistribution(8.0) if k == 2 else LogNormalDistribution(float(rng.normal(-2.5, 0.2)), 0.8)
        std = shared if k in (0, 3) else NormalDistribution(float(rng.uniform(0.8, 1.4)), 0.5)
        d = MultivariateDistribution([NormalDistribution(20.0 + 6.0 * k + float(rng.normal(0, 1)), 2.0), std, dur], [1.0, 0.5, 0.5])
        if k == 4:
            d.freeze()
        st.append(State(d, "s%d" % k))
    for k, s in enumerate(st):
        m.add_transition(m.start, s, 1.0)
        m.add_transition(s, s, 0.4)
        for t in st[k + 1:k + 3]:
            m.add_transition(s, t, 0.3)
        m.add_transition(s, m.end, 0.1)
        if k:
            m.add_transition(s, st[0], 0.05)
    m.bake()
    return m


def training_data(seed, count=12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(5, 40))
        k = np.minimum(np.cumsum(rng.choice([0, 1, 1], n)), 5)
        out.append(np.column_stack([20.0 + 6.0 * k + rng.normal(0, 2.5, n), np.abs(rng.normal(1.2, 0.4, n)) + 0.05,
                                    rng.lognormal(-2.3, 0.9, n)]))
    return out


@pytest.mark.parametrize("algorithm", ["baum-welch", "viterbi"])
def test_one_training_iteration_against_the_oracle(algorithm):
    model, seqs = training_model(3), training_data(4)
    if algorithm == "viterbi":                                                        # the paths must not hang on a near tie
        for s in seqs:
            lp, path, gap, ties, _ = MV.viterbi_ties(model, s)
            assert path is not None and ties == 0 and gap > 1e-9
    want, steps, total = MV.train(model, seqs, 1, algorithm=algorithm, min_std=0.05)
    frozen_before = [list(d.parameters) for d, _ in MV.parts(model.states[4].distribution)]
    got_total = model.train(seqs, max_iterations=1, algorithm=algorithm, min_std=0.05, verbose=False)
    print("improvement %.17g, oracle %.17g" % (got_total, total))
    assert abs(got_total - total) <= 1e-9 * max(1.0, abs(total)) and abs(total) > 1e-3
    got_p, want_p = [], []
    for s, t in zip(model.states[:6], want.states[:6]):
        for (d, _), (e, _) in zip(MV.parts(s.distribution), MV.parts(t.distribution)):
            assert type(d) is type(e)
            got_p += d.parameters
            want_p += e.parameters
    assert_close(got_p, want_p, STAT_TOL, "trained parameters")
    assert_close([p for _, _, p in model.edges], [p for _, _, p in want.edges], STAT_TOL, "trained edges")
    assert [list(d.parameters) for d, _ in MV.parts(model.states[4].distribution)] == frozen_before
    assert model.states[0].distribution.parameters[0][1] is model.states[3].distribution.parameters[0][1]


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_event_and_experiment_apply_hmm_with_features():
    from pypore_amd.DataTypes import Event, Experiment, File
    from pypore_amd.parsers import SpeedyStatSplit
    rng = np.random.default_rng(21)
    levels = [30.0, 45.0, 25.0, 50.0, 35.0]
    m = Model("levels3")
    st = [State(MultivariateDistribution([NormalDistribution(v, 2.0), NormalDistribution(0.5, 0.5), LogNormalDistribution(-3.5, 1.0)],
                                         [1.0, 0.5, 0.25]), "L%d" % i) for i, v in enumerate(levels)]
    m.add_transition(m.start, st[0], 1.0)
    for i, s in enumerate(st):
        m.add_transition(s, s, 0.6)
        if i + 1 < len(st):
            m.add_transition(s, st[i + 1], 0.4)
    m.add_transition(st[-1], m.end, 0.4)
    m.bake()
    second, events = 1.0e5, []
    for k in range(3):
        x = np.concatenate([np.full(int(rng.integers(2000, 6000)), v) + rng.normal(0, 0.6, 1) for v in levels
                            for _ in range(int(rng.integers(1, 3)))])
        x = np.round((x + rng.normal(0, 0.3, x.size)) * 32) / 32
        f = File(current=x, timestep=1000.0 / second)
        ev = Event(current=x, start=0, end=x.size / second, duration=x.size / second, second=second, file=f)
        ev.parse(SpeedyStatSplit(prior_segments_per_second=10))
        assert len(ev.segments) >= 5
        events.append(ev)
    features = ('mean', 'std', 'duration')
    paths = []
    for ev in events:
        tuples = [(s.mean, s.std, s.duration) for s in ev.segments]
        want = m.viterbi(tuples)
        got = ev.apply_hmm(m, features=features)
        assert got[0] == want[0] and [i for i, _ in got[1]] == [i for i, _ in want[1]] and got[1] is not None
        lp, path, gap, ties, _ = MV.viterbi_ties(m, np.array(tuples))
        assert_close([got[0]], [lp], TOL, "viterbi logp")
        assert ties == 0 and gap > 1e-9, (ties, gap)                                  # no decision another log could turn
        assert [i for i, _ in got[1]] == path
        assert ev.apply_hmm(m, 'log_probability', features) == m.log_probability(tuples)
        with pytest.raises(ValueError, match="features"):
            ev.apply_hmm(m)
        paths += [i for i, _ in got[1]]
    exp = Experiment([])
    exp.files = [events[0].file]
    exp.files[0].events = events
    calls, real = [], m.viterbi_batch
    m.viterbi_batch = lambda seqs, device=None: calls.append(len(seqs)) or real(seqs, device)
    try:
        out = exp.apply_hmm(m, features=features)
    finally:
        del m.viterbi_batch
    assert calls == [3] and [i for i, _ in out] == paths
