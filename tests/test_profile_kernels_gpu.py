"""The HmmDevK instantiations of csrc/seg_hmm.hpp (a model with a kernel-density state) where tests/test_profile_gpu.py
does not take them:

1. the emission itself against np.longdouble, through a probe model whose forward entry f[1][s] is one addition on top of
   hmm_emit (profile_oracle.kde_probe_grid: 1 to 5000 points, bandwidths 1e-3 to 1e3, points ordered so that HmmLse
   rescales on every term or on none, equal terms, weights over 300 decades), a distance whose square overflows, and the
   same probe through Viterbi, backward and the E-step;
2. the launch shapes the HmmDev instantiations are tested at in test_hmm_gpu.py and test_hmm_train_gpu.py: in-degrees on
   both sides of the 8-bit backpointer width, a model at the state cap, more than two waves of states whose lanes walk
   different numbers of points, the E-step's global-memory accumulators by the model's own size with a small grid and
   launches cut off the grid's multiples;
3. the upload cache (hmm_upload compares the packed blob) on the appended tables: models that differ in one point, in the
   log weights, in how kde_ptr splits the same points, and a model without kernel densities between them.

The bar is that of test_profile_gpu.py: 1e-12 relative to max(1, |reference|), -inf exactly where the reference has it,
paths identical where the oracle's margin exceeds 1e-9; counts and statistics to 1e-9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import profile_oracle as P  # noqa: E402
import test_hmm_gpu as HG  # noqa: E402
import test_hmm_train_gpu as TG  # noqa: E402
import test_profile_gpu as PG  # noqa: E402

from pypore_amd.hmm import GaussianKernelDensity, Model, NormalDistribution, State  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = PG.TOL
assert TOL == 1e-12


def check_estep(model, seqs, got=None):
    got = model.expected_counts_batch(seqs) if got is None else got
    counts, stats, logp, skipped = P.estep(model, seqs)
    TG.close(got.logp, logp, 1e-12)
    assert got.skipped == skipped
    TG.close(got.counts, counts, 1e-9)
    TG.close(got.stats, stats, 1e-9)
    return got


def ids(path):
    return None if path is None else [i for i, _ in path]


# ---- 1. the emission against long double ----------------------------------------------------------------------------------------
_PROBE = {}


def probe():
    """start -> s_i with probability 1 / K, s_i -> end with probability 1, one kernel-density state per configuration of the
    grid: (model, grid, state index by name, in_lp of every state's one in-edge as baked)."""
    if not _PROBE:
        grid = P.kde_probe_grid()
        model = Model("probe")
        for name, d, _ in grid:
            s = State(d, name)
            model.add_transition(model.start, s, 1.0 / len(grid))
            model.add_transition(s, model.end, 1.0)
        model.bake()
        index = {s.name: i for i, s in enumerate(model.states)}         # (bake orders the emitting states by name)
        f = model.flat
        assert all(f["in_ptr"][k + 1] - f["in_ptr"][k] == 1 for k in range(len(grid)))
        in_lp = {name: float(f["in_lp"][f["in_ptr"][index[name]]]) for name, _, _ in grid}
        _PROBE["case"] = model, grid, index, in_lp
    return _PROBE["case"]


def rel_err(got, ref):
    return float(abs(np.longdouble(got) - ref) / max(1.0, abs(float(ref))))


def test_emission_against_long_double(record_property):
    """f[1][s_i] of the one-observation sequence [x] is in_lp_i + e_i(x): one rounding on top of the device's emission.
    Every state at its own seven observations, and a fixed sample of 2000 other (state, observation) pairs.  The worst
    error per point count is printed (DESIGN.md 7f records it); the assertion is the module's bar, not that figure."""
    model, grid, index, in_lp = probe()
    seqs = [[x] for _, _, xs in grid for x in xs]
    mats = model.forward_batch(seqs)
    assert len(mats) == 7 * len(grid) and all(m.shape == (2, len(grid) + 2) for m in mats)
    L = np.longdouble
    worst = {}

    def check(g, q):
        name, d, _ = grid[g]
        pts, h, w = d.parameters
        ref = L(in_lp[name]) + P.kde_logpdf_longdouble(pts, h, w, seqs[q][0])
        got = mats[q][1][index[name]]
        assert np.isfinite(ref) and np.isfinite(got), (name, seqs[q][0], got)
        err = rel_err(got, ref)
        worst[len(pts)] = max(worst.get(len(pts), 0.0), err)
        return err, name, seqs[q][0]

    own = max(check(g, 7 * g + j) for g in range(len(grid)) for j in range(7))
    rng = np.random.default_rng(11)
    other = max(check(int(g), int(q)) for g, q in zip(rng.integers(len(grid), size=2000), rng.integers(len(seqs), size=2000)))
    print("device emission vs long double, worst per point count:", {n: "%.2e" % e for n, e in sorted(worst.items())})
    print("worst own:", own, "worst other:", other)
    record_property("worst_per_point_count", {str(n): e for n, e in worst.items()})
    assert sorted(worst) == list(P.PROBE_POINTS)
    assert own[0] <= TOL and other[0] <= TOL, (own, other)


def test_overflowing_distance_is_minus_infinity():
    """x = 1e200: (x - p)^2 overflows float64, every term of every state is -inf and so is the emission -- on the device,
    in the float64 oracle and in the host class alike (float64 semantics are the contract; in long double the square is
    finite, about 1e400, and so is the density, which therefore is no reference here)."""
    model, grid, index, _ = probe()
    far = [1e200]
    name, d, xs = grid[0]
    assert d.log_probability(far[0]) == -np.inf
    assert np.isfinite(P.kde_logpdf_longdouble(*d.parameters, far[0]))
    c = P.Compiled(model)
    assert O.log_probability(c, far) == -np.inf and np.all(np.isneginf(c.emissions(far[0])))
    seqs = [[xs[0]], far, [xs[6]], far, []]
    lp = model.log_probability_batch(seqs)
    assert np.isfinite(lp[0]) and np.isfinite(lp[2]) and lp[1] == lp[3] == lp[4] == -np.inf
    assert model.log_probability(far) == -np.inf and model.viterbi(far) == (-np.inf, None)
    vit = model.viterbi_batch(seqs)
    assert vit[1] == vit[3] == vit[4] == (-np.inf, None) and vit[0][1] is not None and vit[2][1] is not None
    f, b = model.forward(far), model.backward(far)
    assert np.all(np.isneginf(f[1])) and np.isneginf(b[0][c.start]) and b[1][c.end] == 0.0
    got = check_estep(model, seqs)
    assert got.skipped == 3 and np.array_equal(np.isneginf(got.logp), [False, True, False, True, True])


def test_probe_through_viterbi_backward_and_the_e_step():
    """The emission in the other kernels: state i takes its observation i mod 7 (every kind of observation, every state
    once), plus the overflowing one.  Viterbi picks the best state (many near-ties: the all-equal-points states of one
    bandwidth are one density), backward's b[0][start] and the E-step's logp are the log probability, and a state's W is the
    sum of its posteriors, which sum to 1 per finite sequence."""
    model, grid, index, _ = probe()
    seqs = [[xs[g % 7]] for g, (_, _, xs) in enumerate(grid)] + [[1e200]]
    c = P.Compiled(model)
    for s, v in zip(seqs, model.viterbi_batch(seqs)):
        PG.check_viterbi(c, s, v)
    want = np.array([O.log_probability(c, s) for s in seqs])
    assert np.isneginf(want[-1]) and np.all(np.isfinite(want[:-1]))
    PG.assert_close(model.log_probability_batch(seqs), want)
    back = model.backward_batch(seqs)
    PG.assert_close([b[0][c.start] for b in back], want)
    for s, b in list(zip(seqs, back))[::40]:
        PG.assert_close(b, O.backward(c, s))
    got = check_estep(model, seqs)
    PG.assert_close(got.logp, want)
    assert got.skipped == 1
    F = [O.forward(c, s) for s in seqs[:-1]]
    post = np.sum([np.exp(f[1][:c.NE] - lp) for f, lp in zip(F, want)], axis=0)      # b[1][s_i] = log 1: s_i -> end
    TG.close(got.stats[:, 0], post, 1e-9)
    assert abs(got.stats[:, 0].sum() - (len(seqs) - 1)) <= 1e-9 * len(seqs)


# ---- 2. launch shapes -----------------------------------------------------------------------------------------------------------
_HUBS = {}


def kde_hub(n_in):
    """test_hmm_gpu._hub_model with every e state a kernel density: 2 to 5 points within 0.3 of the normal's mean at
    bandwidth 0.5 (the normal's std), so an observation still names its state."""
    if n_in not in _HUBS:
        model, h, es = HG._hub_model(n_in)
        rng = np.random.default_rng(1000 + n_in)
        for e in es:
            mean = e.distribution.parameters[0]
            e.distribution = GaussianKernelDensity(mean + rng.uniform(-0.3, 0.3, int(rng.integers(2, 6))), 0.5)
        model.bake()
        assert PG.has_kde(model) and type(h.distribution).__name__ == "NormalDistribution"
        _HUBS[n_in] = model, h, es, P.Compiled(model)
    return _HUBS[n_in]


@pytest.mark.parametrize("n_in", [255, 256, 257, 600])
def test_in_degree_across_the_backpointer_width(n_in):
    """test_hmm_gpu.test_in_degree_across_the_backpointer_width on the HmmDevK Viterbi: 255 in-edges take the 8-bit
    backpointers, 256 and more the 16-bit ones, and from 257 up the winning in-edge into h has an ordinal >= 256."""
    model, h, es, c = kde_hub(n_in)
    ix = {id(s): i for i, s in enumerate(model.states)}
    ins = {}
    for i, j, _ in model.edges:
        ins.setdefault(j, []).append(i)
    assert len(ins[ix[id(h)]]) == n_in and len(ins[ix[id(model.end)]]) == n_in
    assert max(len(v) for v in ins.values()) == n_in
    rng = np.random.default_rng(n_in)
    winners = [0, min(254, n_in - 2), n_in - 2] + ([256, 300 % (n_in - 1), n_in - 3] if n_in > 257 else [])
    seqs = HG._hub_seqs(rng, es, winners)
    PG.check_all(model, seqs, c=c)
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
    """The 16-bit route of the HmmDevK Viterbi with launches cut by hmm_bp_budget, one sequence alone above the budget."""
    from pypore_amd import engine
    model, h, es, c = kde_hub(600)
    rng = np.random.default_rng(5)
    seqs = HG._hub_seqs(rng, es, [256, 598, 400, 3])
    alt = np.stack([3.0 * rng.integers(599, size=20), np.full(20, -50.0)], axis=1).ravel()     # e, h, e, h, ...
    seqs.insert(3, alt + rng.normal(0, 0.1, 40))
    S = len(model.states)
    budget = 9 * S * 2                                  # rows of 16-bit backpointers: 9 (n + 1 <= 9 for the short ones)
    assert (len(seqs[3]) + 1) * S * 2 > budget
    whole = model.viterbi_batch(seqs)
    with LG.options(engine.context(), hmm_bp_budget=budget):
        split = model.viterbi_batch(seqs)
    for s, a, b in zip(seqs, whole, split):
        assert a[0] == b[0] and ids(a[1]) == ids(b[1])
        PG.check_viterbi(c, s, b)
    assert sum(p is not None for _, p in split) >= 5


def kde_line(S):
    """hmm_oracle.line_model(S) with every third emitting state a kernel density of 1 to 3 points around its mean."""
    model = O.line_model(S)
    rng = np.random.default_rng(S + 1)
    for s in [s for s in model.states if not s.is_silent()][::3]:
        mean, std = s.distribution.parameters
        s.distribution = GaussianKernelDensity(mean + rng.uniform(-1, 1, int(rng.integers(1, 4))), std)
    model.bake()
    return model


def test_model_at_the_state_cap():
    """HMM_S_MAX = 4096 states, a third of the emitting ones kernel densities: the two score rows fill 64 KiB of LDS in all
    five HmmDevK kernels, and the E-step's accumulators go to global memory by the model's own size."""
    model = kde_line(4096)
    S, E, NE = len(model.states), len(model.edges), model.flat["n_emit"]
    assert S == 4096 and PG.has_kde(model) and int(np.sum(model.flat["kind"] == 3)) == (NE + 2) // 3
    assert (2 * S + E + 3 * NE + 1) * 8 > 64 << 10
    rng = np.random.default_rng(3)
    seqs = [rng.normal(0, 3, n) for n in (0, 1, 3, 6)]
    PG.check_all(model, seqs)
    got = check_estep(model, seqs)
    assert got.skipped == 1                                # the empty sequence: start reaches end only through a state
    over = kde_line(4097)
    assert len(over.states) == 4097 and PG.has_kde(over)
    for call in (lambda: over.viterbi([0.0]), lambda: over.log_probability_batch([[0.0]]), lambda: over.expected_counts_batch([[0.0]])):
        with pytest.raises(ValueError, match="4096"):
            call()


def test_lanes_walk_different_numbers_of_points():
    """130 kernel-density states on a line, more than two waves of them: lane k owns the states k, k + 64 and k + 128, and
    state k has 1 + 7 k mod 97 points, so neighbouring lanes leave the emission loop at different times."""
    rng = np.random.default_rng(130)
    model = Model("lanes")
    st = []
    for k in range(130):
        mean, h = float(rng.normal(0, 3)), float(rng.uniform(0.5, 2))
        st.append(State(GaussianKernelDensity(mean + rng.uniform(-1, 1, 1 + (7 * k) % 97), h, rng.uniform(0.1, 1, 1 + (7 * k) % 97)),
                        "s%03d" % k))
    for k, s in enumerate(st):
        if k % 64 == 0:
            model.add_transition(model.start, s, 1.0)
        model.add_transition(s, s, 0.3)
        if k + 1 < len(st):
            model.add_transition(s, st[k + 1], 0.5)
        if k + 2 < len(st):
            model.add_transition(s, st[k + 2], 0.1)
        model.add_transition(s, model.end, 0.1)
    model.bake()
    assert model.states[:130] == st and list(np.diff(model.flat["kde_ptr"])) == [1 + (7 * k) % 97 for k in range(130)]
    seqs = [rng.normal(0, 3, n) for n in (0, 1, 2, 5, 9, 12)]
    PG.check_all(model, seqs)
    check_estep(model, seqs)


def test_e_step_in_global_memory_by_size_with_a_small_grid_and_cuts(capfd, record_property):
    """The dense 100-state model of test_hmm_train_gpu.test_accumulators_in_global_memory with kernel-density states: its
    accumulator row does not fit LDS beside the score rows, so hmm_expect_kernel<false, HmmDevK> runs without the option
    being forced.  Under slots_pct 1 the grid G is smaller than the batch, and an hmm_fb_budget cuts the batch into at
    least four launches whose first sequences are no multiples of G."""
    from pypore_amd import engine
    rng = np.random.default_rng(4)
    model = Model("dense")
    st = []
    for i in range(100):
        mean = float(rng.normal(0, 2))
        st.append(State(GaussianKernelDensity(mean + rng.uniform(-1, 1, int(rng.integers(1, 5))), float(rng.uniform(0.5, 2))), "e%03d" % i))
    for s in st:
        model.add_transition(model.start, s, float(rng.uniform(0.1, 1)))
        for t in st:
            model.add_transition(s, t, float(rng.uniform(0.01, 1)))
        model.add_transition(s, model.end, 0.05)
    model.bake()
    S, E, NE = len(model.states), len(model.edges), 100
    assert PG.has_kde(model) and 8 * E + 24 * NE + 16 * S > 64 << 10 and (2 * S + E + 3 * NE + 1) * 8 > 64 << 10
    ctx = engine.context()
    capfd.readouterr()
    with LG.options(ctx, slots_pct=1, debug=1):
        model.expected_counts_batch([rng.normal(0, 2, 2)])
    (slots, pct), = LG.printed_slots(capfd.readouterr().err, 2 * S * 8)      # (no accumulator row in the dynamic LDS)
    assert pct == 1 and 2 <= slots, slots
    seqs = [rng.normal(0, 2, int(rng.integers(1, 5))) for _ in range(2 * slots + 5)]
    G, lengths = slots, [len(s) for s in seqs]
    total = sum((n + 1) * S * 8 for n in lengths)
    budget = next(b for b in (total // d for d in range(4, 40))
                  if len(TG._launch_cuts(lengths, S, b)) >= 3 and all(q % G for q in TG._launch_cuts(lengths, S, b)))
    record_property("geometry", {"G": G, "cuts": TG._launch_cuts(lengths, S, budget)})
    ref = model.expected_counts_batch(seqs)
    with LG.options(ctx, slots_pct=1):
        uncut = model.expected_counts_batch(seqs)
    with LG.options(ctx, slots_pct=1, hmm_fb_budget=budget):
        cut = model.expected_counts_batch(seqs)
        again = model.expected_counts_batch(seqs)
    counts, stats, logp, skipped = P.estep(model, seqs)
    for got in (ref, uncut, cut):
        TG.close(got.logp, logp, 1e-12)
        assert got.skipped == skipped == 0
        TG.close(got.counts, counts, 1e-9)
        TG.close(got.stats, stats, 1e-9)
    for other in (ref, uncut):
        TG.close(cut.counts, other.counts, 1e-12)
        TG.close(cut.stats, other.stats, 1e-12)
        assert np.array_equal(cut.logp, other.logp)
    for x, y in zip(cut[:3], again[:3]):
        assert np.array_equal(x, y)


# ---- 3. the upload cache on the appended tables -----------------------------------------------------------------------------------
def two_state_model(a, b):
    """start -> A, B; A and B loop, reach each other and end: the same topology whatever the two distributions are."""
    m = Model("two")
    A, B = State(a, "A"), State(b, "B")
    m.add_transition(m.start, A, 0.5)
    m.add_transition(m.start, B, 0.5)
    for s, t in ((A, B), (B, A)):
        m.add_transition(s, s, 0.3)
        m.add_transition(s, t, 0.4)
        m.add_transition(s, m.end, 0.3)
    m.bake()
    return m


def test_upload_cache_on_the_appended_tables():
    """hmm_upload reuses the device copy while the packed blob is unchanged.  Four models of one topology and one
    bandwidth whose blobs differ only in the appended tables or little else (the weights are dyadic, so the weighted means
    in param slot 0 are exact):
      moved   one point of A moved:     kde_pt[2], and param[0] (A's weighted mean) with it;
      weight  A's weights changed at the same mean 1.5: kde_lw[0:3] only;
      split   the same five points cut 2 + 3 instead of 3 + 2, at the same means 1.5 and 4.5: kde_ptr[1] and kde_lw (the
              weights of a state sum to 1, so no two splits share their log weights); param and kde_pt are identical.
    A compare that missed one of the tables would decode with the model before.  Every result equals the oracle of its
    own model, and the three visits of `base` agree bit for bit; then the same between `base` and a model of normal
    states, which switches one context between the HmmDevK and the HmmDev instantiations."""
    h = 0.8
    models = {
        "base": two_state_model(GaussianKernelDensity([1, 2, 3], h, [5 / 8, 2 / 8, 1 / 8]), GaussianKernelDensity([4, 5], h, [1 / 2, 1 / 2])),
        "moved": two_state_model(GaussianKernelDensity([1, 2, 3.5], h, [5 / 8, 2 / 8, 1 / 8]), GaussianKernelDensity([4, 5], h, [1 / 2, 1 / 2])),
        "weight": two_state_model(GaussianKernelDensity([1, 2, 3], h, [9 / 16, 6 / 16, 1 / 16]), GaussianKernelDensity([4, 5], h, [1 / 2, 1 / 2])),
        "split": two_state_model(GaussianKernelDensity([1, 2], h, [1 / 2, 1 / 2]), GaussianKernelDensity([3, 4, 5], h, [1 / 8, 2 / 8, 5 / 8])),
        "normal": two_state_model(NormalDistribution(1.5, h), NormalDistribution(4.5, h)),
    }
    flat = {k: m.flat for k, m in models.items()}
    fields = [k for k, v in flat["base"].items() if isinstance(v, np.ndarray)]

    def differing(name):
        return sorted(k for k in fields if not np.array_equal(flat["base"][k], flat[name][k]))

    assert all(flat[k][s] == flat["base"][s] for k in flat for s in flat["base"] if s not in fields)
    assert differing("moved") == ["kde_pt", "param"] and differing("weight") == ["kde_lw"]
    assert differing("split") == ["kde_lw", "kde_ptr"]
    assert list(flat["base"]["kde_ptr"]) == [0, 3, 5] and list(flat["split"]["kde_ptr"]) == [0, 2, 5]
    assert {"kde_lw", "kde_pt", "kde_ptr", "kind"} <= set(differing("normal")) and flat["normal"]["kde_pt"].size == 0
    rng = np.random.default_rng(12)
    seqs = [rng.uniform(0, 6, n) for n in (0, 1, 2, 3, 5, 8)] + [np.array([3.0, 3.2, 2.9])]
    want = {}
    for k, m in models.items():
        c = P.Compiled(m)
        want[k] = ([O.viterbi(c, s) for s in seqs], [O.log_probability(c, s) for s in seqs], P.estep(m, seqs))
    # the models tell these sequences apart by far more than the bar, so a stale device copy cannot pass
    for k in ("moved", "weight", "split", "normal"):
        assert max(abs(a - b) for a, b in zip(want[k][1][1:], want["base"][1][1:])) > 1e-3

    def visit(name):
        m = models[name]
        lp, vit, ex = m.log_probability_batch(seqs), m.viterbi_batch(seqs), m.expected_counts_batch(seqs)
        wv, wl, (counts, stats, logp, skipped) = want[name]
        PG.assert_close(lp, wl)
        for (glp, gpath), (olp, opath, margin) in zip(vit, wv):
            PG.assert_close([glp], [olp])
            assert margin <= 1e-9 or ids(gpath) == opath
        PG.assert_close(ex.logp, logp)
        assert ex.skipped == skipped
        TG.close(ex.counts, counts, 1e-9)
        TG.close(ex.stats, stats, 1e-9)
        return lp, [v[0] for v in vit], [ids(v[1]) for v in vit], ex.counts, ex.stats, ex.logp

    def same(x, y):
        return all(a == b if isinstance(a, list) else np.array_equal(a, b) for a, b in zip(x, y))

    for order in (["base", "moved", "base", "weight", "split", "base"], ["base", "normal", "base", "normal", "base"]):
        seen = [visit(name) for name in order]
        base = [r for name, r in zip(order, seen) if name == "base"]
        assert len(base) == 3 and same(base[0], base[1]) and same(base[0], base[2])
