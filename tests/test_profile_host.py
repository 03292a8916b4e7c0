"""Host-side tests of the kernel-density emission and the profile aligners (no GPU): GaussianKernelDensity against scipy,
the baked flat form, PSSM, the three model builders against probabilities written out here, the path-following loops on
hand-made paths, the MSA score on columns worked by hand, and tests/profile_oracle.py against its own brute force; the
float64 restatements of the density against np.longdouble on the emission probe's grid (profile_oracle.kde_probe_grid), which
tests/test_profile_kernels_gpu.py puts to the device."""
import copy
import math
import os
import sys

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import norm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import profile_oracle as P  # noqa: E402

from pypore_amd import alignment as A  # noqa: E402
from pypore_amd.hmm import (KIND_KDE, KIND_UNIFORM, GaussianKernelDensity, Model, NormalDistribution, State,  # noqa: E402
                            UniformDistribution)


def scipy_kde(points, h, weights, x):
    w = np.asarray(weights, float)
    w = w / w.sum()
    keep = w > 0
    return logsumexp(norm.logpdf(x, np.asarray(points, float)[keep], h), b=w[keep])


# ---- the density -----------------------------------------------------------------------------------------------------
def test_density_against_scipy():
    rng = np.random.default_rng(1)
    for _ in range(200):
        n = int(rng.integers(1, 80))
        pts, h = rng.uniform(0, 60, n), float(rng.uniform(0.2, 5))
        w = rng.uniform(0, 1, n) if rng.random() < 0.5 else None
        d = GaussianKernelDensity(pts, h, w)
        assert abs(sum(d.parameters[2]) - 1.0) < 1e-15 * n
        for x in rng.uniform(-10, 70, 5):
            want = scipy_kde(pts, h, np.ones(n) if w is None else w, x)
            assert abs(d.log_probability(x) - want) <= 1e-13 * max(1.0, abs(want))
            assert abs(P.kde_logpdf(pts, h, d.parameters[2], x) - want) <= 1e-13 * max(1.0, abs(want))


def test_one_point_is_a_normal():
    for p, h, x in [(3.0, 2.0, 1.0), (40.0, 0.3, 41.0), (0.0, 1.0, 0.0), (25.0, 5.0, -300.0)]:
        assert GaussianKernelDensity([p], h).log_probability(x) == pytest.approx(NormalDistribution(p, h).log_probability(x), rel=1e-15, abs=1e-15)
    assert GaussianKernelDensity([7.0]).parameters == [[7.0], 1.0, [1.0]]


def test_weights_are_normalised_and_zero_weights_skipped():
    a = GaussianKernelDensity([1.0, 2.0, 30.0], 0.7, [2.0, 0.0, 6.0])
    assert a.parameters[2] == [0.25, 0.0, 0.75]
    b = GaussianKernelDensity([1.0, 30.0], 0.7, [0.25, 0.75])
    for x in (0.0, 2.0, 29.0, 100.0):
        assert a.log_probability(x) == b.log_probability(x)
    assert a.tables() == ([1.0, 30.0], [math.log(0.25), math.log(0.75)])
    assert a.compiled()[0] == pytest.approx(0.25 * 1 + 0.75 * 30)


def test_far_observation_is_finite():
    d = GaussianKernelDensity([10.0, 12.0, 15.0], 0.5)
    x = 15.0 + 40 * 0.5
    want = scipy_kde([10.0, 12.0, 15.0], 0.5, [1, 1, 1], x)
    assert np.isfinite(d.log_probability(x)) and d.log_probability(x) == pytest.approx(want, rel=1e-13)
    assert np.isfinite(d.log_probability(1e4)) and d.log_probability(1e4) < -1e7


def test_value_errors_freeze_and_repr():
    for args in [([],), ([1.0, float("nan")],), ([1.0, float("inf")],), ([1.0], 0), ([1.0], -1), ([1.0, 2.0], 1, [1.0, -1.0]),
                 ([1.0, 2.0], 1, [1.0, float("nan")]), ([1.0, 2.0], 1, [0.0, 0.0]), ([1.0, 2.0], 1, [1.0, float("inf")])]:
        with pytest.raises(ValueError):
            GaussianKernelDensity(*args)
    d = GaussianKernelDensity([1, 2], 2)
    assert not d.frozen and d.kind == KIND_KDE
    d.freeze()
    assert d.frozen
    d.thaw()
    assert not d.frozen
    assert repr(d) == "GaussianKernelDensity([1.0, 2.0], 2.0, [0.5, 0.5])"


# ---- the density against long double on the probe grid ----------------------------------------------------------------------
def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


# What the float64 restatements may lose against long double, relative to max(1, |value|).  A term lw - d^2 b carries four
# roundings (d, d^2, the product, the difference), each at most eps / 2 of a magnitude the value itself bounds; exp turns
# the error of v - m into a relative one of at most |v - m| eps, which exp(v - m) scales down again (t e^-t <= 1 / e); the N
# positive terms are summed in sequence, whose error grows as sqrt(N) eps in the mean (7.8e-15 at N = 5000; N eps = 5.6e-13
# in the worst case, still inside the 1e-12 bar of the device tests); log1p divides it by 1 + r.  So 1e-14 covers every point
# count of the grid and leaves the device two orders of magnitude of the bar.  (Measured: 9.1e-16 at worst, at N = 200 and 5000.)
HOST_MARGIN = 1e-14


def test_host_restatements_against_long_double_on_the_probe_grid():
    grid = P.kde_probe_grid()
    assert len(grid) == 7 * 5 * 4 * 2 and len({name for name, _, _ in grid}) == len(grid)
    worst = {}
    for name, d, xs in grid:
        pts, h, w = d.parameters
        assert len(xs) == 7
        for x in xs:
            ref = P.kde_logpdf_longdouble(pts, h, w, x)
            assert np.isfinite(ref)
            for got in (d.log_probability(x), P.kde_logpdf(pts, h, w, x)):
                err = float(abs(np.longdouble(got) - ref) / max(1.0, abs(float(ref))))
                worst[len(pts)] = max(worst.get(len(pts), 0.0), err)
    print("host restatements vs long double, worst per point count:", worst)
    assert sorted(worst) == list(P.PROBE_POINTS) and max(worst.values()) <= HOST_MARGIN, worst


def test_overflowing_distance_is_minus_infinity_on_the_host():
    """(x - p)^2 overflows float64 at x = 1e200: the class and the float64 oracle give exactly -inf (float64 semantics are
    the contract).  The long-double value is finite there, about -5e399: it is no yardstick for this case."""
    d = GaussianKernelDensity([0.0, 1.0, 7.25], 1.0, [1.0, 2.0, 3.0])
    assert d.log_probability(1e200) == -np.inf
    with np.errstate(over="ignore"):
        assert P.kde_logpdf(*d.parameters, 1e200) == -np.inf
    assert np.isfinite(P.kde_logpdf_longdouble(*d.parameters, 1e200))


# ---- the flat form -----------------------------------------------------------------------------------------------------
def test_baked_flat_form():
    m = Model("f")
    a = State(GaussianKernelDensity([1.0, 2.0, 4.0], 0.5, [1, 0, 3]), "a")
    b = State(NormalDistribution(3, 2), "b")
    c = State(GaussianKernelDensity([9.0], 2.0), "c")
    u = State(UniformDistribution(0, 4), "d")
    for s, t in [(m.start, a), (a, b), (b, c), (c, u), (u, m.end), (a, a)]:
        m.add_transition(s, t, 0.5)
    m.bake()
    f = m.flat
    assert list(f["kind"][:4]) == [3, 1, 3, 2]
    assert list(f["kde_ptr"]) == [0, 2, 2, 3, 3] and f["kde_ptr"].dtype == np.int32
    assert list(f["kde_pt"]) == [1.0, 4.0, 9.0]
    assert list(f["kde_lw"]) == [math.log(0.25), math.log(0.75), 0.0]
    assert list(f["param"][0:3]) == pytest.approx([0.25 + 3.0, 1 / (2 * 0.25), -math.log(0.5 * math.sqrt(2 * math.pi))], rel=1e-15)
    assert list(f["param"][6:9]) == pytest.approx([9.0, 1 / 8.0, -math.log(2 * math.sqrt(2 * math.pi))], rel=1e-15)
    # a model without kernel densities: empty tables, every other array as before
    plain, _ = O.profile_model(5)
    assert plain.flat["kde_pt"].size == 0 and list(plain.flat["kde_ptr"]) == [0] * (plain.flat["n_emit"] + 1)
    # the M-step leaves the kernel densities alone and recompiles the same tables
    before = copy.deepcopy(a.distribution.parameters)
    m._m_step(np.ones(len(m.edges)), np.ones((4, 3)))
    assert a.distribution.parameters == before and list(m.flat["kde_pt"]) == [1.0, 4.0, 9.0]
    assert b.distribution.parameters != [3.0, 2.0]


# ---- PSSM ------------------------------------------------------------------------------------------------------------------
def test_pssm():
    flat = [1.0, 2.0, 3.0]
    p = A.PSSM(flat)
    assert p.msa == [flat] and p.msa[0] is flat and p.pssm == [[1.0], [2.0], [3.0]] and p.consensus == [1.0, 2.0, 3.0]
    rows = [[1.0, '-', 3.0, '-'], ['-', '-', 5.0, 2.0], [2.0, '-', '-', '-']]
    p = A.PSSM(rows)
    assert rows == [[1.0, 3.0, '-'], ['-', 5.0, 2.0], [2.0, '-', '-']]          # the all-gap column is gone, in place
    assert p.msa is rows and len(p) == 3 and p.pssm == [[1.0, 2.0], [3.0, 5.0], [2.0]]
    assert p.consensus == [1.5, 4.0, 2.0] and p[1] == [3.0, 5.0] and p[0:2] == [[1.0, 2.0], [3.0, 5.0]]
    assert repr(p) == "1.5\n4.0\n2.0"
    dash = "".join(["-"])                                                        # an equal but not identical gap string
    assert A.PSSM([[1.0, dash], [dash, dash]]).pssm == [[1.0]]
    q = P.Pssm([[1.0, '-', 3.0, '-'], ['-', '-', 5.0, 2.0], [2.0, '-', '-', '-']])
    assert (q.msa, q.pssm, q.consensus) == (p.msa, p.pssm, p.consensus)


# ---- builders --------------------------------------------------------------------------------------------------------------
def edge_table(model):
    return {(model.states[i].name, model.states[j].name): p for i, j, p in model.edges}


def check_table(model, want):
    got = edge_table(model)
    assert set(got) == set(want)
    for k, p in want.items():
        assert got[k] == pytest.approx(p, rel=1e-15), k


def test_global_builder():
    pa = A.ProfileAligner([[10.0, 20.0], [12.0, '-']], [11.0, 19.0], bandwidth=1.5)
    m = pa._build_global(pa.master, 0, 60)
    s, e = "Global Profile Aligner-start", "Global Profile Aligner-end"
    assert len(m.states) == 3 * 2 + 1 + 2 and m.finite
    assert [x.name for x in m.states[:5]] == ["I0", "I1", "I2", "M1", "M2"]
    check_table(m, {(s, "I0"): .15, (s, "M1"): .60, (s, "D1"): .25,
                    ("I0", "I0"): .20 / 1.05, ("I0", "M1"): .65 / 1.05, ("I0", "D1"): .20 / 1.05,
                    ("M1", "I1"): .15, ("M1", "M2"): .60, ("M1", "D2"): .25,
                    ("I1", "I1"): .15, ("I1", "M2"): .65, ("I1", "D2"): .20,
                    ("D1", "I1"): .15, ("D1", "M2"): .65, ("D1", "D2"): .20,
                    ("M2", "I2"): .15, ("M2", e): .85, ("I2", "I2"): .15, ("I2", e): .85, ("D2", "I2"): .15, ("D2", e): .85})
    d = {x.name: x.distribution for x in m.states}
    assert d["M1"].parameters == [[10.0, 12.0], 1.5, [0.5, 0.5]] and d["M2"].parameters == [[20.0], 1.5, [1.0]]
    assert d["I0"] is d["I1"] is d["I2"] and d["I0"].kind == KIND_UNIFORM and d["I0"].parameters == [0.0, 60.0]
    for n in (1, 5, 17):
        pa = A.ProfileAligner([float(v) for v in range(n)], [1.0])
        assert len(pa._build_global(pa.master, 0, 60).states) == 3 * n + 1 + 2


def test_local_and_repeat_builders():
    pa = A.ProfileAligner([10.0, 20.0, 30.0], [11.0, 19.0])
    core = {("P0", "M0"): 1 / 3., ("P0", "M1"): 1 / 3., ("P0", "M2"): 1 / 3.,
            ("M0", "I0"): .15, ("M0", "PE"): .05, ("M0", "M1"): .65, ("M0", "D1"): .15,
            ("I0", "I0"): .20 / 1.05, ("I0", "D1"): .20 / 1.05, ("I0", "M1"): .65 / 1.05,
            ("M1", "I1"): .15, ("M1", "PE"): .05, ("M1", "M2"): .80, ("I1", "I1"): .15, ("I1", "M2"): .85,
            ("D1", "I1"): .15, ("D1", "M2"): .85, ("M2", "PE"): 1.0}
    s, e = "Local Profile Aligner-start", "Local Profile Aligner-end"
    local = dict(core)
    local.update({(s, "Q0"): .5, (s, "P0"): .5, ("Q0", "Q0"): .75, ("Q0", "P0"): .25,
                  ("PE", "QE"): .5, ("PE", e): .5, ("QE", "QE"): .75, ("QE", e): .25})
    check_table(pa._build_local(pa.master, 0, 60), local)
    rep = dict(core)
    rep.update({(s, "P0"): .5, (s, "Q"): .5, ("Q", "Q"): .5, ("Q", "P0"): .25, ("Q", e): .25, ("PE", "Q"): .5, ("PE", e): .5})
    check_table(pa._build_repeat(pa.master, 0, 60), rep)
    with pytest.raises(ValueError):
        A.ProfileAligner([1.0, 2.0], [1.0])._build_local(A.PSSM([1.0, 2.0]), 0, 60)


@pytest.mark.parametrize("n", [3, 4, 9])
def test_builders_equal_the_restatement(n):
    rng = np.random.default_rng(n)
    rows = [[float(v) for v in rng.uniform(5, 55, n)] for _ in range(3)]
    rows[1][1] = '-'
    pa = A.ProfileAligner(copy.deepcopy(rows), [1.0], bandwidth=2)
    ref = P.Pssm(copy.deepcopy(rows))
    for mine, theirs in [(pa._build_global, P.build_global), (pa._build_local, P.build_local), (pa._build_repeat, P.build_repeat)]:
        a, b = mine(pa.master, 1, 59), theirs(ref, 1, 59, 2)
        assert [s.name for s in a.states] == [s.name for s in b.states] and a.edges == b.edges
        assert [repr(s.distribution) for s in a.states] == [repr(s.distribution) for s in b.states]


# ---- the path loops ----------------------------------------------------------------------------------------------------------
def test_follow_global_by_hand():
    for mod, pssm in ((A, A.PSSM), (P, P.Pssm)):
        master, slave = pssm([[10.0, 20.0, 30.0], [11.0, '-', 31.0]]), pssm([10.0, 25.0, 30.0])
        mod.follow_global(master, slave, ["s", "M1", "D2", "I2", "M3", "e"])
        assert master.msa == [[10.0, 20.0, '-', 30.0], [11.0, '-', '-', 31.0]] and master.pssm == [[10.0, 11.0], [20.0], '-', [30.0, 31.0]]
        assert slave.msa == [[10.0, '-', 25.0, 30.0]] and slave.pssm == [[10.0], '-', [25.0], [30.0]]
        assert master.consensus == [10.5, 20.0, 30.5] and slave.consensus == [10.0, 25.0, 30.0]     # left alone


def test_follow_local_by_hand():
    for mod, pssm in ((A, A.PSSM), (P, P.Pssm)):
        # offset trim at M1 and the PE cut of one trailing QE
        master, slave = pssm([10.0, 20.0, 30.0, 40.0]), pssm([5.0, 20.0, 30.0, 7.0])
        mod.follow_local(master, slave, ["s", "Q0", "P0", "M1", "M2", "PE", "QE", "e"])
        assert master.msa == [[20.0, 30.0, 40.0]] and master.pssm == [[20.0], [30.0], [40.0]] and master.consensus == [20.0, 30.0, 40.0]
        assert slave.msa == [[5.0, 20.0, 30.0]] and slave.pssm == [[5.0], [20.0], [30.0], [7.0]]
        # an insert lands at i - offset, a delete at i (the reference's arithmetic, kept)
        master, slave = pssm([10.0, 20.0, 30.0, 40.0, 50.0]), pssm([30.0, 33.0, 50.0])
        mod.follow_local(master, slave, ["s", "P0", "M2", "I2", "D3", "M4", "PE", "e"])
        assert master.msa == [['-', 30.0, 40.0, 50.0]] and master.consensus == [30.0, 40.0, 50.0]
        assert slave.msa == [[30.0, 33.0, 50.0, '-']]


# ---- the MSA score -----------------------------------------------------------------------------------------------------------
def test_score_by_hand():
    msa = [[1.0, 3.0, 2.0, 4.0], [3.0, '-', 2.0, 8.0], ['-', '-', 2.0, 6.0]]
    # column 0: two values of std 1 -> 0.5 log(2 pi e) / 4; column 1: one value -> 0; column 2: no spread -> 0;
    # column 3: three values 4, 8, 6 of variance 8/3 -> 0.5 log(2 pi e 8/3) / 9
    want = 0.5 * math.log(2 * math.pi * math.e) / 4 + 0.5 * math.log(2 * math.pi * math.e * 8 / 3) / 9
    assert A.MultipleSequenceAligner([])._score(msa) == pytest.approx(want, rel=1e-14)
    assert P.msa_score(msa) == pytest.approx(want, rel=1e-14)


# ---- the oracle against its own brute force --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(10))
def test_oracle_against_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    model = P.with_kde(lambda: O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0), rng, share=0.7)
    assert any(s.distribution is not None and s.distribution.kind == KIND_KDE for s in model.states)
    c = P.Compiled(model)
    for n in range(6):
        seq = rng.normal(size=n)
        F, logp, best, path = P.brute_force(c, seq)
        lp, vpath, _ = O.viterbi(c, seq)
        if path is None:
            assert vpath is None and O.log_probability(c, seq) == -np.inf
            continue
        assert abs(lp - best) <= 1e-12 * max(1, abs(best)) and vpath == path
        assert abs(P.path_score(c, seq, path) - best) <= 1e-12 * max(1, abs(best))
        assert abs(O.log_probability(c, seq) - logp) <= 1e-12 * max(1, abs(logp))
        got = O.forward(c, seq)
        fin = np.isfinite(F)
        assert np.array_equal(fin, np.isfinite(got)) and np.allclose(got[fin], F[fin], rtol=1e-12, atol=1e-12)
        assert abs(O.backward(c, seq)[0, c.start] - logp) <= 1e-12 * max(1, abs(logp))
        c1, s1, l1 = P.estep_one(model, seq)
        c2, s2, l2 = P.estep_brute_force(model, seq)
        assert np.allclose(c1, c2, rtol=1e-10, atol=1e-12) and np.allclose(s1, s2, rtol=1e-10, atol=1e-12) and abs(l1 - l2) <= 1e-12 * max(1, abs(l2))


def test_restated_alignment_runs_and_keeps_the_sequences():
    rng = np.random.default_rng(7)
    _, seqs = P.derived_sequences(rng, 8, 4)
    score, msa, margin = P.msa_iterative(copy.deepcopy(seqs), max_iterations=2)
    assert len({len(r) for r in msa}) == 1 and margin > 1e-9
    assert sorted([x for x in r if x != '-'] for r in msa) == sorted(seqs)
    prob, m, s, _ = P.align(copy.deepcopy(seqs[:3]), list(seqs[3]), mode="local")
    assert np.isfinite(prob) and [x for x in s.msa[0] if x != '-'] == seqs[3][:len([x for x in s.msa[0] if x != '-'])]
    # more values than columns, all outside the insert range: some insert must emit one of them
    assert P.align([list(seqs[0])], [100.0] * (len(seqs[0]) + 1))[:3] == (-np.inf, None, None)
