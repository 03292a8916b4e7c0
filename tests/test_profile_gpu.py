"""Kernel-density HMM states and the profile aligners on the MI355X (csrc/seg_hmm.hpp HmmDevK instantiations,
pypore_amd.alignment) against tests/profile_oracle.py, with the bar and helpers' pattern of tests/test_hmm_gpu.py:
log probabilities and matrix entries to 1e-12 relative to max(1, |oracle|), -inf exactly where the oracle has it, Viterbi
paths identical where the oracle's winning margin exceeds 1e-9 relative and judged by their own score elsewhere.

What this file draws is moderate: 1 to 200 points per state, bandwidths 0.2 to 5, observations within a few bandwidths and one
far sequence, models of at most 200 states and in-degrees far below 256, and its oracle shares the device's formula.  The
emission against long double over extreme point counts, orders, weights and bandwidths, the 16-bit backpointers, the state
cap, the E-step's global-memory route by the model's own size and the upload cache on the kde_* tables are in
tests/test_profile_kernels_gpu.py, which uses check_all, check_viterbi and assert_close from here."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import profile_oracle as P  # noqa: E402

from pypore_amd import alignment as A  # noqa: E402
from pypore_amd.hmm import KIND_KDE, GaussianKernelDensity, Model, NormalDistribution, State  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


def assert_close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= tol, err.max()


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
        score = P.path_score(c, seq, idx)
        assert score is not None and abs(score - lp) <= 1e-9 * max(1.0, abs(lp))


def check_all(model, seqs, matrices=True, c=None):
    c = P.Compiled(model) if c is None else c
    for s, v in zip(seqs, model.viterbi_batch(seqs)):
        check_viterbi(c, s, v)
    assert_close(model.log_probability_batch(seqs), [O.log_probability(c, s) for s in seqs])
    if matrices:
        for s, f in zip(seqs, model.forward_batch(seqs)):
            assert_close(f, O.forward(c, s))
        for s, b in zip(seqs, model.backward_batch(seqs)):
            assert_close(b, O.backward(c, s))
            assert_close([b[0][c.start]], [O.log_probability(c, s)])


def has_kde(model):
    return any(not s.is_silent() and s.distribution.kind == KIND_KDE for s in model.states)


@pytest.mark.parametrize("seed", range(12))
def test_tiny_models_against_brute_force(seed):
    rng = np.random.default_rng(500 + seed)
    model = P.with_kde(lambda: O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0), rng, share=0.7)
    assert has_kde(model)
    c = P.Compiled(model)
    seqs = [rng.normal(size=n) for n in range(7)]
    check_all(model, seqs)
    for s, (lp, path) in zip(seqs, model.viterbi_batch(seqs)):
        _, logp_bf, best_bf, path_bf = P.brute_force(c, s)
        if path_bf is None:
            assert lp == -np.inf and path is None
        else:
            assert abs(lp - best_bf) <= TOL * max(1, abs(best_bf)) and [i for i, _ in path] == path_bf
            assert abs(model.log_probability(s) - logp_bf) <= TOL * max(1, abs(logp_bf))


def test_random_models_mixing_normal_uniform_and_kernel_density():
    """1 to 200 points per state (more than a wave's 64), some zero weights, bandwidths 0.2 to 5."""
    rng = np.random.default_rng(4242)
    most = 0
    for k in range(40):
        model = P.with_kde(lambda: O.random_model(rng, max_states=200, max_chain=40, finite=k % 4 != 3), rng, share=0.4,
                           max_points=200, lo=-6.0, hi=6.0)
        most = max(most, int(np.diff(model.flat["kde_ptr"]).max()))
        seqs = [rng.normal(0, 2, int(rng.integers(0, 12))) for _ in range(2)] + [rng.normal(0, 40, 3)]   # (far from every point)
        check_all(model, seqs, matrices=k % 4 == 0)
    assert most > 64


def one_point_pair(n=20, seed=5):
    normal, means = O.profile_model(n, seed=seed)
    kde, _ = O.profile_model(n, seed=seed)
    for s in kde._added:
        if not s.is_silent() and type(s.distribution).__name__ == "NormalDistribution":
            s.distribution = GaussianKernelDensity([s.distribution.parameters[0]], s.distribution.parameters[1])
    kde.bake()
    return normal, kde, means


def test_one_point_kernel_density_equals_normal_states():
    normal, kde, means = one_point_pair()
    assert has_kde(kde) and not has_kde(normal)
    seqs = O.profile_events(means, 6, lo=10, hi=80, seed=2)
    for (a, pa), (b, pb) in zip(normal.viterbi_batch(seqs), kde.viterbi_batch(seqs)):
        assert_close([b], [a])
        assert [i for i, _ in pa] == [i for i, _ in pb]
    assert_close(kde.log_probability_batch(seqs), normal.log_probability_batch(seqs))
    for x, y in zip(kde.forward_batch(seqs), normal.forward_batch(seqs)):
        assert_close(x, y)
    for x, y in zip(kde.backward_batch(seqs), normal.backward_batch(seqs)):
        assert_close(x, y)
    ek, en = kde.expected_counts_batch(seqs), normal.expected_counts_batch(seqs)
    assert_close(ek.logp, en.logp)
    assert np.allclose(ek.counts, en.counts, rtol=1e-9, atol=1e-12) and np.allclose(ek.stats, en.stats, rtol=1e-9, atol=1e-9)


def profile_case(rows=6, columns=12, seed=3, count=24):
    msa, _ = P.alignment_case(seed)
    rng = np.random.default_rng(seed)
    template, seqs = P.derived_sequences(rng, columns, count)
    msa = [[float(v + rng.normal(0, 0.8)) if rng.random() > 0.1 else '-' for v in template] for _ in range(rows)]
    pa = A.ProfileAligner(msa, [1.0], bandwidth=1.3)
    return pa._build_global(pa.master, 0, 60), [np.array(s) for s in seqs]


@pytest.mark.parametrize("acc_lds", [1, 0])
def test_expected_counts_against_the_restated_formulas(acc_lds):
    from pypore_amd import engine
    rng = np.random.default_rng(900 + acc_lds)
    cases = [(P.with_kde(lambda: O.random_tiny(rng, finite=k % 2 == 0, silent_chain=k % 3 != 0), rng, share=0.7),
              [rng.normal(size=n) for n in range(6)]) for k in range(6)]
    cases.append(profile_case())
    with LG.options(engine.context(), hmm_expect_lds=acc_lds):
        for model, seqs in cases:
            assert has_kde(model)
            counts, stats, logp, skipped = P.estep(model, seqs)
            got = model.expected_counts_batch(seqs)
            assert_close(got.logp, logp)
            assert got.skipped == skipped
            assert np.allclose(got.counts, counts, rtol=1e-9, atol=1e-12)
            assert np.allclose(got.stats, stats, rtol=1e-9, atol=1e-9)
            again = model.expected_counts_batch(seqs)
            assert all(np.array_equal(x, y) for x, y in zip(got[:3], again[:3]))


def test_train_leaves_kernel_densities_alone(capsys):
    model, seqs = profile_case(seed=8)
    extra = State(NormalDistribution(30.0, 5.0), "N")                     # a normal state beside the profile
    model.add_transition(model.start, extra, 0.2)
    model.add_transition(extra, extra, 0.5)
    model.add_transition(extra, [s for s in model.states if s.name == "M1"][0], 0.5)
    model.bake()
    kdes = [s.distribution for s in model.states if not s.is_silent() and s.distribution.kind == KIND_KDE]
    before = [copy.deepcopy(d.parameters) for d in kdes]
    tables = {k: model.flat[k].copy() for k in ("kde_ptr", "kde_pt", "kde_lw")}
    params = model.flat["param"].copy()
    edges = list(model.edges)
    total = model.train(seqs, max_iterations=3, verbose=False)
    assert np.isfinite(total)
    assert [d.parameters for d in kdes] == before
    assert all(np.array_equal(model.flat[k], v) for k, v in tables.items())
    kd = model.flat["kind"] == KIND_KDE
    assert np.array_equal(model.flat["param"].reshape(-1, 3)[kd], params.reshape(-1, 3)[kd])
    assert extra.distribution.parameters != [30.0, 5.0] and model.edges != edges


def test_ragged_batch_equals_single_calls_and_budget_cuts():
    from pypore_amd import engine
    model, seqs = profile_case(seed=4, count=30)
    seqs = seqs + [np.zeros(0), np.array([100.0] * 40)]                 # an empty and an impossible sequence
    whole_v, whole_l = model.viterbi_batch(seqs), model.log_probability_batch(seqs)
    whole_f, whole_b = model.forward_batch(seqs), model.backward_batch(seqs)
    whole_e = model.expected_counts_batch(seqs)
    assert whole_v[-1] == (-np.inf, None) and whole_e.skipped == 1
    for q, s in enumerate(seqs):
        lp, path = model.viterbi(s)
        assert lp == whole_v[q][0] and (path is None) == (whole_v[q][1] is None)
        assert path is None or [i for i, _ in path] == [i for i, _ in whole_v[q][1]]
        assert model.log_probability(s) == whole_l[q]
        assert np.array_equal(model.forward(s), whole_f[q]) and np.array_equal(model.backward(s), whole_b[q])
    S = len(model.states)
    with LG.options(engine.context(), hmm_bp_budget=S * 16 * 3, hmm_fb_budget=S * 8 * 16 * 3):
        cut_v, cut_e = model.viterbi_batch(seqs), model.expected_counts_batch(seqs)
    for (a, pa), (b, pb) in zip(whole_v, cut_v):
        assert a == b and (pa is None) == (pb is None) and (pa is None or [i for i, _ in pa] == [i for i, _ in pb])
    assert all(np.array_equal(x, y) for x, y in zip(whole_e[:3], cut_e[:3])) and cut_e.skipped == 1


@pytest.mark.parametrize("acc_lds", [1, 0])
def test_expect_launch_shape_with_slots_pct(acc_lds, capfd):
    """The E-step grid of a kernel-density model goes through resident_slots: slots_pct 1 shrinks it, each workgroup then
    carries several sequences, and the sums stay within 1e-12 of the default grid's (logp bit for bit)."""
    from pypore_amd import engine
    model, seqs = profile_case(seed=6, count=400)
    S, E, NE = len(model.states), len(model.edges), model.flat["n_emit"]
    lds = (2 * S + (E + 3 * NE + 1 if acc_lds else 0)) * 8
    ctx = engine.context()
    with LG.options(ctx, hmm_expect_lds=acc_lds):
        ref = model.expected_counts_batch(seqs)
    capfd.readouterr()
    with LG.options(ctx, hmm_expect_lds=acc_lds, slots_pct=1, debug=1):
        small = model.expected_counts_batch(seqs)
    (slots, pct), = LG.printed_slots(capfd.readouterr().err, lds)
    assert pct == 1 and 2 <= slots and len(seqs) >= 2 * slots, slots
    assert np.array_equal(small.logp, ref.logp)
    assert np.allclose(small.counts, ref.counts, rtol=1e-12, atol=1e-12) and np.allclose(small.stats, ref.stats, rtol=1e-12, atol=1e-9)


# ---- the C ABI: a model without kernel densities never reads the appended fields ----------------------------------------------
def test_appended_fields_are_ignored_without_kind_3():
    from pypore_amd import _lib
    model, means = O.profile_model(20, seed=9)
    other, _ = profile_case(seed=2)
    seqs = O.profile_events(means, 10, lo=10, hi=60, seed=3)
    c = O.Compiled(model)
    ctx, off, obs = model._upload(seqs, None)
    base = model._c_model()
    assert not base.kde_ptr and not base.kde_pt and not base.kde_lw                  # NULL, as an older caller leaves them
    alt = _lib.HmmModel()
    ctypes.memmove(ctypes.byref(alt), ctypes.byref(base), ctypes.sizeof(alt))
    f = other.flat                                                                   # valid tables of an unrelated model
    alt.kde_ptr, alt.kde_pt, alt.kde_lw = f["kde_ptr"].ctypes.data, f["kde_pt"].ctypes.data, f["kde_lw"].ctypes.data
    for mode in (_lib.PS_HMM_VITERBI, _lib.PS_HMM_FORWARD, _lib.PS_HMM_BACKWARD):
        la, ma, pa = ctx.hmm_batch(base, mode, obs, off, True)
        lb, mb, pb = ctx.hmm_batch(alt, mode, obs, off, True)
        assert np.array_equal(la.cpu().numpy(), lb.cpu().numpy()) and np.array_equal(ma.cpu().numpy(), mb.cpu().numpy())
        if mode == _lib.PS_HMM_VITERBI:
            (xa, oa, na), (xb, ob, nb) = [(p[0].cpu().numpy(), p[1], p[2].cpu().numpy()) for p in (pa, pb)]
            assert np.array_equal(na, nb) and np.array_equal(oa, ob)
            assert all(np.array_equal(xa[oa[q]:oa[q] + na[q]], xb[ob[q]:ob[q] + nb[q]]) for q in range(len(seqs)))
            assert_close(la.cpu().numpy(), [O.viterbi(c, s)[0] for s in seqs])
        elif mode == _lib.PS_HMM_FORWARD:
            assert_close(la.cpu().numpy(), [O.log_probability(c, s) for s in seqs])
            mat = ma.cpu().numpy()
            assert_close(mat[off[1] + 1:off[2] + 2], O.forward(c, seqs[1]))
        else:
            mat = ma.cpu().numpy()
            assert_close(mat[off[1] + 1:off[2] + 2], O.backward(c, seqs[1]))
    ea, eb = ctx.hmm_expect(base, obs, off), ctx.hmm_expect(alt, obs, off)
    for x, y in zip(ea[:3], eb[:3]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert ea[3] == eb[3]
    import hmm_train_oracle as TO
    counts, stats, logp, _ = TO.estep(model, seqs)
    assert_close(ea[0].cpu().numpy(), logp)
    assert np.allclose(ea[1].cpu().numpy(), counts, rtol=1e-9, atol=1e-12)


def test_bad_kernel_density_tables_are_refused():
    from pypore_amd import _lib
    model, seqs = profile_case(seed=2, count=2)
    ctx, off, obs = model._upload(seqs, None)
    base = model._c_model()
    f = model.flat
    bad_ptr = f["kde_ptr"].copy()
    k = int(np.flatnonzero(f["kind"] == KIND_KDE)[1])
    bad_ptr[k] = bad_ptr[k + 1] + 1                                                   # not monotone
    bad_lw = f["kde_lw"].copy()
    bad_lw[0] = 0.5                                                                   # a log weight above 0
    for field, arr in (("kde_ptr", bad_ptr), ("kde_lw", bad_lw), ("kde_pt", None)):
        m = _lib.HmmModel()
        ctypes.memmove(ctypes.byref(m), ctypes.byref(base), ctypes.sizeof(m))
        setattr(m, field, arr.ctypes.data if arr is not None else None)
        with pytest.raises(Exception, match="kde|kernel-density"):
            ctx.hmm_batch(m, _lib.PS_HMM_FORWARD, obs, off, False)
    assert np.isfinite(model.log_probability(seqs[0]))                                # the context still works


# ---- the aligners end to end -----------------------------------------------------------------------------------------------------
# P.alignment_case(0..21), every seed: P.align_ties gives per alignment the smallest NON-ZERO gap on the winning path, the
# number of exact ties there and whether those are structural (identical operands on both sides: the device, whose exp and
# log1p round differently, ties too, and the shared rule -- lowest source -- picks the same path).  An alignment whose
# non-zero gaps all exceed 1e-9 and whose ties are structural compares whole alignments; any other is only counted.  On the
# CPU (tests/test_viterbi_exact_host.py): seed 3 meets 1 and seed 15 meets 2 alignments with an exact tie, all structural,
# no non-zero gap of the 176 alignments is below 2.1e-4, so the oracle leaves out 0 of 176 (0 of the 220 cases below).
ALIGN_SEEDS = list(range(22))
MAX_TIE_SHARE = 0.05


def same_profile(got, want):
    return got.msa == want.msa and got.pssm == want.pssm and got.consensus == want.consensus


def test_profile_aligner_and_batch_end_to_end():
    cases = ties = 0
    for seed in ALIGN_SEEDS:
        msa, slaves = P.alignment_case(seed)
        for mode in ("global", "local"):
            want = [P.align_ties(copy.deepcopy(msa), list(s), mode) for s in slaves]
            pa = A.ProfileAligner(copy.deepcopy(msa), list(slaves[0]))
            single = pa.global_alignment() if mode == "global" else pa.local_alignment()
            master = copy.deepcopy(msa)
            batch = A.profile_align_batch(master, [list(s) for s in slaves], mode)
            assert master == P.Pssm(copy.deepcopy(msa)).msa                        # all-gap columns deleted, nothing else
            for got, (prob, wm, ws, gap, exact, structural) in zip([single] + batch, [want[0]] + want):
                cases += 1
                assert_close([got[0]], [prob])
                if gap > 1e-9 and structural:
                    assert same_profile(got[1], wm) and same_profile(got[2], ws)
                else:
                    ties += 1
            assert same_profile(single[1], batch[0][1]) and same_profile(single[2], batch[0][2]) and single[0] == batch[0][0]
    assert cases == len(ALIGN_SEEDS) * 2 * 5 and ties <= MAX_TIE_SHARE * cases, (ties, cases)


def test_impossible_slave_and_repeat_alignment():
    msa, slaves = P.alignment_case(1)
    n = len(P.Pssm(copy.deepcopy(msa)).pssm)
    out = A.profile_align_batch(copy.deepcopy(msa), [list(slaves[0]), [100.0] * (n + 1)])
    assert np.isfinite(out[0][0]) and out[1] == (-np.inf, None, None)
    assert A.ProfileAligner(copy.deepcopy(msa), [100.0] * (n + 1)).global_alignment() == (-np.inf, None, None)
    prob, names = A.ProfileAligner(copy.deepcopy(msa), list(slaves[0])).repeat_alignment()
    ref = P.Pssm(copy.deepcopy(msa))
    c = P.Compiled(P.build_repeat(ref))
    lp, path, margin = O.viterbi(c, slaves[0])
    assert_close([prob], [lp])
    assert margin <= 1e-9 or names == [c.states[k].name for k in path[1:-1]]


# Seeds 1, 2, 4, 5 meet no exact tie and no non-zero gap below 1e-2.  Seed 3 meets 1 exact tie, structural.  Seeds 0 and 3
# each meet one decision whose two candidates are the same sum added in two orders and differ by one ulp (relative gaps
# 1.4e-16 and 2.8e-16; M11 entered from I10 or D10).  That is rounding, not structure -- seed 0 never met an exact tie --
# so a device whose emissions differ by ulps may take either side.  The oracle therefore solves these seeds twice, the
# second time taking the other side of every near tie (flip_near), and the device must return one of the two outcomes,
# alignment and score.  (Seed 0: both sides give the same alignment, the near-tie trial is not the one kept; seed 3: two.)
MSA_SEEDS = [0, 1, 2, 3, 4, 5]
MSA_NEAR_TIE_SEEDS = (0, 3)


@pytest.mark.parametrize("seed", MSA_SEEDS)
def test_multiple_sequence_aligner_end_to_end(seed):
    rng = np.random.default_rng(700 + seed)
    _, seqs = P.derived_sequences(rng, int(rng.integers(6, 16)), int(rng.integers(3, 7)))
    want_score, want_msa, gap, exact, structural = P.msa_iterative_ties(copy.deepcopy(seqs), max_iterations=3)
    assert structural and (gap > 1e-9) == (seed not in MSA_NEAR_TIE_SEEDS)     # (found so on the CPU)
    outcomes = [(want_score, want_msa)]
    if not gap > 1e-9:
        outcomes.append(P.msa_iterative_ties(copy.deepcopy(seqs), max_iterations=3, flip_near=True)[:2])
    score, msa = A.MultipleSequenceAligner(copy.deepcopy(seqs)).iterative_alignment(max_iterations=3)
    assert len({len(r) for r in msa}) == 1
    assert sorted([x for x in r if x != '-'] for r in msa) == sorted(seqs)
    assert any(msa == m and abs(score - sc) <= TOL * max(1.0, abs(sc)) for sc, m in outcomes)


def test_profile_above_the_state_cap():
    n = 1366                                                                    # 3 n + 3 = 4101 states
    with pytest.raises(ValueError, match="4096"):
        A.ProfileAligner([float(i % 50) + 1 for i in range(n)], [1.0, 2.0]).global_alignment()
