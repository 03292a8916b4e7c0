"""hmm_oracle.viterbi_exact -- the device's Viterbi restated in plain Python floats -- checked on the CPU before the GPU
tests trust it (tests/test_viterbi_exact_gpu.py), and the tie models of tests/viterbi_ties.py proved not to be vacuous.

  * against the existing oracles (O.viterbi, the numpy dynamic programme with its own emission formula, and O.brute_force):
    logp and the score matrix within 1e-12 relative to max(1, |oracle|), -inf in the same places, the same path wherever
    O.viterbi's margin exceeds 1e-9.  The two differ by ulps (the emission formulas round differently), hence the bound;
  * every tie model: the stated number of tied decisions lies on the winning path, the opposite rule (last candidate, highest
    final state) gives ANOTHER path, and both paths have exactly the same O.path_score.  A kernel that took >= for >, or
    preferred the higher lane or stride, would therefore return a path the GPU test rejects;
  * the profile-aligner seeds with exact ties: whether each tie is structural (identical operands on both sides, so that a
    device whose exp / log1p round differently ties too), judged by solving again with long-double emissions.

Run with -s to see the tie counts and the verdicts."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import profile_oracle as P  # noqa: E402
import viterbi_ties as VT  # noqa: E402

from pypore_amd.hmm import GaussianKernelDensity, Model, NormalDistribution, State  # noqa: E402

TOL = 1e-12


def assert_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin]))
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= TOL, err.max()


def check_against_oracle(model, seqs, c=None):
    c = O.Compiled(model) if c is None else c
    for s in seqs:
        lp, path, mat, ties, other = O.viterbi_exact(model, s)
        want_lp, want_path, margin = O.viterbi(c, s)
        want_mat = O._forward_like(c, np.asarray(s, np.float64), True)[0]
        assert mat.shape == (len(s) + 1, len(model.states))
        assert_close(mat, want_mat)
        if want_path is None:
            assert lp == -np.inf and path is None and other is None and ties == 0
            continue
        assert_close([lp], [want_lp])
        assert path[0] == c.start and other[0] == c.start and len(path) >= len(s) + 1
        if margin > 1e-9:
            assert path == want_path and ties == 0 and other == path
        else:
            score = O.path_score(c, s, path)
            assert score is not None and abs(score - want_lp) <= 1e-9 * max(1.0, abs(want_lp))


@pytest.mark.parametrize("seed", range(12))
def test_tiny_models_against_oracle_and_brute_force(seed):
    rng = np.random.default_rng(seed)
    model = O.random_tiny(rng, finite=seed % 2 == 0, silent_chain=seed % 3 != 0)
    c = O.Compiled(model)
    seqs = [rng.normal(size=n) for n in range(7)]
    check_against_oracle(model, seqs, c)
    for s in seqs:
        lp, path, _, _, _ = O.viterbi_exact(model, s)
        _, _, best_bf, path_bf = O.brute_force(c, s)
        if path_bf is None:
            assert lp == -np.inf and path is None
        else:
            assert abs(lp - best_bf) <= TOL * max(1, abs(best_bf)) and path == path_bf


def test_random_models_against_oracle():
    rng = np.random.default_rng(2025)
    for k in range(60):
        model = O.random_model(rng, max_states=300, max_chain=60, finite=k % 4 != 3)
        check_against_oracle(model, [rng.normal(0, 2, int(rng.integers(0, 12))) for _ in range(2)])


def test_profile_model_against_oracle():
    model, means = O.profile_model(54)
    assert len(model.states) == 165
    check_against_oracle(model, O.profile_events(means, 3, lo=50, hi=400))


def test_one_point_kernel_density_is_the_normal_state_and_more_points_are_refused():
    normal, means = O.profile_model(12, seed=4)
    kde, _ = O.profile_model(12, seed=4, kde=True)
    assert (kde.flat["kind"] == 3).sum() == 12 and np.array_equal(np.diff(kde.flat["kde_ptr"])[kde.flat["kind"][:kde.flat["n_emit"]] == 3], np.ones(12))
    c = P.Compiled(kde)
    for s in O.profile_events(means, 3, lo=10, hi=60, seed=2):
        a, b = O.viterbi_exact(normal, s), O.viterbi_exact(kde, s)
        assert a[1] == b[1]
        assert_close([b[0]], [a[0]])                    # (c + (log 1 - q) against c - q: the same value, other roundings)
        assert_close(b[2], a[2])
        lp, path, margin = O.viterbi(c, s)
        assert_close([b[0]], [lp])
        assert margin <= 1e-9 or b[1] == path
    m = Model("two")
    a = State(GaussianKernelDensity([0.0, 1.0], 1.0), "a")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, a, 0.5)
    m.add_transition(a, m.end, 0.5)
    m.bake()
    with pytest.raises(ValueError, match="one point"):
        O.viterbi_exact(m, [0.5])


def test_impossible_and_empty_sequences():
    from pypore_amd.hmm import UniformDistribution
    u = Model("u")
    a = State(UniformDistribution(0, 1), "a")
    u.add_transition(u.start, a, 1.0)
    u.add_transition(a, a, 0.5)
    u.add_transition(a, u.end, 0.5)
    u.bake()
    lp, path, mat, ties, other = O.viterbi_exact(u, [0.5, 3.0])
    assert lp == -np.inf and path is None and other is None and ties == 0 and mat.shape == (3, 3)
    assert np.isfinite(mat[1, 0]) and np.all(np.isneginf(mat[2]))
    assert O.viterbi_exact(u, [])[:2] == (-np.inf, None)
    lp, path, _, _, _ = O.viterbi_exact(u, [0.0, 1.0])                   # (the support's edges are inside)
    assert lp == 2 * np.log(0.5) and [u.states[k].name for k in path] == ["u-start", "a", "a", "u-end"]
    n = Model("n")
    b = State(NormalDistribution(0, 1), "b")
    n.add_transition(n.start, b, 1.0)
    n.add_transition(b, b, 1.0)
    n.bake()
    assert O.viterbi_exact(n, [])[:2] == (0.0, [n.states.index(n.start)])   # infinite: the empty path ends in start


@pytest.mark.parametrize("name", sorted(VT.TIE_CASES))
def test_tie_models_tie_on_the_winning_path(name):
    """Per sequence: at least the builder's stated number of tied decisions on the winning path (tests/viterbi_ties.py
    derives it from the construction), and for every sequence with a tie the opposite rule's path differs from the rule's
    while both have exactly the same O.path_score.  Every case has a tied sequence."""
    model, seqs, stated, want = VT.tie_case(name)
    c = O.Compiled(model)
    tied = 0
    for s, least, (lp, path, mat, ties, other) in zip(seqs, stated, want):
        if path is None:
            assert least == 0 or name.startswith("diamonds") and len(s) == 0
            continue
        assert ties >= least, (name, len(s), ties, least)
        print("%s: n = %d, %d tied decisions on the winning path (stated: at least %d)" % (name, len(s), ties, least))
        if not least:
            continue
        tied += 1
        assert other != path and len(other) == len(path)
        assert all(a <= b for a, b in zip(path, other))                 # the rule takes the lower state wherever they differ
        a, b = O.path_score(c, s, path), O.path_score(c, s, other)
        assert a is not None and a == b
        assert abs(a - lp) <= 1e-9 * max(1.0, abs(lp))
    assert tied >= 2


def test_launch_plan_restated():
    assert VT.launches([0, 1, 2, 17, 70], 193, 20 * 193) == [(0, 3, 6 * 193), (3, 4, 18 * 193), (4, 5, 71 * 193)]
    assert VT.launches([5, 5], 10, 1) == [(0, 1, 60), (1, 2, 60)]


# ---- the profile-aligner seeds with exact ties ---------------------------------------------------------------------------------
# What tests/test_profile_gpu.py relies on for the seeds it used to leave out.  Figures from this test (python -m pytest -s):
#   P.alignment_case(3):  global, 1 alignment with 1 exact tie, structural; smallest non-zero gap of the seed 4.9e-4
#   P.alignment_case(15): global 1 and local 1 alignment with 1 exact tie each, structural; smallest non-zero gap 1.7e-3
#   multiple-alignment seed 0: no exact tie, but a non-zero gap of 1.4e-16 (M11 entered from I10 or D10: the same sum in
#       two orders of addition) -- rounding, not structure; a device may take either side
#   multiple-alignment seed 3: 1 exact tie, structural, and a non-zero gap of 2.8e-16 of the same kind
ALIGN_TIE_SEEDS = {3: 1, 15: 2}                  # seed -> alignments (of its 2 modes x 4 slaves) that meet an exact tie
MSA_TIE_SEEDS = {0: (0, False), 3: (1, False)}   # seed -> (exact ties met, every non-zero gap > 1e-9)


@pytest.mark.parametrize("seed", sorted(ALIGN_TIE_SEEDS))
def test_profile_alignment_ties_are_structural(seed):
    msa, slaves = P.alignment_case(seed)
    met = 0
    for mode in ("global", "local"):
        for q, s in enumerate(slaves):
            prob, _, _, gap, ties, structural = P.align_ties(copy.deepcopy(msa), list(s), mode)
            assert np.isfinite(prob) and gap > 1e-9
            if ties:
                met += 1
                print("alignment_case(%d) %s slave %d: %d exact tie(s), structural: %s, smallest non-zero gap %.3g"
                      % (seed, mode, q, ties, structural, gap))
                assert structural
                assert P.align(copy.deepcopy(msa), list(s), mode)[3] == 0.0     # (the scalar margin still reads it as a tie)
    assert met == ALIGN_TIE_SEEDS[seed]


@pytest.mark.parametrize("seed", sorted(MSA_TIE_SEEDS))
def test_multiple_alignment_seeds_verdicts(seed):
    rng = np.random.default_rng(700 + seed)
    _, seqs = P.derived_sequences(rng, int(rng.integers(6, 16)), int(rng.integers(3, 7)))
    _, _, gap, ties, structural = P.msa_iterative_ties(copy.deepcopy(seqs), max_iterations=3)
    print("multiple-alignment seed %d: %d exact tie(s), structural: %s, smallest non-zero gap %.3g" % (seed, ties, structural, gap))
    assert structural
    assert (ties, gap > 1e-9) == MSA_TIE_SEEDS[seed]
    assert P.msa_iterative(copy.deepcopy(seqs), max_iterations=3)[2] == (0.0 if ties else gap)
    # the other side of the near tie: another complete alignment of the same sequences (tests/test_profile_gpu.py accepts either)
    score, msa, _, _, _ = P.msa_iterative_ties(copy.deepcopy(seqs), max_iterations=3)
    score2, msa2, gap2, _, _ = P.msa_iterative_ties(copy.deepcopy(seqs), max_iterations=3, flip_near=True)
    assert gap2 <= 1e-9 and len({len(r) for r in msa2}) == 1
    assert sorted([x for x in r if x != '-'] for r in msa2) == sorted(seqs)
    assert (msa2 == msa) == (seed == 0) and abs(score2 - score) <= 1e-12 * max(1.0, abs(score))
