"""Viterbi on the MI355X (csrc/seg_hmm.hpp hmm_fwd_kernel<HMM_VITERBI>, hmm_trace_kernel; csrc/poreseg.hip hmm_viterbi) bit
for bit against hmm_oracle.viterbi_exact, the kernel's operations restated in plain Python floats on the uploaded numbers.
For normal, uniform and one-point kernel-density states the kernel performs only IEEE fp64 additions, subtractions,
multiplications and comparisons (no contraction, no libm call), so every check here is an equality: the log probability
with ==, the path position by position, the score matrix entry by entry (and by its bits), -inf where the oracle has it.
No tolerance and no margin anywhere: at an exact tie the rule decides -- in-edges in ascending source index, a strictly
greater score replaces the best, the lowest source wins; an infinite model ends in the lowest best state of the last row.

Every tie test first asserts on the oracle (tests/viterbi_ties.py, proved on the CPU in tests/test_viterbi_exact_host.py)
that the ties lie on the winning path and that the opposite rule gives another path, so a pass means the device applied
the rule: a kernel that took >= for >, scanned a lane's strided states in the wrong order, preferred the higher lane in
the butterfly or cut a tied backpointer to 8 bits returns a path that differs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import launch_geometry as LG  # noqa: E402
import viterbi_ties as VT  # noqa: E402

pytestmark = pytest.mark.gpu


def run_device(model, seqs):
    """(viterbi_batch's results, and from ctx.hmm_batch(..., want_mat=True): logp, the matrix rows per sequence, the paths)"""
    from pypore_amd import _lib
    vit = model.viterbi_batch(seqs)
    ctx, off, obs = model._upload(seqs, None)
    logp, mat, (path, path_off, path_len) = ctx.hmm_batch(model._c_model(), _lib.PS_HMM_VITERBI, obs, off, want_mat=True)
    logp, mat, path, path_len = logp.cpu().numpy(), mat.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()
    rows = [mat[off[q] + q:off[q + 1] + q + 1] for q in range(len(seqs))]
    paths = [path[path_off[q]:path_off[q] + path_len[q]].tolist() for q in range(len(seqs))]
    return vit, logp, rows, paths


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_exact(model, seqs, want=None):
    """Both device routes against viterbi_exact, sequence by sequence; returns what the device gave."""
    want = [O.viterbi_exact(model, s) for s in seqs] if want is None else want
    got = run_device(model, seqs)
    vit, logp, rows, paths = got
    assert len(vit) == len(logp) == len(seqs)
    for q, (lp, path, mat, _, _) in enumerate(want):
        glp, gpath = vit[q]
        if path is None:
            assert lp == -np.inf and glp == -np.inf and gpath is None, q
            assert logp[q] == -np.inf and paths[q] == [], q
        else:
            assert glp == lp and logp[q] == lp, (q, glp, logp[q], lp)
            assert all(model.states[i] is s for i, s in gpath)
            assert [i for i, _ in gpath] == path, q
            assert paths[q] == path, q
        assert rows[q].shape == mat.shape, q
        assert np.array_equal(np.isneginf(rows[q]), np.isneginf(mat)), q
        assert np.array_equal(rows[q], mat) and same_bits(rows[q], mat), q
    return got


def check_ties(name):
    """The vacuity guard, then the device."""
    model, seqs, stated, want = VT.tie_case(name)
    tied = 0
    for least, (lp, path, _, ties, other) in zip(stated, want):
        if path is not None and least:
            assert ties >= least and other != path
            tied += 1
    assert tied >= 2
    check_exact(model, seqs, want)
    return model, seqs, want


# ---- exact ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder8_adjacent", "ladder64_strided"])
def test_twin_ladder(name):
    """Twins with identical bits in every row, at adjacent indices (adjacent lanes; L = 8) and 64 apart (one lane, two
    strides; L = 64), lengths 0, 1, 2, 17, 70: one tie per visited level, and the path takes the lower twin everywhere."""
    model, seqs, want = check_ties(name)
    for lp, path, _, _, other in want:
        names = [model.states[k].name for k in path]
        assert not any(nm[0] == "b" or nm[-1] == "b" for nm in names if not nm.startswith(("hub", "ladder")))
        assert all(a <= b for a, b in zip(path, other))


@pytest.mark.parametrize("name", ["diamonds7", "diamonds40"])
def test_silent_diamonds(name):
    """7 and 40 diamonds of silent states between the emitting ones: every join ties between its two sources, inside the
    silent phase on row `cur` (7 to 360 ties per sequence); the lower source wins.  The empty sequence is impossible."""
    model, seqs, want = check_ties(name)
    assert want[0][1] is None and len(seqs[0]) == 0
    for lp, path, _, _, _ in want[1:]:
        assert not any(model.states[k].name[0] == "v" for k in path)


@pytest.mark.parametrize("name", ["ladder8_adjacent_infinite", "ladder64_strided_infinite", "all_tied_130_infinite"])
def test_infinite_models_end_in_the_lowest_best_state(name):
    """No `end`: the last row ties between twins on adjacent lanes (L = 8), between two strides of one lane (L = 64), and
    across all 130 states of a model whose states are identical (every lane and three strides tie; state 0 must win)."""
    model, seqs, want = check_ties(name)
    assert not model.finite
    for s, (lp, path, mat, _, other) in zip(seqs, want):
        if len(s):
            best = np.flatnonzero(mat[-1] == lp)
            assert best.size >= 2 and path[-1] == best[0] and other[-1] == best[-1]
            if name.startswith("all_tied"):
                assert best.size == 130 and path[1:] == [0] * len(s) and other[1:] == [129] * len(s)


@pytest.mark.parametrize("name", ["hub600_3_300", "hub600_256_300", "hub255_3_253", "hub257_3_254"])
def test_tied_backpointers_on_both_sides_of_the_width(name):
    """Two in-edges of the hub state h tie (their source states share one distribution): ordinals (3, 300) and (256, 300)
    at in-degree 600 and (3, 254) at 257 on the 16-bit backpointers, (3, 253) at 255 on the 8-bit ones (ordinal 254 is h's
    own loop there, which no other state can tie).  The lower ordinal wins; with (256, 300) a backpointer cut to 8 bits
    among the tied candidates names e0000."""
    model, seqs, want = check_ties(name)
    lo, hi = [int(v) for v in name.split("_")[1:]]
    h = [k for k, s in enumerate(model.states) if s.name == "h"][0]
    for lp, path, _, _, other in want:
        into = [a for a, b in zip(path[:-1], path[1:]) if b == h and a != h]
        into_other = [a for a, b in zip(other[:-1], other[1:]) if b == h and a != h]
        assert model.states[into[0]].name == "e%04d" % lo and model.states[into_other[0]].name == "e%04d" % hi


# ---- launches cut by the backpointer budget -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder64_strided", "hub600_256_300"])
def test_launch_cuts_keep_every_bit(name):
    """hmm_bp_budget cuts the batch into at least 3 launches, one sequence alone exceeding the budget: logp, paths and the
    matrix rows -- those of the later launches too, which hmm_viterbi addresses with mat_row0 = 0 in every launch -- have
    the bits of the uncut call and of the oracle."""
    from pypore_amd import engine
    model, seqs, stated, want = VT.tie_case(name)
    seqs, want = list(seqs), list(want)
    if name.startswith("hub"):                          # a long sequence between the short ones: e, h, e, h, ...
        rng = np.random.default_rng(6)
        alt = np.stack([3.0 * rng.integers(599, size=20), np.full(20, -50.0)], axis=1).ravel() + rng.normal(0, 0.1, 40)
        seqs = [seqs[0], seqs[1], alt, seqs[1], seqs[0]]
        want = [want[0], want[1], O.viterbi_exact(model, alt), want[1], want[0]]
    S = len(model.states)
    row_bytes = S * (2 if name.startswith("hub") else 1)
    budget = 20 * row_bytes
    plan = VT.launches([len(s) for s in seqs], row_bytes, budget)
    assert len(plan) >= 3 and any(size > budget for _, _, size in plan), plan
    whole = check_exact(model, seqs, want)
    with LG.options(engine.context(), hmm_bp_budget=budget):
        cut = check_exact(model, seqs, want)
    for q in range(len(seqs)):
        assert whole[0][q][0] == cut[0][q][0] and whole[1][q] == cut[1][q]
        assert same_bits(whole[2][q], cut[2][q]) and whole[3][q] == cut[3][q]


# ---- no ties, bit for bit ------------------------------------------------------------------------------------------------------
def test_random_models_bit_exact():
    """Normal and uniform states, silent chains of up to 60 levels, every fourth model infinite, lengths 0..11."""
    rng = np.random.default_rng(4096)
    for k in range(40):
        model = O.random_model(rng, max_states=300, max_chain=60, finite=k % 4 != 3)
        check_exact(model, [rng.normal(0, 2, n) for n in (int(rng.integers(0, 12)), int(rng.integers(0, 12)))])


@pytest.mark.parametrize("kde", [False, True])
def test_profile_bit_exact(kde):
    """The 165-state profile over 12 events of 50..400 observations, with normal match states and with one-point
    kernel-density match states (the HmmDevK instantiation, whose one-term log-sum-exp returns its term)."""
    model, means = O.profile_model(54, kde=kde)
    assert len(model.states) == 165 and int((model.flat["kind"] == 3).sum()) == (54 if kde else 0)
    check_exact(model, O.profile_events(means, 12, lo=50, hi=400))


def test_state_cap_bit_exact():
    model = O.line_model(4096)
    assert len(model.states) == 4096
    rng = np.random.default_rng(3)
    check_exact(model, [rng.normal(0, 3, n) for n in (0, 1, 3, 6)])


def test_paths_longer_than_their_slots_bit_exact():
    """Paths through a loop of 20 silent states overflow the default slots: the capacity retry returns the same bits."""
    model = O.chain_model(20)
    S, NE = len(model.states), sum(1 for s in model.states if not s.is_silent())
    rng = np.random.default_rng(8)
    seqs = [rng.normal(0, 0.5, n) for n in (50, 1, 2, 48, 0, 1, 55, 2)] + [np.array([2.0, 2.1, 1.9, 0.0])]
    vit, _, _, paths = check_exact(model, seqs)
    assert any(len(p) > 5 * (2 * (len(s) + 1) + (S - NE) + 1) for p, s in zip(paths, seqs))
