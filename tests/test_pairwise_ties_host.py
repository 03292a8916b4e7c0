"""CPU tests behind test_pairwise_ties_gpu.py: the restatement (tests/pairwise_oracle.py) against its own literal form
and against the recorded reference on tie-heavy inputs (tests/golden/golden_pairwise_ties.npz,
make_golden_pairwise_ties.py), and the conditions that make the inputs of tests/pairwise_ties.py worth running -- that
candidates really tie, that the maximum really is held in several stripes and lane groups, that the marker cases really
trim.  They are asserted here, on the restatement, so that the GPU tests cannot quietly stop exercising the rules."""
import json
import os

import numpy as np
import pytest

import pairwise_oracle as O
import pairwise_ties as T
import test_pairwise_host as H

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest_pairwise_ties.json")))["cases"]


def golden():
    return np.load(os.path.join(HERE, "golden", "golden_pairwise_ties.npz"))


def tie_heavy_pairs():
    """Pairs of every generator at lengths up to 70: for the fill against its literal form."""
    rng = np.random.default_rng(11)
    pairs = []
    for k in (2, 4):
        for m, n in ((1, 1), (1, 9), (2, 2), (33, 70), (70, 33), (64, 65), (70, 70)):
            pairs.append((T.letters(rng, m, k), T.letters(rng, n, k)))
        x = T.letters(rng, 40, k)
        pairs.append((x, x.copy()))
    pairs += [T.periodic(70), T.periodic_transposed(70), T.periodic_square(66)]
    pairs += [T.marker_all_seams(rng, 70, 70, run) for run in (1, 3)] + T.marker_pairs(rng, 66, 40)[::5]
    pairs += [(x, y) for _, x, y, _, _, _ in T.trim_cases()]
    return pairs


@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
def test_anti_diagonal_fill_equals_the_nested_loops_on_ties(local):
    for x, y in tie_heavy_pairs():
        for penalty in T.PENALTIES:
            a, b = O.fill(x, y, penalty, local), O.fill_loops(x, y, penalty, local)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (len(x), len(y), penalty)


def test_integer_alphabets_tie_in_a_tenth_of_the_cells():
    """Four letters at 130 x 130, penalty -1: the diagonal candidate ties a gap candidate and wins in at least 10 % of
    the cells (measured: 22-25 %; values drawn from uniform(20, 26) tie in 0.3-0.4 %)."""
    rng = np.random.default_rng(12)
    for _ in range(3):
        x, y = T.letters(rng, 130, 4), T.letters(rng, 130, 4)
        for local in (False, True):
            assert T.diagonal_tie_share(x, y, -1, local) >= 0.10
    x, y = T.letters(rng, 130, 2), T.letters(rng, 130, 2)
    assert T.diagonal_tie_share(x, y, -1, False) >= 0.10 and T.diagonal_tie_share(x, y, -1, True) >= 0.10


@pytest.mark.parametrize("m", [200, 448])
def test_periodic_pair_holds_its_maximum_in_several_stripes(m):
    x, y = T.periodic(m)
    best, rows, _ = T.maximum_cells(x, y)
    assert best == 21.0 and len(set((rows - 1) // T.STRIPE)) >= 2
    assert O.score_only(x, y, O.LOCAL, -1.0) == (21.0, (7, 7))
    status, first, als = O.align(x, y, O.REPEATED, -1.0, 2)        # the first alignment from (7, 7), then row 14 > n
    assert status == O.INDEX_ERROR and first == 21.0 and len(als) == 1 and als[0][1][0] == 6 and als[0][2][0] == 6


def test_transposed_periodic_pair_holds_its_maximum_in_several_lane_groups():
    x, y = T.periodic_transposed(200)
    best, rows, cols = T.maximum_cells(x, y)
    assert best == 21.0
    held = {r: cols[rows == r] for r in set(rows)}
    assert any(len(set((c - 1) // T.STRIPE)) >= 2 for c in held.values())
    assert O.score_only(x, y, O.LOCAL, -1.0) == (21.0, (7, 7))


def test_square_periodic_pair_ties_two_rows_after_the_first_walk():
    """The repeated mode's second arg-max is tied between two rows (and the walk's mirror clears the other)."""
    x, y = T.periodic_square(130)
    score, pointer = O.fill(x, y, -1.0, True)
    i, j = np.unravel_index(np.argmax(score), score.shape)
    assert not O._walk(score, pointer, x, y, i, j)[0]
    rows = np.nonzero((score == score.max()).any(axis=1))[0]
    assert rows.size >= 2


def test_marker_cases_trim_as_they_are_meant_to():
    seen = {name: (mode, penalty, T.walks(x, y, penalty, mode == O.REPEATED, ml), O.align(x, y, mode, penalty, ml))
            for name, x, y, mode, penalty, ml in T.trim_cases()}
    for name, (mode, penalty, (status, w), got) in seen.items():
        assert status == got[0], name                              # the walk-by-walk account is the restatement's
    partial = lambda w: any(not e and 0 < clean < L for e, L, clean in w)
    nothing = lambda w: not w[-1][0] and w[-1][2] == 0
    assert partial(seen["positive_partial_trim"][2][1]) and seen["positive_partial_trim"][3][0] == O.OK
    for name in ("repeated_trimmed_to_nothing", "positive_trimmed_to_nothing", "positive_markers_trimmed_to_nothing",
                 "positive_repeated_yields_then_nothing"):
        assert nothing(seen[name][2][1]) and seen[name][3][0] == O.INDEX_ERROR, name
    assert len(seen["positive_repeated_yields_then_nothing"][3][2]) == 1
    for name in ("positive_trimmed_to_nothing", "positive_markers_trimmed_to_nothing"):
        assert seen[name][0] == O.LOCAL and seen[name][1] > 0
    # the seam pairs in the repeated mode: every one of them trims some alignment's start, none to nothing
    for x, y in T.marker_pairs(np.random.default_rng(3), 130, 130)[::4]:
        status, w = T.walks(x, y, -1, True, 2)
        assert status == O.OK and partial(w)


def test_ties_manifest_covers_what_the_issue_asks():
    by = lambda **kw: [c for c in MANIFEST if all(c[k] == v for k, v in kw.items())]
    assert 18 <= len(MANIFEST) <= 24 and all(c["grid"] and max(c["m"], c["n"]) <= 200 for c in MANIFEST)
    for mode in H.MODES:
        assert {(c["m"], c["n"]) for c in by(mode=mode)} >= {(63, 64), (65, 64), (129, 129), (130, 130)}
        assert by(name="marker_seams_%s" % mode)
    assert {c["penalty"] for c in MANIFEST} >= {-1, -0.5, 0}
    for name in ("periodic_local", "periodic_repeated", "periodic_transposed_local", "periodic_transposed_repeated"):
        assert by(name=name)
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_pairwise_ties.npz")) \
        < os.path.getsize(os.path.join(HERE, "golden", "golden_pairwise.npz")) // 2
    G = golden()
    for c in MANIFEST:
        x, y = G[c["name"] + "/x"], G[c["name"] + "/y"]
        keep = ~np.isnan(x)
        assert np.array_equal(x[keep], np.round(x[keep])) and np.array_equal(y[~np.isnan(y)], np.round(y[~np.isnan(y)]))


@pytest.mark.parametrize("case", MANIFEST, ids=[c["name"] for c in MANIFEST])
def test_restatement_equals_recorded_reference_on_ties(case):
    x, y, als_ref = H.golden_case(golden(), case)
    status, _, alignments = O.align(x, y, H.MODES[case["mode"]], float(case["penalty"]), case["min_length"])
    H.check_against_golden(case, x, y, status, alignments, als_ref)
