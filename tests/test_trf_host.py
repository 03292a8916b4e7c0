"""NaiveTRF without a GPU: the restatement of the reference's splitter (tests/trf_oracle.py) against the goldens recorded
from the reference (tests/golden/make_golden_trf.py) bit for bit on every case, its two forms against each other, the
invariants the device kernel relies on asserted on every case, the stitching against the recorded rows,
and the argument checks of the public functions, which raise before any library call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trf_cases as C  # noqa: E402
import trf_oracle as O  # noqa: E402

CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
golden, golden_yields, golden_rows, restated, same_bits = C.golden, C.golden_yields, C.golden_rows, C.restated, C.same_bits


def test_cases_are_the_recorded_ones():
    g, m = golden()
    assert sorted(m) == sorted(IDS) and len(set(IDS)) == len(IDS)
    for c in CASES:
        assert np.array_equal(g[c["name"] + "/means"].view(np.int64), c["means"].view(np.int64)), c["name"]
        assert np.array_equal(g[c["name"] + "/stds"].view(np.int64), c["stds"].view(np.int64)), c["name"]
        assert (m[c["name"]]["penalty"], m[c["name"]]["min_score"]) == (c["penalty"], c["min_score"])


def test_cases_cover_what_they_must():
    _, m = golden()
    for cases in (C.grid_cases(), C.offgrid_cases()):
        assert {len(c["means"]) for c in cases} >= set(C.SEAM_SIZES)
        assert {c["penalty"] for c in cases} >= {-0.5, -1.0, -2.0}
        assert any(c["min_score"] == 0.0 for c in cases)
        assert any(m[c["name"]]["row0_end"] for c in cases)
        assert all(len(c["means"]) <= 129 for c in cases) and sum(len(c["means"]) > 70 for c in cases) <= 4
    for c in C.grid_cases():                                    # the grid: every operation of a cell is exact
        assert np.array_equal(c["means"] * 32.0, np.round(c["means"] * 32.0)) and set(c["stds"]) <= {0.5, 1.0, 2.0}
    assert max(v["yields"] for v in m.values()) >= 64           # more yields than a wave has lanes


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    want = golden_yields(case["name"])
    (full, _), (upper, _) = restated(case)
    assert same_bits(full, want)
    assert same_bits(upper, want)                               # the two forms agree: no diagonal, no lower triangle, no -999


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invariants(case):
    (full, info), (upper, uinfo) = restated(case)
    n = len(case["means"])
    assert not info["masked_won"]                               # a masked candidate never wins: masked == excluded
    assert not info["diag_argmax"]                              # a diagonal cell is never the arg-max
    assert not info["left_upper"]                               # walks stay in the strict upper triangle, end cell included
    assert info["walked"] == uinfo["walked"]
    assert all(k >= 1 for k in info["new_cells"])               # progress: every repeat masks a cell that was not masked
    assert len(full) <= (n + 1) ** 2
    for (s, length, i, j), cells in zip(full, info["walked"]):
        assert s > case["min_score"] and length == len(cells) >= 1 and 0 <= i < j <= n
        assert all(1 <= a < b <= n for a, b in cells)
    assert info["stop_score"] <= case["min_score"]


def test_best_equal_to_min_score_stops():
    case = [c for c in CASES if c["name"] == "grid_stop_at_min_score"][0]
    (full, info), _ = restated(case)
    assert info["stop_score"] == case["min_score"] == 4.0 and [y[0] for y in full] == [6.0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stitching(case):
    assert O.stitch(len(case["means"]), golden_yields(case["name"])) == golden_rows(case["name"])


def test_libm_square_finding():
    """The unmodified reference on np.float64 means squares by libm's pow, which is not correctly rounded for every
    operand: the recorder keeps that run where it differs.  Here: the same repeats and rows, scores within one ulp of the
    square per cell of the path (|d^2 / (std std)| <= B per cell, max is 1-Lipschitz)."""
    _, m = golden()
    differing = [v for v in m.values() if v["libm_scores_differing"] != []]
    assert all(v["libm_same_structure"] for v in m.values())
    assert all(not v["grid"] for v in differing)                # on the grid the square is exact whoever takes it
    for v in differing:
        a, b = golden_yields(v["name"]), golden_yields(v["name"], "_libm")
        assert [y[1:] for y in a] == [y[1:] for y in b]
        assert [k for k, (x, y) in enumerate(zip(a, b)) if x[0] != y[0]] == v["libm_scores_differing"]
        for x, y in zip(a, b):
            assert abs(x[0] - y[0]) <= x[1] * 2.0 ** -52 * max(abs(x[0]), 2.0 * x[1])


class _Seg(object):
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


def test_public_names_and_argument_checks(monkeypatch):
    from pypore_amd import alignment, engine
    from pypore_amd.alignment import NaiveTRF, naive_splits_batch, naive_splits_batch_raw, naive_trf_batch  # noqa: F401

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(engine, "context", no_library)
    seq = [_Seg(20.0 + k, 1.0) for k in range(5)]
    with pytest.raises(ValueError, match="min_score"):
        NaiveTRF(seq, min_score=-0.5)
    with pytest.raises(ValueError, match="penalty"):
        NaiveTRF(seq, penalty=0)
    with pytest.raises(ValueError, match="penalty"):
        naive_splits_batch([seq], penalty=0.5)
    with pytest.raises(ValueError, match="mean"):
        NaiveTRF(seq + [_Seg(float("nan"), 1.0)])
    with pytest.raises(ValueError, match="mean"):
        NaiveTRF(seq + [_Seg(float("inf"), 1.0)])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="std"):
            NaiveTRF(seq + [_Seg(21.0, bad)])
        with pytest.raises(ValueError, match="std"):
            naive_splits_batch([(np.array([20.0, 21.0]), np.array([1.0, bad]))])
    with pytest.raises(ValueError, match="2048"):
        naive_splits_batch([(np.zeros(2049), np.ones(2049))])
    with pytest.raises(AssertionError, match="the library was called"):     # valid arguments do reach the library
        NaiveTRF(seq)
    assert alignment._trf_stitch(list("abcdef"), [(4.0, 2, 1, 3)]) == [['a', 'b', 'c', '-'], ['-', 'd', 'e', 'f']]
