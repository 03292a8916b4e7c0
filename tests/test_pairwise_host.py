"""CPU tests of the pairwise aligner: the restatement (tests/pairwise_oracle.py) against the recorded reference
(tests/golden/golden_pairwise.npz, make_golden_pairwise.py), and the class surface and argument errors of
PairwiseAligner, pairwise_align_batch and pairwise_scores -- everything that is decided before a GPU is touched."""
import json
import os

import numpy as np
import pytest

import pairwise_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = json.load(open(os.path.join(HERE, "golden", "manifest_pairwise.json")))["cases"]
MODES = {"global": O.GLOBAL, "local": O.LOCAL, "repeated": O.REPEATED}


def golden():
    return np.load(os.path.join(HERE, "golden", "golden_pairwise.npz"))


def golden_case(G, case):
    """(x, y, [(score, xalign values, yalign values)]) of a manifest entry."""
    name = case["name"]
    x, y = G[name + "/x"], G[name + "/y"]
    ends = np.cumsum(G[name + "/len"])
    als = []
    for k, e in enumerate(ends):
        b = e - G[name + "/len"][k]
        als.append((G[name + "/scores"][k], G[name + "/xalign"][b:e], G[name + "/yalign"][b:e]))
    return x, y, als


def as_values(x, y, alignments):
    """Walk-order index columns -> forward value sequences, NaN for '-' (the golden's form)."""
    out = []
    for s, ci, cj in alignments:
        xa = np.array([x[i] if i >= 0 else np.nan for i in list(ci)[::-1]], dtype=np.float64)
        ya = np.array([y[j] if j >= 0 else np.nan for j in list(cj)[::-1]], dtype=np.float64)
        out.append((s, xa, ya))
    return out


def check_against_golden(case, x, y, status, alignments, als_ref):
    """The three rules: structure exact everywhere; scores exact on grid cases, within the derived bound off the grid."""
    assert ("IndexError" if status else "") == case["raises"], case["name"]
    got = as_values(x, y, alignments)
    assert len(got) == len(als_ref) == case["alignments"], case["name"]
    for (s, xa, ya), (rs, rxa, rya) in zip(got, als_ref):
        assert np.array_equal(xa, rxa, equal_nan=True) and np.array_equal(ya, rya, equal_nan=True), case["name"]
        if case["grid"]:
            assert s == rs, case["name"]
        else:
            assert abs(s - rs) <= case["score_bound"], (case["name"], s, rs, case["score_bound"])


def test_manifest_covers_what_the_goldens_promise():
    names = {c["name"] for c in MANIFEST}
    by = lambda **kw: [c for c in MANIFEST if all(c[k] == v for k, v in kw.items())]
    for grid in (True, False):
        for mode in MODES:
            assert by(grid=grid, mode=mode)
    sizes = {(c["m"], c["n"]) for c in MANIFEST}
    for s in ((1, 1), (1, 17), (17, 1), (63, 64), (64, 63), (65, 64), (64, 65), (129, 65), (65, 129), (129, 129)):
        assert s in sizes
    assert {c["penalty"] for c in MANIFEST} >= {-1, -0.5, -3, 0}
    assert {c["min_length"] for c in by(mode="repeated")} >= {1, 2, 5}
    assert any(c["raises"] == "IndexError" and c["m"] != c["n"] for c in by(mode="local"))
    assert by(name="grid_local_no_positive")[0]["raises"] == "IndexError"
    assert any(c["raises"] == "IndexError" and c["alignments"] > 0 for c in by(mode="repeated"))
    assert by(name="empty_x_local")[0]["raises"] == "IndexError" and by(name="empty_x_repeated")[0]["alignments"] == 0
    assert "marker_repeated" in names and "grid_local_self_40" in names
    for c in by(grid=False):
        assert c["score_diff_observed"] <= c["score_bound"]


@pytest.mark.parametrize("case", MANIFEST, ids=[c["name"] for c in MANIFEST])
def test_restatement_equals_recorded_reference(case):
    x, y, als_ref = golden_case(golden(), case)
    status, _, alignments = O.align(x, y, MODES[case["mode"]], float(case["penalty"]), case["min_length"])
    check_against_golden(case, x, y, status, alignments, als_ref)


def test_empty_global_scores_are_the_border():
    G = golden()
    for name, want in (("empty_x_global", 5 * -1.0), ("empty_y_global", 5 * -3.0), ("empty_both_global", 0.0)):
        assert G[name + "/scores"][0] == want and G[name + "/len"][0] == 0


@pytest.mark.parametrize("local", [False, True])
def test_anti_diagonal_fill_equals_the_nested_loops(local):
    rng = np.random.default_rng(5)
    for m, n, pen in ((1, 1, -1), (7, 13, -0.5), (30, 21, 0), (40, 40, -3)):
        x, y = rng.uniform(20, 24, m), rng.uniform(20, 24, n)
        x[rng.integers(m)] = np.nan
        a, b = O.fill(x, y, pen, local), O.fill_loops(x, y, pen, local)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the Python surface: these fail with ImportError before the feature --------------------------------------------------------

def test_class_surface_and_dotplot():
    from pypore_amd.alignment import PairwiseAligner, pairwise_align_batch, pairwise_scores
    a = PairwiseAligner([1.0, 2.0, '-'], [1.0, 2.5])
    assert (a.m, a.n) == (3, 2) and a.x[2] == '-'
    for name in ("dotplot", "global_alignment", "local_alignment", "local_repeated_alignment", "_score"):
        assert callable(getattr(a, name))
    d = a.dotplot()
    assert d.shape == (4, 3) and d[1, 1] == 3.0 and d[2, 2] == 2.75 and d[3, 1] == 0.0 and not d[0].any() and not d[:, 0].any()
    assert np.array_equal(d[1:, 1:], O.match([1.0, 2.0, np.nan], [1.0, 2.5]))
    assert callable(pairwise_align_batch) and callable(pairwise_scores)
    import inspect
    assert list(inspect.signature(pairwise_align_batch).parameters) == ["pairs", "mode", "penalty", "min_length", "device"]
    assert list(inspect.signature(pairwise_scores).parameters) == ["seqs", "others", "mode", "penalty", "device"]
    assert inspect.isgeneratorfunction(PairwiseAligner.local_repeated_alignment)
    assert "no CPU fallback" in PairwiseAligner.__doc__


def test_overridden_score_is_refused():
    from pypore_amd.alignment import PairwiseAligner

    class Mine(PairwiseAligner):
        def _score(self, x, y):
            return 1.0

    a = Mine([1.0], [1.0])
    with pytest.raises(NotImplementedError):
        a.global_alignment()
    with pytest.raises(NotImplementedError):
        a.local_alignment()
    with pytest.raises(NotImplementedError):
        next(a.local_repeated_alignment())


@pytest.mark.parametrize("bad", [[1.0, float("nan")], [float("inf")], ["x"], [None], ["--"]])
def test_elements_must_be_finite_floats_or_the_marker(bad):
    from pypore_amd.alignment import PairwiseAligner, pairwise_align_batch, pairwise_scores
    with pytest.raises(ValueError):
        PairwiseAligner(bad, [1.0]).global_alignment()
    with pytest.raises(ValueError):
        PairwiseAligner([1.0], bad).local_alignment()
    with pytest.raises(ValueError):
        pairwise_align_batch([([1.0], [2.0]), (bad, [1.0])])
    with pytest.raises(ValueError):
        pairwise_scores([[1.0], bad])
    with pytest.raises(ValueError):
        pairwise_scores([[1.0]], others=[bad])


def test_mode_and_penalty_errors():
    from pypore_amd.alignment import pairwise_align_batch, pairwise_scores
    with pytest.raises(ValueError):
        pairwise_align_batch([([1.0], [1.0])], mode="semi")
    with pytest.raises(ValueError):
        pairwise_scores([[1.0]], mode="local_repeated")
    with pytest.raises(ValueError):
        pairwise_scores([[1.0]], mode=None)
    with pytest.raises(ValueError):
        pairwise_align_batch([([1.0], [1.0])], penalty=float("nan"))
    with pytest.raises(ValueError):
        pairwise_scores([[1.0]], penalty=float("-inf"))


def test_status_codes_match_header():
    import re
    from pypore_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "poreseg.h")).read()
    for name in ("PS_PW_GLOBAL", "PS_PW_LOCAL", "PS_PW_LOCAL_REPEATED", "PS_PW_OK", "PS_PW_INDEX_ERROR"):
        assert int(re.search(r"#define %s\s+(-?\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    assert (O.GLOBAL, O.LOCAL, O.REPEATED, O.OK, O.INDEX_ERROR) == (0, 1, 2, 0, 1)
