"""StatSplit without a GPU: the constructor's rules, the JSON round trip, start / end normalisation, and the host
restatement of its arithmetic (tests/statsplit_oracle.py) against the goldens recorded from the reference
(tests/golden/make_golden_statsplit.py) on every case -- use_log=True included: both run numpy's logarithm."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import statsplit_cases as SC  # noqa: E402
import statsplit_oracle  # noqa: E402
from pypore_amd.parsers import StatSplit, parser  # noqa: E402


def test_constructor_defaults_and_rules():
    p = StatSplit()
    assert (p.min_width, p.max_width, p.min_gain_per_sample, p.window_width, p.use_log, p.splitter) == \
        (1000, 1000000, 0.03, 10000, True, "stepwise")
    assert StatSplit(min_width=0, window_width=10).min_width == 1            # max(min_width, 1)
    assert StatSplit(min_width=-3, window_width=10).min_width == 1
    q = StatSplit(min_width=7, max_width=0, window_width=0)                   # "or" defaults from the min_width given
    assert (q.max_width, q.window_width) == (700, 70)
    q = StatSplit(min_width=7, max_width=None, window_width=None)
    assert (q.max_width, q.window_width) == (700, 70)
    with pytest.raises(AssertionError):
        StatSplit(min_width=100, max_width=99)
    with pytest.raises(AssertionError):
        StatSplit(min_width=100, window_width=199)
    StatSplit(min_width=100, max_width=100, window_width=200)                 # both bounds are inclusive
    with pytest.raises(AssertionError):
        StatSplit(min_width=0, max_width=0, window_width=10)                  # 100 * 0 < max(0, 1)


def test_json_round_trip():
    p = StatSplit(min_width=30, max_width=4000, min_gain_per_sample=0.25, window_width=300, use_log=False, splitter="slanted")
    d = p.to_dict()
    assert d == dict(name="StatSplit", min_width=30, max_width=4000, min_gain_per_sample=0.25, window_width=300, use_log=False,
                     splitter="slanted")
    assert json.loads(p.to_json()) == d
    q = parser.from_json(p.to_json())
    assert type(q) is StatSplit and q.to_dict() == d
    assert StatSplit.from_json(StatSplit().to_json()).to_dict() == StatSplit().to_dict()


def test_importable_where_the_reference_exports_it():
    from pypore_amd import DataTypes
    assert DataTypes.StatSplit is StatSplit


@pytest.mark.parametrize("n,start,end,want", [
    (100, 0, -1, (0, 100)), (100, 10, 90, (10, 90)), (100, -1, -1, (100, 100)), (100, -101, -2, (0, 99)),
    (100, 5, 1000, (5, 100)), (100, 500, 1000, (100, 100)), (100, -51, -11, (50, 90)), (0, 0, -1, (0, 0)),
])
def test_start_end_normalisation(n, start, end, want):
    assert StatSplit._normalise(n, start, end) == want


def test_callable_splitter_is_refused():
    with pytest.raises(NotImplementedError):
        StatSplit(splitter=lambda a, b: None)._params()


def test_threshold_is_formed_as_python_forms_it():
    p = StatSplit(min_width=10, window_width=173, min_gain_per_sample=0.04)
    assert p._params().threshold == 0.04 * 173
    assert (p._params().use_log, p._params().splitter) == (1, 0)
    assert StatSplit(use_log=False, splitter="slanted")._params().splitter == 1


def test_cases_cover_what_they_claim():
    names = [c["name"] for c in SC.CASES]
    assert len(set(names)) == len(names)
    assert max(c["gen"]["n"] for c in SC.CASES) <= 4000
    npz, margins = SC.golden()
    assert sorted(npz.files) == sorted(SC.run_ids(SC.CASES_ALL)) == sorted(margins)
    logs = [k for c, s, lg in SC.runs() if lg for k in [SC.key(c, s, lg)]]
    assert all(margins[k] is not None for k in logs)
    assert 10 * sum(margins[k] < 1e-9 for k in logs) <= len(logs)
    # the palindromes are exact ties: the golden holds the lower of the two steps first, and margin 0 was recorded for it
    for name in ("palindrome", "palindrome_odd"):
        g = SC.BY_NAME[name]["gen"]
        assert npz[name + "/stepwise/var"].tolist() == [g["a"], g["n"] - g["a"]]
    g = SC.BY_NAME["palindrome_narrow"]["gen"]                # ... and here the tie-break decides what is found at all
    b = npz["palindrome_narrow/stepwise/var"].tolist()
    assert b[0] == g["a"] and g["n"] - g["a"] not in b


@pytest.mark.parametrize("run", SC.runs(SC.CASES_ALL), ids=SC.run_ids(SC.CASES_ALL))
def test_oracle_equals_golden(run):
    case, splitter, use_log = run
    start, end = SC.normalised(case)
    with np.errstate(all="ignore"):
        got = statsplit_oracle.segment(SC.build(case), use_log=use_log, splitter=splitter, start=start, end=end, **case["par"])
    assert np.array_equal(got, SC.golden()[0][SC.key(case, splitter, use_log)])
