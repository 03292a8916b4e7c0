"""The state parsers without a GPU: the numpy restatement (tests/state_parser_oracle.py) against the goldens recorded from the
reference (tests/golden/make_golden_state_parsers.py), and the surface of the two classes."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_parser_cases as PC  # noqa: E402
import state_parser_oracle as PO  # noqa: E402

from pypore_amd import parsers  # noqa: E402
from pypore_amd.parsers import FilterDerivativeSegmenter, snakebase_parser  # noqa: E402


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("case", PC.SNAKE_CASES, ids=_ids(PC.SNAKE_CASES))
def test_snakebase_oracle_equals_reference(case):
    got = PO.snakebase_spans(PC.snake_build(case))
    want = PC.golden()[0]["snake/" + case["name"]]
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.all(got[:, 0] < got[:, 1])                       # no span is empty


@pytest.mark.parametrize("case", PC.FD_CASES, ids=_ids(PC.FD_CASES))
def test_filter_derivative_oracle_equals_reference(case):
    assert np.array_equal(PO.filter_derivative_spans(PC.fd_build(case), **case["par"]), PC.golden()[0]["fd/" + case["name"]])


FDY_RECORDED = [c for c in PC.FDY_CASES if c["name"] != "n0"]      # (the reference raises on an empty y)


@pytest.mark.parametrize("case", FDY_RECORDED, ids=_ids(FDY_RECORDED))
def test_filter_derivative_decisions_equal_reference(case):
    par = case["par"]
    got = PO.filter_derivative_spans_from_y(PC.fdy_build(case), par["low_threshold"], par["high_threshold"])
    assert np.array_equal(got, PC.golden()[0]["fdy/" + case["name"]])


def test_goldens_hold_every_case_and_nothing_else():
    npz, man = PC.golden()
    keys = (["snake/" + c["name"] for c in PC.SNAKE_CASES] + ["fd/" + c["name"] for c in PC.FD_CASES] +
            ["fdy/" + c["name"] for c in FDY_RECORDED])
    assert sorted(npz.files) == sorted(keys) == sorted(r["key"] for r in man["cases"])
    assert all(npz[k].dtype == np.int32 and npz[k].ndim == 2 and npz[k].shape[1] == 2 for k in keys)
    assert all(c["gen"].get("n", 0) <= 8192 for c in PC.SNAKE_CASES + PC.FD_CASES)
    assert all(PC.fdy_build(c).size <= 8192 for c in PC.FDY_CASES)


def test_margin_rule_of_the_manifest():
    """At most 1 full-route case in 10 lies below the margin, and those are named."""
    _, man = PC.golden()
    fd = [r for r in man["cases"] if r["key"].startswith("fd/")]
    below = [r["key"] for r in fd if r["margin"] < man["margin_rel"] * r["max_abs_current"]]
    assert man["margin_rel"] == 1e-9 and below == man["below_margin"] and 10 * len(below) <= len(fd)


def test_cases_reach_the_shapes_named():
    npz, man = PC.golden()
    rows = {r["key"]: r for r in man["cases"]}
    assert rows["fdy/one_tic"]["pairs"] == 0 and rows["fdy/odd_tics"]["pairs"] == 3
    assert rows["fdy/many_pairs"]["pairs"] > PC.WAVE and rows["fdy/many_pairs_300"]["pairs"] > 256
    assert any(r["blocks0"] for r in rows.values() if "blocks0" in r) and not all(r["blocks0"] for r in rows.values() if "blocks0" in r)
    # the tie: two pairs tied (not kept), the third a sixteenth above (kept)
    assert npz["fdy/tie"].shape[0] == 2 and npz["fdy/tie_long"].shape[0] == 1
    # pairs of 1, 2, 3 samples have no index above 2; those of 4 and 5 have their maximum there
    assert npz["fdy/short_pairs"].shape[0] == 3
    assert npz["snake/every"].shape[0] == PC.T + 1 and npz["snake/none"].shape[0] == 0


def test_snakebase_threshold_changes_nothing():
    for name in ("coarse_long", "near_threshold", "every", "odd_count"):
        x = PC.snake_build(PC.SNAKE_BY_NAME[name])
        want = PO.snakebase_spans(x)
        for threshold in (0.0, 1e-9, 1.5, 1e9, float("nan")):
            assert np.array_equal(PO.snakebase_spans(x, threshold), want)


def test_oracle_raises_like_scipy_on_short_input():
    for n in range(0, 7):
        with pytest.raises(ValueError):
            PO.filter_derivative_spans(np.arange(n, dtype=np.float64))
    assert PO.filter_derivative_spans(np.arange(7, dtype=np.float64)).tolist() == [[0, 7]]


def test_class_surface():
    assert issubclass(snakebase_parser, parsers.parser) and issubclass(FilterDerivativeSegmenter, parsers.parser)
    assert "snakebase_parser" in parsers.__all__ and "FilterDerivativeSegmenter" in parsers.__all__
    space = {}
    exec("from pypore_amd.parsers import *", space)
    for name in ("snakebase_parser", "FilterDerivativeSegmenter", "SpeedyStatSplit", "StatSplit", "lambda_event_parser",
                 "MemoryParse", "parser"):
        assert name in space
    assert vars(snakebase_parser()) == dict(threshold=1.5)
    assert vars(FilterDerivativeSegmenter()) == dict(low_threshold=1, high_threshold=2, cutoff_freq=1000., sampling_freq=1.e5)
    for cls in (snakebase_parser, FilterDerivativeSegmenter):
        assert callable(cls.parse) and callable(cls.parse_batch)
    from pypore_amd import DataTypes                     # noqa: F401  (the drop-in's `from parsers import *` users)


def test_json_round_trip():
    p = snakebase_parser(threshold=2.25)
    d = json.loads(p.to_json())
    assert d == dict(threshold=2.25, name="snakebase_parser") == p.to_dict()
    q = parsers.parser.from_json(p.to_json())
    assert type(q) is snakebase_parser and q.threshold == 2.25
    p = FilterDerivativeSegmenter(low_threshold=0.5, high_threshold=3, cutoff_freq=2000., sampling_freq=2.5e5)
    assert json.loads(p.to_json()) == dict(low_threshold=0.5, high_threshold=3, cutoff_freq=2000., sampling_freq=2.5e5,
                                           name="FilterDerivativeSegmenter")
    q = parsers.parser.from_json(p.to_json())
    assert type(q) is FilterDerivativeSegmenter and vars(q) == vars(p)


@pytest.mark.parametrize("n", [0, 1, 6])
def test_filter_derivative_short_input_raises_before_any_device_work(n):
    with pytest.raises(ValueError):
        FilterDerivativeSegmenter().parse(np.zeros(n))
    with pytest.raises(ValueError):
        FilterDerivativeSegmenter().parse_batch([np.zeros(100), np.zeros(n)])


def test_c_abi_is_bound():
    from pypore_amd import _lib
    assert "ps_snakebase_f64" in _lib.EXPORTS and "ps_filter_derivative_f64" in _lib.EXPORTS
    L = _lib.lib()
    assert L.ps_snakebase_f64.argtypes is not None and L.ps_filter_derivative_f64.argtypes is not None
    assert [f[0] for f in _lib.FilterDerivativeParams._fields_] == ["low_threshold", "high_threshold", "cutoff_freq",
                                                                    "sampling_freq", "prefiltered"]
