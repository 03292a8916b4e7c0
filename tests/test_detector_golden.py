"""oracle.lambda_events -- what the GPU detector tests trust -- against the reference's own lambda_event_parser
(tests/golden/make_golden_detect.py: chatter, decimal-resolution float64, .abf grids with thresholds at sample values), and
the thresholds engine.detector_thresholds hands the kernels, restated on the host: double(k) * q < threshold' on the
counts the device would read gives the reference's events.  No GPU."""
import numpy as np
import pytest

import oracle
from golden_util import detect_cases, detect_input, detect_npz
from pypore_amd import engine
from pypore_amd.grid import affine_grid
from pypore_amd.parsers import lambda_event_parser

CASES = detect_cases()


def _want(name, i):
    z = detect_npz()
    return z["%s/t%d/starts" % (name, i)], z["%s/t%d/lengths" % (name, i)]


def test_the_golden_covers_what_it_says():
    names = [c["name"] for c in CASES]
    assert sum(n.startswith("chatter") for n in names) >= 3 and sum(n.startswith("decimal") for n in names) >= 6
    assert sum(n.startswith("abf") for n in names) >= 1
    assert sum(sum(c["n_events"]) for c in CASES) >= 20


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_and_host_rules_match_the_reference(case):
    x = detect_input(case["gen"])
    for i, t in enumerate(case["thresholds"]):
        t = float(t)
        ws, wl = _want(case["name"], i)
        st, ln = oracle.lambda_events(np.asarray(x), threshold=t)
        np.testing.assert_array_equal(st, ws)
        np.testing.assert_array_equal(ln, wl)
        P = lambda_event_parser
        host = P(threshold=t, rules=[lambda e: e.duration > P.MIN_DURATION, lambda e: e.min > P.MIN_CURRENT,
                                     lambda e: e.max < t]).parse(np.asarray(x))
        assert [(int(e.start), int(e.duration)) for e in host] == list(zip(ws.tolist(), wl.tolist()))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_count_space_thresholds_give_the_reference_events(case):
    """The device's predicate on the counts it reads, with the thresholds the parser hands it, run through the oracle."""
    x = detect_input(case["gen"])
    if case["gen"]["kind"] == "abf_grid":                  # the file route: counts, scale and offset of the GridArray
        q, o, k = x.quantum, x.offset, x.counts.astype(np.int64)
    else:                                                  # float64 on an affine grid (chatter: a power-of-two one)
        q, o, k = affine_grid(x)
    for i, t in enumerate(case["thresholds"]):
        t = float(t)
        if case["gen"]["kind"] == "abf_grid":
            thr, mc = engine.detector_thresholds(q, t, lambda_event_parser.MIN_CURRENT, offset=o)
        else:
            thr, mc = engine.detector_thresholds(q, t, lambda_event_parser.MIN_CURRENT, values=x, counts=k)
        ws, wl = _want(case["name"], i)
        st, ln = oracle.lambda_events(k.astype(np.float64) * q, threshold=thr, min_current=mc)
        np.testing.assert_array_equal(st, ws)
        np.testing.assert_array_equal(ln, wl)
