"""tests/filter_exact.py on the host: the long-double filtfilt against every scipy golden of the suite (each within its
recorded tolerance) and against the fp64 oracle on the edge cases of tests/test_filter_edges.py (within the bound the
manifest records for each)."""
import json
import os

import numpy as np
import pytest

import filter_exact as fx
from pypore_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
TOL = 1e-11                                # tests/test_filter.py: the order-1 goldens


def _load(stem):
    return json.load(open(os.path.join(G, "manifest_%s.json" % stem))), np.load(os.path.join(G, "golden_%s.npz" % stem))


MAN1, NPZ1 = _load("filter")
MAN_O, NPZ_O = _load("filter_order")
MAN_H, NPZ_H = _load("filter_hi")
EDGES = json.load(open(os.path.join(G, "manifest_filter_edges.json")))


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("case", MAN1["cases"], ids=[c["name"] for c in MAN1["cases"]])
def test_helper_matches_scipy_golden_order_1(case):
    g = case["gen"]
    if g["kind"] == "config2_event":
        k = np.rint(synth.config2_event(g["ev"], n=g["n"], dtype=np.float64) / synth.QUANTUM).astype(np.int64)
    else:
        k = synth.random_dwell_counts(g["n"], g["seed"], g["lo"], g["hi"])
    ref = NPZ1[case["name"] + "/filtered"]
    got = fx.bessel_filtfilt_ld(k.astype(np.float64) * synth.QUANTUM, case["cutoff"], case["second"], 1)
    assert got.dtype == np.longdouble and fx.rel_err(ref, got) <= TOL


@pytest.mark.parametrize("case", MAN_O["cases"], ids=[c["name"] for c in MAN_O["cases"]])
def test_helper_matches_scipy_golden_orders_2_to_4(case):
    g = case["gen"]
    x = synth.random_dwell_counts(g["n"], g["seed"], g["lo"], g["hi"]).astype(np.float64) * synth.QUANTUM
    ref = NPZ_O[case["name"] + "/filtered"]
    assert fx.rel_err(ref, fx.bessel_filtfilt_ld(x, case["cutoff"], case["second"], case["order"])) <= case["tol"]
    # ... and with scipy's own coefficients, as recorded
    assert fx.rel_err(ref, fx.filtfilt_ld(x, NPZ_O[case["name"] + "/b"], NPZ_O[case["name"] + "/a"])) <= case["tol"]


@pytest.mark.parametrize("case", MAN_H["cases"], ids=[c["name"] for c in MAN_H["cases"]])
def test_helper_matches_scipy_golden_orders_5_to_8_and_float64(case):
    g = case["gen"]
    if len(case["chain"]) > 1:
        x = NPZ_H[case["name"] + "/input"]
    elif g["kind"] == "grid":
        x = synth.random_dwell_counts(g["n"], g["seed"], g["lo"], g["hi"]).astype(np.float64) * synth.QUANTUM
    else:
        x = synth.offgrid_trace(g["n"], g["seed"], sigma=g["sigma"])
    order, cutoff = case["chain"][-1]
    ref = NPZ_H[case["name"] + "/filtered"]
    assert fx.rel_err(ref, fx.bessel_filtfilt_ld(x, cutoff, case["second"], int(order))) <= case["tol"]


def test_helper_rejects_what_scipy_rejects():
    with pytest.raises(ValueError):
        fx.filtfilt_ld(np.ones(6), [0.5, 0.5], [1.0, 0.0])
    with pytest.raises(ValueError):
        fx.bessel_filtfilt_ld(np.ones(12), 2000.0, 1e5, 3)


def test_helper_passes_a_constant_through():
    """zi is the steady state of a unit step: a constant input comes out as that constant times the square of the DC gain
    of the float64 coefficients as given, sum(b) / sum(a) (1 to about 1e-12 at order 8), from the first sample to the last."""
    import oracle
    for order, cutoff in ((1, 2000.0), (1, 30000.0), (3, 2000.0), (8, 10000.0)):
        b, a = oracle.bessel_ba(order, cutoff / 5e4)
        gain = np.sum(b.astype(np.longdouble)) / np.sum(a.astype(np.longdouble))
        y = fx.bessel_filtfilt_ld(np.full(500, 7.25), cutoff, 1e5, order)
        assert abs(float(gain) - 1.0) < 1e-11
        assert fx.rel_err(y, np.full(500, np.longdouble(7.25) * gain * gain, dtype=np.longdouble)) < 1e-13


KEYS = sorted(EDGES["cases"])


@pytest.mark.parametrize("key", KEYS)
def test_oracle_is_within_the_recorded_bound_of_the_helper(key):
    """The fp64 oracle on every edge case (its first 2e5 samples) against the long-double result: within the manifest's
    bound max(1e-11, 4 err_ref), and the recorded err_ref is reproduced to a factor of two (other libm, other last bits)."""
    e = EDGES["cases"][key]
    err = fx.measure(e)
    assert e["bound"] == fx.bound_from(e["err_ref"])
    assert err <= e["bound"]
    assert err <= max(2.0 * e["err_ref"], fx.TOL / 4)
