#!/usr/bin/env python3
"""Recorded error of the fp64 oracle for the filter edge cases (tests/test_filter_edges.py), and the bound each case
derives from it.

    python tests/golden/make_golden_filter_edges.py

For every (filter, input) pair of tests/filter_exact.py's case lists: err_ref = max |oracle_fp64 - ld| / max |ld|, ld the
long-double filtfilt of the same input with the oracle's coefficients (tests/filter_exact.py; on the first 2e5 samples of
a longer input), and bound = max(1e-11, 4 * err_ref): what the device result may differ from the long-double reference
by.  1e-11 is the suite's TOL; the factor 4 covers the device and the oracle rounding independently at the same size
(FMA on the order-1 routes, the scan's re-association) and the halo restart (2^-60 fused, 2^-70 ||A^H|| halo kernel).
No bound is taken from a device result: this script runs on the host alone.

Output (committed): manifest_filter_edges.json -- settings and recorded results only.  Needs the oracle built
(make -C oracle); no scipy."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import filter_exact as fx              # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

COMMENT = ("err_ref: fp64 oracle against the long-double reference, relative to max |reference| (first 200000 samples of a "
           "longer input); bound = max(1e-11, 4 * err_ref) holds the device against the long-double reference. "
           "No case needs a factor above 4.")

if __name__ == "__main__":
    cases = {}
    for key, entry in fx.manifest_inputs().items():
        err = fx.measure(entry)
        cases[key] = dict(order=entry["order"], cutoff=entry["cutoff"], second=entry["second"], gen=entry["gen"],
                          err_ref=err, bound=fx.bound_from(err))
        print(key, "%.2e" % err)
    order, cutoff = fx.refused_filter()
    with open(os.path.join(HERE, "manifest_filter_edges.json"), "w") as f:
        json.dump(dict(comment=COMMENT, tol=fx.TOL, factor=4, max_ld=fx.MAX_LD, slow_halo_filter=list(fx.halo_filters()[-1]),
                       refused_filter=[order, cutoff], cases=cases), f, indent=0, sort_keys=True)
