#!/usr/bin/env python3
"""Records what the reference's own lambda_event_parser (parsers.py, default rules) returns on seeded traces where event
detection is easy to get wrong: noise chattering across the threshold, float64 at decimal resolution with samples exactly
at the threshold and at min_current, and .abf grids (inexact header scale, non-zero offset) with thresholds at sample
values.  Only the generator parameters (tests/golden_util.detect_input) and the events' starts and lengths are stored.

Run in the build container only (needs the reference and oracle/build_reference.sh):

    ./oracle/build_reference.sh && python tests/golden/make_golden_detect.py

Outputs (committed): tests/golden/golden_detect.npz + tests/golden/manifest_detect.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shims              # noqa: E402
from golden_util import detect_input      # noqa: E402


def abf_scale():
    """adc_range 10 / instrument_scale 0.0005 / signal_gain 20 / 32768 with the header's fp32 floats (abf._read_meta)."""
    return float(np.float32(10.0)) / float(np.float32(0.0005)) / float(np.float32(20.0)) / float(np.float32(1.0)) / 32768


def hard_count(q, o, lo=50.0, hi=100.0):
    """The first count k (pA in (lo, hi)) whose value x = fl(fl(k q) + o) as a threshold is judged below itself by the count
    test fl(k q) < fl(x - o)."""
    kk = np.arange(1, 32767)
    xs = kk * q + o
    hard = kk[(kk * q < xs - o) & (xs > lo) & (xs < hi)]
    return int(hard[0]) if hard.size else None


def main():
    ref = ref_shims.load_reference_parsers()
    cases, arrays = [], {}

    def record(name, gen, thresholds):
        x = detect_input(gen)
        case = dict(name=name, gen=gen, thresholds=[repr(float(t)) for t in thresholds], n_events=[])
        for i, t in enumerate(thresholds):
            evs = ref.lambda_event_parser(threshold=t).parse(x)
            arrays["%s/t%d/starts" % (name, i)] = np.array([int(e.start) for e in evs], dtype=np.int64)
            arrays["%s/t%d/lengths" % (name, i)] = np.array([int(e.duration) for e in evs], dtype=np.int64)
            case["n_events"].append(len(evs))
        cases.append(case)
        print(name, case["thresholds"], case["n_events"])

    for seed in (1, 2, 3):
        gen = dict(kind="chatter", seed=seed, n=600000, blockades=[[100000, 260000], [330000, 520000]],
                   chatter_at=[99000 + seed, 259500 + 3 * seed, 329000, 519500 + seed], chatter_len=1000)
        if seed == 2:
            gen["plant_counts"] = [[150000, -16], [400000, -15]]           # min exactly -0.5 pA (rejected), one count above
        record("chatter_s%d" % seed, gen, [90.0, 90.0 + 2.0 ** -6, 88.0])
    for per, seed in ((10, 0), (20, 1), (100, 2)):
        step = 1.0 / per
        gen = dict(kind="decimal", seed=seed, n=300000, per_pA=per, blockades=[[100000, 250000]],
                   plant=[[250000, 90.0], [99999, 90.0]])
        record("decimal_%d" % per, gen, [90, 90.0 + step, 45.0])
        gen = dict(kind="decimal", seed=seed + 10, n=300000, per_pA=per, blockades=[[50000, 160000], [170000, 290000]],
                   plant=[[60000, -0.5], [200000, -0.5 + step], [160000, 90.0], [169999, 90.0 - step]])
        record("decimal_%d_min" % per, gen, [90])
    q = abf_scale()
    for off in (1.75, 12.345):
        kt = hard_count(q, off)
        if kt is None:
            continue
        t = kt * q + off
        gen = dict(kind="abf_grid", seed=12, n=300000, scale=repr(q), offset=off, blockades=[[100000, 250000]],
                   plant_counts=[[250000, kt], [99999, kt]])
        record("abf_off%s" % off, gen, [t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), 90.0])

    np.savez_compressed(os.path.join(HERE, "golden_detect.npz"), **arrays)
    with open(os.path.join(HERE, "manifest_detect.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_detect.py", "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
