#!/usr/bin/env python3
"""Wall clock of StatSplit on the GPU (ps_statsplit_f64) at its defaults, BASELINE config 2's shape: 1 024 events of 50 000
samples (synth.config2_event), float64, resident on the device, in ONE call per run.

Modes: stepwise / log (the defaults), stepwise / variance, slanted / variance.  Median of --runs runs after --warmup warm-ups,
each run synchronised, boundaries left on the device (no Segment objects).  Beside them, in the same process:

* SpeedyStatSplit(off_grid="exact")'s device call (ps_segment_exact_f64) on the same events, with the threshold that
  matches StatSplit's (its own is doubled): the same kind of work -- sequential prefix chains, two logarithms per candidate --
  spread over one workgroup per WINDOW where StatSplit has one per event;
* one trace of --long samples (default 10^7) as a single event: one workgroup and one sequential prefix chain bound it;
* the reference's pure-Python StatSplit on one such event, a constant measured on a CPU (REFERENCE_S below), times 1 024.

    python tools/bench_statsplit.py --out profiles/statsplit_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Seconds the reference's own StatSplit(...).parse takes on ONE config-2 event (50 000 samples, defaults), median of 3,
# CPython 3 on one core of the build machine's x86-64 CPU, 2026-10-20.
REFERENCE_S = {"stepwise/log": 0.411, "stepwise/var": 0.196, "slanted/var": 0.821}
REFERENCE_DATE = "2026-10-20"
MODES = [("stepwise/log", "stepwise", True), ("stepwise/var", "stepwise", False), ("slanted/var", "slanted", False)]


def timed(fn, sync, warmup, runs):
    out = None
    ts = []
    for r in range(warmup + runs):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if r >= warmup:
            ts.append(time.perf_counter() - t0)
    return out, dict(median_s=round(statistics.median(ts), 6), min_s=round(min(ts), 6), max_s=round(max(ts), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--long", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pypore_amd import _lib, engine, synth
    from pypore_amd.parsers import StatSplit

    ctx = engine.context(0)
    sync = torch.cuda.synchronize
    n_ev, n = args.events, args.samples
    host = np.concatenate([synth.config2_event(e, n=n, dwell=n // 5) for e in range(n_ev)])
    cur = torch.from_numpy(host).cuda()
    starts = np.arange(n_ev, dtype=np.int64) * n
    lens = np.full(n_ev, n, dtype=np.int64)
    doc = {"device": torch.cuda.get_device_name(0), "events": n_ev, "samples_per_event": n, "runs": args.runs, "warmup": args.warmup,
           "unit": "s", "reference_python_s_per_event": REFERENCE_S, "reference_measured": REFERENCE_DATE, "modes": {}}
    for name, splitter, use_log in MODES:
        p = StatSplit(use_log=use_log, splitter=splitter)
        (b, off), t = timed(lambda: ctx.statsplit_f64(cur, starts, lens, p._params()), sync, args.warmup, args.runs)
        t["boundaries"] = int(off[-1])
        t["samples_per_s"] = round(n_ev * n / t["median_s"])
        t["reference_python_s"] = round(REFERENCE_S[name] * n_ev * n / 50000, 1)
        t["speedup_vs_reference_python"] = round(t["reference_python_s"] / t["median_s"])
        doc["modes"][name] = t
        sys.stderr.write("[bench_statsplit] %s: %s\n" % (name, json.dumps(t)))
    # SpeedyStatSplit's exact route on the same events: threshold min_gain_per_sample * 2 W there, so half the gain per sample
    sp = _lib.split_params(min_width=1000, max_width=1000000, window_width=10000, min_gain_per_sample=0.015)
    (b, off), t = timed(lambda: ctx.segment_exact_f64(cur, starts, lens, sp), sync, args.warmup, args.runs)
    t["boundaries"] = int(off[-1])
    doc["speedy_exact_same_events"] = t
    doc["statsplit_over_speedy_exact"] = round(doc["modes"]["stepwise/log"]["median_s"] / t["median_s"], 3)
    sys.stderr.write("[bench_statsplit] SpeedyStatSplit exact: %s\n" % json.dumps(t))
    del cur
    # one long trace as a single event
    long_n = args.long
    x = synth.counts_to_pa(synth.random_dwell_counts(long_n, 7), np.float64)
    lt = torch.from_numpy(x).cuda()
    doc["long_trace"] = {"samples": long_n}
    for name, splitter, use_log in MODES:
        p = StatSplit(use_log=use_log, splitter=splitter)
        (b, off), t = timed(lambda: ctx.statsplit_f64(lt, np.zeros(1, dtype=np.int64), np.full(1, long_n, dtype=np.int64), p._params()),
                            sync, 1, 3)
        t["boundaries"] = int(off[-1])
        t["samples_per_s"] = round(long_n / t["median_s"])
        doc["long_trace"][name] = t
        sys.stderr.write("[bench_statsplit] long %s: %s\n" % (name, json.dumps(t)))
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
