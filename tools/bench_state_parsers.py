#!/usr/bin/env python3
"""Times the two state parsers on the GPU (ps_snakebase_f64, ps_filter_derivative_f64) on BASELINE config 2's shape -- 1 024
events of 50 000 samples (synth.config2_event), float64, resident on the device, ONE call per run -- and on one trace of
--long samples (default 10^7) as a single event.  HIP events around each call (which synchronises before it returns), median
of --runs after --warmup warm-ups; the spans stay on the device (no Segment objects).

Modes: snakebase; filter-derivative at its defaults (low_threshold 1: on this data no derivative reaches it, the call is
filter + one pass) and at low_threshold 0.05 (the steps of the data become blocks), each also with prefiltered = 1 on the
device filter's own output (the decision kernels alone).  The filter of a batch is one launch (ps_filter_bessel_batch's
kernels; tools/bench_filter_batch.py times it on its own and against the per-event entry).

Two yardsticks from the same run:
* the numpy restatement (tests/state_parser_oracle.py) on one CPU core, timed on --cpu-events events and scaled to all;
* one device-to-device copy of the same bytes: snakebase is one read of the samples, so that is the floor it is held to.

    python tools/bench_state_parsers.py --out profiles/state_parsers_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, runs):
    import torch
    out, ms = None, []
    for r in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return out, dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def cpu_seconds(fn, events):
    fn(events[0][:1000])                                     # (imports and first-call set-up stay outside the clock)
    t0 = time.perf_counter()
    for ev in events:
        fn(ev)
    return time.perf_counter() - t0


def bench(ctx, cur, host_events, starts, lens, modes, warmup, runs, total_events):
    import torch
    import state_parser_oracle as PO
    from pypore_amd import _lib
    n_total = int(lens.sum())
    doc = {}
    dst = torch.empty_like(cur)
    _, t = timed(lambda: dst.copy_(cur), warmup, runs)
    t["GB_per_s_read_plus_write"] = round(2 * 8 * n_total / t["median_ms"] / 1e6, 1)
    doc["d2d_copy_same_bytes"] = t
    del dst
    (sp, off), t = timed(lambda: ctx.snakebase_f64(cur, starts, lens), warmup, runs)
    t["spans"] = int(off[-1])
    t["samples_per_s"] = round(n_total / t["median_ms"] * 1e3)
    t["times_d2d_copy"] = round(t["median_ms"] / doc["d2d_copy_same_bytes"]["median_ms"], 2)
    cpu = cpu_seconds(PO.snakebase_spans, host_events) * total_events / len(host_events)
    t["numpy_one_core_s"] = round(cpu, 3)
    t["speedup_vs_numpy"] = round(cpu * 1e3 / t["median_ms"], 1)
    doc["snakebase"] = t
    sys.stderr.write("[bench_state_parsers] snakebase: %s\n" % json.dumps(t))
    del sp
    y = None
    for name, low in modes:
        par = dict(low_threshold=low, high_threshold=2.0, cutoff_freq=1000., sampling_freq=1.e5)
        full = _lib.FilterDerivativeParams(low, 2.0, 1000., 1.e5, 0)
        pre = _lib.FilterDerivativeParams(low, 2.0, 1000., 1.e5, 1)
        (sp, off), t = timed(lambda: ctx.filter_derivative_f64(cur, starts, lens, full), warmup, runs)
        t["spans"] = int(off[-1])
        t["samples_per_s"] = round(n_total / t["median_ms"] * 1e3)
        cpu = cpu_seconds(lambda ev: PO.filter_derivative_spans(ev, **par), host_events) * total_events / len(host_events)
        t["numpy_scipy_one_core_s"] = round(cpu, 3)
        t["speedup_vs_numpy_scipy"] = round(cpu * 1e3 / t["median_ms"], 1)
        if y is None:                                        # the device filter's output, event after event
            y = ctx.filter_requantise_batch(cur, starts, lens, 1.0, cutoff=1000., sampling_freq=1.e5)[0].contiguous()
        (sp2, off2), t2 = timed(lambda: ctx.filter_derivative_f64(y, starts, lens, pre), warmup, runs)
        t["prefiltered"] = dict(t2, spans=int(off2[-1]))
        doc["filter_derivative/" + name] = t
        sys.stderr.write("[bench_state_parsers] filter_derivative/%s: %s\n" % (name, json.dumps(t)))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--long", type=int, default=10_000_000)
    ap.add_argument("--cpu-events", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pypore_amd import engine, synth

    ctx = engine.context(0)
    n_ev, n = args.events, args.samples
    modes = [("defaults", 1.0), ("low_0.05", 0.05)]
    host = [synth.config2_event(e, n=n, dwell=n // 5) for e in range(n_ev)]
    cur = torch.from_numpy(np.concatenate(host)).cuda()
    doc = {"device": torch.cuda.get_device_name(0), "events": n_ev, "samples_per_event": n, "runs": args.runs, "warmup": args.warmup,
           "timer": "HIP events around one call", "cpu_events_timed": min(args.cpu_events, n_ev)}
    doc["batch"] = bench(ctx, cur, host[:args.cpu_events], np.arange(n_ev, dtype=np.int64) * n, np.full(n_ev, n, dtype=np.int64),
                         modes, args.warmup, args.runs, n_ev)
    del cur, host
    x = synth.counts_to_pa(synth.random_dwell_counts(args.long, 7), np.float64)
    lt = torch.from_numpy(x).cuda()
    doc["long_trace"] = dict(bench(ctx, lt, [x], np.zeros(1, dtype=np.int64), np.full(1, args.long, dtype=np.int64), modes,
                                   args.warmup, args.runs, 1), samples=args.long)
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
