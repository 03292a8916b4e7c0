#!/usr/bin/env python3
"""Times ps_detect_pieces (engine.Context.detect_pieces) and the parser route built on it, everything in one process: HIP events
around each call (every call synchronises before it returns), median of --runs after --warmup warm-ups, every repetition kept.

(a) nominal:  the int16 file trace of synth.file_trace_counts (--samples, default 1e8: a few hundred pieces).  detect_pieces
              beside detect_events on the same tensor, and one device-to-device copy of the trace's bytes beside both; then
              range_stats on the pieces found, so that the composition detect_events + range_stats -- the bar a dedicated
              kernel has to beat -- stands next to it.
(b) many:     a trace of --samples with a piece every few hundred samples, and an adversarial trace of --alt-samples (default
              1e7) whose samples alternate round the threshold (P = n).  detect_pieces beside range_stats on the same pieces
              (the existing way to these numbers once the edges are known; its table upload is part of its call).
(c) parser:   lambda_event_parser(90, rules=R, on_device=True).parse(file current) against the same parser on the host route, on
              trace (a): wall clock of both.  The device route gets the file's counts (grid.Deferred, as File.parse hands them;
              they go up once and stay, so the repetitions time the resident case and the first call is reported apart); the
              host route gets the float64 array, and writing that array out is timed apart as well.

    python tools/bench_detect_pieces.py --out profiles/detect_pieces_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
            ms.append(round(a.elapsed_time(b), 4))
    return out, dict(median_ms=round(statistics.median(ms), 4), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def wall(fn, warmup, runs):
    out, ms = None, []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        out = fn()
        if r >= warmup:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out, dict(median_ms=round(statistics.median(ms), 3), min_ms=min(ms), max_ms=max(ms), all_ms=ms)


def say(name, t):
    sys.stderr.write("[bench_detect_pieces] %s: %s\n" % (name, json.dumps(t)))


def pieces_and_ranges(ctx, x, q, thr, warmup, runs, copy_ms):
    """detect_pieces and range_stats on the pieces it found; the two must agree bit for bit."""
    (edges, stats), t = timed(lambda: ctx.detect_pieces(x, q, thr), warmup, runs)
    n = x.numel()
    t["pieces"] = int(len(edges) - 1)
    t["ns_per_sample"] = round(t["median_ms"] * 1e6 / n, 4)
    t["times_d2d_copy"] = round(t["median_ms"] / copy_ms * 1.0, 2) if copy_ms else None
    rows, tr = timed(lambda: ctx.range_stats(x, edges[:-1], edges[1:], q), warmup, runs)
    tr["equal_bits"] = bool(np.array_equal(rows.view(np.int64), stats.view(np.int64)))
    return edges, t, tr


def d2d(x, warmup, runs):
    import torch
    dst = torch.empty_like(x)
    _, t = timed(lambda: dst.copy_(x), warmup, runs)
    t["GB_per_s_read_plus_write"] = round(2 * x.element_size() * x.numel() / t["median_ms"] / 1e6, 1)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100_000_000)
    ap.add_argument("--alt-samples", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-parser", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    from pypore_amd import engine, synth
    from pypore_amd.grid import Deferred
    from pypore_amd.parsers import lambda_event_parser

    ctx = engine.context(0)
    q, n = synth.QUANTUM, args.samples
    doc = {"device": torch.cuda.get_device_name(0), "samples": n, "alt_samples": args.alt_samples, "runs": args.runs, "warmup": args.warmup,
           "timer": "HIP events around one call (parser: host wall clock)"}

    # (a) the nominal file trace
    counts, events = synth.file_trace_counts(n, 3)
    k16 = counts.astype(np.int16)
    assert np.array_equal(k16, counts)
    del counts
    x = torch.from_numpy(k16).cuda()
    a = {"events_in_trace": len(events)}
    a["d2d_copy"] = copy = d2d(x, args.warmup, args.runs)
    say("d2d copy", copy)
    (st, ln), t = timed(lambda: ctx.detect_events(x, q, threshold=90.0), args.warmup, args.runs)
    t["events"] = int(len(st))
    t["times_d2d_copy"] = round(t["median_ms"] / copy["median_ms"], 2)
    a["detect_events"] = det = t
    say("detect_events", t)
    edges, t, tr = pieces_and_ranges(ctx, x, q, 90.0, args.warmup, args.runs, copy["median_ms"])
    a["detect_pieces"], a["range_stats_on_its_pieces"] = t, tr
    a["composition_detect_events_plus_range_stats_ms"] = round(det["median_ms"] + tr["median_ms"], 4)
    a["detect_pieces_beats_composition"] = bool(t["median_ms"] < det["median_ms"] + tr["median_ms"])
    say("detect_pieces", t)
    say("range_stats on its pieces", tr)
    doc["a_nominal"] = a

    # (b) many pieces: one every few hundred samples; then every sample its own
    rng = np.random.default_rng(11)
    cuts = np.cumsum(rng.integers(100, 500, n // 300 + 2))
    cuts = cuts[cuts < n]
    side = np.zeros(n, dtype=np.int8)
    side[cuts] = 1
    side = np.cumsum(side, dtype=np.int32) & 1
    dense = np.where(side == 0, 3200, 640).astype(np.int16) + rng.integers(-40, 41, n, dtype=np.int16)
    del side
    xb = torch.from_numpy(dense).cuda()
    b = {}
    _, t, tr = pieces_and_ranges(ctx, xb, q, 90.0, args.warmup, args.runs, copy["median_ms"])
    b["every_few_hundred/detect_pieces"], b["every_few_hundred/range_stats"] = t, tr
    say("a piece every few hundred: detect_pieces", t)
    say("a piece every few hundred: range_stats", tr)
    del xb, dense
    m = args.alt_samples
    alt = np.where(np.arange(m) % 2 == 0, 3200, 640).astype(np.int16)
    xa = torch.from_numpy(alt).cuda()
    copy_alt = d2d(xa, args.warmup, args.runs)
    _, t, tr = pieces_and_ranges(ctx, xa, q, 90.0, args.warmup, args.runs, copy_alt["median_ms"])
    b["alternating/d2d_copy"], b["alternating/detect_pieces"], b["alternating/range_stats"] = copy_alt, t, tr
    say("alternating: detect_pieces", t)
    say("alternating: range_stats", tr)
    del xa, alt
    doc["b_many_pieces"] = b

    # (c) the parser, end to end, on trace (a)
    if not args.skip_parser:
        rules = [lambda ev: ev.duration > 1000, lambda ev: ev.duration < 2000000, lambda ev: ev.max < 90]
        cur = Deferred.from_counts(k16, q, 0.0)
        t0 = time.perf_counter()
        first = lambda_event_parser(90, rules=rules, on_device=True).parse(cur)
        c = {"device_first_call_with_upload_ms": round((time.perf_counter() - t0) * 1e3, 3)}
        got, c["on_device"] = wall(lambda: lambda_event_parser(90, rules=rules, on_device=True).parse(cur), 1, args.runs)
        t0 = time.perf_counter()
        values = k16.astype(np.float64) * q
        c["write_out_float64_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        want, c["host"] = wall(lambda: lambda_event_parser(90, rules=rules).parse(values), 1, args.runs)
        c["events"] = len(got)
        c["same_events"] = [(s.start, s.duration) for s in got] == [(s.start, s.duration) for s in want] == [(s.start, s.duration) for s in first]
        c["speedup"] = round(c["host"]["median_ms"] / c["on_device"]["median_ms"], 2)
        say("parser on device", c["on_device"])
        say("parser on host", c["host"])
        doc["c_parser"] = c

    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
