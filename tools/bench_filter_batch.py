#!/usr/bin/env python3
"""Times the batched Bessel filter (ps_filter_bessel_batch) and the two entries that run on its kernels, on BASELINE config 2's
shape: 1 024 events of 50 000 samples (synth.config2_event), resident on the device.  HIP events around each call (which
synchronises before it returns), median of --runs after --warmup warm-ups, every repetition kept.

filter:   order 1 / 2 000 Hz on int16 counts and on float64: ps_filter_bessel_batch (one launch), the same events through
          ps_filter_bessel one by one (the per-event entry: unchanged code), and one device-to-device copy of the output's bytes
          as the yardstick tools/bench_state_parsers.py uses.  The batched filter's algorithmic bytes are
          (element size * 4096 / T + 8) per sample -- every tile loads 4 096 elements for the T it writes --: its GB/s is
          reported next to the copy's.  Order 2 / 2 000 Hz once on the same events, for the record.
callers:  ps_filter_requantise_batch on the int16 events and ps_filter_derivative_f64 (bench_state_parsers' two settings) on the
          float64 events.  --tree DIR times the package of another checkout instead -- the parent commit's, built there -- and
          --parent FILE puts that run's figures next to this build's: a rewired entry clears the bar when its median beats the
          parent's by more than the larger min-max spread of the two runs.

    python tools/bench_filter_batch.py --callers-only --tree ../parent --out parent.json
    python tools/bench_filter_batch.py --parent parent.json --out profiles/filter_batch_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096


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


def say(name, t):
    sys.stderr.write("[bench_filter_batch] %s: %s\n" % (name, json.dumps(t)))


def singles(ctx, samples, fmt, starts, lens, out, order, cutoff):
    """The events through ps_filter_bessel one by one, as a caller without the batch entry does."""
    from pypore_amd import _lib
    es = samples.element_size()
    base, obase, off = samples.data_ptr(), out.data_ptr(), 0
    with ctx.lock:
        for s, n in zip(starts.tolist(), lens.tolist()):
            _lib.check(ctx.L.ps_filter_bessel(ctx.handle, ctypes.c_void_p(base + s * es), ctypes.byref(fmt), n, order, cutoff, 1.e5,
                                              ctypes.c_void_p(obase + 8 * off)), ctx.handle)
            off += n
    return out


def bench_filter(ctx, forms, starts, lens, warmup, runs):
    import torch
    from pypore_amd import _lib
    import filter_exact as fx
    n_total = int(lens.sum())
    T = fx.order1_geometry(int(lens[0]), 2000., 1.e5, 1)["T"]
    doc = {"tile_T": T}
    src = torch.empty(n_total, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    _, t = timed(lambda: dst.copy_(src), warmup, runs)
    t["GB_per_s_read_plus_write"] = round(2 * 8 * n_total / t["median_ms"] / 1e6, 1)
    doc["d2d_copy_output_bytes"] = copy = t
    say("d2d copy", t)
    del src, dst
    for name, samples, q in forms:
        es = samples.element_size()
        fmt = _lib.SampleFormat(_lib.PS_DTYPE_F64, 0, 1.0) if samples.dtype == torch.float64 else ctx._fmt(samples, q, 0)
        (y, _), t = timed(lambda: ctx.filter_bessel_batch(samples, starts, lens, q, cutoff=2000., sampling_freq=1.e5, order=1), warmup, runs)
        bytes_per_sample = es * CHUNK / T + 8
        t["algorithmic_bytes_per_sample"] = round(bytes_per_sample, 3)
        t["GB_per_s"] = round(bytes_per_sample * n_total / t["median_ms"] / 1e6, 1)
        t["share_of_copy_GB_per_s"] = round(t["GB_per_s"] / copy["GB_per_s_read_plus_write"], 3)
        t["times_d2d_copy"] = round(t["median_ms"] / copy["median_ms"], 2)
        out = torch.empty_like(y)
        _, t1 = timed(lambda: singles(ctx, samples, fmt, starts, lens, out, 1, 2000.), warmup, runs)
        t["equal_to_singles"] = bool(torch.equal(out, y))
        t["per_event_entry"] = t1
        t["speedup_vs_per_event_entry"] = round(t1["median_ms"] / t["median_ms"], 2)
        _, t2 = timed(lambda: ctx.filter_bessel_batch(samples, starts, lens, q, cutoff=2000., sampling_freq=1.e5, order=2), 1, 1)
        t["order_2_once_ms"] = t2["median_ms"]
        doc["order1_2000Hz/" + name] = t
        say(name, t)
        del y, out
    return doc


def bench_callers(ctx, i16, f64, q, starts, lens, warmup, runs):
    from pypore_amd import _lib
    doc = {}
    _, t = timed(lambda: ctx.filter_requantise_batch(i16, starts, lens, q, cutoff=2000., sampling_freq=1.e5, order=1), warmup, runs)
    doc["filter_requantise_batch/int16"] = t
    say("filter_requantise_batch", t)
    for name, low in (("defaults", 1.0), ("low_0.05", 0.05)):
        par = _lib.FilterDerivativeParams(low, 2.0, 1000., 1.e5, 0)
        (_, off), t = timed(lambda: ctx.filter_derivative_f64(f64, starts, lens, par), warmup, runs)
        t["spans"] = int(off[-1])
        doc["filter_derivative/" + name] = t
        say("filter_derivative/" + name, t)
    return doc


def judge(new, parent):
    """Per caller: the parent's and this build's figures and whether the bar is cleared."""
    out = {}
    for key, t in new.items():
        p = parent.get(key)
        if p is None:
            continue
        spread = max(t["max_ms"] - t["min_ms"], p["max_ms"] - p["min_ms"])
        out[key] = dict(parent=p, this_build=t, larger_spread_ms=round(spread, 4), gain_ms=round(p["median_ms"] - t["median_ms"], 4),
                        speedup=round(p["median_ms"] / t["median_ms"], 2), clears_bar=bool(p["median_ms"] - t["median_ms"] > spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--callers-only", action="store_true")
    ap.add_argument("--tree", default=None, help="time the package of this checkout (built there) instead of the tool's own")
    ap.add_argument("--parent", default=None, help="JSON of a --callers-only run on the parent commit")
    ap.add_argument("--state-parsers", nargs=2, default=None, metavar=("PARENT", "NEW"),
                    help="two outputs of tools/bench_state_parsers.py, parent commit and this build: their filter-derivative figures go along")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.tree) if args.tree else HERE
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))

    import torch
    from pypore_amd import engine, synth

    ctx = engine.context(0)
    n_ev, n = args.events, args.samples
    host = np.concatenate([synth.config2_event(e, n=n, dwell=n // 5) for e in range(n_ev)])
    k = np.rint(host / synth.QUANTUM)
    assert np.array_equal(k * synth.QUANTUM, host) and np.abs(k).max() < 2 ** 15
    i16 = torch.from_numpy(k.astype(np.int16)).cuda()
    f64 = torch.from_numpy(host).cuda()
    starts, lens = np.arange(n_ev, dtype=np.int64) * n, np.full(n_ev, n, dtype=np.int64)
    doc = {"device": torch.cuda.get_device_name(0), "events": n_ev, "samples_per_event": n, "runs": args.runs, "warmup": args.warmup,
           "timer": "HIP events around one call", "package": os.path.relpath(root, HERE)}
    if not args.callers_only:
        doc["filter"] = bench_filter(ctx, [("int16", i16, synth.QUANTUM), ("float64", f64, 1.0)], starts, lens, args.warmup, args.runs)
    doc["callers"] = bench_callers(ctx, i16, f64, synth.QUANTUM, starts, lens, args.warmup, args.runs)
    if args.parent:
        with open(args.parent) as f:
            doc["callers_vs_parent"] = judge(doc["callers"], json.load(f)["callers"])
    if args.state_parsers:
        docs = []
        for path in args.state_parsers:
            with open(path) as f:
                docs.append({key: t for key, t in json.load(f)["batch"].items() if key.startswith("filter_derivative/")})
        doc["bench_state_parsers_vs_parent"] = judge(docs[1], docs[0])
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
