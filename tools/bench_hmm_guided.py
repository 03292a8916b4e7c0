#!/usr/bin/env python3
"""Times HMM-guided segmentation of a file's events: the per-event loop `ev._merge_by_hmm(model)` (what Event.parse(parser,
hmm=model) runs after its segmentation) against DataTypes.merge_by_hmm(events, model) on the same events, in one process.

Workload: BASELINE config 2 -- 1 024 events of 50 000 samples (synth.step_counts) as the int16 counts of one file whose float64
current has not been written out, segmented ONCE with SpeedyStatSplit(prior_segments_per_second=10); every timed run starts
from those segments again.  The model has the data's five levels, two of them under one name, and a silent state.  The batched
route is timed first: the loop writes the file's float64 current out (its merged segments are views of it), after which the
batched route's stretches would be views too.  Host clock around work that ends in a device synchronisation; median of --runs
after --warmup warm-ups.

Then ps_range_stats alone (engine.Context.range_stats: two launches and the download of the rows) on the merged ranges, beside
one device-to-device copy of the bytes it reads, and the same call at other values of option range_tile (--sweep).

    python tools/bench_hmm_guided.py --out profiles/hmm_guided_bench.json
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


def timed_host(fn, before, warmup, runs):
    import torch
    out, ms = None, []
    for r in range(warmup + runs):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def timed_device(fn, warmup, runs):
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


def level_model():
    from pypore_amd import synth
    from pypore_amd.hmm import Model, NormalDistribution, State
    m = Model("config 2 levels")
    names = ("l50", "l42", "shared", "l38", "shared")           # 55 pA and 47 pA under one name
    emit = [State(NormalDistribution(float(c) * synth.QUANTUM, 2.0), nm) for c, nm in zip(synth.LEVEL_COUNTS, names)]
    quiet = State(None, "quiet")
    for s in emit:
        m.add_transition(m.start, s, 1.0)
        for t in emit:
            m.add_transition(s, t, 0.6 if s is t else 0.08)
        m.add_transition(s, quiet, 0.04)
        m.add_transition(s, m.end, 0.04)
    m.add_transition(quiet, emit[0], 1.0)
    m.bake()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweep", default="1024,2048,4096,8192,16384,32768,65536,262144")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pypore_amd import engine, synth
    from pypore_amd.core import raw_current
    from pypore_amd.DataTypes import Event, File, merge_by_hmm
    from pypore_amd.grid import Deferred
    from pypore_amd.parsers import SpeedyStatSplit

    n_ev, n = args.events, args.samples
    counts = np.concatenate([synth.step_counts(n, n // 5, e) for e in range(n_ev)]).astype(np.int16)
    f = File(current=Deferred.from_counts(counts, synth.QUANTUM, 0.0), timestep=0.01)
    rate = f.second
    # (the file's counts go up once and stay parked, as File.parse's detector leaves them: the events are stretches of that tensor)
    raw_current(f).device_counts(torch.device("cuda", torch.cuda.current_device()), engine._int_counts_tensor)
    f.events =[Event(current=raw_current(f)[e * n:(e + 1) * n], start=e * n / rate, end=(e + 1) * n / rate, duration=n / rate,
                      second=rate, file=f) for e in range(n_ev)]
    f.parse_events(SpeedyStatSplit(prior_segments_per_second=10))
    unmerged = [list(ev.segments) for ev in f.events]
    model = level_model()

    def restore():
        for ev, segs in zip(f.events, unmerged):
            ev.segments = list(segs)

    doc = {"device": torch.cuda.get_device_name(0), "events": n_ev, "samples_per_event": n, "runs": args.runs, "warmup": args.warmup,
           "segments": sum(len(s) for s in unmerged), "timer": "host clock around work that ends in a device synchronisation"}
    _, t = timed_host(lambda: merge_by_hmm(f.events, model), restore, args.warmup, args.runs)
    doc["merge_by_hmm"] = dict(t, file_current_written_out=bool(raw_current(f).built),
                               device_statistics=all("_gpu_stats" in s.__dict__ for ev in f.events for s in ev.segments))
    merged = [[(s.start, len(raw_current(s)), s.hidden_state) for s in ev.segments] for ev in f.events]
    doc["merged_segments"] = sum(len(m) for m in merged)
    sys.stderr.write("[bench_hmm_guided] merge_by_hmm: %s\n" % json.dumps(doc["merge_by_hmm"]))

    def loop():
        for ev in f.events:
            ev.segments = ev._merge_by_hmm(model)
    _, t = timed_host(loop, restore, args.warmup, args.runs)
    doc["per_event_loop"] = t
    doc["speedup"] = round(t["median_ms"] / doc["merge_by_hmm"]["median_ms"], 2)
    doc["same_segments"] = merged == [[(s.start, len(raw_current(s)), s.hidden_state) for s in ev.segments] for ev in f.events]
    sys.stderr.write("[bench_hmm_guided] per-event loop: %s\n" % json.dumps(t))

    # ps_range_stats alone on the merged ranges, beside a device-to-device copy of the bytes it reads
    base = torch.from_numpy(counts).cuda()
    lo = np.array([e * n + s for e, m in enumerate(merged) for s, _, _ in m], dtype=np.int64)
    hi = lo + np.array([k for m in merged for _, k, _ in m], dtype=np.int64)
    ctx = engine.context(0)
    read = int((hi - lo).sum()) * 2
    src = torch.empty(read // 2, dtype=torch.int16, device="cuda")
    dst = torch.empty_like(src)
    _, t = timed_device(lambda: dst.copy_(src), args.warmup, args.runs)
    t["GB_per_s_read_plus_write"] = round(2 * read / t["median_ms"] / 1e6, 1)
    doc["d2d_copy_same_bytes"] = t
    default_tile = ctx.get_option("range_tile")
    _, t = timed_device(lambda: ctx.range_stats(base, lo, hi, synth.QUANTUM), args.warmup, args.runs)
    t.update(ranges=int(lo.size), bytes_read=read, range_tile=default_tile, GB_per_s_read=round(read / t["median_ms"] / 1e6, 1),
             times_d2d_copy=round(t["median_ms"] / doc["d2d_copy_same_bytes"]["median_ms"], 2))
    doc["range_stats"] = t
    sys.stderr.write("[bench_hmm_guided] range_stats: %s\n" % json.dumps(t))
    sweep = {}
    for tile in [int(v) for v in args.sweep.split(",") if v]:
        ctx.set_option("range_tile", tile)
        _, t = timed_device(lambda: ctx.range_stats(base, lo, hi, synth.QUANTUM), args.warmup, args.runs)
        sweep[str(tile)] = t["median_ms"]
    ctx.set_option("range_tile", default_tile)
    doc["range_tile_sweep_median_ms"] = sweep
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
