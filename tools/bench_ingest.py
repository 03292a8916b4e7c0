#!/usr/bin/env python3
"""Wall clock of SpeedyStatSplit(prior_segments_per_second=10).parse(x), Segment objects included, for the 10^8-sample bench
trace (bench.py's stream 0: seed 2024) handed over as

  a  numpy float64 on its power-of-two grid (2^-5 pA),
  b  numpy float64 on an .abf header scale with an offset (counts * 0.030517576675492885 + 12.25),
  c  the float64 CUDA tensor of b.

Median of --runs runs after --warmup warm-ups, each run synchronised, with the spread (min, max) of the runs.  Every run is
split inside the one parse() call it times, by clocks around the functions parse() goes through: `ingest` is its call of
engine.to_device (everything before the segment call; the device is synchronised before the clock stops), of which `upload`
is the time inside engine._staged_upload (the pinned staging; the pageable copy of a short or float32 road is not separable
and stays in `host`), `device` the time inside the library's grid-recovery calls, `host` the rest of the ingest (numpy passes,
the subset, allocations); `segment` = total - ingest is the segment call plus the Segment objects.

    python tools/bench_ingest.py --out this.json [--baseline parent.json]      # one JSON document, also printed

The file works unchanged on a tree from before the device roads (case c is then reported as the error it raises), so the
same script measures both sides: --baseline embeds the other side's document under "parent"."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q_HEADER, OFFSET = 0.030517576675492885, 12.25


class Clock(object):
    """Accumulates the wall time spent inside the functions it wraps."""

    def __init__(self):
        self.acc = {}

    def wrap(self, owner, name, key, after=None):
        fn = getattr(owner, name, None)
        if fn is None:
            return
        clock = self

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                out = fn(*a, **kw)
                if after is not None:
                    after(out)
                return out
            finally:
                clock.acc[key] = clock.acc.get(key, 0.0) + time.perf_counter() - t0
        setattr(owner, name, timed)

    def take(self):
        out, self.acc = self.acc, {}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline", default=None, help="a document this script wrote on the parent commit: embedded under 'parent'")
    ap.add_argument("--label", default="this")
    args = ap.parse_args()

    import torch
    from pypore_amd import engine, synth
    from pypore_amd.parsers import SpeedyStatSplit

    n = args.samples
    ctx = engine.context(0)
    d = synth.dwell_table(2024, n)
    lv = synth.LEVEL_COUNTS[np.arange(len(d)) % 5].astype(np.int32)
    a = ctx.synth_trace(n, 2024, np.cumsum(d), lv, dtype=torch.float32).cpu().numpy().astype(np.float64)
    b = np.rint(a / synth.QUANTUM)
    b *= Q_HEADER
    b += OFFSET
    inputs = {"a": lambda: a, "b": lambda: b, "c": lambda: torch.from_numpy(b).cuda()}

    def sync():
        torch.cuda.synchronize()

    clock = Clock()
    clock.wrap(engine, "_staged_upload", "upload")
    for name in ("grid_check", "grid_counts", "narrow_f64"):
        clock.wrap(engine.Context, name, "device")
    seen = {}

    def ingested(samples):
        sync()
        seen["kind"] = str(samples.tensor.dtype)

    clock.wrap(engine, "to_device", "ingest", after=ingested)    # (the parsers call it through the module: engine.to_device(...))

    doc = {"label": args.label, "samples": n, "runs": args.runs, "warmup": args.warmup, "unit": "s",
           "device": torch.cuda.get_device_name(0), "staged_float64_from": getattr(engine, "_STAGE_F64_MIN", None), "cases": {}}
    for case in args.cases:
        x = inputs[case]()
        sync()
        rows, err, n_seg, kind = [], None, None, None
        for r in range(args.warmup + args.runs):
            try:
                clock.take()
                sync()
                t0 = time.perf_counter()
                segs = SpeedyStatSplit(prior_segments_per_second=10.).parse(x)
                sync()
                total = time.perf_counter() - t0
                parts = clock.take()
                t_ingest = parts.get("ingest", 0.0)
                kind = seen.get("kind")
                n_seg = len(segs)
                del segs
            except ValueError as e:
                err = "ValueError: %s" % e
                break
            if r >= args.warmup:
                up, dev = parts.get("upload", 0.0), parts.get("device", 0.0)
                rows.append(dict(total=total, ingest=t_ingest, upload=up, device=dev, host=t_ingest - up - dev,
                                 segment=total - t_ingest))
        if err:
            doc["cases"][case] = {"error": err}
        else:
            doc["cases"][case] = {"segments": n_seg, "goes_up_as": kind,
                                  "median": {k: round(statistics.median(r_[k] for r_ in rows), 5) for k in rows[0]},
                                  "min_total": round(min(r_["total"] for r_ in rows), 5),
                                  "max_total": round(max(r_["total"] for r_ in rows), 5),
                                  "totals": [round(r_["total"], 5) for r_ in rows]}
        del x
        sys.stderr.write("[bench_ingest] %s %s: %s\n" % (args.label, case, json.dumps(doc["cases"][case])))
        sys.stderr.flush()
    if args.baseline:
        with open(args.baseline) as f:
            doc = {"this": doc, "parent": json.load(f)}
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
