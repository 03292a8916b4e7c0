"""Pairwise aligner throughput (GPU box): writes profiles/pairwise_bench.json.

    python tools/bench_pairwise.py [--seqs 2000] [--reps 5] [--out profiles/pairwise_bench.json]

Three workloads: all-vs-all scores (ps_pairwise_scores) of `--seqs` sequences of 50-400 means in global and local mode, a
batch of 4 096 tracebacks at 100 x 100 (ps_pairwise_batch, each mode), one 1 000 x 1 000 local repeated alignment.  Every
entry: milliseconds per call (median, min, max of the repetitions after two warm-up calls; the host clock around calls
that end in a stream synchronise, uploads and result copies included) and Gcells/s = cells of the DP matrices / median.
Beside it the Python restatement (tests/pairwise_oracle.py, one host core) on a subsample that finishes in seconds; its
Gcells/s are per cell of that subsample, i.e. extrapolated per cell to the whole workload."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import pairwise_oracle as O
from pypore_amd import engine, alignment, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--seqs", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_bench.json"))
args = ap.parse_args()
engine.apply_env_defaults()
ctx = engine.context(0)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2024)


def timed(call):
    for _ in range(2):
        call()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); call(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": args.reps}


def entry(name, cells, gpu, host_cells, host_s, note):
    e = dict(name=name, cells=int(cells), **gpu)
    e["gcells_per_s"] = cells / (gpu["ms_median"] * 1e-3) / 1e9
    e["restatement"] = {"cells": int(host_cells), "seconds": host_s, "gcells_per_s_extrapolated_per_cell": host_cells / host_s / 1e9,
                        "note": note}
    print(json.dumps(e), flush=True)
    return e


results = []
# 1. all-vs-all scores
seqs = [np.round(rng.uniform(20, 60, int(n)) * 100) / 100 for n in rng.integers(50, 401, args.seqs)]
flat, off = alignment._pack(seqs)
t = torch.from_numpy(flat).to(dev)
lens = np.diff(off).astype(np.float64)
cells = lens.sum() ** 2
for mode, name in ((_lib.PS_PW_GLOBAL, "global"), (_lib.PS_PW_LOCAL, "local")):
    gpu = timed(lambda: ctx.pairwise_scores(t, off, t, off, mode, -1.0))
    sub = [(seqs[a], seqs[b]) for a in range(6) for b in range(6)]
    t0 = time.perf_counter()
    for x, y in sub:
        O.score_only(x, y, mode, -1.0)
    results.append(entry("all_vs_all_scores_%s_%d" % (name, args.seqs), cells, gpu, sum(len(x) * len(y) for x, y in sub),
                         time.perf_counter() - t0, "36 of the pairs"))
# 2. 4 096 tracebacks at 100 x 100
xs = [np.round(rng.uniform(20, 40, 100) * 100) / 100 for _ in range(4096)]
pairs = [(x, np.round((x + rng.normal(0, 0.4, 100)) * 100) / 100) for x in xs]
fa, oa = alignment._pack([p[0] for p in pairs]); fb, ob = alignment._pack([p[1] for p in pairs])
ta, tb = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev)
idx = np.arange(4096, dtype=np.int32)
for mode, name in ((0, "global"), (1, "local"), (2, "local_repeated")):
    gpu = timed(lambda: ctx.pairwise_batch(ta, oa, tb, ob, idx, idx, mode, -1.0, 2))
    t0 = time.perf_counter()
    for x, y in pairs[:16]:
        O.align(x, y, mode, -1.0, 2)
    results.append(entry("traceback_batch_4096_100x100_%s" % name, 4096 * 100 * 100, gpu, 16 * 100 * 100, time.perf_counter() - t0,
                         "16 of the pairs"))
# 3. one 1 000 x 1 000 local repeated alignment (a self-alignment: the mirrored writes are in bounds)
x = np.round(rng.uniform(20, 200, 1000) * 100) / 100
fa, oa = alignment._pack([x])
ta = torch.from_numpy(fa).to(dev)
one = np.zeros(1, np.int32)
gpu = timed(lambda: ctx.pairwise_batch(ta, oa, ta, oa, one, one, 2, -1.0, 2))
n_aln = int(ctx.pairwise_batch(ta, oa, ta, oa, one, one, 2, -1.0, 2)[9][0])
t0 = time.perf_counter()
O.align(x[:300], x[:300], O.REPEATED, -1.0, 2)
e = entry("local_repeated_1000x1000", 1000 * 1000, gpu, 300 * 300, time.perf_counter() - t0, "the first 300 x 300 of the pair")
e["alignments"] = n_aln
results.append(e)
doc = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().ps_version().decode(),
       "command": "python tools/bench_pairwise.py --seqs %d --reps %d" % (args.seqs, args.reps),
       "timing": "host clock around calls that end in a stream synchronise (uploads of offsets and result copies included); "
                 "two warm-up calls, then `reps` timed ones",
       "restatement_note": "tests/pairwise_oracle.py on one host core, on the subsample named per entry; its Gcells/s hold per "
                           "cell of that subsample (extrapolated per cell, not measured on the whole workload)",
       "results": results}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(doc, open(args.out, "w"), indent=1)
