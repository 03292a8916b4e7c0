"""Repeat splitter throughput (GPU box): writes profiles/trf_bench.json.

    python tools/bench_trf.py [--seqs 10000] [--reps 5] [--out profiles/trf_bench.json]

Workload: `--seqs` sequences of 50-400 segments (levels uniform in 20 .. 60 pA, stds 0.5 .. 1.5) with one to three planted
re-reads of 3-12 segments each, noisy (sigma 0.3), fixed seed; NaiveSplitter of every sequence in one library call
(ps_trf_split_batch, penalty -1, min_score 2).  Reported: milliseconds per batch (median, min, max of the repetitions after two
warm-up calls; the host clock around calls that end in a stream synchronise, uploads and result copies included), the
repeats found, and filled cells per second -- a sequence of n segments with r repeats fills its strict upper triangle
r + 1 times, n (n - 1) / 2 cells each.  The yardstick from the same run: pairwise_scores in local mode, all-vs-all over the
first 200 sequences' means (cells of the DP matrices per second).  Then one lone sequence of 1 000 segments, in a child
process under its own time limit (--lone-timeout seconds): one wave does all its work."""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--seqs", type=int, default=10000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trf_bench.json"))
ap.add_argument("--lone", type=int, default=0, help="(child) time one sequence of this many segments and print the entry")
ap.add_argument("--lone-timeout", type=float, default=240.0)
args = ap.parse_args()


def sequence(rng, n):
    """n segments: a strand read once with 1-3 planted noisy re-reads of 3-12 segments (the enzyme slipped back)."""
    extra = []
    for _ in range(int(rng.integers(1, 4))):
        extra.append(int(rng.integers(3, 13)))
    base = max(n - sum(extra), 2)
    m, s = list(rng.uniform(20.0, 60.0, base)), list(rng.uniform(0.5, 1.5, base))
    for k in extra:
        k = min(k, base)
        a = int(rng.integers(0, base - k + 1))
        m[a + k:a + k] = list(np.asarray(m[a:a + k]) + rng.normal(0.0, 0.3, k))
        s[a + k:a + k] = s[a:a + k]
    return np.array(m[:n], dtype=np.float64), np.array(s[:n], dtype=np.float64)


import torch
from pypore_amd import engine, alignment, _lib
engine.apply_env_defaults()
ctx = engine.context(0)
dev = torch.device("cuda", 0)


def timed(call):
    for _ in range(2):
        call()
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); call(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": args.reps}


def trf_entry(name, seqs):
    off = np.concatenate(([0], np.cumsum([m.size for m, _ in seqs]))).astype(np.int64)
    mean = torch.from_numpy(np.concatenate([m for m, _ in seqs])).to(dev)
    std = torch.from_numpy(np.concatenate([s for _, s in seqs])).to(dev)
    out = ctx.trf_split_batch(mean, std, off, -1.0, 2.0)
    count = out[6].astype(np.int64)
    slots = count.copy()                                     # the timed calls run once: their slots are the counts
    gpu = timed(lambda: ctx.trf_split_batch(mean, std, off, -1.0, 2.0, 0, slots))
    n = np.diff(off)
    cells = int(((count + 1) * (n * (n - 1) // 2)).sum())
    e = dict(name=name, sequences=len(seqs), segments=int(off[-1]), repeats=int(count.sum()), repeats_max=int(count.max()),
             filled_cells=cells, **gpu)
    e["gcells_per_s"] = cells / (gpu["ms_median"] * 1e-3) / 1e9
    return e


if args.lone:
    print(json.dumps(trf_entry("lone_sequence_%d" % args.lone, [sequence(np.random.default_rng(2025), args.lone)])), flush=True)
    sys.exit(0)

rng = np.random.default_rng(2024)
seqs = [sequence(rng, int(n)) for n in rng.integers(50, 401, args.seqs)]
results = [trf_entry("batch_%d_of_50_400" % args.seqs, seqs)]
print(json.dumps(results[-1]), flush=True)
# the yardstick: local-mode scores, all-vs-all over the first 200 sequences' means
sub = [m for m, _ in seqs[:200]]
flat, off = alignment._pack(sub)
t = torch.from_numpy(flat).to(dev)
gpu = timed(lambda: ctx.pairwise_scores(t, off, t, off, _lib.PS_PW_LOCAL, -1.0))
cells = float(np.diff(off).sum()) ** 2
e = dict(name="yardstick_pairwise_scores_local_200x200", cells=int(cells), **gpu)
e["gcells_per_s"] = cells / (gpu["ms_median"] * 1e-3) / 1e9
results.append(e)
print(json.dumps(e), flush=True)
# one lone sequence of 1 000 segments, in a child process under its own time limit
cmd = [sys.executable, os.path.abspath(__file__), "--lone", "1000", "--reps", str(args.reps)]
try:
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.lone_timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    e = json.loads(lines[-1]) if p.returncode == 0 and lines else {"name": "lone_sequence_1000", "error": "exit status %d" % p.returncode,
                                                                     "stderr": p.stderr[-400:]}
except subprocess.TimeoutExpired:
    e = {"name": "lone_sequence_1000", "error": "not finished within %g s" % args.lone_timeout}
results.append(e)
print(json.dumps(e), flush=True)
doc = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().ps_version().decode(),
       "command": "python tools/bench_trf.py --seqs %d --reps %d" % (args.seqs, args.reps),
       "timing": "host clock around calls that end in a stream synchronise (uploads of offsets and result copies included); "
                 "two warm-up calls, then `reps` timed ones; slots sized to the counts, so no call runs twice",
       "results": results}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(doc, open(args.out, "w"), indent=1)
