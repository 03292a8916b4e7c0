#!/usr/bin/env python3
"""The sweep behind ps_pool_plan's table (include/poreseg.h): the bench's headline job -- T contexts, each on
its own 1e8-sample fp32 trace -- under explicit k0_waves x k0_admit settings, interleaved inside ONE process.  Every round
visits every setting (the order turns round by round) and times K steps and the driver's 20 with a host clock around runs
that end in a device synchronise; the per-call sequence (first to last device event of a call) is summed beside it.
Explicit options win over what "shared_device" plans, so the same script measures a library from before the plan.

usage: pool_plan_sweep.py [--T 16] [--K 100] [--rounds 6] [--waves 0,1,2,3,4] [--admit 0,2,3] [--plan] [--out FILE]
  --plan   also a setting without any override: the library's own plan for this process
The process runs on the hardware queues its caller gives it (GPU_MAX_HW_QUEUES; unset: HIP's 4) and records the value."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np    # noqa: E402
import torch          # noqa: E402
from pypore_amd import _lib, engine, synth    # noqa: E402


def flag(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


T, K, ROUNDS = int(flag("--T", 16)), int(flag("--K", 100)), int(flag("--rounds", 6))
WAVES = [int(v) for v in flag("--waves", "0,1,2,3,4").split(",")]
ADMIT = [int(v) for v in flag("--admit", "0,2,3").split(",")]
OUT = flag("--out", None)
settings = [{"k0_waves": w, "k0_admit": a} for w in WAVES for a in ADMIT]
if "--plan" in sys.argv:
    settings.append({})

n = 100_000_000
params = _lib.split_params(min_width=100, max_width=1000000, window_width=10000, prior_segments_per_second=10., sampling_freq=1e5)
pool = engine.StreamPool(0, T)
ctx0 = pool.contexts[0]
traces = []
for t in range(T):
    sd = 2024 + 1000 * t
    d = synth.dwell_table(sd, n)
    ends = np.cumsum(d)
    lv = synth.LEVEL_COUNTS[np.arange(len(d)) % 5].astype(np.int32)
    traces.append(ctx0.synth_trace(n, sd, ends, lv, dtype=torch.float32))
ev_off = np.array([0, n], dtype=np.int64)
outs = [torch.empty(n // 100 + 1, dtype=torch.int32, device="cuda") for _ in range(T)]
seq = [0.0] * T


def job(cx, k, t):
    r = cx.segment_batch(traces[t], ev_off, params, synth.QUANTUM, want_stats=False, out=outs[t])[0].numel()
    seq[t] += cx.seq_ms()
    return r


import gc    # noqa: E402
gc.collect()
gc.freeze()
ref = pool.run(4 * T, job)[-T:]


def measure(setting, steps):
    pool.overrides = dict(setting)
    pool._shared_now.clear()
    pool.run(T, job)
    for t in range(T):
        seq[t] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = pool.run(steps, job)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(r[k] == ref[k % T] for k in range(len(r))), "boundary counts changed"
    return dt / steps * 1e3, sum(seq) / steps


res = [dict(setting=s, ms=[], seq_ms=[], ms20=[]) for s in settings]
for p in range(ROUNDS):
    order = list(range(len(settings)))
    order = order[p % len(order):] + order[:p % len(order)]
    if p % 2:
        order.reverse()
    for i in order:
        a, b = measure(settings[i], K)
        res[i]["ms"].append(round(a, 4))
        res[i]["seq_ms"].append(round(b, 4))
        res[i]["ms20"].append(round(measure(settings[i], 20)[0], 4))
for r in res:
    for k in ("ms", "seq_ms", "ms20"):
        v = np.array(r[k])
        r[k + "_mean"], r[k + "_median"], r[k + "_sd"] = round(float(v.mean()), 4), round(float(np.median(v)), 4), round(float(v.std(ddof=1)) if len(v) > 1 else 0.0, 4)
    print("%-32s %d steps: mean %.4f median %.4f sd %.4f | sequence %.4f | 20 steps: mean %.4f median %.4f sd %.4f"
          % (r["setting"] or "library's plan", K, r["ms_mean"], r["ms_median"], r["ms_sd"], r["seq_ms_mean"], r["ms20_mean"], r["ms20_median"], r["ms20_sd"]))
doc = {"what": "tools/pool_plan_sweep.py: ms per step of %d contexts on their own 1e8-sample traces, %d rounds, every setting in every round" % (T, ROUNDS),
       "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "contexts": T, "steps": K, "rounds": ROUNDS,
       "library": os.path.basename(_lib.LIB_PATH), "settings": res}
if OUT:
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
