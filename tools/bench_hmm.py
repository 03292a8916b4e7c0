"""HMM decoding on the device (ps_hmm_batch): 10 000 events of 50-400 segment means against a 54-position global
profile HMM (match / insert / delete, 165 states, uniform insert emissions, like the reference tutorial's model).

Prints one JSON line: device time per batch (HIP events around the library call, observations already on the device,
median of --reps) for Viterbi (paths included) and for forward (log probabilities), and the test oracle's host time
(tests/hmm_oracle.py, numpy) measured on the first --oracle-events events and scaled to the batch by observation count.

With --small-calls N also the host's clock around a call where host time dominates: the forward pass of one sequence of two
observations (argument checks, the model's check and packing, one upload, one launch, one synchronisation), median of N calls
in microseconds.

    python tools/bench_hmm.py [--events 10000] [--reps 5] [--oracle-events 40] [--small-calls 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-events", type=int, default=40)
    ap.add_argument("--small-calls", type=int, default=0)
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    from pypore_amd import _lib, engine
    model, means = O.profile_model(54)
    seqs = O.profile_events(means, a.events, lo=50, hi=400)
    off = np.concatenate(([0], np.cumsum([s.size for s in seqs]))).astype(np.int64)
    ctx = engine.context()
    obs = torch.from_numpy(np.concatenate(seqs)).cuda(ctx.device)
    cm = model._c_model()
    res = {"workload": "hmm", "events": a.events, "observations": int(off[-1]), "states": len(model.states),
           "silent_levels": int(model.flat["n_levels"])}
    for name, mode in (("viterbi", _lib.PS_HMM_VITERBI), ("forward", _lib.PS_HMM_FORWARD)):
        ctx.hmm_batch(cm, mode, obs, off)                     # warm-up (model upload, buffers)
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ctx.hmm_batch(cm, mode, obs, off)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        res[name + "_ms"] = float(np.median(ms))
    if a.small_calls:
        off2 = np.array([0, 2], np.int64)
        us = []
        for i in range(20 + a.small_calls):                   # (the first 20: warm-up)
            t = time.perf_counter()
            ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off2)
            us.append((time.perf_counter() - t) * 1e6)
        res.update({"small_call_observations": 2, "small_call_host_us": float(np.median(us[20:]))})
    # a check that the timed batch is the right answer, on a few events
    c = O.Compiled(model)
    vit = model.viterbi_batch(seqs[:3])
    res["check_viterbi_vs_oracle"] = all(abs(v[0] - O.viterbi(c, s)[0]) <= 1e-9 * abs(v[0]) for v, s in zip(vit, seqs[:3]))
    k = min(a.oracle_events, a.events)
    t = time.perf_counter()
    for s in seqs[:k]:
        O.viterbi(c, s)
    tv = time.perf_counter() - t
    t = time.perf_counter()
    for s in seqs[:k]:
        O.log_probability(c, s)
    tf = time.perf_counter() - t
    scale = off[-1] / max(1, off[k])
    res.update({"oracle_sample_events": k, "oracle_viterbi_host_s": round(tv * scale, 1),
                "oracle_forward_host_s": round(tf * scale, 1), "device": torch.cuda.get_device_name(ctx.device)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
