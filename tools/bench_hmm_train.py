"""HMM training on the device: the workload of tools/bench_hmm.py (10 000 events of 50-400 segment means, the 54-position
global profile HMM of 165 states).

Prints one JSON line, each time the median of --reps: the Baum-Welch E-step (ps_hmm_expect: forward pass with the matrix
kept + fused backward-expectation kernel + reduction; HIP events around the library call, observations already on the
device), the forward pass alone for comparison (ps_hmm_batch, no matrix), and one full Model.train iteration on the host's
wall clock (E-step, M-step, re-upload of the model, and the forward pass that measures the improvement).

    python tools/bench_hmm_train.py [--events 10000] [--reps 5]
"""
import argparse
import copy
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
    res = {"workload": "hmm_train", "events": a.events, "observations": int(off[-1]), "states": len(model.states),
           "edges": len(model.edges), "silent_levels": int(model.flat["n_levels"])}

    def timed(fn):
        fn()                                                   # warm-up (model upload, buffers)
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return float(np.median(ms))

    res["forward_ms"] = timed(lambda: ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off))
    res["estep_ms"] = timed(lambda: ctx.hmm_expect(cm, obs, off))
    res["estep_over_forward"] = round(res["estep_ms"] / res["forward_ms"], 3)
    # one train iteration, wall clock, on copies of the model (each starts from the same parameters)
    wall = []
    for _ in range(a.reps):
        m = copy.deepcopy(O.profile_model(54)[0])
        m.expected_counts_batch(seqs[:1])                      # the context and the kernels warm
        t = time.perf_counter()
        m.train(seqs, max_iterations=1, verbose=False)
        wall.append(time.perf_counter() - t)
    # train(max_iterations=1) = E-step + M-step + re-upload + the forward pass of the new model: the iteration is that
    # less one forward pass (the next iteration's E-step starts with it)
    res["train_call_ms"] = round(1e3 * float(np.median(wall)), 2)
    res["train_iteration_ms"] = round(res["train_call_ms"] - res["forward_ms"], 2)
    res["device"] = torch.cuda.get_device_name(ctx.device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
