"""Posterior decoding on the device: the workload of tools/bench_hmm_train.py (10 000 events of 50-400 segment means, the
54-position global profile HMM of 165 states).

Prints one JSON line, each time the median of --reps after one warm-up call, on the host's wall clock around the public
method (upload of the observations, the library call, the results brought back and unpacked):
  map_ms               Model.maximum_a_posteriori_batch: MAP states and their sums only, no dense matrix;
  forward_backward_ms  Model.forward_backward_batch with its dense outputs: the n x n_emit log posteriors of every event and
                       a states x states array of expected counts per event (gigabytes over 10 000 events: most of this
                       time is the copy to the host and the scatter, not the kernel);
  estep_ms             Model.expected_counts_batch in the same process: existing code that runs the same two passes, the
                       yardstick.
and, with HIP events around the library call alone (observations already on the device), the same three on the device:
map_device_ms (ps_hmm_posterior asked for d_map_state and d_map_logp), forward_backward_device_ms (d_post and d_counts_seq)
and estep_device_ms (ps_hmm_expect).

    python tools/bench_posterior.py [--events 10000] [--reps 5] [--out profiles/posterior_bench.json]
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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    from pypore_amd import engine
    model, means = O.profile_model(54)
    seqs = O.profile_events(means, a.events, lo=50, hi=400)
    off = np.concatenate(([0], np.cumsum([s.size for s in seqs]))).astype(np.int64)
    ctx = engine.context()
    obs = torch.from_numpy(np.concatenate(seqs)).cuda(ctx.device)
    cm = model._c_model()
    res = {"workload": "hmm_posterior", "events": a.events, "observations": int(off[-1]), "states": len(model.states),
           "emitting": int(model.flat["n_emit"]), "edges": len(model.edges), "silent_levels": int(model.flat["n_levels"]),
           "reps": a.reps}

    def wall(fn):
        fn()                                                   # warm-up (model upload, buffers)
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize(ctx.device)
            t = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t))
        return round(float(np.median(ms)), 2)

    def device(fn):
        fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return round(float(np.median(ms)), 2)

    res["estep_device_ms"] = device(lambda: ctx.hmm_expect(cm, obs, off))
    res["map_device_ms"] = device(lambda: ctx.hmm_posterior(cm, obs, off, want_post=False, want_map=True))
    res["forward_backward_device_ms"] = device(lambda: ctx.hmm_posterior(cm, obs, off, want_post=True, want_map=False,
                                                                        want_counts=True))
    res["map_over_estep_device"] = round(res["map_device_ms"] / res["estep_device_ms"], 3)
    res["estep_ms"] = wall(lambda: model.expected_counts_batch(seqs))
    res["map_ms"] = wall(lambda: model.maximum_a_posteriori_batch(seqs))
    res["forward_backward_ms"] = wall(lambda: model.forward_backward_batch(seqs))
    res["map_over_estep"] = round(res["map_ms"] / res["estep_ms"], 3)
    res["device"] = torch.cuda.get_device_name(ctx.device)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
