"""Vector HMM emissions on the device: the 165-state profile of tests/hmm_oracle.py (profile_model(54), the model
tools/bench_hmm.py times) on its 10 000 events of 50-400 segments, three ways in one process:
    plain     normal match states, uniform inserts: the univariate kernels (the yardstick);
    vector1   the same model forced through the vector type at D = 1 (every state wrapped as a one-component
              MultivariateDistribution): the same arithmetic through the lane loop over components;
    vector3   D = 3 (tests/multivariate_oracle.py profile3): a match scores (mean, std, duration) as normal, normal and
              log-normal, an insert as uniform, uniform and exponential; every event carries a std and a duration beside
              its means.

Per model the device time per batch (HIP events around the library call, observations already on the device, median of
--reps after one warm-up call) of
    viterbi               ps_hmm_batch, paths included              (Model.viterbi_batch)
    log_probability       ps_hmm_batch forward, no matrix kept      (Model.log_probability_batch)
    expected_counts       ps_hmm_expect                             (Model.expected_counts_batch)
    expected_transitions  ps_hmm_posterior, the counts alone        (Model.expected_transitions_batch)
their ratios to the plain model of the same run, and a check of the timed answers on the first three events: vector1's log
probabilities equal to the plain model's bit for bit.  There is no target.  Prints one JSON line and writes it to --out.

    python tools/bench_multivariate.py [--events 10000] [--reps 5] [--out profiles/multivariate_hmm_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS = ("viterbi", "log_probability", "expected_counts", "expected_transitions")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivariate_hmm_bench.json"))
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    import multivariate_oracle as MV
    from pypore_amd import _lib, engine
    plain, means = O.profile_model(54)
    vector3, _ = MV.profile3(54)
    seqs1 = O.profile_events(means, a.events, lo=50, hi=400)
    seqs3 = MV.profile3_events(means, a.events, lo=50, hi=400)
    models = [("plain", plain, seqs1), ("vector1", MV.wrapped(plain), seqs1), ("vector3", vector3, seqs3)]
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs1]))).astype(np.int64)
    ctx = engine.context()
    res = {"workload": "multivariate_hmm", "events": a.events, "observations": int(off[-1]), "reps": a.reps, "models": {}}
    logp3 = {}
    for name, model, seqs in models:
        obs = torch.from_numpy(np.concatenate([np.asarray(s).reshape(-1) for s in seqs])).cuda(ctx.device)
        cm = model._c_model()
        f = model.flat
        row = {"states": int(f["n_states"]), "emitting": int(f["n_emit"]), "n_dim": int(f["n_dim"]),
               "vector": bool(f["comp_kind"].size), "edges": len(model.edges)}
        calls = (("viterbi", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, obs, off)),
                 ("log_probability", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off)),
                 ("expected_counts", lambda: ctx.hmm_expect(cm, obs, off, model._stat_width)),
                 ("expected_transitions", lambda: ctx.hmm_posterior(cm, obs, off, want_post=False, want_map=False, want_counts=True)))
        for what, call in calls:
            call()                                                # warm-up (model upload, buffers)
            ms = []
            for _ in range(a.reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                t1.synchronize()
                ms.append(t0.elapsed_time(t1))
            row[what + "_ms"] = float(np.median(ms))
        logp3[name] = model.log_probability_batch(seqs[:3])
        res["models"][name] = row
    for name in ("vector1", "vector3"):
        res["models"][name]["ratio_to_plain"] = {
            what: res["models"][name][what + "_ms"] / res["models"]["plain"][what + "_ms"] for what in CALLS}
    res["check_vector1_logp_bits_equal_plain"] = bool(np.array_equal(logp3["vector1"], logp3["plain"]))
    res["device"] = torch.cuda.get_device_name(ctx.device)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
