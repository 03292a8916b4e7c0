"""HMM sampling on the device (ps_hmm_sample): 10 000 walks to `end` of the 54-position global profile HMM of
tools/bench_hmm.py (165 states) and of the D = 3 profile of tools/bench_multivariate.py, with and without paths, beside
Viterbi on the sampled batch in the same process as the yardstick.

Prints one JSON line and writes it to --out: per model the device time per call (HIP events around the library call,
median of --reps) of
    sample_ms            observations only, slots of the exact lengths (one launch);
    sample_path_ms       observations and paths, slots of the exact lengths (one launch);
    sample_guess_ms      observations and paths from the default first guess of the slots (2 n_emit observations a walk),
                         buffers allocated inside the call, and a second call with slots of the exact lengths when some
                         walk did not fit -- what Model.sample_batch pays on the device;
    viterbi_ms           ps_hmm_batch, Viterbi with paths, on the sampled observations already on the device.

    python tools/bench_sample.py [--events 10000] [--reps 5] [--seed 1]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, reps):
    import torch
    call()                                                    # warm-up (model upload, buffers)
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    import multivariate_oracle as MV
    from pypore_amd import _lib, engine
    ctx = engine.context()
    res = {"workload": "hmm_sample", "events": a.events, "reps": a.reps, "seed": a.seed, "models": {}}
    for name, model in (("plain", O.profile_model(54)[0]), ("vector3", MV.profile3(54)[0])):
        cm, tables = model._c_model(), model._sample_tables()["c"]
        f = model.flat
        n = a.events
        _, _, _, lens, flags, (_, _, path_len) = ctx.hmm_sample(cm, tables, a.seed, 0, n, want_path=True)
        lens, path_len, flags = (t.cpu().numpy().astype(np.int64) for t in (lens, path_len, flags))
        _, obs, off, _, _, _ = ctx.hmm_sample(cm, tables, a.seed, 0, n, obs_slots=lens, retry=False)      # packed: exact slots
        row = {"states": int(f["n_states"]), "emitting": int(f["n_emit"]), "n_dim": int(f["n_dim"]), "edges": len(model.edges),
               "observations": int(lens.sum()), "longest": int(lens.max()), "path_states": int(path_len.sum()),
               "truncated": int(np.count_nonzero(flags))}
        row["sample_ms"] = timed(lambda: ctx.hmm_sample(cm, tables, a.seed, 0, n, obs_slots=lens, retry=False), a.reps)
        row["sample_path_ms"] = timed(lambda: ctx.hmm_sample(cm, tables, a.seed, 0, n, want_path=True, obs_slots=lens,
                                                             path_slots=path_len, retry=False), a.reps)
        row["sample_guess_ms"] = timed(lambda: ctx.hmm_sample(cm, tables, a.seed, 0, n, want_path=True), a.reps)
        flat_obs = obs.reshape(-1)
        row["viterbi_ms"] = timed(lambda: ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, flat_obs, off), a.reps)
        row["sample_path_over_viterbi"] = row["sample_path_ms"] / row["viterbi_ms"]
        # the timed batch is the model's: every sequence sampled to `end` is possible
        logp = ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, flat_obs, off)[0].cpu().numpy()
        row["check_all_possible"] = bool(np.all(np.isfinite(logp[flags == 0])))
        res["models"][name] = row
    res["device"] = torch.cuda.get_device_name(ctx.device)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
