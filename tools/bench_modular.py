"""The reference's modular profile HMM on the device: the 54-position Phi29 profile of ModularProfileModel
(Phi29GlobalAlignmentModule; pypore_amd.hmm) baked unmerged, with merge='partial' and with merge='all', beside the
hand-written 165-state profile of tests/hmm_oracle.py (profile_model(54), the model tools/bench_hmm.py times) as the
yardstick.  The modular models take the yardstick's match distributions, so the same 10 000 events of 50-400 segment means
(hmm_oracle.profile_events) fit all four.

Per model: states, emitting states, silent levels, edges, and the device time per batch (HIP events around the library
call, observations already on the device, median of --reps after one warm-up call) of
    viterbi               ps_hmm_batch, paths included              (Model.viterbi_batch)
    log_probability       ps_hmm_batch forward, no matrix kept      (Model.log_probability_batch)
    expected_counts       ps_hmm_expect                             (Model.expected_counts_batch)
    expected_transitions  ps_hmm_posterior, the counts alone        (Model.expected_transitions_batch)
and a check of the timed answers on the first three events: the merged models' log probabilities against the unmerged
model's (1e-12 relative).  There is no target.  Prints one JSON line and writes it to --out.

    python tools/bench_modular.py [--events 10000] [--reps 5] [--out profiles/modular_hmm_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modular_hmm_bench.json"))
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    from pypore_amd import _lib, engine
    from pypore_amd.hmm import ModularProfileModel, Phi29GlobalAlignmentModule, UniformDistribution
    yardstick, means = O.profile_model(54)
    match = {s.name: s.distribution for s in yardstick.states if s.name.startswith("M:")}
    profile = [match["M:%d" % (i + 1)] for i in range(54)]
    models = [("profile_model", yardstick)]
    for merge in (None, "partial", "all"):
        models.append(("modular_" + (merge or "unmerged"),
                       ModularProfileModel(Phi29GlobalAlignmentModule, profile, "Epigenetics-54", UniformDistribution(0, 90), merge=merge)))
    seqs = O.profile_events(means, a.events, lo=50, hi=400)
    off = np.concatenate(([0], np.cumsum([s.size for s in seqs]))).astype(np.int64)
    ctx = engine.context()
    obs = torch.from_numpy(np.concatenate(seqs)).cuda(ctx.device)
    res = {"workload": "modular_hmm", "events": a.events, "observations": int(off[-1]), "reps": a.reps, "models": {}}
    logp3 = {}
    for name, model in models:
        cm = model._c_model()
        f = model.flat
        row = {"states": int(f["n_states"]), "emitting": int(f["n_emit"]), "silent_levels": int(f["n_levels"]), "edges": len(model.edges)}
        calls = (("viterbi", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, obs, off)),
                 ("log_probability", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off)),
                 ("expected_counts", lambda: ctx.hmm_expect(cm, obs, off)),
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
    base = logp3["modular_unmerged"]
    res["check_merged_logp_vs_unmerged"] = bool(all(
        np.all(np.abs(logp3[k] - base) <= 1e-12 * np.maximum(1.0, np.abs(base))) for k in ("modular_partial", "modular_all")))
    res["device"] = torch.cuda.get_device_name(ctx.device)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
