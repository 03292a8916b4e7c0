"""Mixture HMM states on the device: the 165-state profile of tests/hmm_oracle.py (profile_model(54), the model
tools/bench_hmm.py times) on its 10 000 events of 50-400 segments, five ways in one process:
    plain     normal match states, uniform inserts: the HmmDev kernels;
    mix2/8    every one of the 54 match states a MixtureDistribution of 2 / 8 normal components of the state's own std,
              spread around its mean, with unequal weights: the HmmDevM kernels (hmm_emit's component loop);
    kde2/8    the same densities as GaussianKernelDensity(points = the component means, bandwidth = the std, the same
              weights): the HmmDevK kernels, whose point loop does the same exp per point without the kind switch and
              without the component rows of the E-step.  This is the yardstick of the mixture rows.

Per model the device time per batch (HIP events around the library call, observations already on the device, median of
--reps after one warm-up call) of
    viterbi          ps_hmm_batch, paths included                         (Model.viterbi_batch)
    log_probability  ps_hmm_batch forward, no matrix kept                 (Model.log_probability_batch)
    expected_counts  ps_hmm_expect, component rows included for mix       (Model.expected_counts_batch)
    sample           ps_hmm_sample, as many walks as events, exact slots  (Model.sample_batch)
the ratios mix / kde at the same number of components and mix / plain, and a check of the timed answers on the first three
events: the mixture's log probabilities within 1e-12 of the kernel density's.  There is no target.  Prints one JSON line
and writes it to --out.

    python tools/bench_mixture.py [--events 10000] [--reps 5] [--out profiles/mixture_hmm_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS = ("viterbi", "log_probability", "expected_counts", "sample")


def profile_with(make, J, seed=5):
    """profile_model(54) with every match state's NormalDistribution(mean, std) replaced by make(points, std, weights):
    J points spread within 2 std of the mean."""
    import hmm_oracle as O
    model, means = O.profile_model(54)
    rng = np.random.default_rng(seed)
    for s in model.states[:model.flat["n_emit"]]:
        if s.name.startswith("M:"):
            mean, std = s.distribution.parameters
            s.distribution = make((mean + np.linspace(-2.0, 2.0, J) * std).tolist(), std, rng.uniform(0.5, 1.5, J).tolist())
    model.bake()
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_hmm_bench.json"))
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    from pypore_amd import _lib, engine
    from pypore_amd.hmm import GaussianKernelDensity, MixtureDistribution, NormalDistribution
    plain, means = O.profile_model(54)
    seqs = O.profile_events(means, a.events, lo=50, hi=400)
    mix = lambda pts, std, w: MixtureDistribution([NormalDistribution(p, std) for p in pts], w)      # noqa: E731
    kde = lambda pts, std, w: GaussianKernelDensity(pts, std, w)                                      # noqa: E731
    models = [("plain", plain)] + [("%s%d" % (name, J), profile_with(make, J)) for J in (2, 8) for name, make in (("mix", mix), ("kde", kde))]
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    ctx = engine.context()
    obs = torch.from_numpy(np.concatenate(seqs)).cuda(ctx.device)
    res = {"workload": "mixture_hmm", "events": a.events, "observations": int(off[-1]), "reps": a.reps, "models": {}}
    logp3 = {}
    for name, model in models:
        cm, tables = model._c_model(), model._sample_tables()["c"]
        f = model.flat
        row = {"states": int(f["n_states"]), "emitting": int(f["n_emit"]), "edges": len(model.edges),
               "mixture_components": model._n_mix, "kde_points": int(f["kde_pt"].size)}
        lens = ctx.hmm_sample(cm, tables, 1, 0, a.events)[3].cpu().numpy().astype(np.int64)     # the walks' exact lengths
        row["sampled_observations"] = int(lens.sum())
        calls = (("viterbi", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_VITERBI, obs, off)),
                 ("log_probability", lambda: ctx.hmm_batch(cm, _lib.PS_HMM_FORWARD, obs, off)),
                 ("expected_counts", lambda: ctx.hmm_expect(cm, obs, off, 3, mix_rows=model._n_mix)),
                 ("sample", lambda: ctx.hmm_sample(cm, tables, 1, 0, a.events, obs_slots=lens)))
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
    ratio = lambda x, y: {what: res["models"][x][what + "_ms"] / res["models"][y][what + "_ms"] for what in CALLS}    # noqa: E731
    for J in (2, 8):
        res["models"]["mix%d" % J]["ratio_to_kde"] = ratio("mix%d" % J, "kde%d" % J)
        res["models"]["mix%d" % J]["ratio_to_plain"] = ratio("mix%d" % J, "plain")
        res["models"]["kde%d" % J]["ratio_to_plain"] = ratio("kde%d" % J, "plain")
        err = np.abs(logp3["mix%d" % J] - logp3["kde%d" % J]) / np.maximum(1.0, np.abs(logp3["kde%d" % J]))
        res["check_mix%d_logp_within_1e-12_of_kde" % J] = bool(err.max() <= 1e-12)
    res["device"] = torch.cuda.get_device_name(ctx.device)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
