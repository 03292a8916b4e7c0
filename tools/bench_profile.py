"""Kernel-density profile HMMs on the device (GPU box): writes profiles/profile_bench.json.

    python tools/bench_profile.py [--events 10000] [--reps 5] [--out profiles/profile_bench.json]

The batch is tests/hmm_oracle.py profile_events' 10 000 events of 50-400 segment means.  The profile is 54 columns built
by ProfileAligner._build_global (165 states: 54 kernel-density match states, 55 uniform inserts, 54 silent deletes) from
MSAs of P = 1, 8 and 32 rows, so a match state has P points.  Per P: viterbi_batch, log_probability_batch and one
expected_counts_batch, and beside them, in the same run, the 165-state normal profile of tools/bench_hmm.py with the
ratio kernel density / normal.  Then profile_align_batch end to end (model, launch, paths to the host, the gaps put into
a master copy per slave) and one MultipleSequenceAligner.iterative_alignment of 20 sequences.

Every entry: milliseconds per call -- median [min, max] of --reps after two warm-up calls, the host clock around calls
that end in a stream synchronise, uploads and result copies included."""
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
    ap.add_argument("--align-events", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_bench.json"))
    a = ap.parse_args()
    import torch
    import hmm_oracle as O
    import profile_oracle as P
    from pypore_amd import _lib, alignment, engine

    def timed(call):
        for _ in range(2):
            call()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": a.reps}

    def passes(model, seqs):
        return {"viterbi": timed(lambda: model.viterbi_batch(seqs)),
                "log_probability": timed(lambda: model.log_probability_batch(seqs)),
                "expected_counts": timed(lambda: model.expected_counts_batch(seqs))}

    normal, means = O.profile_model(54)
    seqs = O.profile_events(means, a.events, lo=50, hi=400)
    ctx = engine.context()
    doc = {"workload": "profile", "device": torch.cuda.get_device_name(ctx.device), "library": _lib.lib().ps_version().decode(),
           "events": a.events, "observations": int(sum(s.size for s in seqs)), "states": len(normal.states), "profiles": []}
    rng = np.random.default_rng(0)
    for rows in (1, 8, 32):
        msa = [[float(np.clip(m + rng.normal(0, 1.2), 0.5, 89.5)) for m in means] for _ in range(rows)]
        pa = alignment.ProfileAligner(msa, [1.0])
        kde = pa._build_global(pa.master, 0, 90)
        assert len(kde.states) == len(normal.states) == 165
        entry = {"points_per_match_state": rows, "kernel_density": passes(kde, seqs), "normal": passes(normal, seqs)}
        entry["ratio_to_normal"] = {k: entry["kernel_density"][k]["ms_median"] / entry["normal"][k]["ms_median"]
                                    for k in entry["normal"]}
        c = P.Compiled(kde)                                    # the timed batch is the right answer, on a few events
        entry["check_viterbi_vs_oracle"] = all(abs(v[0] - O.viterbi(c, s)[0]) <= 1e-9 * abs(v[0])
                                               for v, s in zip(kde.viterbi_batch(seqs[:2]), seqs[:2]))
        doc["profiles"].append(entry)
        print(json.dumps(entry), flush=True)
    slaves = [[float(np.clip(v, 0.5, 89.5)) for v in s] for s in seqs[:a.align_events]]
    msa8 = [[float(np.clip(m + rng.normal(0, 1.2), 0.5, 89.5)) for m in means] for _ in range(8)]
    doc["profile_align_batch"] = dict(timed(lambda: alignment.profile_align_batch([list(r) for r in msa8], [list(s) for s in slaves],
                                                                                 'global', 0, 90)),
                                      slaves=len(slaves), rows=8, columns=54)
    _, twenty = P.derived_sequences(np.random.default_rng(1), 30, 20)
    doc["iterative_alignment_20_sequences"] = dict(
        timed(lambda: alignment.MultipleSequenceAligner([list(s) for s in twenty]).iterative_alignment(max_iterations=2)),
        sequences=20, template_columns=30, max_iterations=2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
