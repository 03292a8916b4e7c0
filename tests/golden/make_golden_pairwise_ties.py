"""Records the tie-rule goldens of the pairwise aligner: golden_pairwise_ties.npz + manifest_pairwise_ties.json.

    python tests/golden/make_golden_pairwise_ties.py /path/to/reference

The reference is loaded and run as make_golden_pairwise.py does it (its class sliced out in memory, nothing of it
written anywhere); only inputs, outputs and exception class names are stored.  The inputs come from
tests/pairwise_ties.py: integer alphabets of 2 and 4 letters, the periodic pairs and markers at the stripe seams.  Every
value is an integer, so the square of a difference is the same by pow and by product and every sum is exact: all
cases are grid cases and must equal tests/pairwise_oracle.py exactly, scores included.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_pairwise as M  # noqa: E402
import pairwise_ties as T  # noqa: E402


def build_cases():
    """(name, mode, penalty, min_length, maker(rng) -> (x, y))."""
    cases = []
    plan = {"global": [(2, 63, 64, -1), (4, 65, 64, -0.5), (2, 129, 129, 0), (4, 130, 130, -1)],
            "local": [(4, 63, 64, -1), (2, 65, 64, 0), (2, 129, 129, -0.5), (4, 130, 130, -1)],
            "repeated": [(2, 63, 64, -0.5), (4, 65, 64, -1), (4, 129, 129, 0), (2, 130, 130, -1), (4, 130, 130, -0.5)]}
    for mode, rows in plan.items():
        for k, m, n, pen in rows:
            cases.append(("letters%d_%s_%dx%d_pen%s" % (k, mode, m, n, pen), mode, pen, 2,
                          lambda rng, k=k, m=m, n=n: (T.letters(rng, m, k), T.letters(rng, n, k))))
    for mode in ("local", "repeated"):
        cases.append(("periodic_%s" % mode, mode, -1, 2, lambda rng: T.periodic(200)))
        cases.append(("periodic_transposed_%s" % mode, mode, -1, 2, lambda rng: T.periodic_transposed(200)))
    for mode in ("global", "local", "repeated"):
        cases.append(("marker_seams_%s" % mode, mode, -1, 2, lambda rng: T.marker_all_seams(rng, 130, 130)))
    return cases


def main(ref_root):
    cls = M.load_reference(ref_root)
    arrays, manifest = {}, {"cases": [], "note": "see make_golden_pairwise_ties.py; every case is integer-valued (exact)"}
    for k, (name, mode, penalty, min_length, maker) in enumerate(build_cases()):
        seed = 5000 + k
        x, y = maker(np.random.default_rng(seed))
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert max(x.size, y.size) <= 200
        ref = M.run_reference(cls, x, y, mode, penalty, min_length)
        mine = M.run_restatement(x, y, mode, float(penalty), min_length)
        assert M.same_structure(ref, mine) and all(p[0] == q[0] for p, q in zip(ref[1], mine[1])), \
            "%s: restatement != reference" % name
        arrays[name + "/x"], arrays[name + "/y"] = x, y
        arrays[name + "/scores"] = np.array([a[0] for a in ref[1]], dtype=np.float64)
        arrays[name + "/len"] = np.array([a[1].size for a in ref[1]], dtype=np.int64)
        arrays[name + "/xalign"] = np.concatenate([a[1] for a in ref[1]]) if ref[1] else np.zeros(0)
        arrays[name + "/yalign"] = np.concatenate([a[2] for a in ref[1]]) if ref[1] else np.zeros(0)
        manifest["cases"].append({"name": name, "mode": mode, "penalty": penalty, "min_length": min_length, "grid": True,
                                  "m": int(x.size), "n": int(y.size), "seed": seed, "raises": ref[0],
                                  "alignments": len(ref[1])})
        print(name, mode, x.size, y.size, ref[0] or "-", len(ref[1]))
    np.savez_compressed(os.path.join(HERE, "golden_pairwise_ties.npz"), **arrays)
    with open(os.path.join(HERE, "manifest_pairwise_ties.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
