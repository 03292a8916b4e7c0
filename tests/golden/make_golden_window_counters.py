#!/usr/bin/env python3
"""Records the call counters and the boundaries' SHA-256 of the cases of tests/test_window_counters.py, as the library of
the commit BEFORE a change to the window scan gives them: the test then holds the changed library to the same verdicts.

Run on the GPU, with the library of the commit to compare against (the parent of the change) built in the tree:

    python tests/golden/make_golden_window_counters.py

Every case runs three times: once on a context shared by all cases, as in the test, and twice on a fresh one. A counter that the library itself does not reproduce is dropped for that
case and named in the fixture; windows, candidates, tree_deferred and windows_screen may not be dropped (the suite relies on
them elsewhere), and neither may the boundaries.

Output (committed): tests/golden/window_counters.json.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import test_window_counters as twc        # noqa: E402
from pypore_amd import engine             # noqa: E402

RUNS = 3


def main():
    out = {}
    shared = engine.Context(0)             # run 0: one context for all cases in the test's order, as the test has it
    for name in twc.cases():
        runs = []
        for i in range(RUNS):
            ctx = shared if i == 0 and name != "wide_range" else engine.Context(0)
            try:
                _, events, bounds, tm = twc.run_case(ctx, name)
            finally:
                if ctx is not shared:
                    ctx.close()
            runs.append((twc.digest(events, bounds), {k: int(tm[k]) for k in twc.COUNTERS}, int(tm["wide_redo"])))
        assert len({r[0] for r in runs}) == 1, (name, "boundaries differ between runs")
        dropped = [k for k in twc.COUNTERS if len({r[1][k] for r in runs}) != 1]
        assert not set(dropped) & set(twc.REQUIRED), (name, dropped, [r[1] for r in runs])
        out[name] = dict(sha256=runs[0][0], counters={k: v for k, v in runs[0][1].items() if k not in dropped},
                         dropped=dropped, wide_redo=runs[0][2])
        print(name, out[name], flush=True)
    shared.close()
    with open(os.path.join(HERE, "window_counters.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_window_counters.py", "runs_per_case": RUNS, "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
