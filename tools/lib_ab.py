#!/usr/bin/env python3
"""A/B of two builds of libporeseg.so on the bench's headline command, by the protocol of profiles/short_chain_ab.json: rounds of
three FRESH processes, (parent, new, parent) and (new, parent, parent) alternating; the paired difference of a round is its first
parent run minus its new run, parent - parent its two parent runs.  Criterion: the mean paired gain is positive, at least three
standard errors, and larger than the s.d. of parent - parent of the same session.

usage: lib_ab.py --parent pypore_amd/libporeseg_parent.so --out FILE [--rounds 16] [--queues N] [-- bench arguments]
  --parent   the parent commit's library (the new one is the tree's own pypore_amd/libporeseg.so)
  --queues   export GPU_MAX_HW_QUEUES=N to the runs (default: what this process was given)
Every run has a time limit of its own; the first run that fails ends the session (what was measured so far is in FILE)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flag(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stats(v):
    n = len(v)
    m = sum(v) / n
    sd = (sum((x - m) ** 2 for x in v) / (n - 1)) ** 0.5 if n > 1 else 0.0
    return {"mean": round(m, 5), "sd": round(sd, 5), "se": round(sd / n ** 0.5, 5), "min": min(v), "max": max(v), "n": n,
            "median": sorted(v)[n // 2] if n % 2 else round((sorted(v)[n // 2 - 1] + sorted(v)[n // 2]) / 2, 5)}


def main():
    parent = os.path.abspath(flag("--parent", os.path.join(ROOT, "pypore_amd", "libporeseg_parent.so")))
    out = flag("--out", None)
    rounds = int(flag("--rounds", 16))
    queues = flag("--queues", None)
    bench_args = sys.argv[sys.argv.index("--") + 1:] if "--" in sys.argv else []
    env = dict(os.environ)
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    env.pop("PORESEG_LIB", None)
    doc = {"command": " ".join(["python", "bench.py"] + bench_args), "pairs": [], "gpu_max_hw_queues_seen": []}

    def run(which):
        e = dict(env)
        if which == "parent":
            e["PORESEG_LIB"] = parent
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bench_args, env=e, cwd=ROOT, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit("bench.py (%s) ended with status %d: the session ends here" % (which, r.returncode))
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["host"]["library"] == (os.path.basename(parent) if which == "parent" else "libporeseg.so"), d["host"]["library"]
        q = d["host"]["gpu_max_hw_queues"]
        if q not in doc["gpu_max_hw_queues_seen"]:
            doc["gpu_max_hw_queues_seen"].append(q)
        return d["ms_per_step"]

    for r in range(rounds):
        order = ["parent", "new", "parent"] if r % 2 == 0 else ["new", "parent", "parent"]
        got = [run(w) for w in order]
        pa = [g for g, w in zip(got, order) if w == "parent"]
        doc["pairs"].append({"round": r, "order": order, "parent": pa[0], "new": got[order.index("new")], "parent_again": pa[1]})
        p = doc["pairs"]
        doc["parent_ms"] = stats([x["parent"] for x in p])
        doc["new_ms"] = stats([x["new"] for x in p])
        doc["parent_minus_new_ms"] = stats([round(x["parent"] - x["new"], 5) for x in p])
        doc["parent_minus_parent_ms"] = stats([round(x["parent"] - x["parent_again"], 5) for x in p])
        if out:
            with open(out, "w") as f:
                json.dump(doc, f, indent=1)
        print("round %d %s: %s" % (r, order, got), flush=True)
    g, pp = doc["parent_minus_new_ms"], doc["parent_minus_parent_ms"]
    print("parent %.4f new %.4f | gain %.4f +- %.4f (%.1f s.e.) | parent - parent s.d. %.4f | criterion %s"
          % (doc["parent_ms"]["mean"], doc["new_ms"]["mean"], g["mean"], g["se"], g["mean"] / g["se"] if g["se"] else 0.0, pp["sd"],
             "met" if g["mean"] > 0 and g["mean"] >= 3 * g["se"] and g["mean"] > pp["sd"] else "NOT met"))


if __name__ == "__main__":
    main()
