"""The StatSplit cases: inputs from pypore_amd.synth, parameters, and the (splitter, use_log) modes each one runs in.
tests/golden/make_golden_statsplit.py records the reference's boundaries for every (case, mode); the host and GPU tests
read them back (golden key: "<case>/<splitter>/<log|var>").

gen: kind "step" (step_counts: n, dwell, seed), "random_dwell" (n, seed, lo, hi), "palindrome" (n, a, seed); `ramp`: an exact
ramp of that many 2**-10 pA per sample is added (a power of two times a small integer: exact in float64) -- the slanted
splitter's ground.  par: min_width, max_width, window_width, min_gain_per_sample.  start / end: StatSplit.parse's.
"""
import os

import numpy as np

from pypore_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
NT = 256                                   # threads of a recursion workgroup (seg_statsplit.hpp: SS_NT)
ALL = [("stepwise", True), ("stepwise", False), ("slanted", True), ("slanted", False)]
STEP = [("stepwise", True), ("stepwise", False)]
VAR = [("stepwise", False), ("slanted", False)]


def _par(mw, maxw, W, g):
    return dict(min_width=mw, max_width=maxw, window_width=W, min_gain_per_sample=g)


def _one_window(name, cands, mw=30):
    """An event whose first window [0, W) has exactly `cands` candidates, a step inside it."""
    W = 2 * mw + cands - 1
    return dict(name=name, gen=dict(kind="step", n=W + mw + 7, dwell=mw + cands // 2, seed=40 + cands % 17),
                par=_par(mw, 100000, W, 0.03), modes=ALL)


CASES = [
    dict(name="steps", gen=dict(kind="step", n=3000, dwell=600, seed=11), par=_par(50, 100000, 500, 0.03), modes=ALL),
    dict(name="steps_ramp", gen=dict(kind="step", n=2400, dwell=500, seed=12, ramp=3), par=_par(40, 100000, 400, 0.03), modes=ALL),
    dict(name="dwell", gen=dict(kind="random_dwell", n=4000, seed=13, lo=200, hi=900), par=_par(40, 100000, 400, 0.03), modes=ALL),
    dict(name="dwell_ramp", gen=dict(kind="random_dwell", n=3000, seed=14, lo=150, hi=700, ramp=-5), par=_par(30, 100000, 300, 0.05), modes=ALL),
    dict(name="dwell_maxw", gen=dict(kind="random_dwell", n=3000, seed=15, lo=100, hi=500), par=_par(25, 350, 250, 0.2), modes=ALL),
    dict(name="dwell_odd", gen=dict(kind="random_dwell", n=2777, seed=16, lo=90, hi=400), par=_par(17, 100000, 173, 0.04), modes=ALL),
    # exact ties: the two steps of a palindrome are equal gains of the one window that spans it (use_log=False: no logarithm
    # between the sums and the comparison); the lowest index wins
    dict(name="palindrome", gen=dict(kind="palindrome", n=2000, a=600, seed=21), par=_par(100, 100000, 4000, 0.03), modes=VAR),
    dict(name="palindrome_odd", gen=dict(kind="palindrome", n=1501, a=333, seed=22), par=_par(50, 100000, 3000, 0.03), modes=VAR),
    # ... and here it shows in the result: the middle level is narrower than min_width, so whichever step is taken first
    # puts the other one out of every later window's candidates -- the golden holds a = 950, not n - a = 1050
    dict(name="palindrome_narrow", gen=dict(kind="palindrome", n=2000, a=950, seed=20), par=_par(150, 100000, 4000, 0.03), modes=VAR),
    # forced splits on a flat stretch (one level, a threshold no noise reaches): in the loop (a window starts beyond
    # start + max_width) and after it (one window, nothing found, longer than max_width)
    dict(name="flat_inloop", gen=dict(kind="step", n=3000, dwell=5000, seed=23), par=_par(20, 300, 200, 50.0), modes=ALL),
    dict(name="flat_after", gen=dict(kind="step", n=1000, dwell=5000, seed=24), par=_par(20, 300, 2000, 50.0), modes=ALL),
    dict(name="flat_after_tail", gen=dict(kind="step", n=630, dwell=5000, seed=25), par=_par(20, 300, 2000, 50.0), modes=ALL),
    dict(name="maxw_plus_one", gen=dict(kind="step", n=21, dwell=5000, seed=26), par=_par(20, 20, 40, 50.0), modes=ALL),
    dict(name="deepest", gen=dict(kind="step", n=200, dwell=40, seed=27), par=_par(1, 1, 2, 0.03), modes=VAR),
    dict(name="mw1", gen=dict(kind="step", n=300, dwell=60, seed=28), par=_par(1, 50, 20, 0.03), modes=VAR),
    # window sizes: W = 2 mw -- every window has exactly one candidate; an event of 2 mw - 1 and one of 2 mw samples
    # (no window: ps < end - 2 mw never holds)
    dict(name="w_eq_2mw", gen=dict(kind="step", n=400, dwell=100, seed=29), par=_par(50, 100000, 100, 0.03), modes=ALL),
    dict(name="short_2mw_m1", gen=dict(kind="step", n=99, dwell=50, seed=30), par=_par(50, 100000, 100, 0.03), modes=ALL),
    dict(name="short_2mw", gen=dict(kind="step", n=100, dwell=50, seed=31), par=_par(50, 100000, 100, 0.03), modes=ALL),
    dict(name="short_2mw_p1", gen=dict(kind="step", n=101, dwell=50, seed=32), par=_par(50, 100000, 100, 0.03), modes=ALL),
    # candidate counts around the workgroup size
    _one_window("cand_1", 1), _one_window("cand_nt_m1", NT - 1), _one_window("cand_nt", NT), _one_window("cand_nt_p1", NT + 1),
    _one_window("cand_strides", 3 * NT + 5),
    # sub-ranges (stepwise only: the slanted splitter needs end == len)
    dict(name="sub_start", gen=dict(kind="random_dwell", n=3000, seed=33, lo=150, hi=600), par=_par(30, 100000, 300, 0.03), modes=STEP,
         start=517),
    dict(name="sub_end", gen=dict(kind="random_dwell", n=3000, seed=34, lo=150, hi=600), par=_par(30, 100000, 300, 0.03), modes=STEP,
         end=2345),
    dict(name="sub_both", gen=dict(kind="random_dwell", n=3000, seed=35, lo=150, hi=600), par=_par(30, 100000, 300, 0.03), modes=STEP,
         start=400, end=2600),
    dict(name="sub_negative", gen=dict(kind="random_dwell", n=3000, seed=36, lo=150, hi=600), par=_par(30, 100000, 300, 0.03),
         modes=STEP, start=-2500, end=-301),
    dict(name="sub_slanted_start", gen=dict(kind="random_dwell", n=2500, seed=37, lo=150, hi=600, ramp=2), par=_par(30, 100000, 300, 0.03),
         modes=[("slanted", False), ("slanted", True)], start=433),
]
# Large t: 2**24 + 3000 samples, segmented from 2**24 on -- sample indices no float32 holds.  The head is a 4096-sample
# step signal tiled 4096 times, the tail 3000 fresh samples; the ramp (2**-20 pA per sample) keeps every value exact.
BIG_HEAD = 1 << 24
BIG = dict(name="big_t", gen=dict(kind="big", n=BIG_HEAD + 3000, seed=38, ramp20=3), par=_par(30, 100000, 300, 0.03),
           modes=[("slanted", False), ("stepwise", False)], start=BIG_HEAD)
CASES_ALL = CASES + [BIG]
BY_NAME = {c["name"]: c for c in CASES_ALL}


def key(case, splitter, use_log):
    return "%s/%s/%s" % (case["name"], splitter, "log" if use_log else "var")


def runs(cases=None):
    """Every (case, splitter, use_log) of the small cases (or of `cases`)."""
    return [(c, s, lg) for c in (CASES if cases is None else cases) for s, lg in c["modes"]]


def run_ids(cases=None):
    return [key(c, s, lg) for c, s, lg in runs(cases)]


_inputs = {}


def build(case):
    """float64 pA of a case (cached; callers must not write to it)."""
    x = _inputs.get(case["name"])
    if x is None:
        g = case["gen"]
        if g["kind"] == "big":
            head = np.tile(synth.step_counts(4096, 700, g["seed"]), BIG_HEAD // 4096)
            k = np.concatenate((head, synth.random_dwell_counts(g["n"] - BIG_HEAD, g["seed"] + 1, 150, 600)))
        elif g["kind"] == "step":
            k = synth.step_counts(g["n"], g["dwell"], g["seed"])
        elif g["kind"] == "random_dwell":
            k = synth.random_dwell_counts(g["n"], g["seed"], g["lo"], g["hi"])
        elif g["kind"] == "palindrome":
            k = synth.palindrome_counts(g["n"], g["a"], g["seed"])
        else:
            raise ValueError(g["kind"])
        x = synth.counts_to_pa(k, np.float64)
        if g.get("ramp"):
            x = x + np.arange(x.size, dtype=np.float64) * (g["ramp"] * 2.0 ** -10)
        if g.get("ramp20"):
            x = x + np.arange(x.size, dtype=np.float64) * (g["ramp20"] * 2.0 ** -20)
        if x.size <= 100000:                   # (the large-t input is rebuilt where it is used: 128 MiB)
            _inputs[case["name"]] = x
    return x


def normalised(case):
    """(start, end) of a case as subscripts (StatSplit.parse's rule)."""
    n = case["gen"]["n"]
    start, end = case.get("start", 0), case.get("end", -1)
    if start < 0:
        start += n + 1
    if end < 0:
        end += n + 1
    return min(start, n), min(end, n)


_golden = None


def golden():
    """(npz of boundaries, {key: margin or None}) as make_golden_statsplit.py left them."""
    global _golden
    if _golden is None:
        import json
        with open(os.path.join(HERE, "golden", "manifest_statsplit.json")) as f:
            man = json.load(f)
        _golden = (np.load(os.path.join(HERE, "golden", "golden_statsplit.npz")), {r["key"]: r["margin"] for r in man["runs"]})
    return _golden
