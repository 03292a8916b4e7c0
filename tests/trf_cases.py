"""The inputs of the repeat splitter's tests (tests/test_trf_host.py, tests/test_trf_gpu.py) and of the golden recorder
(tests/golden/make_golden_trf.py).  A case: {"name", "means", "stds", "penalty", "min_score", "grid"}.

Grid cases: means on a grid of 2^-5, stds in {1/2, 1, 2} -- the difference, its square, the product of the stds, the quotient
and every sum of the matrix are exact, so exact ties of the maximum and between pointer candidates are real ties.  Off-grid
cases: means that are a sum / 7 and stds that are a square root, as a segment's are.

Sizes: 0, 1, 2, 3 and 63 .. 65, 127 .. 129 -- the stripe seams of the kernel (64 rows per stripe); the cases above 70
segments are few and use widely spaced levels (few chance repeats), because the Python oracle costs n^2 per repeat."""
import json
import os

import numpy as np

import trf_oracle as O

SEAM_SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)


def _levels(rng, n, grid, lo, hi):
    if grid:
        return np.round(rng.uniform(lo, hi, n) * 32.0) / 32.0
    return np.array([np.sum(rng.normal(rng.uniform(lo, hi), 0.5, 7)) / 7 for _ in range(n)], dtype=np.float64)


def _stds(rng, n, grid):
    if grid:
        return rng.choice([0.5, 1.0, 2.0], size=n)
    return np.sqrt(rng.uniform(0.2, 2.5, n))


def _noise(rng, k, grid, noisy):
    if not noisy:
        return np.zeros(k)
    return rng.integers(-6, 7, k) / 32.0 if grid else rng.normal(0.0, 0.2, k)


def planted(rng, n, grid, rereads, lo=20.0, hi=26.0):
    """n segments: a strand of levels read once, with re-reads planted.  rereads: [(k, times, noisy)] -- after some point the
    last k segments are read again `times` times.  Returns (means, stds) of exactly n segments (padded with fresh levels or
    cut at the end)."""
    extra = sum(k * t for k, t, _ in rereads)
    base = max(n - extra, 0)
    m, s = list(_levels(rng, base, grid, lo, hi)), list(_stds(rng, base, grid))
    for k, times, noisy in rereads:
        if base < k:
            continue
        a = int(rng.integers(0, base - k + 1))
        pos = a + k
        for _ in range(times):
            m[pos:pos] = list(np.asarray(m[a:a + k]) + _noise(rng, k, grid, noisy))
            s[pos:pos] = s[a:a + k]
            pos += k
    while len(m) < n:
        m.append(float(_levels(rng, 1, grid, lo, hi)[0]))
        s.append(float(_stds(rng, 1, grid)[0]))
    return np.array(m[:n], dtype=np.float64), np.array(s[:n], dtype=np.float64)


def few_levels(rng, n, n_levels, grid):
    """n segments over n_levels distinct levels: full of exact ties."""
    lv = _levels(rng, n_levels, grid, 20.0, 26.0)
    sd = _stds(rng, n_levels, grid)
    idx = rng.integers(0, n_levels, n)
    return lv[idx], sd[idx]


def _case(name, ms, penalty=-1.0, min_score=2.0, grid=True):
    return {"name": name, "means": ms[0], "stds": ms[1], "penalty": float(penalty), "min_score": float(min_score), "grid": grid}


def _common(grid):
    tag = "grid" if grid else "off"
    rng = np.random.default_rng(20240 + (0 if grid else 1))
    out = []
    for n in SEAM_SIZES:                                        # the stripe seams, a planted re-read where there is room
        wide = n > 70
        rr = [(min(5, n // 3), 1, not grid)] if n >= 3 else []
        out.append(_case("%s_seam_n%d" % (tag, n), planted(rng, n, grid, rr, 10.0 if wide else 20.0, 60.0 if wide else 26.0)))
    for pen in (-0.5, -1.0, -2.0):                              # exact and noisy re-reads of k segments, every penalty
        out.append(_case("%s_exact_pen%g" % (tag, pen), planted(rng, 40, grid, [(6, 1, False)]), penalty=pen))
        out.append(_case("%s_noisy_pen%g" % (tag, pen), planted(rng, 47, grid, [(8, 1, True)]), penalty=pen))
    out.append(_case("%s_three_reads" % tag, planted(rng, 50, grid, [(5, 2, False)])))
    out.append(_case("%s_three_reads_noisy" % tag, planted(rng, 66, grid, [(7, 2, True)])))
    out.append(_case("%s_two_rereads" % tag, planted(rng, 69, grid, [(4, 1, True), (9, 1, False)])))
    for n, nl in ((24, 3), (41, 4), (68, 5)):                   # ties: across lanes, across stripes (68 rows), between candidates
        out.append(_case("%s_levels%d_n%d" % (tag, nl, n), few_levels(rng, n, nl, grid)))
    out.append(_case("%s_levels3_pen-0.5" % tag, few_levels(rng, 30, 3, grid), penalty=-0.5))
    out.append(_case("%s_min_score0" % tag, planted(rng, 33, grid, [(4, 1, True)]), min_score=0.0))
    out.append(_case("%s_min_score3.5" % tag, planted(rng, 45, grid, [(6, 1, True)]), min_score=3.5))
    # an end cell in row 0: the re-read starts at the strand's first segment
    m, s = planted(rng, 30, grid, [], 10.0, 60.0)
    out.append(_case("%s_row0_end" % tag, (np.concatenate((m[:5], m)), np.concatenate((s[:5], s)))))
    for c in out:
        c["grid"] = grid
    return out


def grid_cases():
    out = _common(True)
    # the best score equals min_score exactly and must stop: levels 8 apart (no chance match), a re-read of 3 segments
    # (score 6, yielded) and one of 2 (score 4 = min_score, not yielded)
    m = 8.0 * np.arange(1, 21, dtype=np.float64)
    m = np.concatenate((m[:6], m[3:6], m[6:14], m[12:14], m[14:]))
    out.append(_case("grid_stop_at_min_score", (m, np.ones(m.size)), min_score=4.0))
    return out


def offgrid_cases():
    return _common(False)


def all_cases():
    return grid_cases() + offgrid_cases()


# ---- what the recorder stored (tests/golden/make_golden_trf.py) and the restatement, each computed once and shared ---------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def golden():
    """(golden_trf.npz, {case name: its manifest entry})."""
    if "g" not in _cache:
        _cache["g"] = np.load(os.path.join(GOLDEN, "golden_trf.npz"))
        with open(os.path.join(GOLDEN, "manifest_trf.json")) as f:
            _cache["m"] = {c["name"]: c for c in json.load(f)["cases"]}
    return _cache["g"], _cache["m"]


def golden_yields(name, tag=""):
    g, _ = golden()
    return [(float(s), int(l[0]), int(l[1]), int(l[2])) for s, l in zip(g[name + "/score" + tag], g[name + "/lij" + tag])]


def golden_rows(name):
    return [[int(v) for v in row] for row in golden()[0][name + "/rows"]]


def restated(case):
    """((yields, info) of splits_full, (yields, info) of splits_upper)."""
    key = ("r", case["name"])
    if key not in _cache:
        _cache[key] = tuple(f(case["means"], case["stds"], case["penalty"], case["min_score"]) for f in (O.splits_full, O.splits_upper))
    return _cache[key]


def same_bits(a, b):
    """Two lists of yields are equal, scores bit for bit."""
    return len(a) == len(b) and all(x[1:] == y[1:] and np.float64(x[0]).tobytes() == np.float64(y[0]).tobytes() for x, y in zip(a, b))
