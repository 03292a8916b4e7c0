"""The cases of the state parsers (snakebase_parser, FilterDerivativeSegmenter): seeded inputs and parameters.
tests/golden/make_golden_state_parsers.py records the reference's spans for every case; the host and GPU tests read them back
(golden keys "snake/<name>", "fd/<name>", "fdy/<name>").  No case exceeds 8 192 samples.

Snakebase inputs (`snake_build`), all exact in float64:
  "grid"     a step signal on the 2**-5 pA ADC grid (equal neighbours: about 1 sample in 100); `coarse`: its counts divided
             by that number first (a coarser converter: about 1 in 7 at 16)
  "planted"  a ramp of 0.5 pA per sample that stands still exactly at the positions `hits`: low == hits
  `poke`     {index: value} written into the result (NaN, +-inf)
Filter-derivative inputs: `fd_build` gives a current (random-dwell steps on the ADC grid) that goes through the filter;
`fdy_build` gives a filtered current y directly, as the running sum of chosen steps, so that the derivative holds exactly
the values named -- the decisions at hand (ties, short pairs, pairs across tiles) are then exact on the prefiltered route.
"""
import os

import numpy as np

from pypore_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
T = 2048                                   # positions per compaction tile (seg_state.hpp: SP_TILE)
WAVE = 64

# ---- snakebase ------------------------------------------------------------------------------------------------------------
SNAKE_SIZES = [0, 1, 2, 3, T - 1, T, T + 1, T + 2, 2 * T + 1, 2 * T + 2]


def _grid(name, n, seed, **kw):
    return dict(name=name, gen=dict(kind="grid", n=n, seed=seed, **kw))


def _planted(name, n, hits, **kw):
    return dict(name=name, gen=dict(kind="planted", n=n, hits=sorted(hits), **kw))


SNAKE_CASES = (
    [_grid("grid_n%d" % n, n, 100 + i) for i, n in enumerate(SNAKE_SIZES)] +
    [_grid("coarse_n%d" % n, n, 200 + i, coarse=16) for i, n in enumerate(SNAKE_SIZES)] + [
        _grid("coarse_long", 8192, 231, coarse=16),
        _grid("grid_long", 8191, 232),
        # hits at a tile's last and first position and at m - 1 (m = n - 1 differences)
        _planted("tile_last", 2 * T + 100, [T - 1]),
        _planted("tile_first", 2 * T + 100, [T]),
        _planted("tile_seam", 2 * T + 100, [T - 1, T]),
        _planted("tile_seam_odd", 2 * T + 100, [7, T - 1, T]),
        _planted("last_position", 3 * T + 5, [3 * T + 3]),
        _planted("last_two", 3 * T + 5, [3 * T + 2, 3 * T + 3]),
        _planted("first_position", 300, [0]),
        _planted("first_and_last", T + 1, [0, T - 1]),
        _planted("word_seams", 1000, [63, 64, 127, 128, 255, 256, 511]),
        _planted("none", 2 * T + 1, []),
        _planted("none_short", 2, []),
        _planted("one_of_two", 2, [0]),
        _planted("odd_count", 5000, [10, 999, 2047, 2048, 4100]),
        _planted("even_count", 5000, [10, 999, 2047, 2048, 4100, 4998]),
        dict(name="every", gen=dict(kind="const", n=2 * T + 2, value=47.25)),
        dict(name="every_even_m", gen=dict(kind="const", n=T + 1, value=-3.5)),
        dict(name="every_short", gen=dict(kind="const", n=3, value=0.0)),
        # differences just off the threshold on both sides (1e-3 is no binary fraction: 2**-10 < 1e-3 < 2**-10 + 2**-15)
        dict(name="near_threshold", gen=dict(kind="steps", n=2500, seed=240, choices=[2.0 ** -10, 2.0 ** -10 + 2.0 ** -15, 0.0, 0.5])),
        _grid("nan", 3000, 241, coarse=16, poke={0: "nan", 1500: "nan", 2047: "nan", 2999: "nan"}),
        _grid("inf", 3000, 242, coarse=16, poke={5: "inf", 6: "inf", 2048: "-inf", 2998: "inf"}),
        dict(name="nan_const", gen=dict(kind="const", n=300, value=1.0, poke={100: "nan", 101: "inf", 102: "inf"})),
    ])
SNAKE_BY_NAME = {c["name"]: c for c in SNAKE_CASES}


def snake_build(case):
    g = case["gen"]
    n = g["n"]
    if g["kind"] == "grid":
        k = synth.step_counts(n, 700, g["seed"])
        x = (k // g["coarse"]) * (synth.QUANTUM * g["coarse"]) if g.get("coarse") else synth.counts_to_pa(k, np.float64)
        x = np.asarray(x, dtype=np.float64)
    elif g["kind"] == "planted":
        step = np.full(max(n - 1, 0), 0.5)
        step[np.asarray(g["hits"], dtype=np.int64)] = 0.0
        x = np.concatenate(([12.0], 12.0 + np.cumsum(step)))[:n]
    elif g["kind"] == "const":
        x = np.full(n, g["value"], dtype=np.float64)
    elif g["kind"] == "steps":
        rng = np.random.RandomState(g["seed"])
        step = np.asarray(g["choices"])[rng.randint(0, len(g["choices"]), size=n - 1)] * rng.choice([-1.0, 1.0], size=n - 1)
        x = np.concatenate(([0.0], np.cumsum(step)))
    else:
        raise ValueError(g["kind"])
    x = np.array(x, dtype=np.float64)
    for i, v in g.get("poke", {}).items():
        x[int(i)] = float(v)
    return x


# The batch: 300 events of mixed lengths, empty ones included, whose joints would be hits or would hide hits if a difference
# were taken across them (events of one coarse-grid signal cut at arbitrary places, constants side by side).
def snake_batch():
    rng = np.random.RandomState(77)
    lens = rng.choice([0, 0, 1, 2, 3, 17, 64, 65, 300, 1000, T - 1, T, T + 1, T + 2, 2 * T + 3], size=300)
    total = int(lens.sum())
    k = synth.step_counts(total, 500, 78)
    x = np.asarray((k // 16) * (synth.QUANTUM * 16), dtype=np.float64)
    out, at = [], 0
    for e, ln in enumerate(lens):
        ev = np.array(x[at:at + ln])
        if e % 7 == 0:
            ev[:] = 40.0                         # constant neighbours: equal across the joint
        out.append(ev)
        at += ln
    return out


# ---- filter-derivative: from a current (the full route) ---------------------------------------------------------------------
def _fd(name, n, seed, low, high, cutoff=1000., fs=1.e5, lo=200, hi=900, **kw):
    return dict(name=name, gen=dict(n=n, seed=seed, lo=lo, hi=hi, **kw), par=dict(low_threshold=low, high_threshold=high,
                                                                                cutoff_freq=cutoff, sampling_freq=fs))


FD_CASES = [
    _fd("steps", 6000, 301, 0.05, 2),
    _fd("steps_h0", 6000, 302, 0.05, 0),
    _fd("steps_hneg", 6000, 303, 0.05, -1),
    _fd("steps_h2p5", 6000, 304, 0.05, 2.5),
    _fd("steps_hbig", 6000, 305, 0.05, 1e6),
    _fd("steps_h10", 8192, 306, 0.04, 10),
    _fd("fast_filter", 5000, 307, 0.3, 2, cutoff=10000.),
    _fd("fast_filter_many", 8192, 308, 0.15, 1, cutoff=20000., lo=40, hi=200),
    _fd("slow_filter", 8000, 309, 0.004, 5, cutoff=100.),                 # (pole 0.994: the three-pass scan, not the fused kernel)
    _fd("other_rate", 7000, 310, 0.05, 3, cutoff=5000., fs=2.5e5),
    _fd("low_above_all", 4000, 311, 50.0, 2),
    _fd("low_zero", 3000, 312, 0.0, 2),                                   # (blocks set almost everywhere)
    _fd("low_negative", 3000, 313, -1.0, 2),                              # (every block set: no tic)
    _fd("starts_in_block", 5000, 314, 0.05, 2, head_step=30),
    _fd("tiny", 7, 315, 0.05, 0, lo=2, hi=4),
    _fd("tiny_8", 8, 316, 0.01, -1, lo=2, hi=4),
    _fd("tile_m1", T - 1, 317, 0.05, 2),
    _fd("tile", T, 318, 0.05, 2),
    _fd("tile_p2", T + 2, 319, 0.05, 2),
    _fd("tile_p3", T + 3, 320, 0.05, 2),
    _fd("dense", 8192, 321, 0.02, 1, cutoff=5000., lo=30, hi=120),
    _fd("dense_h0", 8192, 322, 0.02, 0, cutoff=5000., lo=30, hi=120),
]
FD_BY_NAME = {c["name"]: c for c in FD_CASES}


def fd_build(case):
    g = case["gen"]
    x = synth.counts_to_pa(synth.random_dwell_counts(g["n"], g["seed"], g["lo"], g["hi"]), np.float64)
    if g.get("head_step"):                       # a step inside the first samples: the derivative starts above the threshold
        x = np.array(x)
        x[:3] += g["head_step"]
    return x


# ---- filter-derivative: from y (the prefiltered route) ------------------------------------------------------------------------
# deriv: a list of (value, repeat) runs; y is its running sum with alternating signs where `alt` is set.  Values are small
# multiples of 2**-4, so y and every difference of neighbours are exact.
def _fdy(name, runs, low, high, alt=False):
    return dict(name=name, gen=dict(runs=runs, alt=alt), par=dict(low_threshold=low, high_threshold=high, cutoff_freq=1000.,
                                                                sampling_freq=1.e5))


def _blocks(count, gap, block):
    """count blocks: `gap` low derivatives, then the values of `block`."""
    runs = []
    for _ in range(count):
        runs += [(0.25, gap)] + [(v, 1) for v in block]
    return runs + [(0.25, gap)]


FDY_CASES = [
    _fdy("no_tic", [(0.25, 500)], 1.0, 2),
    _fdy("no_tic_all_set", [(2.0, 500)], 1.0, 2),
    _fdy("one_tic", [(0.25, 300), (2.0, 200)], 1.0, 2),
    _fdy("one_pair", [(0.25, 300), (2.0, 1), (3.0, 1), (2.0, 1), (4.0, 1), (2.0, 5), (0.25, 100)], 1.0, 2),
    _fdy("odd_tics", _blocks(3, 50, [2.0, 2.0, 2.0, 3.0, 2.0]) + [(5.0, 40)], 1.0, 2),
    _fdy("blocks0_set", [(2.0, 10)] + _blocks(4, 30, [2.0, 2.0, 2.0, 2.0, 3.0]), 1.0, 2),
    _fdy("blocks0_set_h0", [(2.0, 10)] + _blocks(4, 30, [2.0, 2.0, 2.0, 2.0, 3.0]), 1.0, 0),
    # a pair that spans several tiles (and begins and ends next to tile seams), its maximum in the last tile / in the first
    _fdy("long_pair_late_max", [(0.25, T - 2), (2.0, 2 * T + 5), (7.0, 1), (2.0, 90), (0.25, 50)], 1.0, 2),
    _fdy("long_pair_early_max", [(0.25, T - 1), (2.0, 1), (7.0, 1), (2.0, 2 * T + 9), (0.25, 50)], 1.0, 2),
    _fdy("long_pair_whole_event", [(0.25, 1), (2.0, 3 * T), (3.0, 1), (2.0, 7), (0.25, 1)], 1.0, 2),
    _fdy("long_gap_pair", [(2.0, 3)] + [(0.25, 2 * T + 1), (0.5, 1), (0.25, 3), (2.0, 4), (0.25, 60), (2.0, 4), (0.25, 9)], 1.0, 2),
    # more pairs than a wave has lanes, than a workgroup has waves, than a tile has positions / 2
    _fdy("many_pairs", _blocks(WAVE + 3, 6, [2.0, 2.0, 2.0, 3.0]), 1.0, 2),
    _fdy("many_pairs_300", _blocks(300, 9, [2.0, 3.0, 2.0, 2.5, 4.0, 2.0]), 1.0, 2),
    _fdy("pairs_alternate_keep", sum([_blocks(1, 5, [2.0, 2.0, 2.0, 3.0]) + _blocks(1, 5, [3.0, 2.0, 2.0, 2.0]) for _ in range(200)], []), 1.0, 2),
    _fdy("pairs_every_other_sample", [(2.0, 1), (0.25, 1)] * 2500, 1.0, -1),
    _fdy("pairs_every_other_sample_h0", [(2.0, 1), (0.25, 1)] * 2500, 1.0, 0),
    # pairs shorter than h + 1, exactly h + 1, h + 2 long (h = 2: the first index that counts is 3)
    _fdy("short_pairs", _blocks(1, 9, [2.0]) + _blocks(1, 9, [2.0, 3.0]) + _blocks(1, 9, [2.0, 3.0, 4.0]) +
         _blocks(1, 9, [2.0, 3.0, 4.0, 5.0]) + _blocks(1, 9, [2.0, 3.0, 4.0, 5.0, 6.0]), 1.0, 2),
    _fdy("short_pairs_h2p5", _blocks(1, 9, [2.0, 3.0, 4.0]) + _blocks(1, 9, [2.0, 3.0, 4.0, 5.0]), 1.0, 2.5),
    _fdy("short_pairs_h3", _blocks(1, 9, [2.0, 3.0, 4.0, 5.0]) + _blocks(1, 9, [2.0, 3.0, 4.0, 5.0, 6.0]), 1.0, 3),
    # the maximum exactly tied between left and right: the first one counts, the pair is not kept; one step more and it is
    _fdy("tie", _blocks(2, 20, [2.0, 5.0, 2.0, 5.0, 2.0]) + _blocks(1, 20, [2.0, 5.0, 2.0, 5.0625, 2.0]), 1.0, 2),
    _fdy("tie_long", [(0.25, 10), (6.0, 1), (2.0, 3 * T), (6.0, 1), (2.0, 2), (0.25, 10)], 1.0, 2),
    _fdy("tie_alt_sign", _blocks(3, 20, [2.0, 5.0, 2.0, 5.0, 2.0]), 1.0, 2, alt=True),
    _fdy("h_neg", _blocks(20, 7, [3.0, 2.0]), 1.0, -1),
    _fdy("h_neg_half", _blocks(20, 7, [3.0, 2.0]), 1.0, -0.5),
    _fdy("h_zero", _blocks(20, 7, [3.0, 2.0]) + _blocks(20, 7, [2.0, 3.0]), 1.0, 0),
    _fdy("h_2p5", _blocks(20, 7, [2.0, 2.0, 3.0, 2.0]) + _blocks(20, 7, [2.0, 2.0, 2.0, 3.0]), 1.0, 2.5),
    _fdy("h_huge", _blocks(20, 7, [2.0, 2.0, 3.0, 2.0]), 1.0, 1e6),
    _fdy("h_inf", _blocks(20, 7, [2.0, 2.0, 3.0, 2.0]), 1.0, float("inf")),
    _fdy("low_above_all", _blocks(20, 7, [2.0, 2.0, 3.0, 2.0]), 100.0, 2),
    _fdy("low_equal", [(0.25, 30), (1.0, 30), (0.25, 30), (1.0625, 30), (0.25, 30)], 1.0, -1),     # (deriv == low is not a block)
    _fdy("n0", [], 1.0, 2), _fdy("n1", [], 1.0, 2), _fdy("n2", [(2.0, 1)], 1.0, 2), _fdy("n3", [(2.0, 1), (0.25, 1)], 1.0, -1),
    _fdy("n4", [(0.25, 1), (2.0, 1), (0.25, 1)], 1.0, -1),
    _fdy("tile_edges", [(0.25, T - 1), (2.0, 1), (0.25, 1), (2.0, T - 2), (0.25, 2), (2.0, 1), (0.25, 1)], 1.0, -1),
]
FDY_BY_NAME = {c["name"]: c for c in FDY_CASES}


def fdy_build(case):
    name, g = case["name"], case["gen"]
    if name == "n0":
        return np.zeros(0)
    d = np.concatenate([np.full(r, v) for v, r in g["runs"]] + [np.zeros(0)])
    if g["alt"]:
        d = d * np.where(np.arange(d.size) % 2, -1.0, 1.0)
    return np.concatenate(([40.0], 40.0 + np.cumsum(d)))


_golden = None


def golden():
    """(npz of spans, manifest) as make_golden_state_parsers.py left them."""
    global _golden
    if _golden is None:
        import json
        with open(os.path.join(HERE, "golden", "manifest_state_parsers.json")) as f:
            man = json.load(f)
        _golden = (np.load(os.path.join(HERE, "golden", "golden_state_parsers.npz")), man)
    return _golden
