"""The verdicts of the two window functions of seg_bs.hpp, held to a record: scan_window_bs and screen_window_bs share their
geometry, setup, levels, coarse pass, live-row mask and boundary evaluation (the bs_* helpers in front of them), and a change
to one of those must not move a single decision of either.  The call counters expose the decisions -- how many windows were
scanned, how many the screen proved empty, how many jobs it handed over, how many windows took the contender decision, the
whole-window exact scan or ended as a near tie.  tests/golden/window_counters.json holds them, with the SHA-256 of the
boundaries, as the library gave them before the helpers were shared (tests/golden/make_golden_window_counters.py, run three
times per case: a counter that did not repeat is named there and not compared).

The cases (W = 2 000, min_width 100 unless said; step traces as in test_tree_screen.py, at most 2e5 samples each):
  leaf_edges          leaf lengths around one or two windows, around a whole 256-sample group inside the second window, and
                      W/2 + three or four whole blocks -- int16 and float32.  (With min_width 100 a window that is scanned has
                      more than 200 samples; windows of three and four whole blocks are those of small_min_width.)
  odd_offsets         the same leaf lengths in events cut out of a file trace at odd offsets (EvRef::ph != 0) -- both dtypes
  flat_noise          one level and quiet dwells: nothing inside a subtree job, every window of the screen proven empty
  every_job_splits    every subtree job holds a split
  small_min_width     min_width 8: second windows of 17 .. 48 samples -- fewer than four whole blocks, the exact fallback
  wide_range          levels more than 2^14 counts apart: the 64-bit digest (WIDE, sampling pass), the screen is not launched

The counters are compared only when the suite runs without PORESEG_* route overrides; the boundaries are compared with
oracle.parse always."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from pypore_amd import synth
from test_tree_screen import MW, OP, P, Q, W, interleave, plain_suite, split_jobs_trace, steps, tensor

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_counters.json")
COUNTERS = ("windows", "candidates", "windows_tree", "tree_jobs", "tree_deferred", "windows_screen", "exact_rescans",
            "full_exact_scans", "near_ties")
REQUIRED = ("windows", "candidates", "tree_deferred", "windows_screen")      # deterministic: the other tests rely on it

LEAF_EDGES = [W // 2 + 2 * MW - 1, W // 2 + 2 * MW, W // 2 + 2 * MW + 1, W // 2 + 2 * MW + 2, W // 2 + 255, W // 2 + 256,
              W // 2 + 263, W // 2 + 264, W // 2 + 511, W // 2 + 512, W // 2 + 519, W // 2 + 520,
              W // 2 + 23, W // 2 + 24, W // 2 + 31, W // 2 + 32, W // 2 + 39, W // 2 + 40]
THRESHOLD, MIN_DURATION = 90.0, 1000


def leaf_trace():
    return steps(interleave(LEAF_EDGES, 1, filler=(2300, 4500), repeat=2), 11)


def file_trace():
    """Two events of leaf_trace's dwells between stretches of open channel whose lengths put the events at odd offsets."""
    d = interleave(LEAF_EDGES, 2, repeat=1)
    ev = np.repeat(np.asarray(synth.LEVEL_COUNTS, dtype=np.int64)[np.arange(len(d)) % len(synth.LEVEL_COUNTS)], d)
    half = ev.size // 2
    gap = lambda n: np.full(n, synth.OPEN_COUNTS, dtype=np.int64)
    lv = np.concatenate([gap(9001), ev[:half], gap(9006), ev[half:], gap(9001)])
    return (lv + synth.noise_counts(52, 0, lv.size)).astype(np.int32)


def wide_trace():
    return np.clip((synth.random_dwell_counts(150000, 40, 400, 6000).astype(np.int64) - 1500) * 58, -32768, 32767).astype(np.int32)


# name -> (kind, counts, dtype, parameters of the call and of the oracle)
def cases():
    small = dict(min_width=8)
    out = {}
    for dt in ("int16", "float32"):
        out["leaf_edges_" + dt] = ("batch", leaf_trace, dt, {})
        out["odd_offsets_" + dt] = ("file", file_trace, dt, {})
    out["flat_noise"] = ("batch2", lambda: np.concatenate([steps([60000], 33), steps([3900] * 25, 31)]), "int16", {})
    out["every_job_splits"] = ("batch", lambda: split_jobs_trace(40, 32), "int16", {})
    out["small_min_width"] = ("batch", lambda: steps(interleave([W // 2 + r for r in range(16, 49)], 3, repeat=1), 13), "int16", small)
    out["wide_range"] = ("batch", wide_trace, "int16", {})
    return out


def run_case(ctx, name):
    """One call of the case: (boundaries per event as a list of int arrays, the events' (start, length), the counters)."""
    kind, make, dtype, kw = cases()[name]
    c = make()
    assert c.size <= 200000
    t = tensor(c, dtype)
    if kind == "file":
        st, ln, b, off, _ = ctx.detect_segment_trace(t, Q, P(**kw), threshold=THRESHOLD, min_duration=MIN_DURATION)
        events = [(int(s), int(n)) for s, n in zip(st, ln)]
    else:
        ev_off = np.array([0, c.size] if kind == "batch" else [0, 60000, c.size], dtype=np.int64)
        b, off, _, _ = ctx.segment_batch(t, ev_off, P(**kw), Q, want_stats=False, want_spine=True)
        events = [(int(a), int(e - a)) for a, e in zip(ev_off[:-1], ev_off[1:])]
    tm = ctx.timings()
    b = b.cpu().numpy()
    return c, events, [b[off[e]:off[e + 1]].astype(np.int32) for e in range(len(events))], tm


def digest(events, bounds):
    h = hashlib.sha256()
    for (s, n), b in zip(events, bounds):
        h.update(np.array([s, n, b.size], dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(b, dtype=np.int32).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def ctx():
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases()))
def test_window_verdicts_are_the_recorded_ones(ctx, golden, name):
    from pypore_amd import engine
    rec = golden["cases"][name]
    own = engine.Context(0) if name == "wide_range" else None       # (the 64-bit route is remembered by the context)
    try:
        c, events, bounds, tm = run_case(own or ctx, name)
    finally:
        if own is not None:
            own.close()
    print(name, {k: tm[k] for k in COUNTERS}, "wide_redo", tm["wide_redo"])
    kind, _, _, kw = cases()[name]
    x = synth.counts_to_pa(c, np.float64)
    if kind == "file":
        rs, rl = oracle.lambda_events(x, threshold=THRESHOLD, min_duration=MIN_DURATION)
        assert [e[0] for e in events] == [int(v) for v in rs] and [e[1] for e in events] == [int(v) for v in rl]
        assert len(events) >= 2 and any(s & 1 for s, _ in events)                # an odd phase of the 8-sample blocks
    for (s, n), b in zip(events, bounds):
        np.testing.assert_array_equal(b, oracle.parse(x[s:s + n], **OP(**kw)))
    assert digest(events, bounds) == rec["sha256"]
    if not plain_suite():
        return
    if name == "wide_range":
        assert tm["wide_redo"] == 1 and tm["windows_screen"] == -1
    for k in COUNTERS:
        if k in rec["dropped"]:
            assert k not in REQUIRED
            continue
        assert tm[k] == rec["counters"][k], (k, tm[k], rec["counters"][k])
