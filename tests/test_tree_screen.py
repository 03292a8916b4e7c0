"""The subtree screen (option "tree_screen", seg_device.hpp: tree_screen_kernel + seg_bs.hpp: screen_window_bs): on the narrow
digest a lean kernel proves the windows of the subtree jobs empty and hands the jobs it cannot decide to tree_kernel, with
the index of the first window it left undecided.  Every case runs the same call with the option 1 and 0 and asks for equal
boundaries, offsets and window counts (a window is counted by the kernel that decides it, so a job resumed at the wrong
window shows as a different count), and for the boundaries of oracle.parse.

A subtree job is rec(a, b) between two neighbouring spine anchors, so the dwell lengths of a step trace are its job lengths.
With W = 2 000, min_width 100 a job of length L < W scans [a, b) and then [a + 1000, b) while a + 1000 < b - 200.  The windows
of such a job are nested (all end at b) -- its candidate positions, not its gains: a step that the second window finds can
stay below the threshold in the first one, whose left side then holds another level as well (second_window_piece).  A job
reaches tree_kernel at a later window than its first where a later window holds the job's first split, or is one the
screen cannot judge -- fewer than four whole blocks, or no whole 256-sample group inside.  screen_model() says for a call's
result which jobs these are and how many windows the screen decides in front of them; the hand-over test asks the counters
for exactly that.

The launch list itself is not visible from inside pytest: "the screen was not launched" is read from counters[14] / [15],
which the library sets to -1 from the host flag of the launch (ps_ctx::screen_ran).  The list is compared launch for launch
by tools/launch_order.py under rocprofv3 (--tree-screen 0, --compare ... --names-only)."""
import numpy as np
import pytest

import oracle
from pypore_amd import _lib, synth

Q = synth.QUANTUM
W, MW = 2000, 100


def P(**kw):
    a = dict(min_width=MW, max_width=1000000, window_width=W, prior_segments_per_second=10.)
    a.update(kw)
    return _lib.split_params(**a)


def OP(**kw):
    a = dict(min_width=MW, max_width=1000000, window_width=W, prior_segments_per_second=10.)
    a.update(kw)
    return a


@pytest.fixture(scope="module")
def ctx():
    # (a context of its own: the wide-digest case leaves the context on the 64-bit route for the next calls on its grid)
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def steps(dwells, seed, levels=synth.LEVEL_COUNTS):
    """Step trace in counts: dwell k at levels[k % len(levels)], plus the package's integer noise."""
    dwells = np.asarray(dwells, dtype=np.int64)
    lv = np.repeat(np.asarray(levels, dtype=np.int64)[np.arange(dwells.size) % len(levels)], dwells)
    return (lv + synth.noise_counts(seed, 0, lv.size)).astype(np.int32)


def tensor(c, dtype):
    import torch
    return torch.from_numpy(c.astype(np.int16) if dtype == "int16" else synth.counts_to_pa(c, np.float32)).cuda()


DEFAULTS = {"tree_screen": 1, "stitch_host": 0, "groups": 1, "mode": 0, "slots_pct": 100}


def plain_suite():
    """False when the suite runs under PORESEG_* overrides (verify mode, host stitch, ...: tests/conftest.py): the results are
    compared all the same, what the screen's counters say depends on the route the override chose."""
    from pypore_amd import engine
    return not any(k in engine.DEFAULT_OPTIONS for k in ("mode", "stitch_host", "groups", "prune", "scan_bs", "tree_mw", "tree_screen"))


def both(ctx, call, options=()):
    """call() with tree_screen 1 and 0 (and `options` set for both, restored afterwards): {1: (result, timings), 0: ...}."""
    from pypore_amd import engine
    out = {}
    for name, value in options:
        ctx.set_option(name, value)
    try:
        for on in (1, 0):
            ctx.set_option("tree_screen", on)
            r = call()
            out[on] = (r, ctx.timings())
    finally:
        for name in ["tree_screen"] + [o[0] for o in options]:
            ctx.set_option(name, engine.DEFAULT_OPTIONS.get(name, DEFAULTS[name]))
    t1, t0 = out[1][1], out[0][1]
    print("tree_screen 1: windows %d (subtree %d, screen %d), tree jobs %d, deferred %d | 0: windows %d (subtree %d), deferred %d" %
          (t1["windows"], t1["windows_tree"], t1["windows_screen"], t1["tree_jobs"], t1["tree_deferred"],
           t0["windows"], t0["windows_tree"], t0["tree_deferred"]))
    assert t0["tree_deferred"] == -1 and t0["windows_screen"] == -1          # option 0: the screen is not launched
    assert t1["windows"] == t0["windows"] and t1["windows_tree"] == t0["windows_tree"]
    assert t1["candidates"] == t0["candidates"]
    return out


def check_batch(ctx, c, ev_off, dtype, params=None, oparams=None, options=(), screened=True):
    """segment_batch of the events ev_off of the counts c: option 1 == option 0 == oracle; returns the timings with the screen."""
    params = params if params is not None else P()
    oparams = oparams if oparams is not None else OP()
    ev_off = np.asarray(ev_off, dtype=np.int64)
    t = tensor(c, dtype)
    out = both(ctx, lambda: ctx.segment_batch(t, ev_off, params, Q, want_stats=False, want_spine=True), options)
    (b1, off1, _, sp1), tm = out[1]
    (b0, off0, _, sp0), _ = out[0]
    b1, b0 = b1.cpu().numpy(), b0.cpu().numpy()
    np.testing.assert_array_equal(off1, off0)
    np.testing.assert_array_equal(b1, b0)
    np.testing.assert_array_equal(sp1.cpu().numpy(), sp0.cpu().numpy())
    x = synth.counts_to_pa(c, np.float64)
    for e in range(ev_off.size - 1):
        np.testing.assert_array_equal(b1[off1[e]:off1[e + 1]], oracle.parse(x[ev_off[e]:ev_off[e + 1]], **oparams))
    if not plain_suite():
        tm = dict(tm, overridden=True)
    elif screened:
        assert tm["tree_deferred"] >= 0 and tm["windows_screen"] >= 0           # the screen ran
        assert tm["tree_deferred"] <= tm["tree_jobs"] and tm["windows_screen"] <= tm["windows_tree"]
    else:
        assert tm["tree_deferred"] == -1 and tm["windows_screen"] == -1         # this route launches what it launched before
    return tm, b1, off1, sp1.cpu().numpy()


def jobs_with_a_split(b, sp):
    """Subtree jobs of one event that found something: gaps between neighbouring spine anchors that hold other boundaries."""
    n, inside = 0, False
    for is_spine in sp:
        if is_spine:
            inside = False
        elif not inside:
            n, inside = n + 1, True
    return n


def interleave(edge_lengths, seed, filler=(2300, 6100), repeat=4):
    """Dwells: every edge length `repeat` times, each between two fillers of seeded lengths."""
    rng = np.random.default_rng(seed)
    d = [int(rng.integers(*filler))]
    for L in list(edge_lengths) * repeat:
        d += [int(L), int(rng.integers(*filler))]
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_leaf_length_edges_one_window_or_two(ctx, dtype):
    # W/2 + 2 mw - 1, W/2 + 2 mw: one window; W/2 + 2 mw + 1: a second one of 2 mw + 1 samples
    d = interleave([W // 2 + 2 * MW - 1, W // 2 + 2 * MW, W // 2 + 2 * MW + 1], 1)
    c = steps(d, 11)
    assert c.size <= 200000
    check_batch(ctx, c, [0, c.size], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_second_window_edges_at_min_width_100(ctx, dtype):
    # second window [a + 1000, b): 2 mw samples (not scanned), 2 mw + 1, and the lengths around one whole group inside
    d = interleave([W // 2 + 2 * MW, W // 2 + 2 * MW + 1, W // 2 + 2 * MW + 2, W // 2 + 255, W // 2 + 256, W // 2 + 263,
                    W // 2 + 264, W // 2 + 511, W // 2 + 512, W // 2 + 519, W // 2 + 520], 2, repeat=2)
    c = steps(d, 12)
    assert c.size <= 200000
    check_batch(ctx, c, [0, c.size], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_second_window_edges_three_and_four_whole_blocks(ctx, dtype):
    # min_width 8, W = 200: second windows of 2 mw = 16, 17, ... 48 samples -- 8 * 4 - 1 and 8 * 4 samples of whole blocks
    # (nblk 3 / 4) at every alignment of the window to the 8-sample blocks
    w, mw = 200, 8
    d = interleave([w // 2 + r for r in range(2 * mw, 49)], 3, filler=(230, 610), repeat=2)
    c = steps(d, 13)
    check_batch(ctx, c, [0, c.size], dtype, P(min_width=mw, window_width=w), OP(min_width=mw, window_width=w))


@pytest.mark.gpu
def test_jobs_without_a_window(ctx):
    # dwells of at most 2 mw samples: rec(a, b) scans nothing
    rng = np.random.default_rng(4)
    d = [int(v) for v in rng.integers(MW, 2 * MW + 1, 300)] + [2 * MW] * 20
    c = steps(d, 14)
    check_batch(ctx, c, [0, c.size], "int16")


def split_jobs_trace(n_jobs, seed):
    """Every subtree job holds a split: from each spine anchor a small step (+100 counts) after 1 200 samples and a large
    one after 1 600 -- both candidates of the window that starts at the anchor, the large one wins it, and the small one is
    what rec(anchor, large step) finds in its first window."""
    levels = [1600, 1700, 1100, 1200]
    return steps([1200, 400] * n_jobs + [3000], seed, levels)


SECOND_WINDOW_SEEDS = (113, 238, 667, 677, 806, 1717, 2134, 2903)


def second_window_piece(seed):
    """A subtree job of 1 900 samples whose split lies only in its second window, and the quiet dwell of 3 900 behind it.
    The job: 1 000 samples at +10 counts, 450 at 0, 450 at +12 (noise sigma 32), between two steps of ~600 counts.  Its second
    window [a + 1000, b) sees 450 samples at 0 against 450 at +12: gain 25 .. 34 with these seeds, the threshold is 18.42.  In
    its first window [a, b) the left side of that step holds the +10 stretch as well, whose mean is near the right side's:
    the best gain of the window is 7 .. 9.  (The seeds: eight of those of 1 .. 3000 with a first-window gain below 8.5 and a
    second-window gain above 25 by oracle.score_window; the test checks both against the threshold.)"""
    return steps([1000, 450, 450, 3900], seed, [1510, 1500, 1512, 2100])


def judged_by_the_screen(ps, pe, mw):
    """Whether screen_window_bs has a coarse pass for the window [ps, pe) of an event at offset 0 (seg_bs.hpp: the conditions
    under which it returns `undecided` before it looks at a gain)."""
    g0, g1 = (ps + 7) & ~7, pe & ~7
    nblk, gb0 = (g1 - g0) >> 3, g0 >> 3
    whole_groups = ((gb0 + nblk) >> 5) - ((gb0 + 31) >> 5)                    # 32 blocks = 256 samples each
    return nblk >= 4 and ps + mw >= g0 and pe - mw <= g1 and (nblk + 62) // 63 <= 64 and whole_groups >= 1


def screen_model(x, b, sp, w, mw, thr):
    """What the screen does with the subtree jobs of one event (samples x, boundaries b, spine flags sp): the jobs are the gaps
    between neighbouring spine anchors, job (a, e) starts at the first window that does not end before e (the spine scanned
    the others: left_child_j0), and is handed over at its first window that holds a split (oracle.score_window) or has no
    coarse pass.  A window that holds no split and has a coarse pass counts as proven empty: true of windows whose best gain
    is far below the threshold (the screen bounds the gains inside an 8-sample block from the block's two ends, which costs a
    few units of gain) -- the model returns the largest such gain, for the caller to hold against the threshold.
    Returns (jobs handed over, windows decided in front, jobs handed over behind their first window, largest gain of a window
    counted as proven empty)."""
    anchors = [0] + [int(v) for v in b[sp != 0]]
    half, deferred, windows, later, quiet = w // 2, 0, 0, 0, 0.0
    for a, e in zip(anchors[:-1], anchors[1:]):
        d = e - w - a
        first = ps = a + (0 if d < 0 else d // half + 1) * half
        while ps < e - 2 * mw:
            pe = min(ps + w, e)
            if pe - ps > 2 * mw:
                split, gains = oracle.score_window(x[ps:pe], mw, thr)
                if not judged_by_the_screen(ps, pe, mw) or split >= 0:
                    deferred, later = deferred + 1, later + (ps > first)
                    break
                windows, quiet = windows + 1, max(quiet, float(gains.max()))
            ps += half
    return deferred, windows, later, quiet


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_deferral_hands_the_job_over_at_the_undecided_window(ctx, dtype):
    # jobs with the split in their first window (handed over at j0), jobs with the split only in their second window and quiet
    # jobs whose second window the screen cannot judge (210 .. 400 samples: no whole group inside) -- both handed over at
    # j0 + 1 with the first window counted by the screen --, and quiet jobs it decides entirely
    head = split_jobs_trace(12, 21)
    c = np.concatenate([head] + [second_window_piece(s) for s in SECOND_WINDOW_SEEDS] +
                       [steps(interleave([1210, 1300, 1400], 5, filler=(3900, 3901), repeat=3), 36), steps([3900] * 8, 29)])
    assert c.size <= 200000
    tm, b, off, sp = check_batch(ctx, c, [0, c.size], dtype)
    x = synth.counts_to_pa(c, np.float64)
    thr = oracle.min_gain(**OP())
    # the second-window jobs are what they are meant to be: a job between two anchors, no split in [a, e) as one window, one in
    # [a + 1000, e), and a boundary there that is not a spine anchor
    # (an anchor lies within a few samples of its step)
    anchors = b[sp != 0].astype(np.int64)
    for k in range(len(SECOND_WINDOW_SEEDS)):
        a, e = (int(anchors[np.argmin(np.abs(anchors - v))]) for v in (head.size + 5800 * k, head.size + 5800 * k + 1900))
        assert abs(a - head.size - 5800 * k) <= 4 and abs(e - a - 1900) <= 8 and not np.any((anchors > a) & (anchors < e))
        assert oracle.score_window(x[a:e], MW, thr)[0] < 0 <= oracle.score_window(x[a + W // 2:e], MW, thr)[0]
        assert np.any((b > a + W // 2 + MW) & (b < e - MW))
    found = jobs_with_a_split(b, sp)
    assert found >= 12 + len(SECOND_WINDOW_SEEDS)
    deferred, windows, later, quiet = screen_model(x, b, sp, W, MW, thr)
    print("model: deferred %d (jobs that found something %d, behind their first window %d), windows in front %d, best gain of an empty window %.2f" %
          (deferred, found, later, windows, quiet))
    assert later == len(SECOND_WINDOW_SEEDS) + 9 and deferred == found + 9     # (9: the jobs of 1 210, 1 300 and 1 400 samples)
    assert quiet < 0.6 * thr                                                   # the model's "proven empty" holds with room
    if tm.get("overridden"):
        return
    # the deferred list: every job that holds a split and every job with a window the screen cannot judge, and no other; the
    # screen counted the windows in front of the hand-over -- the first window of every job it handed over at its second --
    # and tree_kernel the rest
    assert tm["tree_deferred"] == deferred
    assert tm["windows_screen"] == windows
    assert tm["windows_tree"] - tm["windows_screen"] >= tm["tree_deferred"]      # tree_kernel decided a window of every job it got


@pytest.mark.gpu
def test_nothing_to_find_defers_nothing(ctx):
    # dwells of 3 900: rec(a, b) starts at its window 2 -- [a + 2000, b) and [a + 3000, b), 1 900 and 900 samples, whole groups
    # inside both -- and holds nothing
    c = steps([3900] * 25, 31)
    tm, b, off, sp = check_batch(ctx, c, [0, c.size], "int16")
    assert sp.all() and b.size >= 20                                           # counts[] all zero: every boundary is a spine anchor
    if tm.get("overridden"):
        return
    assert tm["tree_deferred"] == 0
    assert tm["windows_screen"] == tm["windows_tree"] > 0


@pytest.mark.gpu
def test_every_job_holds_a_split(ctx):
    c = split_jobs_trace(40, 32)
    tm, b, off, sp = check_batch(ctx, c, [0, c.size], "int16")
    found = jobs_with_a_split(b, sp)
    assert found >= 38
    assert tm.get("overridden") or tm["tree_deferred"] >= found


@pytest.mark.gpu
@pytest.mark.parametrize("max_width", [500, 2500])
def test_jobs_longer_than_max_width_are_deferred_whole(ctx, max_width):
    # find_split's forced splits (cparsers.pyx:189-191 inside the loop, :201 behind it) are tree_kernel's: 500 < W/2 reaches the
    # early one at the second window and the late one in the pieces it leaves, 2 500 the early one at the fourth window
    c = steps(interleave([2600, 3100, 4700], 6, filler=(5000, 9000), repeat=3), 41)
    assert c.size <= 200000
    tm, b, off, sp = check_batch(ctx, c, [0, c.size], "int16", P(max_width=max_width), OP(max_width=max_width))
    assert tm.get("overridden") or tm["tree_deferred"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_events_at_odd_offsets_through_the_file_route(ctx, dtype):
    # ps_detect_segment_trace: one digest aligned to the trace, events start at any phase of its blocks (EvRef::ph != 0)
    phases = set()
    for seed in (51, 52):
        c = synth.file_trace_counts(200000, seed, gap=9001 + seed, ev_lo=20000, ev_hi=50000)[0]
        t = tensor(c, dtype)
        out = both(ctx, lambda: ctx.detect_segment_trace(t, Q, P(), threshold=90.0, min_duration=1000))
        (st, ln, b1, off1, _), tm = out[1]
        (st0, ln0, b0, off0, _), _ = out[0]
        assert tm["wide_redo"] != 3
        assert not plain_suite() or (tm["tree_deferred"] >= 0 and tm["windows_screen"] > 0)
        np.testing.assert_array_equal(st, st0)
        np.testing.assert_array_equal(ln, ln0)
        np.testing.assert_array_equal(off1, off0)
        np.testing.assert_array_equal(b1.cpu().numpy(), b0.cpu().numpy())
        x = synth.counts_to_pa(c, np.float64)
        bb = b1.cpu().numpy()
        for e in range(len(st)):
            np.testing.assert_array_equal(bb[off1[e]:off1[e + 1]], oracle.parse(x[st[e]:st[e] + ln[e]], **OP()))
            phases.add(int(st[e]) & 7)
    assert any(p & 1 for p in phases) and any(p != 0 for p in phases)


@pytest.mark.gpu
def test_many_short_events_more_jobs_than_slots(ctx):
    n_ev, n = 1024, 5000
    c = synth.random_dwell_counts(n_ev * n, 61, 210, 600)
    ev_off = np.arange(n_ev + 1) * n
    tm, b, off, sp = check_batch(ctx, c, ev_off, "int16")
    # (4 096: the subtree kernel's slots on 256 CUs at four waves per SIMD; the screen's 7 168 become 1 792 with slots_pct 25)
    tq, bq, _, _ = check_batch(ctx, c, ev_off, "int16", options=[("slots_pct", 25)])
    np.testing.assert_array_equal(b, bq)
    if plain_suite():
        assert tm["tree_jobs"] > 4096 and tm["windows_screen"] > 0
        assert (tq["tree_deferred"], tq["windows_screen"]) == (tm["tree_deferred"], tm["windows_screen"])


@pytest.mark.gpu
def test_host_stitch_route_and_a_one_workgroup_call(ctx):
    c = steps(interleave([1201, 1500, 3900], 7, repeat=2), 71)
    # (the host stitch runs the LDS-window kernels: no digest, no screen)
    check_batch(ctx, c, [0, c.size], "int16", options=[("stitch_host", 1)], screened=False)
    small = steps([1500, 1201, 1300], 72)                                      # three jobs at the most: a grid of one workgroup or two
    check_batch(ctx, small, [0, small.size], "int16")
    one = steps([1201, 900], 73)
    check_batch(ctx, one, [0, one.size], "int16")


@pytest.mark.gpu
def test_other_routes_launch_what_they_launched(ctx):
    from pypore_amd import engine
    # min_width 4: candidates in the ragged ends of a window -- no digest route, the LDS-window kernels take the call
    c = steps(interleave([1201, 1500, 3900], 8, repeat=2), 81)
    check_batch(ctx, c, [0, c.size], "int16", P(min_width=4), OP(min_width=4), screened=False)
    # verify mode and a context without group records keep the subtree kernel alone as well
    check_batch(ctx, c, [0, c.size], "int16", options=[("groups", 0)], screened=False)
    check_batch(ctx, c, [0, c.size], "int16", options=[("mode", 2)], screened=False)
    # the 64-bit digest (levels more than 2^14 counts apart), on a context of its own: it remembers the wide route
    kw = np.clip((synth.random_dwell_counts(150000, 40, 400, 6000).astype(np.int64) - 1500) * 58, -32768, 32767).astype(np.int32)
    wide = engine.Context(0)
    try:
        tm, _, _, _ = check_batch(wide, kw, [0, kw.size], "int16", screened=False)
        assert tm.get("overridden") or tm["wide_redo"] == 1
    finally:
        wide.close()
