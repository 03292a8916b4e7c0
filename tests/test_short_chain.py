"""Option "short_chain" (include/poreseg.h): a segment call on the screened route of the 32-bit digest leaves out the launches it
can do without -- the look-ahead kernel of a pooled call (its bridges walk on in their own wave; if a seam is still deferred
the look-ahead kernel runs behind the stitch, on the device) and, on a repeated layout, the upload kernel (the download kernel of the call before left the
status block zero).  Every case compares short_chain 1 with 0 -- boundaries, offsets, spine flags, segment statistics -- and
with the oracle where it says so.  What was launched is read from the call's counters (timings(): lookahead_skipped,
upload_skipped, seams_resumed, repairs).

Shapes: W = 2 000, min_width 100 as in test_tree_screen.py; at most 2e5 samples a trace, so tiles are 4 W = 8 000 samples long."""
import numpy as np
import pytest

import oracle
from pypore_amd import synth
from test_tree_screen import MW, OP, P, Q, W, plain_suite, steps, tensor

SKIPPED = ("lookahead_skipped", "upload_skipped", "seams_resumed")
# (a pooled call splits the seams' windows between the bridge and whoever finishes them differently under the option: four
#  look-ahead waves scan up to three windows beyond a hit, a single wave none -- every other kernel's work is the same)
WORK = ("windows_spine", "windows_tree", "windows_screen", "tree_deferred", "tree_jobs", "tiles")
LONE = WORK + ("windows", "candidates", "windows_bridge", "exact_rescans", "near_ties")


@pytest.fixture()
def ctx():
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def call(ctx, t, ev_off, short_chain, params=None, stats=False):
    """One segment_batch under short_chain 0 / 1: (boundaries, offsets, spine flags, statistics or None, timings)."""
    ctx.set_option("short_chain", short_chain)
    r = ctx.segment_batch(t, np.asarray(ev_off, dtype=np.int64), params if params is not None else P(), Q,
                          want_stats=stats, want_spine=True)
    tm = ctx.timings()
    return r[0].cpu().numpy(), np.array(r[1]), r[3].cpu().numpy(), (r[2].cpu().numpy() if stats else None), tm


def same(a, b):
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    if a[3] is not None:
        np.testing.assert_array_equal(a[3], b[3])


def against_oracle(r, c, ev_off, **okw):
    x = synth.counts_to_pa(c, np.float64)
    b, off = r[0], r[1]
    for e in range(len(ev_off) - 1):
        np.testing.assert_array_equal(b[off[e]:off[e + 1]], oracle.parse(x[ev_off[e]:ev_off[e + 1]], **OP(**okw)))


def on_and_off(ctx, c, ev_off, dtype, shared, stats=False, oracle_too=True, params=None):
    """short_chain 1 == 0 (== oracle) for one input; pooled: as a context that shares the device with `shared` - 1 others."""
    t = tensor(c, dtype)
    ctx.set_option("shared_device", shared)
    try:
        r0 = call(ctx, t, ev_off, 0, params, stats)
        r1 = call(ctx, t, ev_off, 1, params, stats)
        r1b = call(ctx, t, ev_off, 1, params, stats)          # (the repeated layout: no upload on the short route)
    finally:
        ctx.set_option("shared_device", 1)
    same(r1, r0)
    same(r1b, r0)
    if oracle_too:
        against_oracle(r1, c, ev_off)
    print("shared %d %s: short_chain 0 %s | 1 %s | 1 again %s" % (shared, dtype, {k: r0[4][k] for k in SKIPPED + ("repairs", "windows_bridge")},
                                                                 {k: r1[4][k] for k in SKIPPED + ("repairs", "windows_bridge")}, {k: r1b[4][k] for k in SKIPPED}))
    assert all(r0[4][k] == 0 for k in SKIPPED)                # option 0: every launch as before
    return r0, r1, r1b


def random_steps(n, seed, lo=200, hi=4000):
    rng = np.random.default_rng(seed)
    d = []
    while sum(d) < n:
        d.append(int(rng.integers(lo, hi)))
    return steps(d, seed)[:n]


# ---- 1. one event, many tiles ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [1, 16])
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_one_event_many_tiles(ctx, dtype, shared):
    c = random_steps(200000, 5)
    for stats in (False, True):
        r0, r1, r1b = on_and_off(ctx, c, [0, c.size], dtype, shared, stats=stats, oracle_too=not stats)
        if not plain_suite():
            continue
        assert r1[4]["tiles"] >= 20
        assert r1[4]["lookahead_skipped"] == (1 if shared > 1 else 0)
        # (a call with statistics leaves the status block as it is: the next call's upload stays)
        assert r1[4]["upload_skipped"] == 0 and r1b[4]["upload_skipped"] == (0 if stats else 1)
        for k in (LONE if shared <= 1 else WORK):
            assert r1[4][k] == r0[4][k] == r1b[4][k], k
        assert r1[4]["seams_resumed"] == 0 and r1[4]["repairs"] == r0[4]["repairs"] == 0


# ---- 2. offsets at their edges ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [1, 16])
def test_offsets_at_their_edges(ctx, shared):
    # 37 events: empty ones (the first, two in a row, the last), events of at most 2 min_width samples, ordinary ones
    rng = np.random.default_rng(7)
    lens = [0, 2 * MW, 9000, 0, 0, 2 * MW - 1, 1, 2 * MW + 1]
    while len(lens) < 36:
        lens.append(int(rng.choice([0, 150, 2 * MW, 2500, 7000, 12000])))               # (about 1.3e5 samples in all)
    lens.append(0)                                              # last and empty: first_item[e] == n_items
    assert len(lens) == 37
    ev_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = random_steps(int(ev_off[-1]), 8, 300, 2500)
    for dtype in ("float32", "int16"):
        r0, r1, r1b = on_and_off(ctx, c, ev_off, dtype, shared)
        assert r1[1][-1] == r1[0].size and r1[1][-1] == r1[1][-2]
        if plain_suite():
            assert r1[4]["upload_skipped"] == 0 and r1b[4]["upload_skipped"] == 1


# ---- 3. the deferral hand-over ---------------------------------------------------------------------------------------------
def flat_stretch_trace():
    """Steps, a stretch of 20 W samples without one (five tiles long), steps again."""
    rng = np.random.default_rng(21)
    d = [int(v) for v in rng.integers(300, 3000, 20)] + [20 * W + 700] + [int(v) for v in rng.integers(300, 3000, 20)]
    return steps(d, 22)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_deferred_seam_is_finished_on_the_device(ctx, dtype):
    c = flat_stretch_trace()
    assert c.size <= 200000
    r0, r1, r1b = on_and_off(ctx, c, [0, c.size], dtype, 16)
    if plain_suite():
        # the bridge ran out of its 16 windows: the look-ahead kernel finished the seam behind the stitch, no host stitch
        assert r1[4]["lookahead_skipped"] == 1 and r1[4]["seams_resumed"] >= 1
        assert 1 <= r1[4]["repairs"] < 1000000 and r1[4]["repairs"] >= r1[4]["seams_resumed"]
        # ... and the next calls launch it in the chain again, as option 0 does (with their upload: the call before had two rounds)
        assert r1b[4]["lookahead_skipped"] == 0 and r1b[4]["seams_resumed"] == 0 and r1b[4]["repairs"] == 0
        assert r1b[4]["upload_skipped"] == 0 and r1b[4]["windows_bridge"] == r0[4]["windows_bridge"]
        assert r0[4]["repairs"] == 0                          # option 0: the look-ahead kernel walked the stretch
    # lone: the look-ahead kernel as before
    l0, l1, _ = on_and_off(ctx, c, [0, c.size], dtype, 1)
    same(l1, r1)
    if plain_suite():
        assert l1[4]["lookahead_skipped"] == 0 and l1[4]["seams_resumed"] == 0 and l1[4]["repairs"] == 0
        for k in LONE:
            assert l1[4][k] == l0[4][k], k


@pytest.mark.gpu
@pytest.mark.parametrize("patience", [1, 5])
def test_patience_of_a_pooled_bridge(ctx, patience):
    # patience 1: every seam whose first window holds no split is finished by the look-ahead kernel behind the stitch
    c = np.concatenate([random_steps(80000, 31, 1500, 6000), flat_stretch_trace()])
    assert c.size <= 200000
    ctx.set_option("bridge_patience", patience)
    r0, r1, _ = on_and_off(ctx, c, [0, 80000, c.size], "int16", 16)
    if plain_suite():
        assert r1[4]["seams_resumed"] >= 1 and 1 <= r1[4]["repairs"] < 1000000


@pytest.mark.gpu
def test_more_deferred_seams_than_second_chance_slots(ctx):
    # 3 000 tiles of 4 W (W = 200, min_width 8), dwells of 1.5 to 4.5 W, patience 1: a fifth of the seams is deferred (the others
    # join at once: a tile's last anchor usually is an anchor of the next tile's chain), more than the 512 slots of the second
    # chance's side buffer -- the look-ahead kernel takes them all, the host stitch none
    w, mw = 200, 8
    c = random_steps(2400000, 35, 300, 900)
    t = tensor(c, "int16")
    p = P(min_width=mw, window_width=w)
    ctx.set_tiling(4 * w, 0)
    ctx.set_option("bridge_patience", 1)
    ctx.set_option("shared_device", 16)
    r0 = call(ctx, t, [0, c.size], 0, p)
    r1 = call(ctx, t, [0, c.size], 1, p)
    r1b = call(ctx, t, [0, c.size], 1, p)                     # (the look-ahead launch is kept after a call that needed it)
    ctx.set_option("shared_device", 1)
    l1 = call(ctx, t, [0, c.size], 1, p)
    same(r1, r0)
    same(r1b, r0)
    same(l1, r0)
    print("tiles %d, seams resumed %d, repairs %d" % (r1[4]["tiles"], r1[4]["seams_resumed"], r1[4]["repairs"]))
    if plain_suite():
        assert r1[4]["seams_resumed"] > 512 and r1[4]["seams_resumed"] <= r1[4]["repairs"] < 1000000
        assert r0[4]["repairs"] == 0 and l1[4]["repairs"] == 0 and l1[4]["seams_resumed"] == 0
        assert r1b[4]["lookahead_skipped"] == 0 and r1b[4]["repairs"] == 0 and r1b[4]["seams_resumed"] == 0
        for k in WORK:
            assert r1[4][k] == r0[4][k] == r1b[4][k], k
        assert r1b[4]["windows_bridge"] == r0[4]["windows_bridge"]


# ---- 4. the clean-block protocol -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [1, 16])
def test_clean_block_protocol(ctx, shared):
    c = random_steps(120000, 41)
    t = tensor(c, "float32")
    la, lb = [0, c.size], [0, 50000, 50000, c.size]
    ctx.set_option("shared_device", shared)
    ref_a, ref_b = call(ctx, t, la, 0), call(ctx, t, lb, 0)
    against_oracle(ref_a, c, la)
    against_oracle(ref_b, c, lb)
    plain = plain_suite()

    def check(r, ref, upload_skipped):
        same(r, ref)
        if plain:
            assert r[4]["upload_skipped"] == upload_skipped
            for k in (LONE if shared <= 1 else WORK):
                assert r[4][k] == ref[4][k], k
    check(call(ctx, t, la, 1), ref_a, 0)                      # (the call before ran under option 0: it left the block as it was)
    check(call(ctx, t, la, 1), ref_a, 1)                      # the same layout again: no upload
    check(call(ctx, t, la, 1), ref_a, 1)
    check(call(ctx, t, lb, 1), ref_b, 0)                      # another layout: its tables go up
    check(call(ctx, t, lb, 1), ref_b, 1)
    # a call that fails by its input (a sample off the grid), then a good one on the same layout
    bad = t.clone()
    bad[60001] += 0.37 * Q
    with pytest.raises(ValueError, match="integer multiple"):
        call(ctx, bad, lb, 1)
    check(call(ctx, t, lb, 1), ref_b, 0)
    check(call(ctx, t, lb, 1), ref_b, 1)
    # a call with statistics does not clear the status block -- the next call's upload stays
    rs0, rs1 = call(ctx, t, lb, 0, stats=True), call(ctx, t, lb, 1, stats=True)
    same(rs1, rs0)
    same(ref_b, rs1)                                          # (boundaries, offsets, spine flags: as without statistics)
    if plain:
        assert rs1[4]["upload_skipped"] == 0
    check(call(ctx, t, lb, 1), ref_b, 0)
    check(call(ctx, t, lb, 1), ref_b, 1)
    # the same layout on a route the option leaves alone: its upload runs although the block is clean
    ctx.set_option("tree_screen", 0)
    check(call(ctx, t, lb, 1), call(ctx, t, lb, 0), 0)
    ctx.set_option("tree_screen", 1)
    check(call(ctx, t, lb, 1), ref_b, 0)
    check(call(ctx, t, lb, 1), ref_b, 1)
    # something else on the context between two calls (the detector uses the status block): the upload runs
    ctx.detect_events(t, Q, threshold=90.0, min_duration=1000)
    check(call(ctx, t, lb, 1), ref_b, 0)
    ctx.set_option("shared_device", 1)


@pytest.mark.gpu
def test_offsets_beyond_the_small_block_keep_the_upload(ctx):
    # the offsets ride behind the status block up to 64 KB of them (8 191 events) and download_kernel brings both back; 9 000
    # events of 16 samples have a buffer of their own and come back by plain copies: nobody clears the block, the upload stays
    n_ev = 9000
    ev_off = np.arange(n_ev + 1, dtype=np.int64) * 16
    c = random_steps(int(ev_off[-1]), 51, 200, 800)
    t = tensor(c, "int16")
    p = P(min_width=8, window_width=200)
    r0 = call(ctx, t, ev_off, 0, p)
    r1 = call(ctx, t, ev_off, 1, p)
    r1b = call(ctx, t, ev_off, 1, p)
    same(r1, r0)
    same(r1b, r0)
    assert r1[1][-1] == 0 or r1[0].size == r1[1][-1]
    for r in (r1, r1b):
        assert r[4]["upload_skipped"] == 0


# ---- 5. untouched routes ---------------------------------------------------------------------------------------------------
ROUTES = {"scan_bs 0": [("scan_bs", 0)], "verify mode": [("mode", 2)], "tree_screen 0": [("tree_screen", 0)], "tree_mw 1": [("tree_mw", 1)],
          "groups 0": [("groups", 0)]}
RESTORE = {"scan_bs": 1, "mode": 0, "tree_screen": 1, "tree_mw": 0, "groups": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shared", [1, 16])
def test_untouched_routes(ctx, route, shared):
    from pypore_amd import engine
    c = np.concatenate([random_steps(60000, 61), flat_stretch_trace()])
    for name, value in ROUTES[route]:
        ctx.set_option(name, value)
    try:
        r0, r1, r1b = on_and_off(ctx, c, [0, 60000, c.size], "int16", shared, oracle_too=(route == "scan_bs 0"))
    finally:
        for name, _ in ROUTES[route]:
            ctx.set_option(name, engine.DEFAULT_OPTIONS.get(name, RESTORE[name]))
    for r in (r1, r1b):                                       # no launch left out: the list is the one of option 0
        assert all(r[4][k] == 0 for k in SKIPPED), r[4]
        for k in LONE + ("repairs",):
            assert r[4][k] == r0[4][k], k


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [1, 16])
def test_wide_digest_is_untouched(ctx, shared):
    # levels more than 2^14 counts apart: the call is redone on the 64-bit digest, whose launches stay as they were
    kw = np.clip((synth.random_dwell_counts(150000, 40, 400, 6000).astype(np.int64) - 1500) * 58, -32768, 32767)
    t = tensor(kw, "int16")
    ctx.set_option("shared_device", shared)
    r0 = call(ctx, t, [0, kw.size], 0)
    r1 = call(ctx, t, [0, kw.size], 1)
    r1b = call(ctx, t, [0, kw.size], 1)
    ctx.set_option("shared_device", 1)
    same(r1, r0)
    same(r1b, r0)
    if plain_suite():
        assert r0[4]["wide_redo"] == 1 and r1b[4]["wide_redo"] == 1
        for r in (r1, r1b):
            assert r[4]["upload_skipped"] == 0
            for k in LONE + ("repairs",):
                assert r[4][k] == r0[4][k], k


# ---- 6. work counters ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_work_counters(ctx, dtype):
    c = np.concatenate([random_steps(80000, 71, 200, 4000), flat_stretch_trace()])
    ev_off = [0, 30000, 80000, c.size]
    l0, l1, l1b = on_and_off(ctx, c, ev_off, dtype, 1)
    p0, p1, p1b = on_and_off(ctx, c, ev_off, dtype, 16)
    same(p1, l1)
    if not plain_suite():
        return
    for k in LONE:
        assert l1[4][k] == l0[4][k] == l1b[4][k], k                     # lone contexts: everything
    for k in WORK:
        assert p1[4][k] == p0[4][k] == p1b[4][k] == l0[4][k], k         # pooled: all but the bridge / look-ahead split ...
    assert p1[4]["windows"] - p1[4]["windows_bridge"] == p0[4]["windows"] - p0[4]["windows_bridge"]    # ... which is all that differs
