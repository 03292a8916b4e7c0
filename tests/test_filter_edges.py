"""The Bessel filter kernels (csrc/seg_filter.hpp) and their host side (ps_filter_bessel, filter_order_n, ps_requantise,
ps_filter_requantise_batch) at tile seams, in batches and at scale.

References: the long-double filtfilt of tests/filter_exact.py for n <= 2e5, the fp64 oracle beyond.  Bounds: per case from
tests/golden/manifest_filter_edges.json -- max(1e-11, 4 * err_ref), err_ref the oracle's own distance from the long-double
result, measured on the host (tests/golden/make_golden_filter_edges.py); never from a device result.  Every case names the
launch geometry it claims and asserts it from the host restatement of the library's formulas (filter_exact.order1_geometry,
halo_geometry); the *_geometry tests do that without a GPU over the same case lists."""
import functools
import json
import os
import types

import numpy as np
import pytest

import filter_exact as fx
import oracle
from launch_geometry import options
from pypore_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
MAN = json.load(open(os.path.join(HERE, "golden", "manifest_filter_edges.json")))
Q = synth.QUANTUM
OFF_GRID = r"status -6"                  # what _lib.check raises for PS_ERR_OFF_GRID: ps_segment's error for off-grid data
BAD_ARG = r"status -1"


def ids(cases):
    return [c["id"] for c in cases]


def entry(order, cutoff, second, gen):
    return MAN["cases"][fx.key_of(order, cutoff, second, gen)]


@functools.lru_cache(maxsize=8)
def _ld(key):
    e = MAN["cases"][key]
    x, _ = fx.make_input(e["gen"])
    return fx.bessel_filtfilt_ld(x[:fx.MAX_LD], e["cutoff"], e["second"], e["order"])


def check(got, order, cutoff, second, gen, what=""):
    """got against the long-double reference (n <= MAX_LD) or the fp64 oracle (longer), within the manifest's bound."""
    e = entry(order, cutoff, second, gen)
    assert e["bound"] == fx.bound_from(e["err_ref"])
    assert got.dtype == np.float64
    if got.size <= fx.MAX_LD:
        err = fx.rel_err(got, _ld(fx.key_of(order, cutoff, second, gen)))
    else:
        x, _ = fx.make_input(gen)
        err = fx.rel_err(got, oracle.bessel_filtfilt(x, cutoff, second, order))
    print("%s %s: %.3e (bound %.3e)" % (fx.key_of(order, cutoff, second, gen), what, err, e["bound"]))
    assert err <= e["bound"], (what, err, e["bound"])


def to_dev(dtype, x, k):
    import torch
    if dtype == "i16":
        assert np.abs(k).max() < 2 ** 15
        return torch.from_numpy(k.astype(np.int16)).cuda()
    if dtype == "f32":
        return torch.from_numpy((k * Q).astype(np.float32)).cuda()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def poison(n):
    """Fills the allocator's free blocks of an n-double result with NaN: an output the kernels leave unwritten must not
    show the correct values of the call before."""
    import torch
    held = [torch.full((max(1, n),), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    del held


def run(ctx, dev, cutoff, second, order=1, fused=1, offset_counts=0):
    poison(dev.numel())
    with options(ctx, filter_fused=fused):
        return ctx.filter_bessel(dev, Q, cutoff=cutoff, sampling_freq=second, order=order, offset_counts=offset_counts).cpu().numpy()


def context():
    from pypore_amd import engine
    return engine.context(0)


# ---- the helper's platform -------------------------------------------------------------------------------------------
def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


def test_manifest_holds_every_case():
    want = fx.manifest_inputs()
    assert set(want) == set(MAN["cases"])
    for key, e in MAN["cases"].items():
        assert e["bound"] == fx.bound_from(e["err_ref"]) and e["gen"] == want[key]["gen"]
    assert MAN["slow_halo_filter"] == list(fx.halo_filters()[-1]) and MAN["refused_filter"] == list(fx.refused_filter())


# ---- fused order-1 kernel: tile seams ---------------------------------------------------------------------------------
FUSED = fx.fused_cases()


@pytest.mark.parametrize("case", FUSED, ids=ids(FUSED))
def test_fused_seam_geometry(case):
    """The host picks H (1024, 960, 576, 384, 192, 64 for 650, 700, 1200, 2000, 5000, 24000 Hz at 100 kHz) and
    T = 4096 - 2 H; kT-1 / kT / kT+1: n + 12 there, k or k + 1 tiles, the last owning T - 1, T, 1 elements."""
    g = fx.order1_geometry(case["n"], case["cutoff"], case["second"], 1)
    assert g["route"] == "fused" and g["H"] == case["H"] == fx.FUSED_HALOS[case["cutoff"]] and g["T"] == case["T"] == 4096 - 2 * g["H"]
    assert case["n"] > 6 and fx.order1_geometry(case["n"], case["cutoff"], case["second"], 0)["route"] == "scan"
    H, T, what = g["H"], g["T"], case["what"]
    if what[0].isdigit():                                  # "kT-1", "kT+0", "kT+1"
        k, d = int(what[0]), int(what[2:])
        assert g["total"] == k * T + d and g["tiles"] == k + (d == 1) and g["last_owns"] == {-1: T - 1, 0: T, 1: 1}[d]
    else:
        assert case["n"] == {"n7": 7, "n8": 8, "H-1": H - 1, "H": H, "H+1": H + 1, "T-13": T - 13, "T-12": T - 12}[what]
        assert g["tiles"] == 1 and g["total"] <= T


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED, ids=ids(FUSED))
def test_fused_seams(case):
    """Geometry: test_fused_seam_geometry (H, T, tiles, last tile's share).  The fused kernel and the three-pass scan on
    the same input, each against the long-double reference, and against each other at the suite's 2e-14."""
    test_fused_seam_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    exact = run(ctx, dev, case["cutoff"], case["second"], fused=0)
    fused = run(ctx, dev, case["cutoff"], case["second"], fused=1)
    assert fused.shape == exact.shape == (case["n"],)
    check(fused, 1, case["cutoff"], case["second"], case["gen"], "fused")
    check(exact, 1, case["cutoff"], case["second"], case["gen"], "scan")
    assert np.max(np.abs(fused - exact)) <= fx.ROUTE_TOL * np.max(np.abs(exact))


STRADDLE = fx.straddle_cases()


@pytest.mark.parametrize("case", STRADDLE, ids=ids(STRADDLE))
def test_route_switch_geometry(case):
    """640 Hz: h_req > 1024, the scan whatever filter_fused says; 650 Hz: h_req <= 1024, H = 1024, T = 2048, 4 tiles."""
    lo = fx.order1_geometry(case["n"], 640.0, case["second"], 1)
    hi = fx.order1_geometry(case["n"], 650.0, case["second"], 1)
    assert lo["route"] == "scan" and lo["h_req"] > 1024 and lo["n_chunks"] == 2
    assert hi["route"] == "fused" and hi["h_req"] <= 1024 and hi["H"] == 1024 and hi["T"] == 2048 and hi["tiles"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", STRADDLE, ids=ids(STRADDLE))
def test_route_switch_at_h_req_1024(case):
    """Geometry: test_route_switch_geometry.  Both sides of the switch on one input, each against the reference."""
    test_route_switch_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    slow1, slow0 = run(ctx, dev, 640.0, case["second"], fused=1), run(ctx, dev, 640.0, case["second"], fused=0)
    np.testing.assert_array_equal(slow1, slow0)                    # the same kernels either way
    check(slow1, 1, 640.0, case["second"], case["gen"], "640 Hz scan")
    fast1, fast0 = run(ctx, dev, 650.0, case["second"], fused=1), run(ctx, dev, 650.0, case["second"], fused=0)
    check(fast1, 1, 650.0, case["second"], case["gen"], "650 Hz fused")
    check(fast0, 1, 650.0, case["second"], case["gen"], "650 Hz scan")
    assert np.max(np.abs(fast1 - fast0)) <= fx.ROUTE_TOL * np.max(np.abs(fast0))


# ---- negative and vanishing pole -------------------------------------------------------------------------------------
NEG = fx.negpole_cases()


@pytest.mark.parametrize("case", NEG, ids=ids(NEG))
def test_negative_pole_geometry(case):
    """alpha = (4 - wo) / (4 + wo) <= 0 at and above a quarter of the sampling rate (about 1e-17 of either sign exactly at
    the quarter): the fused route refuses, the scan runs; n = 7: one chunk, lead 4077; 4084: one chunk, lead 0; 12293: 4."""
    g = fx.order1_geometry(case["n"], case["cutoff"], case["second"], 1)
    if case["cutoff"] == case["second"] / 4:
        assert abs(g["alpha"]) < 1e-15
    else:
        assert -1.0 < g["alpha"] < -0.02 and g["route"] == "scan"
    assert (g["n_chunks"], g["lead"]) == {7: (1, 4077), 4084: (1, 0), 12293: (4, 4079)}[case["n"]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", NEG, ids=ids(NEG))
def test_negative_pole(case):
    """Geometry: test_negative_pole_geometry.  Against the long-double reference; filter_fused 1 and 0 give the same bits
    wherever the host restatement says the fused route is not taken (alpha <= 0), 2e-14 where a vanishing positive pole
    takes it."""
    test_negative_pole_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    on, off = run(ctx, dev, case["cutoff"], case["second"], fused=1), run(ctx, dev, case["cutoff"], case["second"], fused=0)
    check(on, 1, case["cutoff"], case["second"], case["gen"], "filter_fused 1")
    check(off, 1, case["cutoff"], case["second"], case["gen"], "filter_fused 0")
    if fx.order1_geometry(case["n"], case["cutoff"], case["second"], 1)["route"] == "scan":
        np.testing.assert_array_equal(on, off)
    else:
        assert np.max(np.abs(on - off)) <= fx.ROUTE_TOL * np.max(np.abs(off))


# ---- three-pass scan ----------------------------------------------------------------------------------------------------
LEAD = fx.scan_lead_cases()
CHUNKS = fx.scan_chunk_cases()


@pytest.mark.parametrize("case", LEAD + CHUNKS, ids=ids(LEAD + CHUNKS))
def test_scan_geometry(case):
    """lead = padded - total is 1, 0, 4095 for n + 12 = 4096 k - 1, 4096 k, 4096 k + 1; n_chunks 1, 2, 1023, 1024, 1025,
    2049 give 1, 1, 1, 1, 2, 3 chunks per thread of the carry kernel."""
    g = fx.order1_geometry(case["n"], case["cutoff"], case["second"], case["fused"])
    assert g["route"] == "scan" and g["lead"] == case["lead"] and g["n_chunks"] == case["n_chunks"]
    assert g["per"] == case.get("per", 1) and g["trips"] == 1


def test_big_scan_geometry():
    """n = 3.4e7: 8 301 chunks, 9 per thread of the carry kernel: its loop of eight takes a second trip."""
    g = fx.order1_geometry(fx.BIG_N, 100.0, fx.SECOND, 1)
    assert g["route"] == "scan" and g["n_chunks"] == 8301 and g["per"] == 9 and g["trips"] == 2 and g["lead"] == 884


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAD, ids=ids(LEAD))
def test_scan_lead(case):
    """Geometry: test_scan_geometry (lead, n_chunks).  Against the long-double reference; a slow cutoff takes the scan
    under either value of filter_fused, with the same bits."""
    test_scan_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    got = run(ctx, dev, case["cutoff"], case["second"], fused=case["fused"])
    check(got, 1, case["cutoff"], case["second"], case["gen"])
    if case["fused"]:
        np.testing.assert_array_equal(got, run(ctx, dev, case["cutoff"], case["second"], fused=0))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHUNKS, ids=ids(CHUNKS))
def test_scan_chunks_per_carry_thread(case):
    """Geometry: test_scan_geometry (n_chunks, per).  Long-double reference up to 2e5 samples, the fp64 oracle beyond, at
    the bound of the input's 2e5 prefix (order 1: the 1e-11 floor)."""
    test_scan_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    check(run(ctx, dev, case["cutoff"], case["second"], fused=case["fused"]), 1, case["cutoff"], case["second"], case["gen"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["i16", "f64"])
def test_scan_carry_loop_second_trip(dtype):
    """Geometry: test_big_scan_geometry (8 301 chunks, per 9, two trips).  Against the fp64 oracle at the bound of the
    suite's large order-1 trace, 1e-10 max |ref|."""
    test_big_scan_geometry()
    ctx = context()
    x, k = fx.make_input(fx.gen_for(dtype, fx.BIG_N, seed=37))
    dev = to_dev(dtype, x, k)
    got = run(ctx, dev, 100.0, fx.SECOND)
    del dev
    ref = oracle.bessel_filtfilt(x, 100.0, fx.SECOND)
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print("carry loop, two trips, %s: %.3e" % (dtype, err))
    assert err <= fx.ORACLE_TOL


# ---- orders 2..8: the halo kernel ------------------------------------------------------------------------------------
HALO = fx.halo_cases()


@pytest.mark.parametrize("case", HALO, ids=ids(HALO))
def test_halo_geometry(case):
    """S = max(1024, 4 H) outputs per thread, 64 threads per workgroup: m = n + 2 pad at S - 1, S, S + 1 (1, 1, 2 segments),
    2 S + 1, 64 S - 1, 64 S (one workgroup), 64 S + 1, 65 S + 3 (two); 2 S + H: the last-but-one segment has
    hi < m <= hi + H, its backward pass starts at the end of the sequence; 2 S + H + 1: the first length where it does not."""
    g = fx.halo_geometry(case["n"], case["order"], case["cutoff"], case["second"])
    S, H, m = g["S"], g["H"], g["m"]
    assert (H, S, m) == (case["H"], case["S"], case["m"]) and 0 < H <= 8192 and H % 64 == 0 and case["n"] > g["pad"]
    want = {"S-1": (S - 1, 1, 1), "S": (S, 1, 1), "S+1": (S + 1, 2, 1), "2S+1": (2 * S + 1, 3, 1), "2S+H": (2 * S + H, 3, 1),
            "2S+H+1": (2 * S + H + 1, 3, 1), "64S-1": (64 * S - 1, 64, 1), "64S": (64 * S, 64, 1), "64S+1": (64 * S + 1, 65, 2),
            "65S+3": (65 * S + 3, 66, 2)}[case["what"]]
    assert (m, g["nseg"], g["groups"]) == want
    hi = (g["nseg"] - 1) * S                               # end of the last-but-one segment
    if case["what"] in ("S+1", "2S+1", "2S+H", "64S+1", "65S+3"):
        assert hi < m <= hi + H
    if case["what"] == "2S+H+1":
        assert m == hi + H + 1


def test_halo_filters_found_by_search():
    order, cutoff = fx.halo_filters()[-1]
    assert order == 5 and 4096 < fx.halo_of(order, cutoff, fx.SECOND) <= 8192
    assert [fx.halo_of(o, c, fx.SECOND) for o, c in fx.HALO_FILTERS] == [c["H"] for c in HALO if c["what"] == "S" and c["dtype"] == "i16"][:4]
    order, cutoff = fx.refused_filter()
    assert order == 3 and fx.halo_of(order, cutoff, fx.SECOND) == 0
    assert fx.halo_of(order, round(cutoff / 0.98 ** 2, 1), fx.SECOND) > 4096       # (just above it: a long halo, not none)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALO, ids=ids(HALO))
def test_halo_seams(case):
    """Geometry: test_halo_geometry (H, S, m, nseg, workgroups).  Long-double reference up to 2e5 samples; longer inputs
    against the fp64 oracle at 4 err_ref of their 2e5 prefix."""
    test_halo_geometry(case)
    ctx = context()
    x, k = fx.make_input(case["gen"])
    dev = to_dev(case["dtype"], x, k)
    check(run(ctx, dev, case["cutoff"], case["second"], order=case["order"]), case["order"], case["cutoff"], case["second"], case["gen"])


@pytest.mark.gpu
def test_halo_refusal_leaves_the_context_usable():
    """An order-3 filter whose state no halo up to 8192 forgets (test_halo_filters_found_by_search) is refused on the host;
    the 2 kHz order-1 filter right after it is correct (fused, H 384, T 3328, two full tiles)."""
    import torch
    ctx = context()
    order, cutoff = fx.refused_filter()
    assert fx.halo_of(order, cutoff, fx.SECOND) == 0
    case = [c for c in FUSED if c["id"] == "2000Hz-2T+0-i16"][0]
    x, k = fx.make_input(case["gen"])
    for dev in (to_dev("i16", x, k), to_dev("f32", x, k), torch.from_numpy(x).cuda()):
        with pytest.raises(ValueError, match="does not run on the device"):
            ctx.filter_bessel(dev, Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order)
    check(run(ctx, to_dev("i16", x, k), 2000.0, fx.SECOND), 1, 2000.0, fx.SECOND, case["gen"])


# ---- status and addressing ----------------------------------------------------------------------------------------------
ROUTES3 = [("fused", 1, 2000.0), ("scan", 1, 100.0), ("halo", 3, 2000.0)]
N_STATUS = 20_000


def test_status_routes_geometry():
    """2 kHz: fused, T = 3328 (sample 3332 lies in tile 1 and in the right halo of tile 0, sample 5000 in the middle of
    tile 1); 100 Hz: the scan, 5 chunks; order 3 at 2 kHz: the halo kernel."""
    g = fx.order1_geometry(N_STATUS, 2000.0, fx.SECOND, 1)
    assert g["route"] == "fused" and g["T"] == 3328 and g["H"] == 384 and g["tiles"] == 7
    assert g["T"] <= 3332 + 6 < g["T"] + g["H"] and g["T"] + g["H"] < 5000 + 6 < 2 * g["T"] - g["H"]
    assert fx.order1_geometry(N_STATUS, 100.0, fx.SECOND, 1)["route"] == "scan"
    assert fx.halo_geometry(N_STATUS, 3, 2000.0, fx.SECOND)["nseg"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [0, N_STATUS - 1, 5000, 3332], ids=["first", "last", "mid-tile", "halo"])
@pytest.mark.parametrize("route", ROUTES3, ids=[r[0] for r in ROUTES3])
def test_off_grid_sample_raises_on_every_route(route, pos):
    """Geometry: test_status_routes_geometry.  One fp32 sample half a quantum off the grid -- also index 0 and n - 1,
    which every thread loads for the odd extension -- raises the library's off-grid error; the next clean call on the
    same context succeeds with the bits it had before."""
    import torch
    test_status_routes_geometry()
    _, order, cutoff = route
    ctx = context()
    _, k = fx.make_input(fx.gen_for("f32", N_STATUS))
    clean = (k * Q).astype(np.float32)
    dirty = clean.copy()
    dirty[pos] += np.float32(Q / 2)
    assert dirty[pos] != clean[pos]
    before = ctx.filter_bessel(torch.from_numpy(clean).cuda(), Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order).cpu().numpy()
    with pytest.raises(ValueError, match=OFF_GRID):
        ctx.filter_bessel(torch.from_numpy(dirty).cuda(), Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order)
    after = ctx.filter_bessel(torch.from_numpy(clean).cuda(), Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order).cpu().numpy()
    np.testing.assert_array_equal(before, after)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,start", [("i16", 1), ("i16", 3), ("f32", 1), ("f32", 3), ("f64", 1)])
@pytest.mark.parametrize("route", ROUTES3, ids=[r[0] for r in ROUTES3])
def test_views_at_odd_elements(route, dtype, start):
    """dev[1:] and dev[3:] (2-, 4- and 8-byte samples at an odd element of their allocation) give the bits of the same
    data in a tensor of its own.  n = 9001: 3 fused tiles, 3 chunks, several halo segments."""
    _, order, cutoff = route
    ctx = context()
    x, k = fx.make_input(fx.gen_for(dtype, 9001 + start))
    dev = to_dev(dtype, x, k)
    view = dev[start:]
    fresh = view.clone()
    assert view.data_ptr() == dev.data_ptr() + start * dev.element_size() and fresh.data_ptr() != view.data_ptr()
    a = ctx.filter_bessel(view, Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order).cpu().numpy()
    b = ctx.filter_bessel(fresh, Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(a)) and a.shape == (9001,)


# ---- the batch entry ------------------------------------------------------------------------------------------------------
BATCHES = [(1, "ascending"), (2, "ascending"), (2, "descending"), (40, "ascending"), (40, "descending"), (40, "shuffled")]


@pytest.mark.parametrize("route", fx.BATCH_ROUTES, ids=[r[0] for r in fx.BATCH_ROUTES])
def test_batch_geometry(route):
    """Routes by the host restatement; events: odd starts, lengths padlen + 1 .. 3e5, two overlapping, inside the trace,
    in ascending, descending and shuffled length."""
    _, order, cutoff, want = route
    padlen = 3 * (order + 1)
    if order == 1:
        assert fx.order1_geometry(50_001, cutoff, fx.SECOND, 1)["route"] == want
    else:
        assert want == "halo" and fx.halo_of(order, cutoff, fx.SECOND) > 0
    for n_ev, arr in BATCHES:
        st, ln = fx.batch_events(order, n_ev, arr)
        assert len(st) == len(ln) == n_ev and np.all(st % 2 == 1) and np.all(st + ln <= fx.BATCH_TRACE_N) and ln.min() > padlen
        assert fx.BATCH_CHECKED in list(zip(st.tolist(), ln.tolist()))
        if n_ev > 1:
            assert ln.min() == padlen + 1
            assert {"ascending": np.all(np.diff(ln) >= 0), "descending": np.all(np.diff(ln) <= 0),
                    "shuffled": np.any(np.diff(ln) > 0) and np.any(np.diff(ln) < 0)}[arr]
        if n_ev == 40:
            assert ln.max() == 300_000
            a, b = [i for i in range(40) if ln[i] in (fx.BATCH_CHECKED[1], 300_000)]
            assert max(st[a], st[b]) < min(st[a] + ln[a], st[b] + ln[b])               # overlapping


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", fx.DTYPES)
@pytest.mark.parametrize("route", fx.BATCH_ROUTES, ids=[r[0] for r in fx.BATCH_ROUTES])
def test_batch_equals_the_single_calls(route, dtype):
    """Geometry: test_batch_geometry.  ctx.filter_requantise_batch on one device trace: every event's filtered current is
    bit-equal to ctx.filter_bessel on that stretch alone (the same kernels on the same scratch, in order), its (rounded,
    centre, step) equal ctx.requantise of that current; one event is also held to the long-double reference."""
    test_batch_geometry(route)
    _, order, cutoff, _ = route
    ctx = context()
    x, k = fx.make_input(fx.batch_gen(dtype, sliced=False))
    dev = to_dev(dtype, x, k)
    oc = fx.BATCH_OFFSET if dtype == "i16" else 0
    single = {}
    for n_ev, arr in BATCHES:
        st, ln = fx.batch_events(order, n_ev, arr)
        filt, rnd, off, centre, step = ctx.filter_requantise_batch(dev, st, ln, Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order,
                                                                   offset_counts=oc)
        filt, rnd = filt.cpu().numpy(), rnd.cpu().numpy()
        assert off[-1] == ln.sum() == filt.size == rnd.size
        for e in range(n_ev):
            s, l = int(st[e]), int(ln[e])
            if (s, l) not in single:
                y = ctx.filter_bessel(dev[s:s + l], Q, cutoff=cutoff, sampling_freq=fx.SECOND, order=order, offset_counts=oc)
                z, c, sp = ctx.requantise(y)
                single[(s, l)] = (y.cpu().numpy(), z.cpu().numpy(), c, sp)
            y, z, c, sp = single[(s, l)]
            np.testing.assert_array_equal(filt[off[e]:off[e + 1]], y, err_msg="event %d of %d (%s)" % (e, n_ev, arr))
            np.testing.assert_array_equal(rnd[off[e]:off[e + 1]], z, err_msg="event %d of %d (%s)" % (e, n_ev, arr))
            assert (centre[e], step[e]) == (c, sp)
    check(single[fx.BATCH_CHECKED][0], order, cutoff, fx.SECOND, fx.batch_gen(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("route", fx.BATCH_ROUTES, ids=[r[0] for r in fx.BATCH_ROUTES])
def test_batch_refusals_reset_the_context(route):
    """A batch with one event of padlen samples, and one with one off-grid fp32 event, raise ValueError; the next batch on
    the same context returns what it returned before them (defer_sync and the status word are reset)."""
    import torch
    _, order, cutoff, _ = route
    ctx = context()
    _, k = fx.make_input(fx.batch_gen("f32", sliced=False))
    clean = (k * Q).astype(np.float32)
    dev = torch.from_numpy(clean).cuda()
    st, ln = fx.batch_events(order, 40, "shuffled")
    kw = dict(cutoff=cutoff, sampling_freq=fx.SECOND, order=order)
    good = [t.cpu().numpy() if hasattr(t, "cpu") else np.array(t) for t in ctx.filter_requantise_batch(dev, st, ln, Q, **kw)]
    short = ln.copy()
    short[17] = 3 * (order + 1)
    with pytest.raises(ValueError, match=BAD_ARG):
        ctx.filter_requantise_batch(dev, st, short, Q, **kw)
    again = [t.cpu().numpy() if hasattr(t, "cpu") else np.array(t) for t in ctx.filter_requantise_batch(dev, st, ln, Q, **kw)]
    for a, b in zip(good, again):
        np.testing.assert_array_equal(a, b)
    dirty = clean.copy()
    e = int(np.argmin(ln))                                  # the shortest event: queued last
    dirty[st[e] + ln[e] // 2] += np.float32(Q / 2)
    with pytest.raises(ValueError, match=OFF_GRID):
        ctx.filter_requantise_batch(torch.from_numpy(dirty).cuda(), st, ln, Q, **kw)
    again = [t.cpu().numpy() if hasattr(t, "cpu") else np.array(t) for t in ctx.filter_requantise_batch(dev, st, ln, Q, **kw)]
    for a, b in zip(good, again):
        np.testing.assert_array_equal(a, b)


# ---- re-quantisation ------------------------------------------------------------------------------------------------------
RQ_STATS_CAP = 1024 * 8 * 256            # requant_stats_kernel: min(1024, ceil(n / 2048)) workgroups
RQ_ROUND_CAP = 65535 * 4 * 256           # requant_round_kernel: min(65535, ceil(n / 1024)) workgroups
RQ_N = [RQ_STATS_CAP - 1, RQ_STATS_CAP, RQ_STATS_CAP + 1, 68_000_001]


def host_fine_grid(x):
    """DataTypes.Event._on_fine_grid on a bare current."""
    from pypore_amd.DataTypes import Event
    return Event._on_fine_grid(types.SimpleNamespace(current=x))


def test_requantise_grid_caps_geometry():
    """2 097 151 and 2 097 152 samples: 1 024 workgroups of the statistics kernel, one trip; 2 097 153: capped, a second
    trip; 68 000 001 > 65 535 * 1 024 = 67 107 840: the rounding kernel's cap too."""
    assert RQ_STATS_CAP == 2_097_152 and RQ_ROUND_CAP == 67_107_840
    assert [min(1024, (n + 2047) // 2048) for n in RQ_N] == [1024] * 4 and [(n + 2047) // 2048 > 1024 for n in RQ_N] == [False, False, True, True]
    assert [(n + 1023) // 1024 > 65535 for n in RQ_N] == [False, False, False, True]


@pytest.mark.gpu
@pytest.mark.parametrize("n", RQ_N)
def test_requantise_beyond_the_grid_caps(n):
    """Geometry: test_requantise_grid_caps_geometry.  Against DataTypes.Event._on_fine_grid: the same step, every value on
    the grid, one constant shift of at most one step (the two means may differ in the last bits), |count| < 2**22."""
    import torch
    test_requantise_grid_caps_geometry()
    ctx = context()
    rng = np.random.default_rng(n % 1000)
    x = rng.standard_normal(n)
    np.cumsum(x, out=x)
    x *= 40.0 / np.sqrt(n)
    x += 55.0 + 0.4 * rng.standard_normal(n)
    rounded, step, _ = host_fine_grid(x)
    z, centre, dstep = ctx.requantise(torch.from_numpy(x).cuda())
    z = z.cpu().numpy().astype(np.float64)
    assert z.shape == (n,) and dstep == step and np.abs(z).max() < 2 ** 22 * step
    np.testing.assert_array_equal(np.rint(z / step) * step, z)
    shift = np.rint((rounded - z) / step)
    assert shift.min() == shift.max() and abs(shift[0]) <= 1
    assert abs(centre - np.mean(x)) <= step


@pytest.mark.gpu
def test_requantise_at_power_of_two_spans():
    """Spans of exactly 2**k / 1.01 and the floats next to it: the step doubles there.  The current is symmetric about 0,
    so both sides centre on 0 and the rounded values must be equal, not only the step."""
    import torch
    ctx = context()
    rng = np.random.default_rng(5)
    for k in (-3, 0, 7):
        steps = set()
        for u in (-16, -2, -1, 0, 1, 2, 16):               # (16 ulps: beyond the rounding of log2 near k)
            span = 2.0 ** k / 1.01
            for _ in range(abs(u)):
                span = float(np.nextafter(span, np.inf if u > 0 else -np.inf))
            v = span * rng.random(2047)
            x = np.concatenate(([span, -span], v, -v))
            rounded, step, c0 = host_fine_grid(x)
            z, centre, dstep = ctx.requantise(torch.from_numpy(x).cuda())
            assert step == 2.0 ** (int(np.ceil(np.log2(span * 1.01))) - 22) and dstep == step and centre == c0 == 0.0
            np.testing.assert_array_equal(z.cpu().numpy().astype(np.float64), rounded)
            steps.add(step)
        assert steps == {2.0 ** (k - 22), 2.0 ** (k - 21)}


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_requantise_rejects_non_finite(bad):
    import torch
    ctx = context()
    x = np.linspace(-1.0, 1.0, 5000)
    for pos in (0, 2500, 4999):
        y = x.copy()
        y[pos] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            ctx.requantise(torch.from_numpy(y).cuda())
    z, _, step = ctx.requantise(torch.from_numpy(x).cuda())
    assert step == 2.0 ** -21 and float(z.abs().max()) == 1.0
