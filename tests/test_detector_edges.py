"""Event detection at its edges, on every route, against oracle.lambda_events on the float64 values.

Routes: ps_detect_events (edge_scan_kernel -> piece_minmax_kernel -> events_from_edges), ps_detect_segment_trace with
single_pass 1 (K0's 2-bit block classes -> edge_cls_kernel) and with single_pass 0 (the two calls).  Cases: noise that
chatters across the threshold, edges planted at every residue of the 8-sample blocks, of DET_PER, of an edge_cls_kernel
lane's 512 samples and of DET_CHUNK, every n mod 8, min_duration / min_current / threshold boundaries, the edge-list
overflow rerun on fresh contexts, unaligned views, int16 rails and counts too wide for the single pass."""
import numpy as np
import pytest

import oracle
from pypore_amd import _lib, synth

Q = synth.QUANTUM                      # 2^-5 pA per count: 90 pA is count 2880
KTHR = 2880
HI, LO = 3520, 1440                    # open channel 110 pA, blockade 45 pA
PARAMS = dict(prior_segments_per_second=10., min_width=100, max_width=1000000, window_width=10000)
ROUTES = [("int16", 0), ("int16", 1234), ("int16", -1234), ("float32", 0), ("float32", 1234)]


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: no state left by other modules (a wide trace puts a context on the two calls for
    the next calls of its quantum), and none left for them."""
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _upload(k, dtype, oc, pad=0):
    """Counts k -> (CUDA tensor the kernels read as k, float64 pA the oracle reads).  int16: k - oc with offset_counts oc;
    float32: k * Q (offset_counts is not added to float samples).  pad > 0: a view `pad` elements into a larger buffer."""
    import torch
    k = np.asarray(k, dtype=np.int64)
    if dtype == "int16":
        raw = k - oc
        assert raw.min(initial=0) >= -32768 and raw.max(initial=0) <= 32767
        host = raw.astype(np.int16)
    else:
        host = (k * Q).astype(np.float32)
    buf = torch.from_numpy(np.concatenate([np.zeros(pad, host.dtype), host, np.zeros(8, host.dtype)])).cuda()
    return buf[pad:pad + k.size], k.astype(np.float64) * Q


def _check(ctx, k, dtype="int16", oc=0, threshold=90.0, min_duration=0, min_current=-0.5, pad=0, wide=False, want=None):
    """Every route against the oracle; the single pass's boundaries against the two calls'.  Returns (starts, lengths)."""
    t, x = _upload(k, dtype, oc, pad)
    if pad:
        assert t.data_ptr() % 16 != 0
    rs, rl = oracle.lambda_events(x, threshold=threshold, min_duration=min_duration, min_current=min_current)
    if want is not None:
        assert list(zip(rs.tolist(), rl.tolist())) == want           # (the case is what it says it is)
    params = _lib.split_params(**PARAMS)
    # (the single pass first: a wide trace's segment_events would put the context on the two calls for the next calls)
    s1, l1, b1, o1, _ = ctx.detect_segment_trace(t, Q, params, threshold, min_duration, min_current, oc)
    assert (ctx.timings()["wide_redo"] == 3) == wide, "no fallback to the two calls" if wide else "the single pass fell back"
    np.testing.assert_array_equal(s1, rs)
    np.testing.assert_array_equal(l1, rl)
    st, ln = ctx.detect_events(t, Q, threshold, min_duration, min_current, oc)
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(ln, rl)
    ctx.set_option("single_pass", 0)
    try:
        s0, l0, b0, o0, _ = ctx.detect_segment_trace(t, Q, params, threshold, min_duration, min_current, oc)
    finally:
        ctx.set_option("single_pass", 1)
    np.testing.assert_array_equal(s0, rs)
    np.testing.assert_array_equal(l0, rl)
    np.testing.assert_array_equal(o1, o0)
    np.testing.assert_array_equal(b1.cpu().numpy(), b0.cpu().numpy())
    if len(st):
        b2, o2, _ = ctx.segment_events(t, st, ln, params, Q, oc)
        np.testing.assert_array_equal(o1, o2)
        np.testing.assert_array_equal(b1.cpu().numpy(), b2.cpu().numpy())
    return rs, rl


def _steps(n, toggles, start_below=False, seed=0, noise=3):
    """Counts that alternate between the open channel and a blockade at the sample positions `toggles` (an edge at each),
    with noise that never reaches the threshold."""
    rng = np.random.default_rng(seed)
    lvl = np.zeros(n, dtype=np.int64)
    for p in sorted(set(int(p) for p in toggles if 0 < p < n)):
        lvl[p:] ^= 1
    below = lvl == 1 if not start_below else lvl == 0
    return np.where(below, LO, HI) + rng.integers(-noise, noise + 1, n)


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
def test_chatter_across_the_threshold(ctx, dtype, oc):
    """Noise straddling the threshold around long blockades: several edges in one 8-sample block, runs of mixed blocks,
    crossings on the block boundaries between mixed and uniform blocks."""
    rng = np.random.default_rng(100 + oc % 7)
    n = 200003
    k = HI + rng.integers(-40, 41, n)
    k[30000:90000] = LO + rng.integers(-40, 41, 60000)
    k[120000:190000] = LO + rng.integers(-40, 41, 70000)
    for a in (29000, 89000, 119003, 189005):                      # 1000 samples of chatter at every transition
        k[a:a + 1000] = KTHR + rng.integers(-3, 3, 1000)
    k[60000:60008] = [KTHR - 1, KTHR, KTHR - 1, KTHR, KTHR - 1, KTHR, KTHR - 1, KTHR]   # 8 edges in one block
    k[70000:70016] = KTHR                                         # a uniform block at the threshold between mixed ones
    k[70016:70024] = KTHR - 1
    k[70008:70009] = KTHR - 1
    # crossings exactly on block boundaries: uniform above | mixed, below first and above last | uniform below | mixed, above
    # first and below last | ...
    up, dn = KTHR, KTHR - 1
    blocks = ([up] * 8, [dn, up, dn, up, up, up, up, up], [dn] * 8, [up, dn, up, dn, dn, dn, dn, dn])
    for j, b in enumerate(range(150000, 150800, 8)):
        k[b:b + 8] = blocks[j % 4]
    for md in (0, 5, 1000):
        _check(ctx, k, dtype, oc, min_duration=md)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
@pytest.mark.parametrize("start_below", [False, True])
def test_edges_at_every_residue_and_seam(ctx, dtype, oc, start_below):
    n = 4096 * 17 + 123
    toggles = {1, n - 1}
    toggles |= {1000 + 17 * j for j in range(64)}                                    # every residue mod 8 and mod 16
    toggles |= {512 * m + d for m in (1, 2, 62, 63, 64, 65, 127, 128) for d in (-8, -1, 0, 1, 8)}   # lane 0 / 63, thread seams
    toggles |= {4096 * c + d for c in range(1, 17) for d in (-9, -8, -1, 0, 1, 7, 8, 4000)}        # DET_CHUNK ragged ends
    k = _steps(n, toggles, start_below, seed=oc & 0xff)
    edges = np.flatnonzero((k[1:] < KTHR) != (k[:-1] < KTHR)) + 1
    assert {int(e) % 8 for e in edges} == set(range(8)) and {int(e) % 16 for e in edges} == set(range(16))
    assert {1, n - 1, 4096, 512 * 63, 512 * 64} <= set(edges.tolist())
    for md in (0, 7, 300):
        _check(ctx, k, dtype, oc, min_duration=md)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
def test_every_length_and_n_mod_8(ctx, dtype, oc):
    ns = list(range(1, 18)) + [4095, 4096, 4097] + [4096 * 2 + r for r in range(8)] + [8 * 1000 + r for r in range(8)]
    for n in ns:
        inside = _steps(n, [n // 2], seed=n)                     # ends inside an event
        _check(ctx, inside, dtype, oc)
        _check(ctx, _steps(n, [n // 3, (2 * n) // 3], start_below=True, seed=n), dtype, oc)   # starts below the threshold
        _check(ctx, np.full(n, LO), dtype, oc, want=[(0, n)])     # one event: the whole trace


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
def test_min_duration_and_min_current_boundaries(ctx, dtype, oc):
    n = 20000
    k = _steps(n, [3001, 3001 + 1000, 9005, 9005 + 2000, 15000, 15000 + 1500], seed=1)
    _check(ctx, k, dtype, oc, min_duration=1000, want=[(9005, 2000), (15000, 1500)])      # exactly min_duration: rejected
    _check(ctx, k, dtype, oc, min_duration=999, want=[(3001, 1000), (9005, 2000), (15000, 1500)])
    # min_current -0.5 pA is count -16: an event whose minimum is exactly there is rejected, one count above it is kept
    k2 = k.copy()
    k2[9500] = -16
    k2[15700] = -15
    _check(ctx, k2, dtype, oc, min_duration=999, want=[(3001, 1000), (15000, 1500)])
    _check(ctx, k2, dtype, oc, min_duration=999, min_current=-16.5 * Q, want=[(3001, 1000), (9005, 2000), (15000, 1500)])
    _check(ctx, k2, dtype, oc, min_duration=999, min_current=-15 * Q, want=[(3001, 1000)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
def test_thresholds_at_beyond_and_between_counts(ctx, dtype, oc):
    rng = np.random.default_rng(5)
    n = 50000
    k = KTHR + rng.integers(-2, 3, n)
    k[10000:30000] = KTHR - 1 + rng.integers(-1, 1, 20000)
    for thr in (1.0e4, -100.0, 90.0, 90.0 - Q, 90.0 + Q, 90.0 + Q / 2, 90.0 - Q / 3, (KTHR + 2) * Q, (KTHR - 2.5) * Q):
        for md in (0, 3000):
            _check(ctx, k, dtype, oc, threshold=thr, min_duration=md)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_edge_list_overflow_reruns_on_fresh_contexts(ctx, dtype):
    """More than 65 536 edges: detect_edges' first attempt overflows on a fresh context (det_tics only grows) and reruns
    with room for all of them -- on both routes, with the shared context's result."""
    from pypore_amd import engine
    rng = np.random.default_rng(9)
    n = 400000
    runs = rng.integers(1, 5, n // 2)
    lvl = np.repeat(np.arange(runs.size) & 1, runs)[:n]
    k = np.where(lvl == 1, KTHR - 1 - rng.integers(0, 30, lvl.size), KTHR + rng.integers(0, 30, lvl.size))
    k[100000:300000] = LO + rng.integers(-40, 41, 200000)
    edges = np.count_nonzero((k[1:] < KTHR) != (k[:-1] < KTHR))
    assert edges > 65536 + 4096
    t, x = _upload(k, dtype, 0)
    params = _lib.split_params(**PARAMS)
    want = _check(ctx, k, dtype, 0, min_duration=1000)
    assert len(want[0]) == 1
    for route in ("detect_events", "detect_segment_trace"):
        fresh = engine.Context(0)
        try:
            if route == "detect_events":
                st, ln = fresh.detect_events(t, Q, 90.0, 1000, -0.5)
            else:
                st, ln, b, o, _ = fresh.detect_segment_trace(t, Q, params, 90.0, 1000, -0.5)
                assert fresh.timings()["wide_redo"] != 3
                b2, o2, _ = ctx.segment_events(t, st, ln, params, Q)
                np.testing.assert_array_equal(b.cpu().numpy(), b2.cpu().numpy())
            np.testing.assert_array_equal(st, want[0])
            np.testing.assert_array_equal(ln, want[1])
        finally:
            fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,oc", ROUTES)
@pytest.mark.parametrize("pad", [1, 3])
def test_unaligned_views(ctx, dtype, oc, pad):
    n = 4096 * 5 + 37
    toggles = {4096 * c + d for c in range(1, 5) for d in (-1, 0, 1, 5)} | {3, 17, 515, n - 2}
    k = _steps(n, toggles, seed=pad)
    _check(ctx, k, dtype, oc, pad=pad)
    _check(ctx, k, dtype, oc, pad=pad, min_duration=2000)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_int16_rails_and_counts_too_wide_for_the_single_pass(dtype):
    """|k - k_0| >= 2^14 about the trace's first sample: the single pass takes the two calls itself (wide_redo == 3) and is
    still right.  Counts at the int16 rails.  (A context of its own: a wide trace leaves the context on the two calls for
    later calls of the same quantum.)"""
    from pypore_amd import engine
    rng = np.random.default_rng(2)
    n = 60000
    k = HI + rng.integers(-40, 41, n)
    k[10000:25000] = -32768 + rng.integers(0, 3, 15000)           # a blockade at the lower rail
    k[40000:52000] = LO + rng.integers(-40, 41, 12000)
    k[30000:30010] = 32767                                        # the upper rail in the open channel
    fresh = engine.Context(0)
    try:
        _check(fresh, k, dtype, 0, min_duration=1000, min_current=-1.0e4, wide=True, want=[(10000, 15000), (40000, 12000)])
    finally:
        fresh.close()
    fresh = engine.Context(0)
    try:
        # narrow: every count within 2^14 of the first -- no fallback, counts near the rail with an offset
        k2 = 32767 - 200 + rng.integers(-40, 41, n)
        k2[30000:30010] = 32767
        k2[10000:25000] = 32767 - 16000 + rng.integers(0, 3, 15000)
        k2[40000:52000] = 32767 - 16000 + rng.integers(0, 40, 12000)
        assert np.abs(k2 - k2[0]).max() < 1 << 14
        _check(fresh, k2, dtype, 0, threshold=(32767 - 8000) * Q, min_duration=1000, wide=False,
               want=[(10000, 15000), (40000, 12000)])
        if dtype == "int16":
            _check(fresh, k2 + 1234, dtype, 1234, threshold=(32767 - 8000 + 1234) * Q, min_duration=1000, wide=False,
                   want=[(10000, 15000), (40000, 12000)])
    finally:
        fresh.close()


# ---- the public surface: the caller's float64 values decide, whatever grid they lie on ----------------------------------

def _events(segs):
    return [(int(s.start), int(s.duration)) for s in segs]


def _default_rules(threshold):
    from pypore_amd.parsers import lambda_event_parser as P
    return P(threshold=threshold, rules=[lambda e: e.duration > P.MIN_DURATION, lambda e: e.min > P.MIN_CURRENT,
                                         lambda e: e.max < threshold])


@pytest.mark.gpu
def test_decimal_resolution_through_the_parser():
    """float64 at 0.1 pA (no power-of-two grid, the counts of a recovered affine grid go up): a sample of exactly 90.0 is not
    below threshold=90."""
    from pypore_amd.parsers import lambda_event_parser
    rng = np.random.default_rng(0)
    x = np.round(110 + rng.normal(0, 1.5, 300000), 1)
    x[100000:250000] = np.round(45 + rng.normal(0, 1.5, 150000), 1)
    x[250000] = 90.0
    got = _events(lambda_event_parser(threshold=90).parse(x))
    rs, rl = oracle.lambda_events(x, threshold=90.0)
    assert got == _events(_default_rules(90).parse(x)) == list(zip(rs.tolist(), rl.tolist())) == [(100000, 150000)]


def _abf_with_a_threshold_sample(path):
    """An .abf with an inexact header scale and a non-zero offset, and a threshold t equal to the value of the sample that
    ends its blockade, chosen where fl(k q) < t - offset although x = fl(fl(k q) + offset) == t (searched for)."""
    from pypore_amd import abf
    rng = np.random.default_rng(12)
    n = 300000
    path = abf.write_abf(path, np.zeros(16, np.int16), adc_range=10.0, adc_resolution=32768, instrument_scale=0.0005,
                         signal_gain=20.0, instrument_offset=1.75)
    _, _, q, o = abf.read_abf_counts(path)
    kk = np.arange(1, 32767)
    xs = kk * q + o
    hard = kk[(kk * q < xs - o) & (xs > 50) & (xs < 100)]
    assert hard.size, "no count of this grid where the thresholds in count space part"
    kt = int(hard[0])
    k = np.rint((110 + rng.normal(0, 1.5, n)) / q).astype(np.int64)
    k[100000:250000] = np.rint((45 + rng.normal(0, 1.5, 150000)) / q)
    k[250000] = kt
    path = abf.write_abf(path, k.astype(np.int16), adc_range=10.0, adc_resolution=32768, instrument_scale=0.0005,
                         signal_gain=20.0, instrument_offset=1.75)
    return path, float(kt * q + o)


@pytest.mark.gpu
def test_abf_with_inexact_scale_and_offset_at_a_sample_valued_threshold(tmp_path):
    from pypore_amd import abf, pipeline
    from pypore_amd.DataTypes import File
    from pypore_amd.parsers import lambda_event_parser
    path, t = _abf_with_a_threshold_sample(str(tmp_path / "t.abf"))
    _, x = abf.read_abf(path)
    assert x[250000] == t
    rs, rl = oracle.lambda_events(np.asarray(x), threshold=t)
    want = list(zip(rs.tolist(), rl.tolist()))
    assert want == [(100000, 150000)] == _events(_default_rules(t).parse(np.asarray(x)))
    assert _events(lambda_event_parser(threshold=t).parse(x)) == want
    f = File(path)
    f.parse(lambda_event_parser(threshold=t))
    rate = f.second
    assert [(int(np.rint(e.start * rate)), int(np.rint(e.duration * rate))) for e in f.events] == want
    _, st, ln, _ = pipeline.parse_abf(path, threshold=t)
    assert list(zip(st.tolist(), ln.tolist())) == want
