"""Per-segment statistics on the device (K2: segstat_bs_kernel on the narrow digest, segstat_kernel on the wide digest and
the LDS-window route) against the exact integer statistics of tests/segstat_exact.py, at the oracle's boundaries, on every
route -- the route that ran asserted from the context's counters -- with int16 and float32 input.  The geometry each route
must cover is asserted here too, so that dropping a case fails instead of passing quietly."""
import os

import numpy as np
import pytest

import oracle
import segstat_exact as se
from pypore_amd import _lib, synth

pytestmark = pytest.mark.gpu

NARROW = dict(min_width=8, max_width=1000000, window_width=2000, prior_segments_per_second=10.)
WIDE = dict(min_width=100, max_width=1000000, window_width=10000, prior_segments_per_second=10.)
LDS = dict(min_width=7, max_width=1000000, window_width=2000, prior_segments_per_second=10.)
Q_FINE = 2.0 ** -15


@pytest.fixture
def ctx():
    """A context of its own per test: the wide-route memory of a context (the next calls on a grid start where the last
    one ended) must not carry a route from one test into the next."""
    from pypore_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _upload(k, dtype, q, offset_counts=0):
    import torch
    if dtype == "int16":
        raw = np.asarray(k, dtype=np.int64) - offset_counts
        assert raw.min(initial=0) >= -32768 and raw.max(initial=0) <= 32767
        return torch.from_numpy(raw.astype(np.int16)).cuda()
    kk = np.asarray(k, dtype=np.int64)
    assert np.abs(kk).max(initial=0) < 2 ** 23
    return torch.from_numpy((kk.astype(np.float64) * q).astype(np.float32)).cuda()


def _check_call(events, b, boff, st, q, kw, k_tr0, what):
    """Boundaries of every event equal the oracle's, every row passes check_rows.  Returns the segments' ranges per event."""
    b = b.cpu().numpy()
    st = st.cpu().numpy()
    out = []
    for e, k in enumerate(events):
        ref_b = oracle.parse(np.asarray(k, dtype=np.float64) * q, **kw) if len(k) else np.zeros(0, np.int32)
        np.testing.assert_array_equal(b[boff[e]:boff[e + 1]], ref_b, err_msg="%s, event %d" % (what, e))
        r = se.ranges_of(np.concatenate(([0], ref_b, [len(k)])))
        rows = st[boff[e] + e:boff[e + 1] + e + 1]
        k0 = int(k[0]) if len(k) else 0
        se.assert_rows(rows, se.Exact(k, r, q), (k0, k_tr0 if k_tr0 is not None else k0), "%s, event %d" % (what, e))
        out.append(r)
    return out


def _batch(ctx, events, dtype, q, kw, offset_counts=0):
    buf = np.concatenate([np.asarray(k, dtype=np.int64) for k in events]) if events else np.zeros(0, np.int64)
    off = np.concatenate(([0], np.cumsum([len(k) for k in events]))).astype(np.int64)
    t = _upload(buf, dtype, q, offset_counts)
    b, boff, st = ctx.segment_batch(t, off, _lib.split_params(**kw), q, offset_counts=offset_counts if dtype == "int16" else 0)
    return b, boff, st


def _quiet(seed, centre, n_seg=8):
    return se.quiet_trace(seed, n_seg=n_seg, centre=centre)


# ---- route 1: the narrow digest (segstat_bs_kernel) ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_narrow_digest_geometry_sweep(dtype, ctx):
    """One event that is the whole trace and ends on a chunk multiple: every (a mod 8, b mod 8), lengths 8..40, segments
    within one chunk, across one and many, starting and ending on a chunk boundary, the last one at the trace's end."""
    centre, q, sigma = (1500, synth.QUANTUM, 12.0) if dtype == "int16" else (200_000, Q_FINE, 40.0)
    k = se.narrow_trace(11, centre=centre, sigma=sigma)
    k = k[:len(k) // se.CHUNK * se.CHUNK]
    b, boff, st = _batch(ctx, [k], dtype, q, NARROW)
    tm = ctx.timings()
    assert tm["wide_redo"] == 0 and tm["near_ties"] >= 0                 # the block-sum scan on the 32-bit digest
    (r,) = _check_call([k], b, boff, st, q, NARROW, None, "narrow " + dtype)
    cov = se.coverage(r)
    assert len(cov["pairs"]) == 64
    assert set(range(8, 41)) <= cov["lengths"]
    assert all(cov[c] for c in ("in_one_chunk", "across_one", "across_many", "starts_on_chunk", "ends_on_chunk"))
    assert r[-1][1] == len(k) and len(k) % se.CHUNK == 0


@pytest.mark.parametrize("offset_counts", [20000, -20000])
def test_narrow_digest_int16_rails_short_empty_and_quiet_events(offset_counts, ctx):
    """int16 at both rails (clipped: constant segments at the rail), events of 0..7 samples (shorter than min_width), a
    constant event and, with the positive offset, quiet segments at ~30 000 counts."""
    rng = np.random.default_rng(5 + (offset_counts > 0))
    top, bottom = 32767 + offset_counts, -32768 + offset_counts
    events = [np.clip(se.narrow_trace(21, centre=top - 300)[:20000], bottom, top),
              np.clip(se.narrow_trace(22, centre=bottom + 300)[:20000], bottom, top)]
    events += [rng.integers(-50, 50, n) + offset_counts for n in range(0, 8)]
    events.append(np.full(5000, offset_counts + 77))
    if offset_counts > 0:
        events.append(_quiet(31, 30000))
    b, boff, st = _batch(ctx, events, "int16", synth.QUANTUM, NARROW, offset_counts)
    tm = ctx.timings()
    assert tm["wide_redo"] == 0 and tm["near_ties"] >= 0
    _check_call(events, b, boff, st, synth.QUANTUM, NARROW, None, "narrow rails %d" % offset_counts)
    allk = np.concatenate(events)
    assert allk.max() == top and allk.min() == bottom
    assert st.cpu().numpy()[boff[10] + 10, 1] == 0.0 and np.ptp(events[10]) == 0          # the constant event


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_narrow_digest_events_at_every_start_residue(dtype, ctx):
    """segment_events on stretches of one buffer that start at every residue mod 8 (each event's own digest)."""
    q = synth.QUANTUM if dtype == "int16" else Q_FINE
    centre = 1500 if dtype == "int16" else 100_000
    events, starts, pos = [], [], 3
    for j in range(8):
        k = se.narrow_trace(40 + j, centre=centre)[:15000 + 37 * j]
        pos += (j - pos) % 8                       # start residue j
        starts.append(pos); events.append(k); pos += len(k) + 5
    buf = np.full(pos + 8, centre, dtype=np.int64)
    for s, k in zip(starts, events):
        buf[s:s + len(k)] = k
    t = _upload(buf, dtype, q)
    b, boff, st = ctx.segment_events(t, np.array(starts), np.array([len(k) for k in events]), _lib.split_params(**NARROW), q,
                                     want_stats=True)
    tm = ctx.timings()
    assert tm["wide_redo"] == 0 and tm["near_ties"] >= 0
    assert {s % 8 for s in starts} == set(range(8))
    _check_call(events, b, boff, st, q, NARROW, int(buf[0]), "segment_events " + dtype)


# ---- route 2: the wide digest (segstat_kernel) -----------------------------------------------------------------------
def _wide_events(dtype):
    if dtype == "int16":
        q = synth.QUANTUM
        quiet = _quiet(51, 30000)
        quiet[:3000] = 3000 + np.rint(np.random.default_rng(9).normal(0, 0.5, 3000)).astype(np.int64)   # 27 000 below
        noisy = se.narrow_trace(52, centre=1500)[:40000]
        noisy[20000:] += 27000
        return q, [quiet, noisy, np.full(3000, 29000), np.arange(1, 6)]
    q = Q_FINE
    quiet = _quiet(53, 30000)
    quiet[:2000] -= 27000
    # (two segments of 20 000 samples near 2^20 counts: sum k^2 ~ 2^54, beyond what fp64 holds exactly about count 0)
    big = se.step_counts(np.random.default_rng(54), [20000, 20000], [1_000_000, 1_060_000], 100.0)
    return q, [quiet, big, np.full(3000, 1_000_001), np.arange(1_000_000, 1_000_006)]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_wide_digest_statistics(dtype, ctx):
    q, events = _wide_events(dtype)
    b, boff, st = _batch(ctx, events, dtype, q, WIDE)
    assert ctx.timings()["wide_redo"] == 1
    rs = _check_call(events, b, boff, st, q, WIDE, None, "wide " + dtype)
    if dtype == "float32":                            # the uncentred sums would no longer be exact in fp64
        assert min(se.Exact(events[1], rs[1], q).s2) > 2 ** 53 and len(rs[1]) == 2
    assert st.cpu().numpy()[boff[2] + 2, 1] == 0.0                     # the constant event


# ---- route 3: the LDS-window kernels (segstat_kernel) ----------------------------------------------------------------
@pytest.mark.parametrize("how", ["min_width_7", "mode_1", "scan_bs_0"])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_lds_window_route_statistics(how, dtype, ctx):
    kw = dict(LDS) if how == "min_width_7" else dict(NARROW)
    if how == "mode_1":
        ctx.set_option("mode", 1)
    if how == "scan_bs_0":
        ctx.set_option("scan_bs", 0)
    q = synth.QUANTUM if dtype == "int16" else Q_FINE
    centre = 30000
    events = [_quiet(61, centre, n_seg=6), se.narrow_trace(62, centre=centre - 1000)[:30000], np.arange(3) + centre,
              np.full(2000, centre + 3)]
    b, boff, st = _batch(ctx, events, dtype, q, kw)
    tm = ctx.timings()
    assert tm["near_ties"] == -1 and tm["wide_redo"] == 0              # (-1: the LDS-window kernels, which do not count)
    _check_call(events, b, boff, st, q, kw, None, "LDS %s %s" % (how, dtype))
    assert st.cpu().numpy()[boff[3] + 3, 1] == 0.0


# ---- route 4: the single pass (segstat_bs_kernel on the trace-aligned digest; its fallback to the two calls) -----------
Q_SP = 2.0 ** -9                                      # 110 pA open channel = 56 320 counts, threshold 90 pA = 46 080
OPEN = 56320


def _single_pass_trace(level, seed):
    rng = np.random.default_rng(seed)
    parts, pos = [], 0
    for j in range(8):
        gap = 20000 + (j - 20000 - pos) % 8 + 8        # the event starts at residue j of the trace
        parts.append(OPEN + np.rint(rng.normal(0, 3.0, gap)).astype(np.int64)); pos += gap
        if j % 2:
            ev = se.quiet_trace(seed + j, n_seg=4, centre=level)[:12000]
        else:
            ev = se.narrow_trace(seed + j, centre=level)[:6000 + 8 * j]
        parts.append(ev); pos += len(ev)
    parts.append(OPEN + np.rint(rng.normal(0, 3.0, 20000)).astype(np.int64))
    return np.concatenate(parts)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("level,route", [(43000, 0), (20000, 3)])
def test_single_pass_statistics(dtype, level, route, ctx):
    """Events ~13 000 counts below the open channel stay on the trace-aligned digest (wide_redo 0); 36 000 below, the
    counts leave 2^14 about the trace's first sample and the call falls back to the two calls (wide_redo 3)."""
    k = _single_pass_trace(level, 70 + level % 7)
    oc = 40000 if dtype == "int16" else 0
    t = _upload(k, dtype, Q_SP, oc)
    params = _lib.split_params(**NARROW)
    det = dict(threshold=90.0, min_duration=1000)
    st, ln, b, boff, stats = ctx.detect_segment_trace(t, Q_SP, params, offset_counts=oc if dtype == "int16" else 0,
                                                      want_stats=True, **det)
    assert ctx.timings()["wide_redo"] == route
    x = k.astype(np.float64) * Q_SP
    rs, rl = oracle.lambda_events(x, **det)
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(ln, rl)
    assert len(st) == 8 and {int(s) % 8 for s in st} == set(range(8))
    events = [k[s:s + n] for s, n in zip(st, ln)]
    _check_call(events, b, boff, stats, Q_SP, NARROW, int(k[0]), "single pass %s level %d" % (dtype, level))


# ---- route 5: the public surface on an .abf with a real header -------------------------------------------------------
def test_public_surface_on_a_real_abf_header(tmp_path):
    """SpeedyStatSplit.parse, Event.parse and File.parse_events on int16 data with a patch-clamp header (scale
    10 V / 0.0005 V/pA / 20 / 32768, non-zero offsets): Segment.mean / std / min / max against the exact statistics of the
    float64 current the object holds (segstat_exact.public_errors)."""
    from pypore_amd import abf
    from pypore_amd.DataTypes import File
    from pypore_amd.grid import grid_of
    from pypore_amd.parsers import SpeedyStatSplit, lambda_event_parser
    rng = np.random.default_rng(81)
    parts = []
    for j in range(4):
        parts.append(3600 + np.rint(rng.normal(0, 2.0, 30000 + j)).astype(np.int64))
        ev = se.quiet_trace(82 + j, n_seg=24, centre=1500 + 300 * j, sigma=0.5 + 10 * (j % 2))[:110000]
        assert len(ev) == 110000                    # (lambda_event_parser keeps events longer than 100 000 samples)
        parts.append(ev)
    parts.append(3600 + np.rint(rng.normal(0, 2.0, 30000)).astype(np.int64))
    counts = np.concatenate(parts).astype(np.int16)
    path = os.path.join(str(tmp_path), "real_header.abf")
    abf.write_abf(path, counts, adc_range=10.0, adc_resolution=32768, instrument_scale=0.0005, programmable_gain=20.0,
                  instrument_offset=0.25, signal_offset=-1.5)
    f = File(path)
    f.parse(lambda_event_parser(threshold=90))
    x = np.asarray(f.current)
    kk, q, off = grid_of(f.current)
    kk = np.asarray(kk, dtype=np.int64)
    assert off != 0.0 and np.log2(q) != np.rint(np.log2(q)) and len(f.events) == 4

    def in_samples(segs):                           # (an event's segments: start / end / duration in seconds)
        sec = f.second
        return [type("Seg", (), dict(start=int(round(s.start * sec)), end=int(round(s.end * sec)),
                                      duration=int(round(s.duration * sec)), mean=s.mean, std=s.std, min=s.min, max=s.max))
                for s in segs]

    def check(segs, a, what):
        n = sum(s.duration for s in segs) if segs else 0
        errs = se.public_errors(segs, x[a:a + n], kk[a:a + n], q, off, (int(kk[a]), int(kk[0])))
        bad = [(i, e) for i, e in enumerate(errs) if e is not None]
        assert not bad, "%s: %s" % (what, bad[:4])

    parser = SpeedyStatSplit(prior_segments_per_second=10.)
    for ev in f.events:
        ev.parse(parser)
        a = int(round(ev.start * f.second))
        check(in_samples(ev.segments), a, "Event.parse")
        check(parser.parse(f.current[a:a + len(ev.current)]), a, "SpeedyStatSplit.parse")
    f.parse_events(parser)
    for ev in f.events:
        a = int(round(ev.start * f.second))
        check(in_samples(ev.segments), a, "File.parse_events")
