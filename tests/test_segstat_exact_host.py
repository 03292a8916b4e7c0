"""The exact-statistics checker (tests/segstat_exact.py) on the CPU: it agrees with the oracle on the golden vectors, it
rejects rows that miss or double-count a single sample, it accepts the centred K2 formula and rejects the formula about
count 0 on quiet segments at high levels."""
import numpy as np
import pytest

import oracle
import segstat_exact as se
from golden_util import cases, input_counts, input_pa
from pypore_amd import synth

NARROW = dict(min_width=8, max_width=1000000, window_width=2000, prior_segments_per_second=10.)
QUIET = dict(min_width=100, max_width=1000000, window_width=10000, prior_segments_per_second=10.)
Q_FINE = 2.0 ** -15


def _designed():
    """(name, counts, q, oracle params) of the designed traces: the narrow-route geometry sweep, quiet int16 segments at
    ~30 000 counts, fine-grid float32 counts near 2^22 (quiet and noisy)."""
    fine = se.quiet_trace(23, centre=4_100_000, sigma=0.5)
    return [("geometry", se.narrow_trace(1), synth.QUANTUM, NARROW),
            ("quiet_30000", se.quiet_trace(2), synth.QUANTUM, QUIET),
            ("quiet_fine", fine, Q_FINE, QUIET),
            ("fine_noisy", se.narrow_trace(3, centre=4_190_000, sigma=100.0), Q_FINE, NARROW)]


@pytest.fixture(scope="module")
def designed():
    out = []
    for name, k, q, kw in _designed():
        b = oracle.parse(k.astype(np.float64) * q, **kw)
        out.append((name, k, q, se.ranges_of(np.concatenate(([0], b, [len(k)])))))
    return out


def test_exact_reference_agrees_with_oracle_and_numpy_on_goldens():
    n_seg = 0
    for case in cases("parse")[:10]:
        k = input_counts(case).astype(np.int64)
        if k.size == 0:
            continue
        x = input_pa(case)
        b = oracle.parse(x, **case["params"])
        r = se.ranges_of(np.concatenate(([0], b, [len(k)])))
        got = se.Exact(k, r, synth.QUANTUM).floats()
        np.testing.assert_allclose(got, oracle.segment_stats(x, b), rtol=1e-12, atol=0)
        npy = np.array([[x[a:z].mean(), x[a:z].std(), x[a:z].min(), x[a:z].max()] for a, z in r])
        np.testing.assert_allclose(got, npy, rtol=1e-12, atol=0)
        n_seg += len(r)
    assert n_seg > 100


def test_exact_sums_beyond_int64_squares():
    """Counts near 2^22 over 10^6 samples: sum k^2 ~ 2^64 -- still exact (Python ints)."""
    k = np.full(1_000_000, 4_194_301, dtype=np.int64)
    k[::3] += 2
    ref = se.Exact(k, [(0, k.size), (5, 17)], 1.0)
    vals, cnt = np.unique(k, return_counts=True)
    assert ref.s1[0] == sum(int(v) * int(c) for v, c in zip(vals, cnt))
    assert ref.s2[0] == sum(int(v) * int(v) * int(c) for v, c in zip(vals, cnt))
    assert ref.s2[0] > 2 ** 63


@pytest.mark.parametrize("kind", ["head+1", "tail-1", "head-1", "tail+1", "drop_interior"])
def test_checker_sees_one_sample(kind, designed):
    """Rows formed over [a+1, b), [a, b-1), [a-1, b), [a, b+1) or [a, b) without one interior sample, by the centred
    formula: the checker rejects at least 99 % of the segments of every designed trace."""
    rng = np.random.default_rng(7)
    for name, k, q, r in designed:
        ref = se.Exact(k, r, q)
        c = (int(k[0]), int(k[0]))
        a, b = r[:, 0].copy(), r[:, 1].copy()
        keep = np.ones(len(r), dtype=bool)
        if kind == "head+1":
            a += 1
        elif kind == "tail-1":
            b -= 1
        elif kind == "head-1":
            a -= 1; keep = a >= 0
        elif kind == "tail+1":
            b += 1; keep = b <= len(k)
        if kind == "drop_interior":
            rows = np.empty((len(r), 4))
            for i, (a0, b0) in enumerate(r):
                j = int(rng.integers(a0 + 1, b0 - 1))
                kk = np.delete(k[a0:b0], j - a0)
                rows[i] = se.emulate_rows(kk, [(0, len(kk))], q, centre=c[0])[0]
        else:
            a, b = np.clip(a, 0, len(k)), np.clip(b, 0, len(k))
            rows = se.emulate_rows(k, np.stack([a, b], 1), q, centre=c[0])
        ok = se.check_rows(rows, ref, c)[keep]
        assert keep.sum() >= len(r) - 1 and len(r) > 10
        assert ok.mean() <= 0.01, "%s / %s: %d of %d mutated rows accepted" % (name, kind, ok.sum(), len(ok))


def test_checker_accepts_the_centred_formula_about_either_centre(designed):
    for name, k, q, r in designed:
        ref = se.Exact(k, r, q)
        k_tr0 = int(k[0]) + 5000                    # (a trace that starts elsewhere than the event)
        for c in (int(k[0]), k_tr0):
            rows = se.emulate_rows(k, r, q, centre=c)
            se.assert_rows(rows, ref, (int(k[0]), k_tr0), "%s, centred on %d" % (name, c))


@pytest.mark.parametrize("name", ["quiet_30000", "quiet_fine"])
def test_checker_rejects_the_formula_about_count_zero_on_quiet_high_levels(name, designed):
    (k, q, r), = [(k, q, r) for n, k, q, r in designed if n == name]
    ref = se.Exact(k, r, q)
    ok = se.check_rows(se.emulate_rows(k, r, q, centre=None), ref, (int(k[0]), int(k[0])))
    # (a row about count 0 can still land within the bar when its two roundings happen to cancel: a few per cent)
    assert len(r) >= 10 and ok.mean() <= 0.1, "%d of %d uncentred rows accepted" % (ok.sum(), len(ok))


def test_checker_edge_rows():
    k = np.array([5, 5, 5, 5, 9, 1, 4, 7], dtype=np.int64)
    ref = se.Exact(k, [(0, 4), (4, 8), (8, 8)], 0.5)
    good = se.emulate_rows(k, [(0, 4), (4, 8), (8, 8)], 0.5, centre=5)
    assert np.isnan(good[2]).all()
    se.assert_rows(good, ref, (5, 5))
    for i, j, v in ((0, 1, 1e-300), (1, 2, good[1, 2] + 2 ** -50), (1, 3, np.nextafter(good[1, 3], 0)), (2, 0, 0.0),
                    (1, 1, good[1, 1] * (1 + 1e-13)), (1, 0, good[1, 0] * (1 + 1e-14))):
        bad = good.copy()
        bad[i, j] = v
        assert not se.check_rows(bad, ref, (5, 5))[i], (i, j)
    with pytest.raises(ValueError):                 # the bound needs the centred sums below 2^53
        se.check_rows(np.zeros((1, 4)), se.Exact(np.full(1000, 4_000_000), [(0, 1000)], 1.0), (0, 0))
