"""Grid recovery, the parts that need no GPU: grid.affine_grid on currents built from known counts (its results by
construction), the subset helpers it shares with grid.affine_grid_device, and affine_grid_device's own host loop -- the
refinements, the re-centring, the refusals -- driven by a numpy stand-in for the two library calls.  The currents built from
known counts that both this file and test_ingest_gpu.py use are defined here."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from pypore_amd import _lib, engine, grid

ic = sys.modules[__name__]                     # (the constructions below, under the name test_ingest_gpu.py imports them by)

# ---- float64 currents built from known ADC counts (shared with test_ingest_gpu.py) -------------------------------------
Q = 0.030517576675492885                       # 10 V / 0.0005 V/pA / 20 / 32768 as an .abf header gives it: no power of two
OFFSETS = (0.0, 12.25, -3.7)
TOL = 1e-6                                     # affine_grid's tolerance on |k - rint k|


def current_of(counts, q=Q, offset=0.0):
    """float64(counts) * q + offset with the reader's two roundings (read_abf.py:210)."""
    x = np.asarray(counts).astype(np.float64)
    x *= q
    if offset:
        x += offset
    return x


def noisy_counts(n, seed=0, lo=-20, hi=20):
    """n counts that visit every value of a narrow band (neighbouring counts occur: the first candidate is the spacing)."""
    return np.random.default_rng(seed).integers(lo, hi, size=n).astype(np.int64)


def recentred(counts):
    """What affine_grid returns for counts whose neighbours occur: the counts minus their mid-range."""
    counts = np.asarray(counts, dtype=np.int64)
    return counts - (int(counts.min()) + int(counts.max()) + 1) // 2


def rails_counts(n=70001, seed=5):
    """Both int16 rails and everything between."""
    c = np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int64)
    c[17], c[n - 3] = -32768, 32767
    return c


def refinement_counts(n=200000, seed=7):
    """Even counts, plus 1 at the indices 1::3: the subset (stride 3 at this length) sees even counts only, so the first
    candidate is twice the spacing and the second pass finds it."""
    c = 2 * np.random.default_rng(seed).integers(-40, 40, size=n).astype(np.int64)
    c[1::3] += 1
    return c


def tolerance_current(d, offset=12.25, n=140001, seed=9):
    """Samples 1 and n - 2 (off the subset, stride 2 at this length) moved by d * Q off the grid."""
    x = current_of(noisy_counts(n, seed), Q, offset)
    x[1] += d * Q
    x[n - 2] -= d * Q
    return x


TOLERANCE_D = (2e-7, 9e-7, 1.2e-6, 2e-6, 0.5)


def check_on_host(x, origin, q, tol=TOL):
    """The numbers ps_grid_check_f64 reports, from numpy: (max_frac, min_frac_above, min_count, max_count, n_nonfinite,
    n_undefined)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = (x - origin) / q
        kr = np.rint(k)
        f = np.abs(k - kr)
    ok = ~np.isnan(f)
    above = f[ok & (f > tol)]
    return (float(f[ok].max()) if ok.any() else 0.0, float(above.min()) if above.size else np.inf,
            float(np.nanmin(kr)) if (~np.isnan(kr)).any() else np.inf, float(np.nanmax(kr)) if (~np.isnan(kr)).any() else -np.inf,
            int((~np.isfinite(x)).sum()), int((~ok).sum()))


# ---- grid.affine_grid and its helpers --------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (63, 64, 65, 255, 256, 257, engine.INGEST_PASS - 1, engine.INGEST_PASS, engine.INGEST_PASS + 1,
           2 * engine.INGEST_PASS + 5, 140001, 200000)


def _assert_grid(x, counts, q, offset, got):
    """affine_grid's result for counts whose neighbours occur: the spacing and the offset to within the rounding of the
    values, the counts exactly (minus their mid-range), and the values back from them to within float64 rounding."""
    gq, go, gk = got
    mid = (int(counts.min()) + int(counts.max()) + 1) // 2
    assert abs(gq / q - 1.0) < 1e-9
    assert abs(go - (offset + mid * q)) < 1e-6 * q
    assert gk.dtype == np.int64
    np.testing.assert_array_equal(gk, ic.recentred(counts))
    assert np.max(np.abs(gk * gq + go - x)) < 1e-6 * q


@pytest.mark.parametrize("offset", ic.OFFSETS)
@pytest.mark.parametrize("n", LENGTHS)
def test_affine_grid_returns_the_counts_a_current_was_built_from(n, offset):
    counts = ic.noisy_counts(n, seed=n)
    x = ic.current_of(counts, ic.Q, offset)
    _assert_grid(x, counts, ic.Q, offset, grid.affine_grid(x))
    # the helpers it is made of: the same subset, the same candidate -- here the spacing itself, no refinement
    u, q0 = grid.subset_candidate(x[::grid.subset_step(n)])
    assert grid.subset_step(n) == max(1, n // 65536) and u[0] == x[::grid.subset_step(n)].min()
    assert q0 == grid.affine_grid(x)[0]


def test_affine_grid_on_the_shortest_arrays():
    q, o, k = grid.affine_grid(np.zeros(0))
    assert (q, o, k.size, k.dtype) == (1.0, 0.0, 0, np.int64)
    for x in (np.array([12.25]), np.array([-3.7, -3.7])):
        q, o, k = grid.affine_grid(x)
        assert (q, o) == (1.0, x[0]) and not k.any() and k.size == x.size
        assert grid.subset_candidate(x)[1] is None
    x = ic.current_of([5, 9], ic.Q, 12.25)                   # two values: their gap is the spacing
    q, o, k = grid.affine_grid(x)
    assert q == x[1] - x[0] and k.tolist() == [-1, 0] and o == x[0] + 1 * q
    x = ic.current_of([4, 5, 7], ic.Q, -3.7)
    q, o, k = grid.affine_grid(x)
    assert abs(q / ic.Q - 1) < 1e-9 and k.tolist() == [-2, -1, 1]


def test_affine_grid_recentres_a_trace_on_both_rails():
    counts = ic.rails_counts()
    for offset in ic.OFFSETS:
        x = ic.current_of(counts, ic.Q, offset)
        _assert_grid(x, counts, ic.Q, offset, grid.affine_grid(x))
        assert grid.affine_grid(x)[2].min() == -32768 and grid.affine_grid(x)[2].max() == 32767


def test_affine_grid_refines_a_candidate_that_is_twice_the_spacing():
    counts = ic.refinement_counts()
    x = ic.current_of(counts, ic.Q, 12.25)
    assert grid.subset_step(x.size) == 3
    _, q0 = grid.subset_candidate(x[::3])
    assert abs(q0 / (2 * ic.Q) - 1) < 1e-9
    _assert_grid(x, counts, ic.Q, 12.25, grid.affine_grid(x))


@pytest.mark.parametrize("d", ic.TOLERANCE_D)
def test_affine_grid_at_its_tolerance(d):
    x = ic.tolerance_current(d)
    assert grid.subset_step(x.size) == 2
    if d in (1.2e-6, 2e-6):
        with pytest.raises(ValueError, match="not on an ADC grid"):
            grid.affine_grid(x)
        return
    q, o, k = grid.affine_grid(x)
    counts = ic.noisy_counts(x.size, 9)
    if d == 0.5:                                             # accepted on the half spacing
        assert abs(q / (ic.Q / 2) - 1) < 1e-9
        want = 2 * counts
        want[1] += 1
        want[x.size - 2] -= 1
        np.testing.assert_array_equal(k, ic.recentred(want))
    else:
        assert abs(q / ic.Q - 1) < 1e-9
        np.testing.assert_array_equal(k, ic.recentred(counts))


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_affine_grid_refuses_samples_that_are_not_finite(where, bad):
    x = ic.current_of(ic.noisy_counts(4099, 3), ic.Q, 12.25)
    x[{"first": 0, "middle": 2048, "last": 4098}[where]] = bad
    with np.errstate(all="ignore"), pytest.raises(ValueError):
        grid.affine_grid(x)


# ---- affine_grid_device's host loop, on a stand-in for the library ---------------------------------------------------------
class _HostContext(object):
    """ps_grid_check_f64 / ps_grid_counts_f64 restated in numpy for host tensors."""

    def __init__(self):
        self.checks = 0

    def grid_check(self, x, origin, q, tol=1e-6):
        self.checks += 1
        return _lib.GridReport(*ic.check_on_host(x.numpy(), origin, q, tol))

    def grid_counts(self, x, origin, q, centre):
        return torch.from_numpy((np.rint((x.numpy() - origin) / q).astype(np.int64) - centre).astype(np.int16))


@pytest.fixture
def host_ctx(monkeypatch):
    ctx = _HostContext()
    monkeypatch.setattr(engine, "context", lambda device=None: ctx)
    return ctx


def _same_as_host(x, ctx):
    try:
        with np.errstate(all="ignore"):
            want = grid.affine_grid(x)
    except ValueError:
        with pytest.raises(ValueError, match="not on an ADC grid"):
            grid.affine_grid_device(torch.from_numpy(x))
        return None
    q, o, k = grid.affine_grid_device(torch.from_numpy(x))
    assert (q, o) == want[:2] and k.dtype == torch.int16
    np.testing.assert_array_equal(k.numpy(), want[2])
    return q, o, k


def test_device_loop_takes_the_decisions_of_affine_grid(host_ctx):
    for n in (0, 1, 2, 3, 65, engine.INGEST_PASS + 1):
        for offset in ic.OFFSETS:
            assert _same_as_host(ic.current_of(ic.noisy_counts(n, n), ic.Q, offset), host_ctx) is not None
    assert _same_as_host(np.array([-3.7, -3.7]), host_ctx)[:2] == (1.0, -3.7)
    assert _same_as_host(ic.current_of(ic.rails_counts(), ic.Q, -3.7), host_ctx) is not None
    before = host_ctx.checks
    assert _same_as_host(ic.current_of(ic.refinement_counts(), ic.Q, 12.25), host_ctx) is not None
    assert host_ctx.checks == before + 2                     # twice the spacing, then the spacing
    for d in ic.TOLERANCE_D:
        assert (_same_as_host(ic.tolerance_current(d), host_ctx) is None) == (d in (1.2e-6, 2e-6))
    assert _same_as_host(100.0 + np.random.default_rng(1).normal(size=5000), host_ctx) is None
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 2048, 4098):
            x = ic.current_of(ic.noisy_counts(4099, 3), ic.Q, 12.25)
            x[at] = bad
            assert _same_as_host(x, host_ctx) is None


def test_device_loop_refuses_counts_beyond_int16(host_ctx):
    x = ic.current_of(np.arange(70000) % 70000, ic.Q, 12.25)
    assert grid.affine_grid(x)[2].max() > 32767              # (the host road refuses these in _int_counts_tensor)
    with pytest.raises(ValueError, match="beyond int16"):
        grid.affine_grid_device(torch.from_numpy(x))
    assert engine.COUNTS_BEYOND_INT16.startswith("ADC counts beyond int16")


def test_the_calls_are_bound_and_the_launch_constants_agree():
    for name in ("ps_grid_check_f64", "ps_grid_counts_f64", "ps_narrow_f64"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    for method in ("grid_check", "grid_counts", "narrow_f64"):
        assert callable(getattr(engine.Context, method))
    # the lengths of the GPU tests are built from these two: they must be the kernels' own
    hdr = open(os.path.join(ROOT, "pypore_amd", "csrc", "seg_ingest.hpp")).read()
    nt, unroll, cap = (int(re.search(r"constexpr int %s = (\d+);" % c, hdr).group(1)) for c in ("ING_NT", "ING_UNROLL", "ING_GRID_MAX"))
    assert "ING_T = ING_NT * 2 * ING_UNROLL" in hdr and nt * 2 * unroll == engine.INGEST_PASS and cap == engine.INGEST_GRID_MAX


def test_a_refusal_of_one_road_is_told_from_an_error():
    """Only detect_quantum's and the float32 check's refusals send a current on to the next road."""
    with pytest.raises(engine.GridRefusal):
        engine.detect_quantum(ic.current_of(ic.noisy_counts(100), ic.Q, 12.25))
    assert issubclass(engine.GridRefusal, ValueError)
