"""HMM sampling on the device at every decision's edge (ps_hmm_sample, csrc/seg_hmm.hpp hmm_sample_kernel; models and
crafted tables in tests/sample_edges.py).  tests/test_hmm_sample_gpu.py checks the typical walk on friendly models; an
ordinary table never puts a drawn u on the edge of a decision, so here the tables are made for it:

  a. a drawn u equal to a row entry, and an ulp either side of it, in out_cdf, kde_cdf and mix_cdf;
  b. rows with repeated entries in front, in the middle and at the end, and rows that pass 1.0 by an ulp;
  c. rows of 1 to 4093 entries, equal and geometric, against the oracle's linear scan;
  d. `first + q` crossing a 32-bit word, the last accepted `first`, seeds at and beyond 64 bits;
  e. draws chosen for u0 near 0 and 1 and u1 near 1/4 and 3/4, against mpmath at 50 digits;
  f. max_length around a walk's own length with forty silent levels behind every emission;
  g. ragged and empty slots in buffers filled with a sentinel: no lane writes outside its own;
  h. the library's refusal of a row that gives mass to an entry the model calls impossible.

Crafted tables go to the device and to the oracle alike (sample_oracle.walk and mixture_oracle.walk take the tables as an
argument).  Lengths, flags, paths and uniform values are compared with ==, other values at TOL = 1e-12 max(1, |ref|), the
bar of tests/test_hmm_sample_gpu.py.  The chosen draws of e. are held to the same bar against mpmath; the host test
tests/test_hmm_sample_edges_host.py holds the oracle to it first.  Measured on one MI355X: the largest error of a chosen
draw against mpmath was 3.4e-15, on a log-normal of sigma 10.

yahmm is not available to compare against; nothing here is compared with it."""
import collections
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_edges as E  # noqa: E402
import sample_models as SM  # noqa: E402
import sample_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
N = 200
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
OBS_SENTINEL = 0x7FF8DEAD0000BEEF                            # a NaN no draw produces
PATH_SENTINEL = 0x7FFFFFFF

Got = collections.namedtuple("Got", "obs path flag")

_models = {}


def cached(key, build):
    """Models are built once and shared; the tests that train or change one build their own."""
    if key not in _models:
        _models[key] = build()
    return _models[key]


def product_arrays(m):
    t = m._sample_tables()
    return {k: t[k].copy() for k in ("out_cdf", "emit_param", "kde_cdf")}


def c_tables(arrays):
    """The _lib.HmmSampleTables over the arrays (the caller keeps them alive)."""
    from pypore_amd import _lib
    c = _lib.HmmSampleTables()
    for k, count in (("out_cdf", "n_cdf"), ("emit_param", "n_param"), ("kde_cdf", "n_kde")):
        setattr(c, k, arrays[k].ctypes.data if arrays[k].size else None)
        setattr(c, count, arrays[k].size)
    return c


def c_model_with(m, **fields):
    """A copy of the model's struct with some arrays replaced (the caller keeps them alive)."""
    from pypore_amd import _lib
    cm = _lib.HmmModel()
    ctypes.memmove(ctypes.byref(cm), ctypes.byref(m._c_model()), ctypes.sizeof(cm))
    for k, a in fields.items():
        setattr(cm, k, a.ctypes.data)
    return cm


def device_walks(m, n, seed, first=0, length=0, max_length=1000000, cm=None, ct=None):
    from pypore_amd import _lib, engine
    rc, obs, off, lens, flags, (path, path_off, path_len) = engine.context(None).hmm_sample(
        m._c_model() if cm is None else cm, m._sample_tables()["c"] if ct is None else ct, seed, first, n, length, max_length,
        want_path=True)
    assert rc == _lib.PS_OK
    D = m.flat["n_dim"]
    obs, lens, flags = obs.cpu().numpy().reshape(-1, D), lens.cpu().numpy(), flags.cpu().numpy()
    path, path_len = path.cpu().numpy(), path_len.cpu().numpy()
    return [Got(obs[off[q]:off[q] + lens[q]], path[path_off[q]:path_off[q] + path_len[q]].tolist(), int(flags[q])) for q in range(n)]


def same_value(got, want, exact):
    return got == want if exact else abs(got - want) <= TOL * max(1.0, abs(want))


def compare(got, want):
    """Lengths, flags and paths ==, uniform values ==, the others within TOL; returns the largest relative error seen."""
    worst = 0.0
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.flag == w.flag and g.path == w.path, (q, g.flag, w.flag, g.path, w.path)
        assert g.obs.shape[0] == len(w.obs), (q, g.obs.shape, len(w.obs))
        for t, (row, exact) in enumerate(zip(w.obs, w.exact)):
            for c, (v, ex) in enumerate(zip(row, exact)):
                assert same_value(g.obs[t, c], v, ex), (q, t, c, g.obs[t, c], v)
                if not ex:
                    worst = max(worst, abs(g.obs[t, c] - v) / max(1.0, abs(v)))
    return worst


def against_the_oracle(m, n, seed, first=0, length=0, max_length=1000000):
    """The model's own tables on the device against the oracle's; returns the oracle's walks."""
    want = E.oracle_walks(m, E.oracle_tables(m), n, seed, first, length, max_length)
    compare(device_walks(m, n, seed, first, length, max_length), want)
    return want


# ---- a. ties and neighbours --------------------------------------------------------------------------------------------
TIE_Q, TIE_LANE = 4242, 40


@pytest.mark.parametrize("table", ["out_cdf", "kde_cdf", "mix_cdf"])
def test_a_drawn_u_on_a_row_entry_and_an_ulp_either_side(table):
    """Walk TIE_Q's deciding u is computed on the host and written into the row: `u < cdf[i]` is false at cdf[i] == u and
    at the double below, true at the double above, so the linear scan takes i + 1, i + 1 and i."""
    if table == "out_cdf":
        m, j = cached("fork4", lambda: E.hub([1.0] * 4, "fork4", own_state=False)), 0
        lo, hi = E.hub_row(m)
    elif table == "kde_cdf":
        m, j = cached("kde4", lambda: E.kde_model(4, "equal")), 1
        lo, hi = 0, 4
    else:
        m, j = cached("mix4", lambda: E.mixture_model([1.0] * 4)), 1
        lo, hi = 0, 4
    assert hi - lo == 4
    u = SO.block(SEED, TIE_Q, j)[0]
    assert 0.01 < u < 0.99
    T = E.oracle_tables(m)
    for i in range(3):
        for v, above in E.neighbours(u):
            row = E.crafted(4, i, float(v))
            T[table] = list(T[table])
            T[table][lo:hi] = row
            if table == "mix_cdf":
                arr = np.array(T[table], np.float64)
                cm, ct = c_model_with(m, mix_cdf=arr), None
            else:
                arrays = product_arrays(m)
                arrays[table][lo:hi] = row
                cm, ct = None, c_tables(arrays)
            want = E.oracle_walks(m, T, 65, SEED, TIE_Q - TIE_LANE)
            got = device_walks(m, 65, SEED, TIE_Q - TIE_LANE, cm=cm, ct=ct)
            compare(got, want)
            taken = i if above else i + 1
            value = got[TIE_LANE].obs[0, 0]
            assert want[TIE_LANE].path[1] == (taken if table == "out_cdf" else 0)
            assert 10.0 * taken - 5.0 < value < 10.0 * taken + 5.0, (table, i, v, u, value)


# ---- b. flat rows ------------------------------------------------------------------------------------------------------
PAST = 1.0 + 2.0 ** -52

FLAT = {   # name -> (the hub's training counts, the row given to device and oracle; None: the product's own table)
    "product": ((0, 0, 3, 0, 0, 2, 0, 0), None),
    "front-middle-end": ((0, 1, 1, 0, 0, 1, 1, 0), [0.0, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0, 1.0]),
    "past-one": ((1, 0, 2, 2, 0, 0, 0, 1), [0.2, 0.2, 0.6, PAST, PAST, PAST, PAST, 1.0]),
    "past-one-then-closed": ((1, 0, 2, 2, 0, 1, 0, 0), [0.2, 0.2, 0.6, PAST, PAST, 1.0, 1.0, 1.0])}


@pytest.mark.parametrize("name", sorted(FLAT))
def test_flat_rows_and_rows_that_pass_one(name):
    """An entry equal to its predecessor is never taken: the crafted flats stand where one M-step left probability 0, so
    the rows agree with out_lp wherever the library looks."""
    counts, row = FLAT[name]
    m = E.trained_hub(counts, "flat")
    lo, hi = E.hub_row(m)
    T, arrays = E.oracle_tables(m), product_arrays(m)
    if row is None:
        row = arrays["out_cdf"][lo:hi].tolist()
        assert row == T["out_cdf"][lo:hi] and row[:2] == [0.0, 0.0] and 0.0 < row[2] == row[3] == row[4] < 1.0 and row[5:] == [1.0] * 3
    T["out_cdf"][lo:hi] = row
    arrays["out_cdf"][lo:hi] = row
    rising = {i for i, (a, b) in enumerate(zip([0.0] + row, row)) if b > a}
    assert rising <= {i for i, c in enumerate(counts) if c > 0} and len(rising) < 8
    want = E.oracle_walks(m, T, N, SEED)
    compare(device_walks(m, N, SEED, ct=c_tables(arrays)), want)
    taken = {w.path[2] for w in want}
    assert taken <= rising and len(taken) >= 2, (taken, rising)


# ---- c. fan-out --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("n", E.FAN_OUT)
def test_fan_out_of_a_state(n, form):
    m = E.hub(E.weights(n, form), "hub%d" % n)
    assert m.flat["n_states"] == n + 3 <= 4096
    want = against_the_oracle(m, N, SEED)
    taken = {w.path[2] for w in want}
    assert len(taken) >= (min(n, 50) if form == "equal" else min(n, 2))


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("n", E.KDE_POINTS)
def test_fan_out_of_a_kernel_density(n, form):
    m = E.kde_model(n, form)
    assert m.flat["kde_pt"].size == n
    want = against_the_oracle(m, N, SEED)
    assert len({round(w.obs[0][0] / 10.0) for w in want}) >= (min(n, 50) if form == "equal" else min(n, 2))


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("n", E.MIX_COMPONENTS)
def test_fan_out_of_a_mixture(n, form):
    m = E.mixture_model(E.weights(n, form))
    assert m._mix["mix_cdf"].size == n
    want = against_the_oracle(m, N, SEED)
    assert len({w.obs[0][0] // 10 for w in want}) >= (min(n, 20) if form == "equal" else min(n, 2))


# ---- d. the counter words ----------------------------------------------------------------------------------------------
LAST_FIRST = 2 ** 63 - 1 - 65


@pytest.mark.parametrize("name", ["kde", "vector3"])
def test_first_across_a_word_and_at_the_end_of_its_range(name):
    m = cached(name, SM.MODELS[name][0])
    for first in (2 ** 32 - 3, LAST_FIRST):
        against_the_oracle(m, 65, SEED, first)
    with pytest.raises(ValueError, match="first must be >= 0 and first \\+ n_seq fit in int64"):
        m.sample_batch(65, seed=SEED, first=LAST_FIRST + 1)
    # through Model.sample_batch as well: the last accepted value
    seqs, paths = m.sample_batch(65, path=True, seed=SEED, first=LAST_FIRST)
    want = E.oracle_walks(m, E.oracle_tables(m), 65, SEED, LAST_FIRST)
    assert [[i for i, _ in p] for p in paths] == [w.path for w in want] and [len(s) for s in seqs] == [len(w.obs) for w in want]


def test_seeds_at_and_beyond_64_bits():
    m = cached("kde", SM.MODELS["kde"][0])
    walks = {}
    for seed in (0, 2 ** 64 - 1, -1, 2 ** 64 + 7, 7):
        against_the_oracle(m, 65, seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            walks[seed] = [s.tobytes() for s in m.sample_batch(65, seed=seed)]
    assert walks[-1] == walks[2 ** 64 - 1] and walks[2 ** 64 + 7] == walks[7]         # a seed is taken modulo 2^64
    assert len({tuple(w) for w in walks.values()}) == 3


# ---- e. chosen draws ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.DRAW_MODELS))
def test_chosen_draws_against_mpmath(name, record_property):
    """The device's log, sqrt, cos and exp where the formulas are touchy, against the definition at 50 digits.
    Measured on one MI355X, the largest error per model: exponential 1.1e-16, kde 6.1e-17, lognormal 3.0e-15, normal
    4.0e-16, vector3 3.4e-15 (its log-normal component; the oracle's own largest is 3.0e-15)."""
    import mpmath
    build, blocks = E.DRAW_MODELS[name]
    m = build()
    T = E.oracle_tables(m)
    worst = 0.0
    for (j, which, at), Q in sorted(E.CHOSEN.items()):
        if j not in blocks:
            continue
        got = device_walks(m, 1, E.CHOSEN_SEED, Q)[0]
        ref = E.first_emission_mp(m, T, E.CHOSEN_SEED, Q)
        assert got.flag == 0 and got.obs.shape == (1, len(ref))
        errs = [E.error_mp(v, r) for v, r in zip(got.obs[0], ref)]
        for v, r, err in zip(got.obs[0], ref, errs):
            print("%s block %d %s near %g (Q = %d): device %.17g, mpmath %s, error %.3g" % (name, j, which, at, Q, v, mpmath.nstr(r, 20), err))
        worst = max([worst] + errs)
        assert max(errs) <= TOL, (name, j, which, at, got.obs[0].tolist(), ref)
    print("%s: largest error against mpmath %.3g" % (name, worst))
    record_property("largest_error_against_mpmath", worst)


# ---- f. stops with silent levels ---------------------------------------------------------------------------------------
def test_stops_with_forty_silent_levels():
    from pypore_amd import engine
    m = cached("chained", E.chained)
    NL = m.flat["n_levels"]
    assert NL >= E.CHAIN_LEVELS
    T = E.oracle_tables(m)
    full = E.oracle_walks(m, T, 65, SEED)
    q0 = next(q for q, w in enumerate(full) if len(w.obs) >= 3)
    L = len(full[q0].obs)
    assert len(full[q0].path) == 1 + L * (E.CHAIN_LEVELS + 1) + 1 and full[q0].flag == 0
    flags = {}
    for max_length in (L, L - 1, L + 1, 1):
        want = against_the_oracle(m, 65, SEED, max_length=max_length)
        flags[max_length] = want[q0].flag
        assert len(want[q0].obs) == min(L, max_length) and all(len(w.obs) <= max_length for w in want)
    assert flags == {L: 1, L - 1: 1, L + 1: 0, 1: 1}             # (at max_length = L the walk stands in e, not yet in end)
    want = against_the_oracle(m, 65, SEED, length=L - 1, max_length=L - 1)
    assert {w.flag for w in want} == {0} and len(want[q0].obs) == L - 1          # the `length` check comes first
    # the longest path there can be must fit in int32: (max_length + 1) (n_levels + 1) + 2
    largest = (2 ** 31 - 1 - 2) // (NL + 1) - 1
    assert (largest + 1) * (NL + 1) + 2 <= 2 ** 31 - 1 < (largest + 2) * (NL + 1) + 2
    ctx, cm, ct = engine.context(None), m._c_model(), m._sample_tables()["c"]
    with pytest.raises(ValueError, match="max_length %d with %d silent levels: a path could exceed int32" % (largest + 1, NL)):
        ctx.hmm_sample(cm, ct, SEED, 0, 4, max_length=largest + 1)
    compare(device_walks(m, 4, SEED, max_length=largest), full[:4])


# ---- g. slots and neighbours -------------------------------------------------------------------------------------------
def raw_call(m, seed, n, obs_slots, path_slots):
    """ps_hmm_sample itself on buffers filled with the sentinels: (rc, obs as int64 bits [slots, D], off, lens, flags, path,
    path_off, path_len), numpy."""
    import torch
    from pypore_amd import engine
    from pypore_amd.engine import _offsets, _ptr
    ctx = engine.context(None)
    dev = torch.device("cuda", ctx.device)
    D = m.flat["n_dim"]
    off, off_p = _offsets(np.concatenate(([0], np.cumsum(obs_slots))))
    path_off, path_off_p = _offsets(np.concatenate(([0], np.cumsum(path_slots))))
    bits = torch.full((max(int(off[-1]), 1) * D,), OBS_SENTINEL, dtype=torch.int64, device=dev)
    path = torch.full((max(int(path_off[-1]), 1),), PATH_SENTINEL, dtype=torch.int32, device=dev)
    lens, flags, path_len = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    cm, ct = m._c_model(), m._sample_tables()["c"]
    rc = ctx.L.ps_hmm_sample(ctx.handle, ctypes.byref(cm), ctypes.byref(ct), ctypes.c_uint64(seed), 0, n, 0, 1000000,
                             ctypes.c_void_p(bits.data_ptr()), off_p, _ptr(lens), _ptr(flags), ctypes.c_void_p(path.data_ptr()),
                             path_off_p, _ptr(path_len))
    return (rc, bits.cpu().numpy().reshape(-1, D), off, lens.cpu().numpy(), flags.cpu().numpy(), path.cpu().numpy(), path_off,
            path_len.cpu().numpy())


def check_slots(m, want, out, obs_slots, path_slots):
    from pypore_amd import _lib
    rc, bits, off, lens, flags, path, path_off, path_len = out
    values = bits.view(np.float64)
    assert lens.tolist() == [len(w.obs) for w in want] and path_len.tolist() == [len(w.path) for w in want]
    assert flags.tolist() == [w.flag for w in want]
    short = any(len(w.obs) > c for w, c in zip(want, obs_slots)) or any(len(w.path) > c for w, c in zip(want, path_slots))
    assert rc == (_lib.PS_ERR_CAPACITY if short else _lib.PS_OK)
    own, own_path = np.zeros(bits.shape[0], bool), np.zeros(path.shape[0], bool)
    for q, w in enumerate(want):
        rows = min(len(w.obs), int(obs_slots[q]))
        own[off[q]:off[q] + rows] = True
        for t in range(rows):                                                        # whole rows only
            assert all(same_value(values[off[q] + t, c], w.obs[t][c], w.exact[t][c]) for c in range(bits.shape[1])), (q, t)
        kept = min(len(w.path), int(path_slots[q]))
        own_path[path_off[q]:path_off[q] + kept] = True
        assert path[path_off[q]:path_off[q] + kept].tolist() == w.path[:kept], q
    assert np.all(bits[~own] == OBS_SENTINEL) and np.all(bits[own] != OBS_SENTINEL)
    assert np.all(path[~own_path] == PATH_SENTINEL) and np.all(path[own_path] != PATH_SENTINEL)
    return short


SLOT_MODELS = {"silent": SM.silent, "kde": SM.kde, "vector3": SM.vector3, "mixture": E.mix_model}


@pytest.mark.parametrize("name", sorted(SLOT_MODELS))
def test_ragged_slots_and_the_neighbours_slots(name):
    """Context.hmm_sample hands the kernel torch.empty buffers, where a stray write cannot be seen: here every element the
    walk does not own must still hold its sentinel.  Lanes 63, 64 and 65 -- the last of a wave and the first two of the next
    workgroup -- are among the short ones."""
    m, n = cached("slots-" + name, SLOT_MODELS[name]), 130
    want = E.oracle_walks(m, E.oracle_tables(m), n, SEED)
    L, P = np.array([len(w.obs) for w in want], np.int64), np.array([len(w.path) for w in want], np.int64)
    assert L.min() >= 1 and P.min() >= 3 and L.max() > 4
    q = np.arange(n)
    obs_slots = np.choose(q % 4, [np.zeros(n, np.int64), np.ones(n, np.int64), L, L + 3])
    path_slots = np.choose((q // 4) % 4, [np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2, np.int64), P])
    obs_slots[63:66], path_slots[63:66] = (0, 1, 0), (1, 0, 2)
    assert check_slots(m, want, raw_call(m, SEED, n, obs_slots, path_slots), obs_slots, path_slots)
    fits = [k for k in range(n) if L[k] <= obs_slots[k] and P[k] <= path_slots[k]]
    assert fits and len(fits) < n / 4                                                # some walks fit both slots, most do not
    # everything fits: PS_OK, and the three spare rows behind every sequence keep their sentinel
    assert not check_slots(m, want, raw_call(m, SEED, n, L + 3, P), L + 3, P)
    assert not check_slots(m, want, raw_call(m, SEED, n, L, P + 1), L, P + 1)


# ---- h. the refusal of a row that gives mass to an impossible entry ------------------------------------------------------
def test_mass_on_an_impossible_entry_is_refused():
    from pypore_amd import engine
    ctx = engine.context(None)
    says = "%s of state %d: entry %d rises above its predecessor, its log probability is -inf"
    # an out-edge: the row closed only in its last entry, as the tables were built before
    m = E.trained_hub((1, 2, 4, 0), "impossible")
    f, k = m.flat, E.hub_state(m)
    lo, hi = E.hub_row(m)
    arrays = product_arrays(m)
    assert arrays["out_cdf"][lo:hi].tolist()[2:] == [1.0, 1.0] and np.isneginf(f["out_lp"][hi - 1])
    arrays["out_cdf"] = E.rows_closed_in_the_last_entry(np.exp(f["out_lp"]), f["out_ptr"])
    assert arrays["out_cdf"][lo + 2] == 1.0 - 2.0 ** -53 and arrays["out_cdf"][hi - 1] == 1.0
    with pytest.raises(ValueError, match=says % ("out_cdf", k, 3)):
        ctx.hmm_sample(m._c_model(), c_tables(arrays), 1, 0, 4)
    against_the_oracle(m, 65, SEED)                                                   # the product's row is accepted
    # a kernel-density point: the flat form leaves points of weight 0 out, so the struct is made by hand
    m = cached("kde", SM.MODELS["kde"][0])
    f = m.flat
    assert f["kde_ptr"].tolist()[:3] == [0, 1, 7]
    lw = f["kde_lw"].copy()
    lw[3] = -np.inf                                                                   # state 1's third point
    cm = c_model_with(m, kde_lw=lw)
    with pytest.raises(ValueError, match=says % ("kde_cdf", 1, 2)):
        ctx.hmm_sample(cm, m._sample_tables()["c"], 1, 0, 4)
    arrays, T = product_arrays(m), E.oracle_tables(m)
    arrays["kde_cdf"][3] = arrays["kde_cdf"][2]
    T["kde_cdf"][3] = T["kde_cdf"][2]
    want = E.oracle_walks(m, T, 65, SEED)
    compare(device_walks(m, 65, SEED, cm=cm, ct=c_tables(arrays)), want)
    assert want != E.oracle_walks(m, E.oracle_tables(m), 65, SEED)                    # (the point was in use)
    # a mixture component
    m = E.mixture_model([1, 2, 4, 0], "impossible-mix")
    cdf = m._mix["mix_cdf"].copy()
    assert cdf.tolist() == [1 / 7, 3 / 7, 1.0, 1.0] and np.isneginf(m._mix["mix_lw"][3])
    cdf[2] = 1.0 - 2.0 ** -53
    with pytest.raises(ValueError, match=says % ("mix_cdf", 0, 3)):
        ctx.hmm_sample(c_model_with(m, mix_cdf=cdf), m._sample_tables()["c"], 1, 0, 4)
    against_the_oracle(m, 65, SEED)
