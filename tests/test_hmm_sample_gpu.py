"""HMM sampling on the device (Model.sample_batch, Context.hmm_sample, ps_hmm_sample) against tests/sample_oracle.py: every
walk's length, flag and path bit for bit, uniform emissions bit for bit and the others to 1e-12 (they pass through the
device's log, cos and exp), batch cuts, the capacity contract, the stops, the statistics of 20 000 walks against the model
they were drawn from, the sampled paths against Viterbi and the forward pass, and Baum-Welch on sampled data.

yahmm is not available to compare against; nothing here is compared with it."""
import math
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_models as SM  # noqa: E402
import sample_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = (20260917, (0x9E3779B9 << 32) | 0x7F4A7C15)          # the second one has a live high key word
FIRSTS = (0, 2 ** 32 + 5)
N_MAX = 200
TOL = 1e-12                                                   # values that pass through the device's libm

_models, _walks = {}, {}


def model(name):
    if name not in _models:
        _models[name] = SM.MODELS[name][0]()
    return _models[name]


def oracle(name, seed, first, n=N_MAX):
    """The oracle's first n walks of (model, seed, first): computed once for N_MAX, shared, never changed."""
    key = (name, seed, first)
    if key not in _walks:
        _walks[key] = SO.batch(model(name), N_MAX, seed, first, length=SM.MODELS[name][1])
    return _walks[key][:n]


def quiet_batch(m, *a, **kw):
    """sample_batch with its truncation warning swallowed (the tests that are about the warning catch it themselves)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return m.sample_batch(*a, **kw)


def compare(m, seqs, paths, want):
    """Lengths and paths ==, uniform values ==, the others within TOL; returns the largest relative error seen."""
    worst = 0.0
    D = m.flat["n_dim"]
    assert len(seqs) == len(paths) == len(want)
    for q, (x, p, w) in enumerate(zip(seqs, paths, want)):
        assert x.dtype == np.float64 and x.shape == ((len(w.obs),) if D == 1 else (len(w.obs), D)), (q, x.shape, len(w.obs))
        assert [i for i, _ in p] == w.path, (q, [i for i, _ in p], w.path)
        assert all(s is m.states[i] for i, s in p)
        got = x.reshape(len(w.obs), D)
        for t, (row, exact) in enumerate(zip(w.obs, w.exact)):
            for c in range(D):
                if exact[c]:
                    assert got[t, c] == row[c], (q, t, c, got[t, c], row[c])
                else:
                    err = abs(got[t, c] - row[c]) / max(1.0, abs(row[c]))
                    assert err <= TOL, (q, t, c, got[t, c], row[c])
                    worst = max(worst, err)
    return worst


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_MAX])
@pytest.mark.parametrize("name", sorted(SM.MODELS))
def test_exact_walk(name, n):
    m = model(name)
    length = SM.MODELS[name][1]
    worst = 0.0
    for seed in SEEDS:
        for first in FIRSTS:
            want = oracle(name, seed, first, n)
            seqs, paths = quiet_batch(m, n, length=length, path=True, seed=seed, first=first)
            worst = max(worst, compare(m, seqs, paths, want))
            ctx_flags = _flags(m, n, seed, first, length)
            assert ctx_flags == [w.flag for w in want]
    print("%s n=%d: largest emission error %.3g" % (name, n, worst))


def _flags(m, n, seed, first, length, max_length=1000000):
    from pypore_amd import engine
    _, _, _, lens, flags, _ = engine.context(None).hmm_sample(m._c_model(), m._sample_tables()["c"], seed, first, n, length,
                                                              max_length)
    return flags.cpu().numpy().tolist()


def test_batch_cuts_repeats_and_seeds():
    for name in ("chain4", "vector3", "kde"):
        m = model(name)
        seed = SEEDS[1]
        whole, wp = quiet_batch(m, 200, path=True, seed=seed)
        a, ap = quiet_batch(m, 70, path=True, seed=seed)
        b, bp = quiet_batch(m, 130, path=True, seed=seed, first=70)
        again = quiet_batch(m, 200, seed=seed)
        other = quiet_batch(m, 200, seed=seed + 1)
        assert [x.tobytes() for x in whole] == [x.tobytes() for x in a + b] == [x.tobytes() for x in again]
        assert [[i for i, _ in p] for p in wp] == [[i for i, _ in p] for p in ap + bp]
        assert [x.tobytes() for x in whole] != [x.tobytes() for x in other]
        assert sum(x.shape == y.shape and np.array_equal(x, y) and x.size > 0 for x, y in zip(whole, other)) == 0


def test_sample_is_the_batch_of_one():
    m = model("silent")
    want = SO.batch(m, 1, 99)[0]
    seq, path = m.sample(path=True, seed=99)
    assert isinstance(seq, list) and all(type(v) is float for v in seq) and [i for i, _ in path] == want.path
    assert seq == quiet_batch(m, 1, seed=99)[0].tolist() and m.sample(seed=99) == seq
    v = model("vector3")
    rows = v.sample(seed=5)
    assert isinstance(rows, list) and all(isinstance(r, list) and len(r) == 3 for r in rows)
    a, b = m.sample(), m.sample()                              # seed=None: os.urandom, two calls differ (but for 2^-64)
    assert isinstance(a, list) and isinstance(b, list)
    assert m.sample_batch(0) == [] and m.sample_batch(0, path=True) == ([], [])


def test_capacity_contract_and_retry():
    from pypore_amd import _lib, engine
    name, seed, n = "silent", SEEDS[0], 65
    m, want = model(name), oracle(name, SEEDS[0], 0, 65)
    ctx = engine.context(None)
    rc, obs, off, lens, flags, (path, path_off, path_len) = ctx.hmm_sample(
        m._c_model(), m._sample_tables()["c"], seed, 0, n, want_path=True, obs_slots=np.ones(n, np.int64),
        path_slots=np.full(n, 2, np.int64), retry=False)
    assert rc == _lib.PS_ERR_CAPACITY                                          # (every path is longer than two states)
    assert lens.cpu().numpy().tolist() == [len(w.obs) for w in want]
    assert path_len.cpu().numpy().tolist() == [len(w.path) for w in want]
    assert flags.cpu().numpy().tolist() == [w.flag for w in want]
    obs, path = obs.cpu().numpy().reshape(-1), path.cpu().numpy()
    fitting = [q for q, w in enumerate(want) if len(w.obs) == 1]
    assert fitting, "the batch needs a walk of one observation"
    for q, w in enumerate(want):                                               # what fits its slot is written: here the prefixes
        assert path[path_off[q]:path_off[q] + 2].tolist() == w.path[:2]
        assert compare_value(obs[off[q]], w.obs[0][0], w.exact[0][0])
    # observation slots that fit beside path slots that do not, and the other way round
    big = np.array([len(w.obs) for w in want], np.int64)
    pbig = np.array([len(w.path) for w in want], np.int64)
    rc, obs, off, lens, _, (path, path_off, path_len) = ctx.hmm_sample(
        m._c_model(), m._sample_tables()["c"], seed, 0, n, want_path=True, obs_slots=big, path_slots=np.full(n, 2, np.int64), retry=False)
    assert rc == _lib.PS_ERR_CAPACITY and path_len.cpu().numpy().tolist() == pbig.tolist()
    obs = obs.cpu().numpy().reshape(-1)
    for q, w in enumerate(want):
        assert all(compare_value(obs[off[q] + t], w.obs[t][0], w.exact[t][0]) for t in range(len(w.obs)))
    rc, _, _, lens, _, (path, path_off, path_len) = ctx.hmm_sample(
        m._c_model(), m._sample_tables()["c"], seed, 0, n, want_path=True, obs_slots=big, path_slots=pbig, retry=False)
    assert rc == _lib.PS_OK
    path = path.cpu().numpy()
    assert [path[path_off[q]:path_off[q + 1]].tolist() for q in range(n)] == [w.path for w in want]
    # the retry path: the same request through sample_batch, whose first guess is 2 n_emit = 4 observations a walk
    assert max(len(w.obs) for w in want) > 4
    seqs, paths = m.sample_batch(n, path=True, seed=seed)
    compare(m, seqs, paths, want)


def compare_value(got, want, exact):
    return got == want if exact else abs(got - want) <= TOL * max(1.0, abs(want))


def test_stops():
    lp = SM.loop()
    want = SO.batch(lp, 100, 3, max_length=16)
    with pytest.warns(RuntimeWarning) as rec:
        seqs, paths = lp.sample_batch(100, path=True, seed=3, max_length=16)
    rec = [r for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(rec) == 1 and "%d of 100" % sum(w.flag == 1 for w in want) in str(rec[0].message)
    assert all(len(x) <= 16 for x in seqs) and [len(x) for x in seqs] == [len(w.obs) for w in want]
    assert _flags(lp, 100, 3, 0, 0, 16) == [w.flag for w in want] and sum(w.flag == 1 for w in want) > 90
    compare(lp, seqs, paths, want)
    # a fixed length on the infinite ring: exactly that many, the path ends in the state that emitted the last one
    r = model("ring")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                                  # (nothing is truncated: no warning)
        seqs, paths = r.sample_batch(100, length=10, path=True, seed=4)
    assert all(len(x) == 10 for x in seqs) and all(p[-1][0] < r.flat["n_emit"] for p in paths)
    compare(r, seqs, paths, SO.batch(r, 100, 4, length=10))
    # a fixed length on a finite model: the prefix of the untruncated walk
    c = model("chain4")
    full = oracle("chain4", SEEDS[0], 0)
    seqs, paths = c.sample_batch(N_MAX, length=3, path=True, seed=SEEDS[0])
    assert [len(x) for x in seqs] == [min(3, len(w.obs)) for w in full]
    assert len({len(x) for x in seqs}) > 1
    for x, p, w in zip(seqs, paths, full):
        assert [i for i, _ in p] == w.path[:len(p)]
        assert all(compare_value(x[t], w.obs[t][0], False) for t in range(len(x)))
    assert _flags(c, N_MAX, SEEDS[0], 0, 3) == [0] * N_MAX
    # a state without out-edges: flag 2, and the warning counts it
    d = SM.dead_end()
    want = SO.batch(d, 100, 8)
    assert _flags(d, 100, 8, 0, 0) == [w.flag for w in want] and {w.flag for w in want} == {0, 2}
    with pytest.warns(RuntimeWarning, match="%d of 100" % sum(w.flag == 2 for w in want)):
        seqs, paths = d.sample_batch(100, path=True, seed=8)
    compare(d, seqs, paths, want)
    assert all((p[-1][1].name == "b") == (w.flag == 2) for p, w in zip(paths, want))


def chain_moments(m):
    """(mean, variance) of the number of emissions of a walk from start to end, solved from the transition matrix: with
    r_i = 1 for an emitting state, the count from state i is N_i = r_i + N_next, so m = r + P m and the second moment
    s = r^2 + 2 r (P m) + P s over the transient states (`end` absorbs with N = 0)."""
    f = m.flat
    S, end = f["n_states"], f["end"]
    P = np.zeros((S, S))
    for i, j, p in m.edges:
        P[i, j] = p
    keep = [i for i in range(S) if i != end]
    P = P[np.ix_(keep, keep)]
    r = np.array([1.0 if i < f["n_emit"] else 0.0 for i in keep])
    A = np.eye(len(keep)) - P
    mean = np.linalg.solve(A, r)
    second = np.linalg.solve(A, r * r + 2 * r * (P @ mean))
    s = keep.index(f["start"])
    return mean[s], second[s] - mean[s] ** 2


def test_it_samples_the_model():
    m, n = model("chain4"), 20000
    f = m.flat
    seqs, paths = m.sample_batch(n, path=True, seed=424242)
    idx = [np.array([i for i, _ in p]) for p in paths]
    # every out-edge's frequency among the departures from its source
    src = np.concatenate([p[:-1] for p in idx])
    dst = np.concatenate([p[1:] for p in idx])
    for i, j, p in m.edges:
        left = int(np.count_nonzero(src == i))
        freq = np.count_nonzero((src == i) & (dst == j)) / left
        assert abs(freq - p) <= 5 * math.sqrt(p * (1 - p) / left), (i, j, freq, p)
    # every emitting state's values
    em = np.concatenate([p[p < f["n_emit"]] for p in idx])
    x = np.concatenate(seqs)
    assert em.size == x.size
    for k in range(f["n_emit"]):
        mu, sd = m.states[k].distribution.parameters
        v = x[em == k]
        assert v.size > 1000
        assert abs(v.mean() - mu) <= 5 * sd / math.sqrt(v.size), (k, v.mean(), mu)
        assert abs(v.var(ddof=1) - sd * sd) <= 5 * sd * sd * math.sqrt(2.0 / (v.size - 1)), (k, v.var(ddof=1), sd * sd)
    # the mean length
    mean, var = chain_moments(m)
    lengths = np.array([len(s) for s in seqs])
    print("mean length %.4f, solved %.4f (standard error %.4f)" % (lengths.mean(), mean, math.sqrt(var / n)))
    assert abs(lengths.mean() - mean) <= 5 * math.sqrt(var / n)


def joint_log_probability(m, seq, path):
    """The path's log probability together with its observations, summed on the host in walk order."""
    f = m.flat
    lp = {(int(i), int(f["out_dst"][e])): float(f["out_lp"][e]) for i in range(f["n_states"])
          for e in range(f["out_ptr"][i], f["out_ptr"][i + 1])}
    rows = np.asarray(seq).reshape(len(seq), -1)
    total, t = 0.0, 0
    for (i, _), (j, s) in zip(path[:-1], path[1:]):
        total += lp[(i, j)]
        if not s.is_silent():
            total += s.distribution.log_probability(rows[t] if f["n_dim"] > 1 else float(rows[t][0]))
            t += 1
    assert t == len(seq)
    return total


@pytest.mark.parametrize("name", ["phi29", "vector3"])
def test_against_the_other_kernels(name):
    m = model(name)
    seqs, paths = m.sample_batch(200, path=True, seed=SEEDS[0])              # (no warning: these models have no dead end)
    assert all(p[-1][1] is m.end for p in paths)
    vit = m.viterbi_batch(seqs)
    fwd = m.log_probability_batch(seqs)
    for x, p, (vlp, vpath), flp in zip(seqs, paths, vit, fwd):
        joint = joint_log_probability(m, x, p)
        assert math.isfinite(joint) and vpath is not None and math.isfinite(flp)
        assert joint <= vlp + 1e-9 and joint <= flp + 1e-9 and vlp <= flp + 1e-9, (joint, vlp, flp)


def test_round_trip_through_training():
    m = SM.chain4()                                                           # its own model: training changes it
    f = m.flat
    seqs, paths = m.sample_batch(2000, path=True, seed=31337)
    em = np.concatenate([np.array([i for i, _ in p if i < f["n_emit"]]) for p in paths])
    true = [tuple(s.distribution.parameters) for s in m.states[:f["n_emit"]]]
    total = m.train(seqs, max_iterations=5, verbose=False)
    assert total >= 0
    for k, (mu, sd) in enumerate(true):
        n_k = int(np.count_nonzero(em == k))
        got = m.states[k].distribution.parameters[0]
        assert n_k > 100 and abs(got - mu) <= 5 * sd / math.sqrt(n_k), (k, got, mu, n_k)


def test_the_library_refuses_bad_arguments_and_tables():
    import ctypes
    from pypore_amd import _lib, engine
    ctx = engine.context(None)
    m, r = model("kde"), model("ring")
    cm, t = m._c_model(), m._sample_tables()

    def call(tables=None, cmodel=cm, seed=1, first=0, n=4, **kw):
        return ctx.hmm_sample(cmodel, t["c"] if tables is None else tables, seed, first, n, **kw)

    for kw, msg in ((dict(length=-1), "negative length"), (dict(max_length=0), "max_length"), (dict(first=-1), "first"),
                    (dict(n=-1), "negative sequence count"), (dict(max_length=2 ** 31 - 1), "int32")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="a length must be given"):
        ctx.hmm_sample(r._c_model(), r._sample_tables()["c"], 1, 0, 4)

    def tables(**change):
        arrays = {k: t[k].copy() for k in ("out_cdf", "emit_param", "kde_cdf")}
        for k, (i, v) in change.items():
            arrays[k][i] = v
        c = _lib.HmmSampleTables()
        for k, count in (("out_cdf", "n_cdf"), ("emit_param", "n_param"), ("kde_cdf", "n_kde")):
            setattr(c, k, arrays[k].ctypes.data)
            setattr(c, count, arrays[k].size)
        return c, arrays                                                      # (the arrays live as long as the caller holds them)

    last = int(m.flat["out_ptr"][1]) - 1                                      # the last out-edge of state 0
    for change, msg in ((dict(out_cdf=(last, 0.999)), "out_cdf of state 0"), (dict(out_cdf=(0, -0.5)), "out_cdf of state 0"),
                        (dict(kde_cdf=(6, 0.5)), "kde_cdf of state 1"), (dict(kde_cdf=(2, float("nan"))), "kde_cdf of state 1"),
                        (dict(emit_param=(3, float("inf"))), "emit_param 3")):
        c, keep = tables(**change)
        with pytest.raises(ValueError, match=msg):
            call(tables=c)
    c, keep = tables()
    c.n_param -= 2
    with pytest.raises(ValueError, match="sampling tables of"):
        call(tables=c)
    c, keep = tables()
    c.kde_cdf = None
    with pytest.raises(ValueError, match="null sampling table"):
        call(tables=c)
    c, keep = tables()                                                        # an equal copy is accepted and gives the same walks
    a, b = call(tables=c, n=65, want_path=True), call(n=65, want_path=True)
    assert a[0] == b[0] == _lib.PS_OK and a[3].cpu().tolist() == b[3].cpu().tolist()
    assert ctypes.sizeof(_lib.HmmSampleTables) == 48
