"""The part of the HMM model's upload the CPU cannot see (csrc/poreseg.hip hmm_upload over csrc/hmm_plan.hpp): a context keeps
the device copy of the last model's blob and uploads again only when the blob differs, and the kernels read every table through
the pointers hmm_blob_resolve aimed at that copy.  tests/test_hmm_plan_host.py checks layout, packing and pointers on the host;
here one context is handed five tiny models in turn -- plain, the same with other parameters (a blob of equal size: only the
comparison's bytes tell them apart), kernel-density states of 2 points, a vector model of D = 2, mixture states of 2 components;
three emitting states and one silent level each -- and runs Viterbi, forward, backward, the E-step, the posterior and the
sampler on sequences of 0, 1 and 5 observations for each, the whole round twice.  Every result of the second round == the
first's (the model before it was another one both times) and == what a fresh context gives for that model alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = {"start": {"a": 0.5, "b": 0.5}, "a": {"a": 0.3, "b": 0.4, "c": 0.2, "end": 0.1}, "b": {"b": 0.3, "c": 0.5, "end": 0.2},
     "c": {"c": 0.4, "a": 0.3, "end": 0.3}}
X = [[], [2.5], [0.25, 3.5, 2.75, 6.5, 0.5]]
X2 = [[], [[2.5, 0.5]], [[0.25, 1.5], [3.5, 0.75], [2.75, 2.0], [6.5, 0.125], [0.5, 3.0]]]       # D = 2, the second component > 0


def distributions(name):
    from pypore_amd import hmm as H
    N, U, L, E = H.NormalDistribution, H.UniformDistribution, H.LogNormalDistribution, H.ExponentialDistribution
    return {"plain": lambda: [N(0, 1), N(3, 1), U(-2, 8)],
            "plain2": lambda: [N(0.5, 1), N(3, 1.5), U(-2, 8)],
            "kde": lambda: [H.GaussianKernelDensity([-0.5, 0.5], 0.8), H.GaussianKernelDensity([2.5, 3.5], 0.8, [1, 2]),
                            H.GaussianKernelDensity([5, 6], 1.0)],
            "vector": lambda: [H.MultivariateDistribution([N(0, 1), E(1.0)]), H.MultivariateDistribution([N(3, 1), L(0, 1)], [1, 0.5]),
                               H.MultivariateDistribution([U(-2, 8), N(1, 2)])],
            "mixture": lambda: [H.MixtureDistribution([N(0, 1), N(1, 2)]), H.MixtureDistribution([N(3, 1), U(0, 6)], [1, 3]),
                                H.MixtureDistribution([N(6, 1), E(0.5)])]}[name]()


def model(name):
    from pypore_amd import hmm as H
    m = H.Model(name)
    s = dict(zip("abc", (H.State(d, name=k) for k, d in zip("abc", distributions(name)))), start=m.start, end=m.end)
    for a, row in P.items():
        for b, p in row.items():
            m.add_transition(s[a], s[b], p)
    m.bake()
    return m


def everything(ctx, m):
    """Every entry point's results for the model, as host arrays."""
    import torch
    from pypore_amd import _lib
    f = m.flat
    assert f["n_emit"] == 3 and f["n_levels"] == 1
    seqs = m._sequences(X2 if f["n_dim"] == 2 else X)
    off = np.concatenate(([0], np.cumsum([s.shape[0] for s in seqs]))).astype(np.int64)
    obs = torch.from_numpy(np.concatenate([s.reshape(-1) for s in seqs])).to(torch.device("cuda", ctx.device))
    cm, out = m._c_model(), []
    for mode in (_lib.PS_HMM_VITERBI, _lib.PS_HMM_FORWARD, _lib.PS_HMM_BACKWARD):
        logp, mat, path = ctx.hmm_batch(cm, mode, obs, off, True)
        out += [logp, mat]
        if path:
            p, p_off, p_len = path
            out += [p_len] + [p[p_off[q]:p_off[q] + int(p_len[q])] for q in range(len(seqs))]
    logp, counts, stats, skipped = ctx.hmm_expect(cm, obs, off, m._stat_width, mix_rows=m._n_mix)
    out += [logp, counts, stats, np.array([skipped])]
    logp, post, state, map_logp, counts = ctx.hmm_posterior(cm, obs, off, want_post=True, want_map=True, want_counts=True)
    out += [logp, post, state, map_logp, counts]
    _, walks, w_off, lens, flags, (p, p_off, p_len) = ctx.hmm_sample(cm, m._sample_tables()["c"], 12345, 0, 4, max_length=1000, want_path=True)
    out += [lens, flags, p_len] + [walks[w_off[q]:w_off[q] + int(lens[q])] for q in range(4)] + [p[p_off[q]:p_off[q] + int(p_len[q])] for q in range(4)]
    return [np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in out]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_one_context_many_models():
    from pypore_amd import engine
    names = ("plain", "plain2", "kde", "vector", "mixture")
    models = {n: model(n) for n in names}
    ctx = engine.Context(0)
    try:
        first = {n: everything(ctx, models[n]) for n in names}
        again = {n: everything(ctx, models[n]) for n in names}
        back = everything(ctx, models["plain"])                # (mixture -> plain: the largest blob, then the smallest)
    finally:
        ctx.close()
    for n in names:
        assert np.isfinite(first[n][0][1:]).all(), (n, first[n][0])       # the sequences of 1 and 5 observations have a path
        assert same(first[n], again[n]), n
        fresh = engine.Context(0)
        try:
            assert same(first[n], everything(fresh, models[n])), n
        finally:
            fresh.close()
    assert same(first["plain"], back)
    assert not same(first["plain"], first["plain2"])           # (the two equal-sized blobs are two models)
