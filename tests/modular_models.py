"""Models and sequences that tests/test_profile_builders_host.py, tests/test_profile_builders_gpu.py and
tools/bench_modular.py share: profiles of NormalDistribution(mean, 1.5) states for the reference's builders
(pypore_amd.hmm: ModularProfileModel and its three board modules, Phi29ProfileHMM, Hel308ProfileHMM), the fork model, and
sequences that walk a profile.  Everything is built from fixed numbers or a seeded generator, so two calls give equal
models."""
import numpy as np

from pypore_amd.hmm import (GlobalAlignmentModule, Hel308ProfileHMM, ModularProfileModel, NanoporeGlobalAlignmentModule,
                            NormalDistribution, Phi29GlobalAlignmentModule, Phi29ProfileHMM, UniformDistribution)

STD = 1.5
MODULES = {"phi29": Phi29GlobalAlignmentModule, "nanopore": NanoporeGlobalAlignmentModule, "global": GlobalAlignmentModule}


def means(n):
    """n levels in [20, 70], neighbours at least 8 apart (far more than STD), no two positions within 2 of each other
    among the first 12."""
    if n <= 3:
        return np.array([20.0, 35.0, 50.0][:n])
    rng = np.random.default_rng(n)
    out = [35.0]
    while len(out) < n:
        m = float(rng.uniform(20, 70))
        if abs(m - out[-1]) >= 8 and (len(out) < 2 or abs(m - out[-2]) >= 4):
            out.append(round(m, 3))
    return np.array(out)


def profile(n):
    return [NormalDistribution(float(m), STD) for m in means(n)]


def insert():
    return UniformDistribution(0, 90)


def modular(n, module="phi29", merge=None, name="modular"):
    return ModularProfileModel(MODULES[module], profile(n), name, insert(), merge=merge)


FORK_MEANS = {"a": (30.0, 32.0), "b": (40.0, 42.0)}
FORK_SEQS = {"a": np.array([20.0, 30.0, 32.0, 50.0]), "b": np.array([20.0, 40.0, 42.0, 50.0])}


def fork_profile():
    """4 positions, means 20, {a: 30, b: 40}, {a: 32, b: 42}, 50: forks {a, b} at positions 1 and 2."""
    return [NormalDistribution(20.0, STD)] + [{k: NormalDistribution(FORK_MEANS[k][j], STD) for k in ("a", "b")} for j in (0, 1)] \
        + [NormalDistribution(50.0, STD)]


def fork_model(merge=None, module="phi29"):
    return ModularProfileModel(MODULES[module], fork_profile(), "fork", insert(), merge=merge)


def fork8_profile():
    """8 positions with a fork {a, b} at position 3: branch a keeps the profile's level, b lies 6 above it."""
    p = profile(8)
    m = float(means(8)[3])
    p[3] = {"a": NormalDistribution(m, STD), "b": NormalDistribution(m + 6.0, STD)}
    return p


def fork8_model(merge=None, module="phi29"):
    return ModularProfileModel(MODULES[module], fork8_profile(), "fork8", insert(), merge=merge)


def linear(kind, n, **kw):
    if kind == "phi29":
        return Phi29ProfileHMM(profile(n), verbose=False, **kw)
    return Hel308ProfileHMM(profile(n), **kw)


def size(model):
    """(states, emitting states, silent levels, edges, largest in-degree) of a baked model."""
    f = model.flat
    return (f["n_states"], f["n_emit"], f["n_levels"], len(model.edges), int(np.diff(f["in_ptr"]).max()))


def walk(mu, offset=0.3):
    """One observation per position, `offset` above its level."""
    return np.asarray(mu, np.float64) + offset


def walk_with_backslip(mu, at, offset=0.3):
    """walk(), but after position `at` the sequence steps back to at - 1 and comes forward again."""
    mu = np.asarray(mu, np.float64)
    idx = list(range(at + 1)) + [at - 1, at] + list(range(at + 1, mu.size))
    return mu[idx] + offset


def noisy_walk(mu, length, seed):
    """About `length` observations through the profile with repeats and skips and noise of sigma 1, one backslip."""
    rng = np.random.default_rng(seed)
    mu = np.asarray(mu, np.float64)
    idx = np.minimum(np.cumsum(rng.choice([0, 1, 1, 2], length)) * mu.size // max(1, length), mu.size - 1)
    at = length // 2
    idx = np.concatenate((idx[:at], idx[max(at - 2, 0):at], idx[at:]))
    return mu[idx] + rng.normal(0, 1.0, idx.size)


def emitting_names(model, path):
    """The names of the emitting states on a path of state indices."""
    ne = model.flat["n_emit"]
    return [model.states[i].name for i in path if i < ne]


def edges_into(model, prefix, suffix):
    """Indices into model.edges of the edges whose target is a state named prefix + ... + suffix from another state."""
    out = []
    for e, (i, j, _) in enumerate(model.edges):
        name = model.states[j].name
        if name.startswith(prefix) and name.endswith(suffix):
            out.append(e)
    return out
