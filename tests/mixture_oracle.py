"""Test-side oracle for the mixture states of pypore_amd.hmm (MixtureDistribution), written on its own from the module
docstring, in the manner of tests/multivariate_oracle.py:

  * the component log densities written out again (`component`), a mixture's terms  log w_j + l_j(x)  (`terms`), its
    density, their log-sum-exp (`emission`, which also restates the normal, uniform and kernel-density states a mixture
    model may hold), and its responsibilities (`responsibilities`);
  * the log-space dynamic programmes of tests/hmm_oracle.py, handed a per-observation emission table through the
    `Compiled` view as tests/multivariate_oracle.py does: forward, backward, Viterbi with its near-tie report, posterior
    decoding (posterior_oracle.posterior);
  * brute force over every state path of a tiny model: the forward matrix (`brute_force`) and the E-step with the
    component rows (`estep_brute_force`);
  * the E-step with the component rows behind the states' (`estep_one`, `estep`), Viterbi training's counts
    (`viterbi_counts`), the M-step -- component distributions pooled per object over plain states and mixture slots, mixture
    weights pooled per mixture object -- (`m_step`) and the training loop (`train`);
  * the sampling tables and the walk with the two-block mixture draw (`tables`, `walk`, `batch`) on sample_oracle's Philox
    blocks, `pick` and `draw`;
  * the models and inputs the GPU tests use, so that tests/test_mixture_host.py can examine the same inputs with the oracle
    alone.

yahmm is not available to compare against; nothing here is compared with it."""
import collections
import copy
import math

import numpy as np

import hmm_oracle as O
import hmm_train_oracle as T
import posterior_oracle as PO
import sample_oracle as SO

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution,  # noqa: E402
                            MixtureDistribution, Model, NormalDistribution, State, UniformDistribution)

NEG = -np.inf


# ---- emissions --------------------------------------------------------------------------------------------------------
def component(d, x):
    """Log density of x under a univariate distribution, from its `parameters`."""
    name, p = type(d).__name__, d.parameters
    if name == "NormalDistribution":                       # (a product, not ** 2: far out it overflows to inf, as the device's)
        return -math.log(p[1] * math.sqrt(2 * math.pi)) - (x - p[0]) * (x - p[0]) / (2 * p[1] ** 2)
    if name == "UniformDistribution":
        return -math.log(p[1] - p[0]) if p[0] <= x <= p[1] else NEG
    if name == "LogNormalDistribution":
        if not x > 0:
            return NEG
        y = math.log(x)
        return (-math.log(p[1] * math.sqrt(2 * math.pi)) - (y - p[0]) ** 2 / (2 * p[1] ** 2)) - y
    if name == "ExponentialDistribution":
        return math.log(p[0]) - p[0] * x if x >= 0 else NEG
    raise TypeError("no formula for %r" % (d,))


def is_mixture(distribution):
    return type(distribution).__name__ == "MixtureDistribution"


def slots(distribution):
    """[(component, weight)] of a mixture, [] of anything else."""
    return list(zip(*distribution.parameters)) if is_mixture(distribution) else []


def lse(values):
    """log sum exp of the values > -inf: the largest plus log1p of the others' exp; -inf when there is none."""
    v = [float(t) for t in values if t > NEG]
    if not v:
        return NEG
    i = int(np.argmax(v))
    return v[i] + math.log1p(math.fsum(math.exp(t - v[i]) for j, t in enumerate(v) if j != i))


def terms(distribution, x):
    """log w_j + l_j(x) per component of a mixture; -inf for a component of weight 0."""
    return [math.log(w) + component(d, x) if w > 0 else NEG for d, w in slots(distribution)]


def emission(distribution, x):
    """Log density of x in an emitting state of a scalar model: normal, uniform, kernel density or mixture."""
    if is_mixture(distribution):
        return lse(terms(distribution, x))
    if type(distribution).__name__ == "GaussianKernelDensity":
        points, h, weights = distribution.parameters
        return -math.log(h * math.sqrt(2 * math.pi)) + lse(math.log(w) - (x - p) * (x - p) / (2 * h * h)
                                                             for p, w in zip(points, weights) if w > 0)
    return component(distribution, x)


def responsibilities(distribution, x):
    """exp(term_j - density) per component, 0 for a term of -inf; all 0 where the density is -inf."""
    v = terms(distribution, x)
    e = lse(v)
    return [math.exp(t - e) if (e > NEG and t > NEG) else 0.0 for t in v]


def table(model, seq):
    """e[t][k]: the log density of observation t in emitting state k, (n, n_emit)."""
    ne = T.n_emit(model)
    x = np.asarray(seq, np.float64).reshape(-1)
    return np.array([[emission(model.states[k].distribution, v) for k in range(ne)] for v in x.tolist()],
                    np.float64).reshape(len(x), ne)


class Compiled(O.Compiled):
    """hmm_oracle.Compiled (edges of probability 0 left out) whose emissions come from the table of the sequence last bound."""

    def __init__(self, model, edges=None):
        O.Compiled.__init__(self, T.View(model, edges))
        self.model = model
        self.E = None

    def bind(self, seq):
        self.E = table(self.model, seq)
        return np.arange(self.E.shape[0], dtype=np.float64)

    def emissions(self, t):
        return self.E[int(t)]


def forward(model, seq):
    c = Compiled(model)
    return O.forward(c, c.bind(seq))


def backward(model, seq):
    c = Compiled(model)
    return O.backward(c, c.bind(seq))


def log_probability(model, seq):
    c = Compiled(model)
    return O.log_probability(c, c.bind(seq))


def viterbi_ties(model, seq):
    """hmm_oracle.viterbi_ties on the table: (logp, path or None, smallest non-zero relative gap, exact ties, where)."""
    c = Compiled(model)
    return O.viterbi_ties(c, c.bind(seq))


def posterior(model, seq):
    c = Compiled(model)
    return PO.posterior(c, c.bind(seq), model.edges)


def brute_force(model, seq):
    """Every state path enumerated: (forward matrix, log_probability, best score, best path)."""
    c = Compiled(model)
    E = table(model, seq)
    n = E.shape[0]
    found, ends = {}, []

    def step(k, t, lp, path):
        found.setdefault((t, k), []).append(lp)
        if t == n and (not c.finite or k == c.end):
            ends.append((lp, path))
        for l, w in c.outs[k]:
            if l < c.NE:
                if t < n and E[t, l] > NEG:
                    step(l, t + 1, lp + w + E[t, l], path + [l])
            else:
                step(l, t, lp + w, path + [l])

    step(c.start, 0, 0.0, [c.start])
    F = np.full((n + 1, c.S), NEG)
    for (t, k), v in found.items():
        F[t, k] = lse(v)
    if not ends:
        return F, NEG, NEG, None
    scores = [e[0] for e in ends]
    best = int(np.argmax(scores))
    return F, lse(scores), scores[best], ends[best][1]


# ---- training ---------------------------------------------------------------------------------------------------------
def mix_ptr(model):
    """ptr[k] .. ptr[k+1]: the component rows of emitting state k (table order: states ascending, slots ascending)."""
    ptr = [0]
    for s in model.states[:T.n_emit(model)]:
        ptr.append(ptr[-1] + len(slots(s.distribution)))
    return ptr


def state_shift(distribution):
    """The shift of a state's (W, A, B): normal mean, uniform low, kernel density the weighted mean of its points,
    mixture 0 (its row holds the raw moments)."""
    if is_mixture(distribution):
        return 0.0
    if type(distribution).__name__ == "GaussianKernelDensity":
        points, _, weights = distribution.parameters
        return math.fsum(p * w for p, w in zip(points, weights))
    return distribution.parameters[0]


def slot_deviation(d, x):
    """y - c of a mixture component: y = log x for a log-normal one; c = normal mean, log-normal mu, exponential 0,
    uniform low."""
    name = type(d).__name__
    y = math.log(x) if name == "LogNormalDistribution" else x
    return y - (0.0 if name == "ExponentialDistribution" else d.parameters[0])


def add_rows(stats, model, ptr, k, x, g):
    """What state k's posterior g at observation x adds: its own row, and its components' rows by their responsibilities."""
    dist = model.states[k].distribution
    d = x - state_shift(dist)
    stats[k] += (g, g * d, g * d * d)
    for j, r in enumerate(responsibilities(dist, x) if is_mixture(dist) else []):
        if r > 0:
            dv = slot_deviation(dist.parameters[0][j], x)
            stats[len(ptr) - 1 + ptr[k] + j] += (g * r, g * r * dv, g * r * dv * dv)


def estep_one(model, seq, edges=None):
    """(counts aligned with model.edges, stats [NE + n_mix, 3], logp) of one sequence; zeros for logp = -inf."""
    edges = model.edges if edges is None else edges
    c = Compiled(model, edges)
    idx = c.bind(seq)
    x = np.asarray(seq, np.float64).reshape(-1)
    n, NE, ptr = idx.size, c.NE, mix_ptr(model)
    counts, stats = np.zeros(len(edges)), np.zeros((NE + ptr[-1], 3))
    F = O.forward(c, idx)
    logp = O.final(c, F[n], False)[0]
    if not logp > NEG:
        return counts, stats, logp
    B = O.backward(c, idx)
    for e, (k, l, p) in enumerate(edges):
        if not p > 0:
            continue
        lp = math.log(p)
        v = F[:n, k] + lp + c.E[:, l] + B[1:, l] - logp if l < NE else F[:, k] + lp + B[:, l] - logp
        counts[e] = np.exp(v[v > NEG]).sum() if v.size else 0.0
    for t in range(n):
        for k in range(NE):
            if F[t + 1, k] > NEG and B[t + 1, k] > NEG:
                add_rows(stats, model, ptr, k, float(x[t]), math.exp(F[t + 1, k] + B[t + 1, k] - logp))
    return counts, stats, logp


def estep(model, seqs, edges=None):
    """Batch E-step: (counts, stats, logp array, skipped)."""
    edges = model.edges if edges is None else edges
    counts, stats, logp = np.zeros(len(edges)), np.zeros((T.n_emit(model) + mix_ptr(model)[-1], 3)), []
    for s in seqs:
        cc, st, lp = estep_one(model, s, edges)
        logp.append(lp)
        if lp > NEG:
            counts += cc
            stats += st
    logp = np.array(logp, np.float64)
    return counts, stats, logp, int(np.sum(~(logp > NEG)))


def estep_brute_force(model, seq):
    """The E-step of one sequence by enumerating every complete path and weighting its edges, its emissions and their
    components' responsibilities by the path's posterior."""
    c = Compiled(model)
    E = table(model, seq)
    x = np.asarray(seq, np.float64).reshape(-1)
    n, NE, ptr = E.shape[0], c.NE, mix_ptr(model)
    index = {(i, j): e for e, (i, j, _) in enumerate(model.edges)}
    paths = []

    def step(k, t, lp, used, emitted):
        if t == n and (not c.finite or k == c.end):
            paths.append((lp, used, emitted))
        for l, w in c.outs[k]:
            if l < NE:
                if t < n and E[t, l] > NEG:
                    step(l, t + 1, lp + w + E[t, l], used + [index[(k, l)]], emitted + [(l, t)])
            else:
                step(l, t, lp + w, used + [index[(k, l)]], emitted)

    step(c.start, 0, 0.0, [], [])
    counts, stats = np.zeros(len(model.edges)), np.zeros((NE + ptr[-1], 3))
    if not paths:
        return counts, stats, NEG
    logp = lse([p[0] for p in paths])
    for lp, used, emitted in paths:
        w = math.exp(lp - logp)
        for e in used:
            counts[e] += w
        for k, t in emitted:
            add_rows(stats, model, ptr, k, float(x[t]), w)
    return counts, stats, logp


def viterbi_counts(model, seqs):
    """Viterbi training's statistics: weight 1 per consumed observation in its state, shared out over the state's
    components by their responsibilities: (counts, stats, scores, skipped)."""
    index = {(i, j): e for e, (i, j, _) in enumerate(model.edges)}
    NE, ptr = T.n_emit(model), mix_ptr(model)
    counts, stats, scores, skipped = np.zeros(len(model.edges)), np.zeros((NE + ptr[-1], 3)), [], 0
    for s in seqs:
        lp, path = viterbi_ties(model, s)[:2]
        scores.append(lp)
        if path is None:
            skipped += 1
            continue
        for a, b in zip(path[:-1], path[1:]):
            counts[index[(a, b)]] += 1
        t = 0
        for k in path:
            if k < NE:
                add_rows(stats, model, ptr, k, float(s[t]), 1.0)
                t += 1
    return counts, stats, np.array(scores, np.float64), skipped


def m_step(model, counts, stats, transition_pseudocount=0.0, use_pseudocount=False, edge_inertia=0.0,
           distribution_inertia=0.0, min_std=0.01, pseudocounts=None):
    """The M-step on `model` in place: its edges list; its normal, log-normal and exponential distributions, each updated
    once from the rows pooled over every plain state and mixture slot that holds the object; its mixtures' weights, each
    mixture once from the W of its slots pooled over the states that hold it."""
    NE, ptr = T.n_emit(model), mix_ptr(model)
    stats = np.asarray(stats, np.float64).reshape(NE + ptr[-1], 3)
    new_edges, by_src = list(model.edges), {}
    for e, (i, j, p) in enumerate(model.edges):
        by_src.setdefault(i, []).append(e)
    for i, es in by_src.items():
        cnt = [counts[e] + transition_pseudocount + (pseudocounts[e] if use_pseudocount else 0.0) for e in es]
        tot = sum(cnt)
        for e, ce in zip(es, cnt):
            a, b, old = model.edges[e]
            new_edges[e] = (a, b, edge_inertia * old + (1 - edge_inertia) * (ce / tot if tot > 0 else old))
    model.edges = new_edges
    pool, order, weights = {}, [], collections.OrderedDict()
    for k in range(NE):
        whole = model.states[k].distribution
        if is_mixture(whole):
            held = [(d, NE + ptr[k] + j) for j, (d, _) in enumerate(slots(whole))]
            if not whole.frozen:
                acc = weights.setdefault(id(whole), [whole, [0.0] * len(held)])
                acc[1] = [a + stats[row, 0] for a, (_, row) in zip(acc[1], held)]
        else:
            held = [(whole, k)]
        for d, row in held:
            if d.frozen or whole.frozen:
                continue
            if id(d) not in pool:
                pool[id(d)] = [d, 0.0, 0.0, 0.0]
                order.append(id(d))
            acc = pool[id(d)]
            acc[1:] = [acc[1] + stats[row, 0], acc[2] + stats[row, 1], acc[3] + stats[row, 2]]
    keep = distribution_inertia
    for key in order:
        d, W, A, B = pool[key]
        name = type(d).__name__
        if not W > 0 or name in ("UniformDistribution", "GaussianKernelDensity"):
            continue
        if name == "ExponentialDistribution":
            if A > 0:
                d.parameters = [keep * d.parameters[0] + (1 - keep) * (W / A)]
            continue
        loc0, scale0 = d.parameters                       # normal: mean, std of x; log-normal: mu, sigma of log x
        loc = loc0 + A / W
        scale = max(math.sqrt(max(B / W - (A / W) ** 2, 0.0)), min_std)
        d.parameters = [keep * loc0 + (1 - keep) * loc, keep * scale0 + (1 - keep) * scale]
    for whole, W in weights.values():
        tot = sum(W)
        if tot > 0:
            whole.parameters[1] = [min(keep * old + (1 - keep) * (w / tot), 1.0) for old, w in zip(whole.parameters[1], W)]


def train(model, seqs, max_iterations, stop_threshold=1e-9, min_iterations=0, algorithm="baum-welch", **kw):
    """The training loop of the module docstring on a deep copy of `model`: (the copy, [improvements], total)."""
    saved, model._c, model._s = (model._c, model._s), None, None
    try:
        m = copy.deepcopy(model)
    finally:
        model._c, model._s = saved
    pc = T.pseudocounts_of(m)
    stat = viterbi_counts if algorithm == "viterbi" else estep
    counts, stats, logp, _ = stat(m, seqs)
    keep = logp > NEG
    seqs = [s for s, k in zip(seqs, keep) if k]
    initial = float(np.sum(logp[keep]))
    improvement, it, total, steps = np.inf, 0, 0.0, []
    while improvement > stop_threshold or it < min_iterations:
        if max_iterations is not None and it >= max_iterations:
            break
        m_step(m, counts, stats, pseudocounts=pc, **kw)
        counts, stats, logp, _ = stat(m, seqs)
        trained = float(np.sum(logp))
        improvement = trained - initial
        total += improvement
        initial = trained
        steps.append(improvement)
        it += 1
    return m, steps, total


# ---- sampling ---------------------------------------------------------------------------------------------------------
def tables(model):
    """dict(out_cdf, emit_param, kde_cdf, mix_ptr, mix_cdf, mix_draw, mix_dist) as lists, from model.flat and the states'
    distributions: emit_param (0, 0) for a mixture state; mix_cdf the running sum of the state's weights, added one by
    one, exactly 1.0 from the state's last component of positive weight on; mix_draw by sample_oracle.emit_pair."""
    f = model.flat
    emit, cdf, draw, dist = [], [], [], []
    for s in model.states[:f["n_emit"]]:
        held = slots(s.distribution)
        emit.extend((0.0, 0.0) if held else SO.emit_pair(s.distribution))
        if held:
            last = max(j for j, (_, w) in enumerate(held) if w > 0)
            run = 0.0
            for j, (d, w) in enumerate(held):
                run = run + w
                cdf.append(1.0 if j >= last else run)
                draw.extend(SO.emit_pair(d))
                dist.append(d)
    return dict(out_cdf=SO.running(np.exp(f["out_lp"]), f["out_ptr"]), emit_param=emit,
                kde_cdf=SO.running(np.exp(f["kde_lw"]), f["kde_ptr"]), mix_ptr=mix_ptr(model), mix_cdf=cdf, mix_draw=draw,
                mix_dist=dist)


Walk = collections.namedtuple("Walk", "obs path flag exact comp")


def walk(model, TB, seed, Q, length=0, max_length=1000000):
    """One walk of a scalar model: Walk(obs: floats, path: state indices from start on, flag 0 / 1 / 2, exact: per
    observation whether it passed through no libm function -- a uniform draw --, comp: per observation the mixture
    component it was drawn from, as its index in the tables, -1 for another state).  A mixture emission takes two blocks:
    the first component i of the state with u0 < mix_cdf[i], then that component's draw from the next block."""
    f = model.flat
    NE, end = f["n_emit"], f["end"]
    ptr, dst, kptr, kpt = f["out_ptr"], f["out_dst"], f["kde_ptr"], f["kde_pt"]
    k, j, flag = f["start"], 0, 1
    obs, exact, comp, path = [], [], [], [k]
    for _ in range((max_length + 1) * (f["n_levels"] + 1) + 1):
        if k == end or (length > 0 and len(obs) >= length):
            flag = 0
            break
        if len(obs) >= max_length:
            break
        e0, e1 = int(ptr[k]), int(ptr[k + 1])
        if e0 == e1:
            flag = 2
            break
        k = int(dst[SO.pick(TB["out_cdf"], e0, e1, SO.block(seed, Q, j)[0])])
        j += 1
        path.append(k)
        if k < NE:
            d = model.states[k].distribution
            u0, u1 = SO.block(seed, Q, j)
            j += 1
            if is_mixture(d):
                i = SO.pick(TB["mix_cdf"], TB["mix_ptr"][k], TB["mix_ptr"][k + 1], u0)
                u0, u1 = SO.block(seed, Q, j)
                j += 1
                d = TB["mix_dist"][i]
                obs.append(SO.draw(d, TB["mix_draw"][2 * i], TB["mix_draw"][2 * i + 1], u0, u1))
                comp.append(i)
            elif isinstance(d, GaussianKernelDensity):
                p = float(kpt[SO.pick(TB["kde_cdf"], int(kptr[k]), int(kptr[k + 1]), u0)])
                u0, u1 = SO.block(seed, Q, j)
                j += 1
                obs.append(p + TB["emit_param"][2 * k + 1] * SO.normal(u0, u1))
                comp.append(-1)
            else:
                obs.append(SO.draw(d, TB["emit_param"][2 * k], TB["emit_param"][2 * k + 1], u0, u1))
                comp.append(-1)
            exact.append(isinstance(d, UniformDistribution))
    return Walk(obs, path, flag, exact, comp)


def batch(model, n, seed, first=0, length=0, max_length=1000000):
    TB = tables(model)
    return [walk(model, TB, seed, first + q, length, max_length) for q in range(n)]


# ---- models and inputs ------------------------------------------------------------------------------------------------
def wrapped(plain):
    """The baked normal / uniform model built again from its own construction graph with every emitting state's
    distribution inside a one-component mixture of weight 1: the same states, order, edges and probabilities."""
    m = Model(plain.name)
    twin = {id(plain.start): m.start, id(plain.end): m.end}
    shared = {}
    for s in plain._added:
        if id(s) in twin:
            continue
        d = s.distribution
        if d is not None:
            d = shared.setdefault(id(d), MixtureDistribution([copy.deepcopy(d)]))
        twin[id(s)] = State(d, s.name)
        m.add_state(twin[id(s)])
    for (x, y), p in plain._edges.items():
        m.add_transition(twin[id(x)], twin[id(y)], p, pseudocount=plain._pseudo[(x, y)])
    m.bake()
    return m


def mixed_components(rng, count, level):
    """`count` components of mixed kinds around the positive level, and their weights: with more than one, one of weight 0."""
    kinds = [NormalDistribution(level + float(rng.normal(0, 2)), float(rng.uniform(0.6, 2.0))),
             UniformDistribution(level - float(rng.uniform(3, 6)), level + float(rng.uniform(3, 6))),
             LogNormalDistribution(math.log(level) + float(rng.normal(0, 0.05)), float(rng.uniform(0.05, 0.2))),
             ExponentialDistribution(1.0 / level),
             NormalDistribution(level - 5.0, float(rng.uniform(0.6, 1.5))),
             LogNormalDistribution(math.log(level + 4.0), 0.1),
             UniformDistribution(0.0, 90.0)]
    first = int(rng.integers(len(kinds)))
    comps = [kinds[(first + j) % len(kinds)] for j in range(count)]
    weights = [float(w) for w in rng.uniform(0.2, 1.0, count)]
    if count > 1:
        weights[int(rng.integers(count))] = 0.0
    return comps, weights


MIX_LANES = (0, 5, 20, 63, 64, 70, 100, 129)


def line_model(n_emit, seed=0):
    """n_emit emitting states on a left-to-right line with self-loops and skips, start entering every 16th.  The states
    at MIX_LANES (lanes 0, 5, 20 and 63 of the first stride of 64, lanes 0, 6, 36 and 1 of the next ones) are mixtures of
    1, 2 and 7 components in turn, of mixed kinds, one of weight 0 where there are several; the others are normal, every
    ninth uniform.  Levels are
    positive, so log-normal and exponential components take part."""
    rng = np.random.default_rng(1000 * seed + n_emit)
    levels = rng.uniform(20, 60, n_emit)
    m = Model("mixline%d" % n_emit)
    st, turn = [], 0
    for i in range(n_emit):
        if i in MIX_LANES:
            d = MixtureDistribution(*mixed_components(rng, (1, 2, 7)[turn % 3], float(levels[i])))
            turn += 1
        elif i % 9 == 4:
            d = UniformDistribution(float(levels[i]) - 8.0, float(levels[i]) + 8.0)
        else:
            d = NormalDistribution(float(levels[i]), float(rng.uniform(0.8, 2.0)))
        st.append(State(d, "s%04d" % i))
    for i, s in enumerate(st):
        if i % 16 == 0:
            m.add_transition(m.start, s, 1.0)
        m.add_transition(s, s, 0.3)
        if i + 1 < n_emit:
            m.add_transition(s, st[i + 1], 0.5)
        if i + 2 < n_emit:
            m.add_transition(s, st[i + 2], 0.1)
        m.add_transition(s, m.end, 0.1)
    m.bake()
    return m, levels


def line_sequences(levels, seed):
    """Sequences of lengths 0, 1, 2 and 65 walking along the line's levels, and one far below every level, which every
    log-normal, exponential and uniform component excludes."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, 2, 65):
        idx = np.minimum(np.cumsum(rng.choice([0, 1, 1, 2], n)), len(levels) - 1) if n else np.zeros(0, np.int64)
        out.append(levels[idx] + rng.normal(0, 1.0, n))
    return out + [np.full(3, -5.0)]


def silent_model(finite, seed=0):
    """Six emitting states -- three of them mixtures, one holding a kernel density beside them -- and a chain of five
    silent states entered from the emitting ones: silent levels under the mixture type."""
    rng = np.random.default_rng(50 + seed)
    m = Model("mixsilent")
    lv = [20.0, 28.0, 36.0, 44.0, 52.0, 60.0]
    ds = [MixtureDistribution(*mixed_components(rng, 2, lv[0])), NormalDistribution(lv[1], 2.0),
          MixtureDistribution(*mixed_components(rng, 7, lv[2])), GaussianKernelDensity([lv[3] - 1, lv[3] + 2], 1.5, [1, 3]),
          MixtureDistribution(*mixed_components(rng, 1, lv[4])), UniformDistribution(lv[5] - 9, lv[5] + 9)]
    st = [State(d, "e%d" % i) for i, d in enumerate(ds)]
    chain = [State(None, "c%d" % i) for i in range(5)]
    m.add_transition(m.start, chain[0], 0.5)
    m.add_transition(m.start, st[0], 0.5)
    for a, b in zip(chain[:-1], chain[1:]):
        m.add_transition(a, b, 0.6)
    for i, c in enumerate(chain):
        m.add_transition(c, st[i], 0.4)
    m.add_transition(chain[-1], st[5], 0.6)
    for i, s in enumerate(st):
        m.add_transition(s, s, 0.3)
        m.add_transition(s, st[(i + 1) % 6], 0.4)
        m.add_transition(s, chain[i % 5], 0.2)
        if finite:
            m.add_transition(s, m.end, 0.1)
    m.bake()
    return m, np.array(lv)


def tiny_model(finite):
    """Three emitting states (a mixture of three kinds with a zero weight, a normal, a two-component mixture) and one
    silent state: small enough to enumerate every path of a sequence of five."""
    m = Model("mixtiny")
    a = State(MixtureDistribution([NormalDistribution(1.0, 1.0), UniformDistribution(0.0, 4.0), LogNormalDistribution(0.5, 0.5),
                                   ExponentialDistribution(0.7)], [0.4, 0.3, 0.0, 0.3]), "a")
    b = State(NormalDistribution(2.5, 1.0), "b")
    c = State(MixtureDistribution([LogNormalDistribution(0.8, 0.4), NormalDistribution(-1.0, 0.8)], [0.25, 0.75]), "c")
    s = State(None, "s")
    for x, y, p in ((m.start, a, 0.6), (m.start, s, 0.4), (s, b, 0.5), (s, c, 0.5), (a, a, 0.3), (a, b, 0.3), (a, s, 0.3),
                    (b, c, 0.5), (b, a, 0.3), (c, c, 0.4), (c, s, 0.3), (c, a, 0.2)):
        m.add_transition(x, y, p)
    if finite:
        for x in (a, b, c):
            m.add_transition(x, m.end, 0.1)
    m.bake()
    return m


TINY_SEQUENCES = ([], [1.2], [0.7, 2.9], [1.5, -0.8, 2.2], [3.1, 0.4, 1.1, -1.6, 2.0], [5.0, -0.5])


def bimodal_model(split=4.0, weight=0.5, std=1.5):
    """Two states: `a` bimodal -- a mixture of two normals `split` either side of 30 -- and `b` normal at 45."""
    m = Model("bimodal")
    a = State(MixtureDistribution([NormalDistribution(30.0 - split, std), NormalDistribution(30.0 + split, std)],
                                  [weight, 1.0 - weight]), "a")
    b = State(NormalDistribution(45.0, 2.0), "b")
    for x, y, p in ((m.start, a, 0.7), (m.start, b, 0.3), (a, a, 0.6), (a, b, 0.3), (a, m.end, 0.1), (b, b, 0.5), (b, a, 0.4),
                    (b, m.end, 0.1)):
        m.add_transition(x, y, p)
    m.bake()
    return m


def training_model():
    """Five states: two hold one mixture object (its weights are pooled), one mixture shares a component object with a
    plain normal state, one mixture is frozen, one mixture has a log-normal, an exponential and a zero-weight slot."""
    shared_mix = MixtureDistribution([NormalDistribution(24.0, 2.0), NormalDistribution(30.0, 2.0)], [0.6, 0.4])
    shared_comp = NormalDistribution(40.0, 2.5)
    frozen = MixtureDistribution([NormalDistribution(50.0, 2.0), NormalDistribution(55.0, 2.0)], [0.5, 0.5])
    frozen.freeze()
    kinds = MixtureDistribution([LogNormalDistribution(math.log(62.0), 0.06), ExponentialDistribution(1.0 / 60.0),
                                 NormalDistribution(66.0, 2.0), UniformDistribution(50.0, 80.0)], [0.4, 0.1, 0.0, 0.5])
    ds = [shared_mix, shared_mix, MixtureDistribution([shared_comp, NormalDistribution(35.0, 2.0)], [0.7, 0.3]), shared_comp,
          frozen, kinds]
    m = Model("mixtrain")
    st = [State(d, "s%d" % i) for i, d in enumerate(ds)]
    for k, s in enumerate(st):
        m.add_transition(m.start, s, 1.0)
        m.add_transition(s, s, 0.4)
        for t in st[k + 1:k + 3]:
            m.add_transition(s, t, 0.3)
        m.add_transition(s, m.end, 0.1)
        if k:
            m.add_transition(s, st[0], 0.05)
    m.bake()
    return m


def training_data(seed=4, count=12):
    rng = np.random.default_rng(seed)
    centres = np.array([26.0, 27.0, 38.0, 41.0, 52.0, 63.0])
    out = []
    for _ in range(count):
        n = int(rng.integers(5, 40))
        k = np.minimum(np.cumsum(rng.choice([0, 1, 1], n)), 5)
        out.append(centres[k] + rng.normal(0, 2.5, n))
    return out


def viterbi_inputs():
    """[(name, model, sequences)]: every input on which the GPU tests demand the oracle's Viterbi path."""
    out = []
    for n_emit in (63, 64, 65, 130):
        model, levels = line_model(n_emit)
        out.append(("line%d" % n_emit, model, line_sequences(levels, 7 + n_emit)))
    for finite in (True, False):
        model, levels = silent_model(finite)
        rng = np.random.default_rng(3 + finite)
        out.append(("silent-%s" % ("finite" if finite else "infinite"), model,
                    [levels[rng.integers(0, 6, n)] + rng.normal(0, 1.0, n) for n in (0, 1, 2, 65)]))
    for finite in (True, False):
        out.append(("tiny-%s" % ("finite" if finite else "infinite"), tiny_model(finite),
                    [np.array(s, np.float64) for s in TINY_SEQUENCES]))
    out.append(("train", training_model(), training_data()))
    return out
