"""Test-side oracle for the vector models of pypore_amd.hmm (MultivariateDistribution, LogNormalDistribution,
ExponentialDistribution), written on its own from the module docstring:

  * the component log densities written out again (`component`), beside a np.longdouble version (`component_ld`), and a
    state's emission, the weighted sum in ascending d from the first product (`emission`);
  * the log-space dynamic programmes of tests/hmm_oracle.py, which read the emissions through their `Compiled` view: here
    the view (`Compiled`) takes them from a per-observation table e[t][k] (`table`) and the programmes are handed the
    observations' indices 0 .. n-1 instead of the observations (`bind`), so forward, backward, Viterbi with its near-tie
    report (hmm_oracle.viterbi_ties) and posterior decoding (posterior_oracle.posterior) run unchanged on any emission;
  * a brute-force enumerator over every state path of a tiny model (`brute_force`);
  * the E-step with W and (A_d, B_d) per component (`estep_one`, `estep`), Viterbi training's counts (`viterbi_counts`), the
    M-step pooled per distribution object over states and component slots (`m_step`) and the training loop (`train`);
  * `viterbi_exact`: the device's Viterbi restated operation by operation on model.flat (comp_kind / comp_param / comp_w)
    in Python floats, which gives the device's bits for models without log-normal components (the device's log is not
    numpy's bit for bit; a log-normal component raises ValueError);
  * the models and inputs the GPU tests use (`line_model`, `silent_model`, `hub_model`, `wrapped`, `profile3`,
    `lognormal_cases`), so that the host tests can examine the same inputs with the oracle alone."""
import copy
import math

import numpy as np

import hmm_oracle as O
import hmm_train_oracle as T
import posterior_oracle as PO

from pypore_amd.hmm import (ExponentialDistribution, LogNormalDistribution, Model, MultivariateDistribution,  # noqa: E402
                            NormalDistribution, State, UniformDistribution)

NEG = -np.inf


# ---- emissions --------------------------------------------------------------------------------------------------------
def component(d, x):
    """Log density of the value x under a univariate distribution, from its `parameters` (module docstring formulas)."""
    name, p = type(d).__name__, d.parameters
    if name == "NormalDistribution":
        return -math.log(p[1] * math.sqrt(2 * math.pi)) - (x - p[0]) ** 2 / (2 * p[1] ** 2)
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


def component_ld(d, x):
    """The same in np.longdouble (parameters and x taken as the doubles they are)."""
    L = np.longdouble
    name, p, x = type(d).__name__, [L(v) for v in d.parameters], L(x)
    two_pi = 2 * L(np.pi) if np.finfo(L).eps == np.finfo(np.float64).eps else 8 * np.arctan(L(1))
    if name == "NormalDistribution":
        return -np.log(p[1] * np.sqrt(two_pi)) - (x - p[0]) ** 2 / (2 * p[1] ** 2)
    if name == "UniformDistribution":
        return -np.log(p[1] - p[0]) if p[0] <= x <= p[1] else L(NEG)
    if name == "LogNormalDistribution":
        if not x > 0:
            return L(NEG)
        y = np.log(x)
        return (-np.log(p[1] * np.sqrt(two_pi)) - (y - p[0]) ** 2 / (2 * p[1] ** 2)) - y
    if name == "ExponentialDistribution":
        return np.log(p[0]) - p[0] * x if x >= 0 else L(NEG)
    raise TypeError("no formula for %r" % (d,))


def parts(distribution):
    """[(component, weight)] of a state's distribution: a MultivariateDistribution's own, or the distribution itself."""
    if type(distribution).__name__ == "MultivariateDistribution":
        return list(zip(*distribution.parameters))
    return [(distribution, 1.0)]


def emission(distribution, row, fn=component):
    """w_0 l_0(x_0) + w_1 l_1(x_1) + ... in ascending d, starting from the first product."""
    total = None
    for (d, w), x in zip(parts(distribution), row):
        term = w * fn(d, x)
        total = term if total is None else total + term
    return total


def rows(model, seq):
    """The sequence as an (n, D) float64 array, D = the model's components per state."""
    D = len(parts(model.states[0].distribution)) if not model.states[0].is_silent() else 1
    return np.asarray(seq, np.float64).reshape(-1, D)


def table(model, seq):
    """e[t][k]: the log density of observation t in emitting state k, (n, n_emit)."""
    ne = T.n_emit(model)
    x = rows(model, seq)
    return np.array([[emission(model.states[k].distribution, r) for k in range(ne)] for r in x.tolist()],
                    np.float64).reshape(len(x), ne)


class Compiled(O.Compiled):
    """hmm_oracle.Compiled (edges of probability 0 left out, as hmm_train_oracle.View does) whose emissions come from the
    table of the sequence last bound: emissions(t) = e[t]."""

    def __init__(self, model, edges=None):
        O.Compiled.__init__(self, T.View(model, edges))
        self.model = model
        self.E = None

    def bind(self, seq):
        """Sets the table of `seq`; returns what the dynamic programmes are handed in its place: the indices 0 .. n-1."""
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
    """posterior_oracle.posterior on the table, counts aligned with model.edges."""
    c = Compiled(model)
    return PO.posterior(c, c.bind(seq), model.edges)


def brute_force(model, seq):
    """Every state path enumerated: (forward matrix, log_probability, best score, best path)."""
    c = Compiled(model)
    E = table(model, seq)
    n = E.shape[0]
    terms, ends = {}, []

    def walk(k, t, lp, path):
        terms.setdefault((t, k), []).append(lp)
        if t == n and (not c.finite or k == c.end):
            ends.append((lp, path))
        for l, w in c.outs[k]:
            if l < c.NE:
                if t < n and E[t, l] > NEG:
                    walk(l, t + 1, lp + w + E[t, l], path + [l])
            else:
                walk(l, t, lp + w, path + [l])

    walk(c.start, 0, 0.0, [c.start])
    F = np.full((n + 1, c.S), NEG)
    for (t, k), v in terms.items():
        F[t, k] = O.lse_rows(np.array(v)[None, :])[0]
    if not ends:
        return F, NEG, NEG, None
    scores = np.array([e[0] for e in ends])
    best = int(np.argmax(scores))
    return F, O.lse_rows(scores[None, :])[0], scores[best], ends[best][1]


# ---- training ---------------------------------------------------------------------------------------------------------
def shifts_and_logs(model):
    """(shift [NE, D], takes-the-logarithm [NE, D]) of the components' statistics: normal mean, log-normal mu (of log x),
    exponential 0, uniform low."""
    ne = T.n_emit(model)
    sh, lg = [], []
    for k in range(ne):
        for d, _ in parts(model.states[k].distribution):
            name = type(d).__name__
            sh.append(0.0 if name == "ExponentialDistribution" else d.parameters[0])
            lg.append(name == "LogNormalDistribution")
    return np.array(sh, np.float64).reshape(ne, -1), np.array(lg, bool).reshape(ne, -1)


def deviations(model, seq):
    """y - c per (observation, state, component), with y = log x for a log-normal component (0 where x <= 0: such an
    observation has posterior 0 there)."""
    sh, lg = shifts_and_logs(model)
    x = np.broadcast_to(rows(model, seq)[:, None, :], (len(rows(model, seq)),) + sh.shape)
    y = np.where(lg[None], np.log(np.where(x > 0, x, 1.0)), x)
    return np.where(lg[None] & ~(x > 0), 0.0, y - sh[None])


def estep_one(model, seq, edges=None):
    """(counts aligned with model.edges, stats [NE, 1 + 2 D]: W then (A_d, B_d), logp) of one sequence; zeros for -inf."""
    edges = model.edges if edges is None else edges
    c = Compiled(model, edges)
    idx = c.bind(seq)
    n, NE = idx.size, c.NE
    dev = deviations(model, seq)
    counts, stats = np.zeros(len(edges)), np.zeros((NE, 1 + 2 * dev.shape[2]))
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
    if n:
        both = np.isfinite(F[1:, :NE]) & np.isfinite(B[1:, :NE])
        with np.errstate(invalid="ignore"):
            g = np.where(both, np.exp(F[1:, :NE] + B[1:, :NE] - logp), 0.0)
        stats[:, 0] = g.sum(axis=0)
        stats[:, 1::2] = (g[:, :, None] * dev).sum(axis=0)
        stats[:, 2::2] = (g[:, :, None] * dev * dev).sum(axis=0)
    return counts, stats, logp


def estep(model, seqs, edges=None):
    """Batch E-step: (counts, stats, logp array, skipped)."""
    edges = model.edges if edges is None else edges
    counts, stats, logp = np.zeros(len(edges)), None, []
    for s in seqs:
        cc, st, lp = estep_one(model, s, edges)
        stats = np.zeros_like(st) if stats is None else stats
        logp.append(lp)
        if lp > NEG:
            counts += cc
            stats += st
    logp = np.array(logp, np.float64)
    return counts, stats, logp, int(np.sum(~(logp > NEG)))


def viterbi_counts(model, seqs):
    """Viterbi training's statistics, weight 1 per consumed observation: (counts, stats, scores, skipped)."""
    index = {(i, j): e for e, (i, j, _) in enumerate(model.edges)}
    NE = T.n_emit(model)
    counts, stats, scores, skipped = np.zeros(len(model.edges)), None, [], 0
    for s in seqs:
        dev = deviations(model, s)
        stats = np.zeros((NE, 1 + 2 * dev.shape[2])) if stats is None else stats
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
                stats[k, 0] += 1.0
                stats[k, 1::2] += dev[t, k]
                stats[k, 2::2] += dev[t, k] ** 2
                t += 1
    return counts, stats, np.array(scores, np.float64), skipped


def m_step(model, counts, stats, transition_pseudocount=0.0, use_pseudocount=False, edge_inertia=0.0,
           distribution_inertia=0.0, min_std=0.01, pseudocounts=None):
    """The M-step on `model` in place: its edges list, and its component distributions, each updated once from the
    statistics pooled over every (state, slot) that holds the object."""
    NE = T.n_emit(model)
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
    pool, order = {}, []
    for k in range(NE):
        whole = model.states[k].distribution
        for slot, (d, _) in enumerate(parts(whole)):
            if d.frozen or whole.frozen:
                continue
            if id(d) not in pool:
                pool[id(d)] = [d, 0.0, 0.0, 0.0]
                order.append(id(d))
            acc = pool[id(d)]
            acc[1] += stats[k, 0]
            acc[2] += stats[k, 1 + 2 * slot]
            acc[3] += stats[k, 2 + 2 * slot]
    keep = distribution_inertia
    for key in order:
        d, W, A, B = pool[key]
        name = type(d).__name__
        if not W > 0 or name == "UniformDistribution":
            continue
        if name == "ExponentialDistribution":
            if A > 0:
                d.parameters = [keep * d.parameters[0] + (1 - keep) * (W / A)]
            continue
        loc0, scale0 = d.parameters                       # normal: mean, std of x; log-normal: mu, sigma of log x
        loc = loc0 + A / W
        scale = max(math.sqrt(max(B / W - (A / W) ** 2, 0.0)), min_std)
        d.parameters = [keep * loc0 + (1 - keep) * loc, keep * scale0 + (1 - keep) * scale]


def train(model, seqs, max_iterations, stop_threshold=1e-9, min_iterations=0, algorithm="baum-welch", **kw):
    """The training loop of the module docstring on a deep copy of `model`: (the copy, [improvements], total)."""
    saved, model._c = model._c, None
    try:
        m = copy.deepcopy(model)
    finally:
        model._c = saved
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


# ---- the device's Viterbi, bit for bit --------------------------------------------------------------------------------
def viterbi_exact(model, seq):
    """The device's Viterbi on a vector model (csrc/seg_hmm.hpp hmm_fwd_kernel<HMM_VITERBI, .., HmmDevV>, hmm_emit,
    hmm_trace_kernel) restated operation by operation in Python floats on model.flat, in the manner of
    hmm_oracle.viterbi_exact: in-edges scanned in ordinal order from -inf (`start` at t = 0 from 0.0), replaced only by a
    strictly greater score; an emitting state takes  best + emission  where best > -inf; the emission is the sum over its
    components in ascending d of  w * l  from the first product, with l = c - (d*d)*b (normal, d = x - a), c inside
    [a, b] else -inf (uniform), c - x*b for x >= 0 else -inf (exponential).  A log-normal component raises ValueError.
    Returns (logp, path as state indices or None, the (n+1) x S score matrix)."""
    f = model.flat
    S, NE, D, start, end = f["n_states"], f["n_emit"], f["n_dim"], f["start"], f["end"]
    ck, cp, cw = f["comp_kind"].tolist(), f["comp_param"].tolist(), f["comp_w"].tolist()
    if len(ck) != NE * D or 5 in ck:
        raise ValueError("viterbi_exact takes a vector model without log-normal components")
    in_ptr, in_src, in_lp, level_ptr = f["in_ptr"].tolist(), f["in_src"].tolist(), f["in_lp"].tolist(), f["level_ptr"].tolist()
    xs = np.asarray(seq, np.float64).reshape(-1, D).tolist()
    n, ninf = len(xs), float("-inf")

    def emit(k, row):
        s = 0.0
        for d in range(D):
            i = k * D + d
            a, b, c, x = cp[3 * i], cp[3 * i + 1], cp[3 * i + 2], row[d]
            if ck[i] == 1:
                u = x - a
                l = c - (u * u) * b
            elif ck[i] == 2:
                l = c if (x >= a and x <= b) else ninf
            else:
                l = c - x * b if x >= 0.0 else ninf
            wl = cw[i] * l
            s = s + wl if d else wl
        return s

    def scan(row, k, best):
        arg, e0 = 0, in_ptr[k]
        for o in range(in_ptr[k + 1] - e0):
            v = row[in_src[e0 + o]] + in_lp[e0 + o]
            if v > best:
                best, arg = v, o
        return best, arg

    F, bp = [], []
    for t in range(n + 1):
        row, b = [ninf] * S, [0] * S
        if t > 0:
            for k in range(NE):
                best, b[k] = scan(F[t - 1], k, ninf)
                row[k] = best + emit(k, xs[t - 1]) if best > ninf else ninf
        for L in range(len(level_ptr) - 1):
            for k in range(level_ptr[L], level_ptr[L + 1]):
                row[k], b[k] = scan(row, k, 0.0 if (t == 0 and k == start) else ninf)
        F.append(row)
        bp.append(b)
    mat = np.array(F, np.float64).reshape(n + 1, S)
    if f["finite"]:
        logp, k = F[n][end], end
    else:
        logp = max(F[n])
        k = F[n].index(logp)
    if not logp > ninf:
        return ninf, None, mat
    t, path = n, [k]
    while not (t == 0 and k == start):
        e = in_ptr[k] + bp[t][k]
        if k < NE:
            t -= 1
        k = in_src[e]
        path.append(k)
    return logp, path[::-1], mat


# ---- models and inputs of the tests -----------------------------------------------------------------------------------
# Components by letter: n normal, u uniform, l log-normal, e exponential.  The models rotate the letters from state to
# state, so every slot of an observation meets every kind: observations are drawn positive, where all of them have mass.
def random_component(rng, letter):
    if letter == "n":
        return NormalDistribution(float(rng.normal(2, 1.5)), float(rng.uniform(0.5, 2)))
    if letter == "u":
        lo = float(rng.uniform(-6, -3))
        return UniformDistribution(lo, lo + float(rng.uniform(14, 18)))
    if letter == "l":
        return LogNormalDistribution(float(rng.normal(0.5, 0.5)), float(rng.uniform(0.3, 1.0)))
    return ExponentialDistribution(float(rng.uniform(0.3, 2)))


def random_state_distribution(rng, letters, unit_weights=False):
    comps = [random_component(rng, c) for c in letters]
    return MultivariateDistribution(comps, None if unit_weights else [float(rng.uniform(0.5, 2)) for _ in comps])


def draw(rng, letters, n):
    """n observations for components `letters`: (n, D), or 1-D for D = 1."""
    cols = [rng.lognormal(0.5, 0.7, n) for _ in letters]
    x = np.stack(cols, axis=1) if n else np.zeros((0, len(letters)))
    return x.reshape(-1) if len(letters) == 1 else x


def cycle(letters, k):
    """The component letters of state k: `letters` rotated by k, so every slot meets every kind."""
    return "".join(letters[(k + d) % len(letters)] for d in range(len(letters)))


def line_model(n_emit, letters, seed=0, rotate=True):
    """hmm_oracle.line_model's shape with n_emit vector states of len(letters) components: a left-to-right line with
    self-loops and skips, start entering every 64th state, every state leaving to end (finite)."""
    rng = np.random.default_rng(1000 * n_emit + seed)
    m = Model("vline")
    st = [State(random_state_distribution(rng, cycle(letters, k) if rotate else letters), "s%04d" % k) for k in range(n_emit)]
    for i, s in enumerate(st):
        if i % 64 == 0:
            m.add_transition(m.start, s, 1.0)
        m.add_transition(s, s, 0.3)
        if i + 1 < len(st):
            m.add_transition(s, st[i + 1], 0.5)
        if i + 2 < len(st):
            m.add_transition(s, st[i + 2], 0.1)
        m.add_transition(s, m.end, 0.1)
    m.bake()
    return m


def silent_model(letters, seed=0, finite=True, n_emit=6, chain=5):
    """n_emit vector states and a chain of `chain` silent states (levels 1 .. chain above start) that the emitting states
    enter anywhere and leave from its end; random edges among the emitting states."""
    rng = np.random.default_rng(seed)
    m = Model("vsilent")
    st = [State(random_state_distribution(rng, cycle(letters, k)), "e%02d" % k) for k in range(n_emit)]
    ch = [State(None, "c%02d" % i) for i in range(chain)]
    for a, b in zip(ch[:-1], ch[1:]):
        m.add_transition(a, b, float(rng.uniform(0.3, 1)))
    m.add_transition(m.start, st[0], 0.6)
    m.add_transition(m.start, ch[0], 0.4)
    for s in st:
        for t in st:
            if rng.random() < 0.5:
                m.add_transition(s, t, float(rng.uniform(0.05, 1)))
        m.add_transition(s, s, 0.3)
        m.add_transition(s, ch[int(rng.integers(chain))], float(rng.uniform(0.05, 0.5)))
        if finite and rng.random() < 0.5:
            m.add_transition(s, m.end, float(rng.uniform(0.05, 0.5)))
    for i, c in enumerate(ch):
        m.add_transition(c, st[int(rng.integers(n_emit))], float(rng.uniform(0.2, 1)))
    if finite:
        m.add_transition(st[-1], m.end, 0.2)
        m.add_transition(ch[-1], m.end, 0.1)
    m.bake()
    return m


def hub_model(n_in, letters="ne"):
    """hmm_oracle.hub_model's shape with vector states: a hub h with n_in in-edges (16-bit backpointers beyond 255).  The
    first component of e<i> is normal at 3 i with std 0.5 (h's at -50), so an observation's first value names its state."""
    rng = np.random.default_rng(n_in)

    def dist(mean, std):
        return MultivariateDistribution([NormalDistribution(mean, std)] + [random_component(rng, c) for c in letters[1:]])
    m = Model("vhub")
    h = State(dist(-50.0, 1.0), "h")
    es = [State(dist(3.0 * i, 0.5), "e%04d" % i) for i in range(n_in - 1)]
    for e in es:
        m.add_transition(m.start, e, 1.0)
        m.add_transition(e, h, 0.8)
        m.add_transition(e, m.end, 0.2)
        m.add_transition(h, e, 0.4 / len(es))
    m.add_transition(h, h, 0.4)
    m.add_transition(h, m.end, 0.2)
    m.bake()
    return m


def hub_sequence(n_in, letters="ne", seed=0):
    """e5, h, e200, h, h, e17: first values at the states' levels, the others positive."""
    rng = np.random.default_rng(seed)
    first = np.array([15.0, -50.0, 600.0, -50.2, -49.5, 51.0]) + rng.normal(0, 0.1, 6)
    return np.column_stack([first] + [rng.lognormal(0.0, 0.5, 6) for _ in letters[1:]])


def wrapped(plain):
    """The baked model `plain` (normal and uniform states) built again with every emitting state's distribution wrapped
    as a one-component MultivariateDistribution of weight 1 -- a vector model of n_dim 1 with the same states, order and
    edges -- beside an ExponentialDistribution state without edges, which no path can reach (bake drops it)."""
    twin = {id(plain.start): None, id(plain.end): None}
    m = Model(plain.name)
    twin[id(plain.start)], twin[id(plain.end)] = m.start, m.end
    shared = {}
    for s in plain._added:
        if id(s) in twin:
            continue
        d = s.distribution
        if d is not None:
            d = shared.setdefault(id(d), MultivariateDistribution([copy.deepcopy(d)]))
        twin[id(s)] = State(d, s.name)
        m.add_state(twin[id(s)])
    m.add_state(State(ExponentialDistribution(1.0), "zz-unreachable"))
    for (a, b), p in plain._edges.items():
        m.add_transition(twin[id(a)], twin[id(b)], p, pseudocount=plain._pseudo[(a, b)])
    m.bake()
    return m


def profile3(n=54, seed=0):
    """hmm_oracle.profile_model(n) (3n + 3 states; n = 54: 165) rebuilt with D = 3 match and insert states: a match
    scores (mean, std, duration) as normal at its level, normal around 1.0 and log-normal; an insert as uniform on [0, 90],
    uniform on [0, 10] and exponential.  Returns (model, match means)."""
    plain, means = O.profile_model(n, seed)
    rng = np.random.default_rng(seed + 77)
    insert = MultivariateDistribution([UniformDistribution(0, 90), UniformDistribution(0, 10), ExponentialDistribution(8.0)])
    twin = {id(plain.start): None}
    m = Model("profile3")
    twin[id(plain.start)], twin[id(plain.end)] = m.start, m.end
    for s in plain._added:
        if id(s) in twin:
            continue
        d = s.distribution
        if d is not None and type(d).__name__ == "NormalDistribution":
            d = MultivariateDistribution([NormalDistribution(*d.parameters), NormalDistribution(float(rng.uniform(0.8, 1.5)), 0.4),
                                          LogNormalDistribution(float(rng.normal(-2.5, 0.3)), float(rng.uniform(0.5, 0.9)))],
                                         [1.0, 0.5, 0.25])
        elif d is not None:
            d = insert
        twin[id(s)] = State(d, s.name)
    for (a, b), p in plain._edges.items():
        m.add_transition(twin[id(a)], twin[id(b)], p)
    m.bake()
    return m, means


def profile3_events(means, count, lo=50, hi=400, seed=1):
    """hmm_oracle.profile_events' walks with a std and a duration beside every mean: (n, 3) each."""
    rng = np.random.default_rng(seed + 5)
    out = []
    for x in O.profile_events(means, count, lo, hi, seed):
        out.append(np.column_stack([x, np.abs(rng.normal(1.1, 0.4, x.size)) + 0.05, rng.lognormal(-2.5, 0.8, x.size)]))
    return out


LOGNORMAL_LENGTHS = (0, 1, 2, 65)


def lognormal_cases():
    """[(name, model, sequences)]: every input with log-normal components that the GPU tests decode by Viterbi.  The host
    test asserts that the oracle alone finds no near tie (margin above 1e-9) on any of them."""
    cases = []
    for n_emit, letters in ((5, "l"), (63, "nl"), (64, "lne"), (65, "ul"), (127, "nle")):
        model = line_model(n_emit, letters, seed=3)
        rng = np.random.default_rng(50 + n_emit)
        cases.append(("line%d-%s" % (n_emit, letters), model, [draw(rng, letters, n) for n in LOGNORMAL_LENGTHS]))
    for finite in (True, False):
        model = silent_model("nle", seed=21 + finite, finite=finite)
        rng = np.random.default_rng(60 + finite)
        cases.append(("silent-%s" % ("finite" if finite else "infinite"), model, [draw(rng, "nle", n) for n in LOGNORMAL_LENGTHS]))
    model, means = profile3(54)
    cases.append(("profile3", model, profile3_events(means, 3, lo=30, hi=70, seed=2)))
    return cases
