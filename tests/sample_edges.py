"""Models, crafted tables and references for the edge tests of HMM sampling (tests/test_hmm_sample_edges_host.py on the
CPU, tests/test_hmm_sample_edges_gpu.py on the device).  Everything here runs on the host; every call builds a fresh,
equal model (fixed numbers only); every std, sigma and bandwidth is <= 10, as in tests/sample_models.py.

The walks' reference stays tests/sample_oracle.py (mixture_oracle.walk for a scalar model, which adds the mixture states):
both take the tables as an argument, so a crafted row goes to the device and to the oracle alike.  The emission values of
the chosen draws have a second reference, draw_mp: the four draw formulas of include/poreseg.h evaluated by mpmath at 50
digits from the table's doubles and the exact dyadic u0, u1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixture_oracle as MX  # noqa: E402
import sample_oracle as SO  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution,  # noqa: E402
                            MixtureDistribution, Model, MultivariateDistribution, NormalDistribution, State,
                            UniformDistribution)

TOP = 1.0 - 2.0 ** -53                                       # the largest u a block gives


# ---- tables the old way and row properties ------------------------------------------------------------------------------
def rows_closed_in_the_last_entry(p, ptr):
    """The tables as they were built before the row rule: the running sum, only the row's last entry stored as 1.0."""
    out = np.zeros(len(p), np.float64)
    for k in range(len(ptr) - 1):
        run = 0.0
        for e in range(int(ptr[k]), int(ptr[k + 1])):
            run = run + float(p[e])
            out[e] = run
        if ptr[k + 1] > ptr[k]:
            out[int(ptr[k + 1]) - 1] = 1.0
    return out


def check_rows(cdf, p, ptr, what):
    """The table invariant: per row no entry below its predecessor, an entry equal to its predecessor (the first: to 0)
    exactly where the probability is 0, and 1.0 from the last positive entry on.  Returns the number of rows looked at."""
    rows = 0
    for k in range(len(ptr) - 1):
        lo, hi = int(ptr[k]), int(ptr[k + 1])
        if lo == hi:
            continue
        rows += 1
        prev, last = 0.0, max(e for e in range(lo, hi) if p[e] > 0)
        for e in range(lo, hi):
            assert cdf[e] >= prev, (what, k, e - lo, cdf[e], prev)
            assert (cdf[e] == prev) == (not p[e] > 0), (what, k, e - lo, cdf[e], prev, p[e])
            assert (cdf[e] == 1.0) == (e >= last), (what, k, e - lo, cdf[e], last - lo)
            prev = cdf[e]
    return rows


# ---- hubs: one state whose row is the subject ------------------------------------------------------------------------
def target(i):
    """Target i of a hub: uniform on [10 i, 10 i + 1), so a sampled value names the edge taken and compares with ==."""
    return UniformDistribution(10.0 * i, 10.0 * i + 1.0)


def hub(weights, name="hub", own_state=True):
    """start -> hub (silent) -> one uniform target per weight -> end.  The hub's out-edges stand in target order (the
    targets' names sort as their numbers).  weights > 0; bake normalises them.  len(weights) + 3 states.  A walk picks
    the hub's edge with its second block.  own_state=False: `start` itself is the hub, and the pick is the first block."""
    m = Model(name)
    h = State(None, "hub") if own_state else m.start
    if own_state:
        m.add_transition(m.start, h, 1.0)
    for i, w in enumerate(weights):
        t = State(target(i), "t%04d" % i)
        m.add_transition(h, t, float(w))
        m.add_transition(t, m.end, 1.0)
    m.bake()
    return m


def hub_state(m):
    names = [s.name for s in m.states]
    return names.index("hub") if "hub" in names else int(m.flat["start"])


def hub_row(m):
    """(lo, hi) of the hub's row in out_cdf."""
    k = hub_state(m)
    return int(m.flat["out_ptr"][k]), int(m.flat["out_ptr"][k + 1])


def trained_hub(counts, name="trained"):
    """A hub whose out-edges hold counts / sum(counts) after one M-step: a count of 0 leaves an edge of probability 0
    (log probability -inf) in its place.  Every other edge gets the count 1, the distributions no statistics."""
    m = hub([1.0] * len(counts), name)
    train_hub(m, counts)
    return m


def train_hub(m, counts):
    k = hub_state(m)
    c = np.ones(len(m.edges))
    own = [e for e, (i, _, _) in enumerate(m.edges) if i == k]
    assert len(own) == len(counts)
    c[own] = counts
    m._m_step(c, np.zeros((m.flat["n_emit"], 3)))
    return m


FAN_OUT = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 600, 4093)    # 4093 targets + hub + start + end = 4096 states
KDE_POINTS = (1, 2, 3, 64, 65, 1000)
MIX_COMPONENTS = (1, 2, 7, 33)
FORMS = ("equal", "rising", "falling")


def weights(n, form):
    """equal: 1 each.  rising: r^(n-1-i), so the row's leading entries lie far below 2^-53.  falling: r^i, so the row
    climbs to 1.0 in steps of an ulp and then stands still.  r = 1/2, or nearer 1 where 2^-(n-1) would leave 1e-300."""
    if form == "equal":
        return [1.0] * n
    r = max(0.5, 10.0 ** (-300.0 / max(n - 1, 1)))
    return [r ** (n - 1 - i if form == "rising" else i) for i in range(n)]


def kde_model(n, form, bandwidth=0.25):
    """start -> one kernel-density state of n points 10 apart -> end."""
    m = Model("kde%d" % n)
    k = State(GaussianKernelDensity([10.0 * i for i in range(n)], bandwidth=bandwidth, weights=weights(n, form)), "k")
    m.add_transition(m.start, k, 1.0)
    m.add_transition(k, m.end, 1.0)
    m.bake()
    return m


def mixture_model(w, name="mix"):
    """start -> one mixture state of len(w) uniform components (target(i)) of weights w -> end."""
    m = Model(name)
    s = State(MixtureDistribution([target(i) for i in range(len(w))], w), "m")
    m.add_transition(m.start, s, 1.0)
    m.add_transition(s, m.end, 1.0)
    m.bake()
    return m


def crafted(n, i, v):
    """A row of n entries that ascends strictly through cdf[i] = v (0 < v < 1, i < n - 1) and closes in 1.0."""
    row = [v / 2.0 ** (i - j) for j in range(i)] + [v] + [v + (1.0 - v) * (j - i) / (n - i) for j in range(i + 1, n - 1)] + [1.0]
    assert len(row) == n and all(a < b for a, b in zip(row, row[1:])) and row[0] > 0
    return row


def neighbours(u):
    """(value, whether a row entry of that value is above u): u itself, the next double up, the next double down."""
    return ((u, False), (np.nextafter(u, 1.0), True), (np.nextafter(u, 0.0), False))


# ---- stops: a silent chain behind every emission -----------------------------------------------------------------------
CHAIN_LEVELS = 40


def chained():
    """Finite: start -> e; e -> c00 -> ... -> c39, forty silent levels; c39 -> e (0.8) | end (0.2)."""
    m = Model("chained")
    e = State(NormalDistribution(3.0, 2.0), "e")
    chain = [State(None, "c%02d" % i) for i in range(CHAIN_LEVELS)]
    m.add_transition(m.start, e, 1.0)
    for a, b in zip([e] + chain, chain):
        m.add_transition(a, b, 1.0)
    m.add_transition(chain[-1], e, 0.8)
    m.add_transition(chain[-1], m.end, 0.2)
    m.bake()
    return m


# ---- chosen draws ------------------------------------------------------------------------------------------------------
# Sequences whose block j has a uniform within 2^-12 of a place where the draw formulas are touchy: u0 at 0 (log(1 - u0)
# leaves 0) and at 1 (its largest argument), u1 at 1/4 and 3/4 (the cosine crosses zero).  Found once by search_chosen()
# -- for each j and place the first Q >= 0 under CHOSEN_SEED -- and kept as constants; the host test asserts what they are.
CHOSEN_SEED = 20261020
NEAR = 2.0 ** -12
PLACES = (("u0", 0.0), ("u0", 1.0), ("u1", 0.25), ("u1", 0.75))


def near(u0, u1, place):
    which, at = place
    return abs((u0 if which == "u0" else u1) - at) <= NEAR


def search_chosen(blocks=(1, 2, 3), limit=200000):
    found = {}
    for j in blocks:
        for place in PLACES:
            found[(j,) + place] = next(Q for Q in range(limit) if near(*SO.block(CHOSEN_SEED, Q, j), place))
    return found


CHOSEN = {(1, "u0", 0.0): 2759, (1, "u0", 1.0): 5329, (1, "u1", 0.25): 2884, (1, "u1", 0.75): 169,      # (block j, which
          (2, "u0", 0.0): 984, (2, "u0", 1.0): 6606, (2, "u1", 0.25): 3362, (2, "u1", 0.75): 1634,       # uniform, place) -> Q:
          (3, "u0", 0.0): 2093, (3, "u0", 1.0): 5999, (3, "u1", 0.25): 3821, (3, "u1", 0.75): 11585}     # sample with first = Q


def one_state(distribution, name):
    """start -> s -> end: the first emission draws from block 1 (a kernel-density state: the point from 1, the value from
    2; a vector state of D = 3: its components from 1, 2, 3)."""
    m = Model(name)
    s = State(distribution, "s")
    m.add_transition(m.start, s, 1.0)
    m.add_transition(s, m.end, 1.0)
    m.bake()
    return m


# name -> (builder, the blocks of the first emission whose (u0, u1) enter a libm function)
DRAW_MODELS = {
    "normal": (lambda: one_state(NormalDistribution(-7.5, 10.0), "normal"), (1,)),
    "lognormal": (lambda: one_state(LogNormalDistribution(0.5, 10.0), "lognormal"), (1,)),
    "exponential": (lambda: one_state(ExponentialDistribution(0.03), "exponential"), (1,)),
    "kde": (lambda: one_state(GaussianKernelDensity([-40.0, 1.5, 300.0], bandwidth=10.0, weights=[2, 1, 1]), "kde"), (2,)),
    "vector3": (lambda: one_state(MultivariateDistribution([LogNormalDistribution(-2.0, 10.0), NormalDistribution(1e3, 10.0),
                                                            ExponentialDistribution(8.0)]), "vector3"), (1, 2, 3))}


def draw_mp(d, a, b, u0, u1):
    """One draw by the project's definition (include/poreseg.h ps_hmm_sample) at 50 digits: a, b, u0, u1 and the constant
    6.283185307179586 enter as the doubles they are.  Returns an mpf."""
    import mpmath
    with mpmath.workdps(50):
        a, b, u0, u1 = [mpmath.mpf(float(v)) for v in (a, b, u0, u1)]
        if isinstance(d, UniformDistribution):
            return a + u0 * b
        if isinstance(d, ExponentialDistribution):
            return -mpmath.log(1 - u0) / b
        v = a + b * mpmath.sqrt(-2 * mpmath.log(1 - u0)) * mpmath.cos(mpmath.mpf(SO.TWO_PI) * u1)
        return mpmath.exp(v) if isinstance(d, LogNormalDistribution) else +v


def error_mp(got, ref):
    """|got - ref| / max(1, |ref|) as a float, the subtraction at 50 digits."""
    import mpmath
    with mpmath.workdps(50):
        return float(abs(mpmath.mpf(float(got)) - ref) / max(mpmath.mpf(1), abs(ref)))


def first_emission_mp(m, T, seed, Q):
    """The first emission of walk Q of a one_state model, by draw_mp: a list of n_dim mpf."""
    k = [s.name for s in m.states].index("s")
    d = m.states[k].distribution
    if isinstance(d, GaussianKernelDensity):
        i = SO.pick(T["kde_cdf"], int(m.flat["kde_ptr"][k]), int(m.flat["kde_ptr"][k + 1]), SO.block(seed, Q, 1)[0])
        return [draw_mp(NormalDistribution(0, 1), float(m.flat["kde_pt"][i]), T["emit_param"][2 * k + 1], *SO.block(seed, Q, 2))]
    comps = SO.parts(d)
    return [draw_mp(c, T["emit_param"][2 * (k * len(comps) + i)], T["emit_param"][2 * (k * len(comps) + i) + 1],
                    *SO.block(seed, Q, 1 + i)) for i, c in enumerate(comps)]


# ---- walks of any model, in one shape ----------------------------------------------------------------------------------
def oracle_tables(m):
    """The oracle's tables of any model: mixture_oracle's for a scalar model (they add the mixture tables to
    sample_oracle's), sample_oracle's for a vector model."""
    return SO.tables(m) if m._vector else MX.tables(m)


def oracle_walks(m, T, n, seed, first=0, length=0, max_length=1000000):
    """n walks as sample_oracle.Walk tuples with obs as rows of n_dim floats and exact per row and component."""
    if "mix_cdf" not in T:
        return [SO.walk(m, T, seed, first + q, length, max_length) for q in range(n)]
    out = []
    for q in range(n):
        w = MX.walk(m, T, seed, first + q, length, max_length)
        out.append(SO.Walk([[v] for v in w.obs], w.path, w.flag, [[e] for e in w.exact]))
    return out


def mix_model():
    """The mixture suite's finite model with silent levels and a kernel-density state beside its mixtures."""
    return MX.silent_model(True)[0]
