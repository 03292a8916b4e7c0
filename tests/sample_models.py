"""Small models that tests/test_hmm_sample_host.py and tests/test_hmm_sample_gpu.py sample from.  Every call builds a fresh,
equal model (fixed numbers only); every std, sigma and bandwidth is <= 10."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modular_models as MM  # noqa: E402

from pypore_amd.hmm import (ExponentialDistribution, GaussianKernelDensity, LogNormalDistribution, Model,  # noqa: E402
                            MultivariateDistribution, NormalDistribution, State, UniformDistribution)

CHAIN = (("a", 0.0, 1.0), ("b", 10.0, 2.0), ("c", 20.0, 1.5), ("d", 30.0, 0.5))      # name, mean, std


def chain4():
    """Finite: start -> a -> b -> c -> d -> end, every state with a self-loop, b with a way back to a and a way out."""
    m = Model("chain4")
    a, b, c, d = [State(NormalDistribution(mu, sd), nm) for nm, mu, sd in CHAIN]
    m.add_transition(m.start, a, 1.0)
    for s, t, p in ((a, a, 0.5), (a, b, 0.5), (b, b, 0.3), (b, c, 0.5), (b, a, 0.1), (b, m.end, 0.1), (c, c, 0.4), (c, d, 0.6),
                    (d, d, 0.6), (d, m.end, 0.4)):
        m.add_transition(s, t, p)
    m.bake()
    return m


def silent():
    """Finite: a silent diamond (s1 -> u | v -> j), then a silent chain of three levels (j -> c1 -> c2 -> c3) into a normal
    state e and a uniform state f, which loop, go back through the diamond, or end."""
    m = Model("silent")
    s1, u, v, j, c1, c2, c3 = [State(None, nm) for nm in ("s1", "u", "v", "j", "c1", "c2", "c3")]
    e, f = State(NormalDistribution(5.0, 2.0), "e"), State(UniformDistribution(-3.0, 4.5), "f")
    for s, t, p in ((m.start, s1, 1.0), (s1, u, 0.3), (s1, v, 0.7), (u, j, 1.0), (v, j, 1.0), (j, c1, 1.0), (c1, c2, 1.0),
                    (c2, c3, 1.0), (c3, e, 0.45), (c3, f, 0.55), (e, e, 0.25), (e, s1, 0.35), (e, m.end, 0.4), (f, f, 0.2),
                    (f, s1, 0.3), (f, e, 0.1), (f, m.end, 0.4)):
        m.add_transition(s, t, p)
    m.bake()
    return m


def ring():
    """Infinite: three normal states in a ring, two of them with a self-loop; nothing enters `end`."""
    m = Model("ring")
    r = [State(NormalDistribution(10.0 * i, 1.0 + i), "r%d" % i) for i in range(3)]
    for s, t, p in ((m.start, r[0], 0.6), (m.start, r[2], 0.4), (r[0], r[0], 0.2), (r[0], r[1], 0.8), (r[1], r[1], 0.1),
                    (r[1], r[2], 0.9), (r[2], r[0], 1.0)):
        m.add_transition(s, t, p)
    m.bake()
    return m


def phi29(merge=None):
    return MM.linear("phi29", 5, merge=merge)


def kde():
    """Finite: two kernel-density states, one point and seven (unequal weights, one of them 0), beside a normal and a uniform
    state."""
    m = Model("kde")
    one = State(GaussianKernelDensity([12.0], bandwidth=0.7), "k1")
    seven = State(GaussianKernelDensity([1.0, 2.5, 3.0, 7.0, 8.5, 9.0, 15.0], bandwidth=0.4, weights=[5, 1, 0, 2, 0.5, 3, 0.25]), "k7")
    n, un = State(NormalDistribution(-4.0, 1.0), "n"), State(UniformDistribution(20.0, 30.0), "un")
    for s, t, p in ((m.start, one, 0.5), (m.start, seven, 0.5), (one, seven, 0.6), (one, one, 0.2), (one, m.end, 0.2),
                    (seven, seven, 0.5), (seven, n, 0.2), (seven, one, 0.1), (seven, m.end, 0.2), (n, seven, 0.4), (n, un, 0.2), (n, m.end, 0.4),
                    (un, un, 0.3), (un, m.end, 0.7)):
        m.add_transition(s, t, p)
    m.bake()
    return m


def vector3():
    """Finite, D = 3: three states whose components cover normal, uniform, log-normal and exponential in every slot order,
    all weights != 1."""
    m = Model("vector3")
    w = [0.5, 2.0, 1.5]
    x = State(MultivariateDistribution([NormalDistribution(40.0, 3.0), UniformDistribution(0.5, 2.5), LogNormalDistribution(-1.0, 0.5)], w), "x")
    y = State(MultivariateDistribution([ExponentialDistribution(0.25), NormalDistribution(1.0, 0.2), UniformDistribution(-1.0, 1.0)], w), "y")
    z = State(MultivariateDistribution([LogNormalDistribution(3.0, 0.25), ExponentialDistribution(40.0), NormalDistribution(0.0, 10.0)], w), "z")
    for s, t, p in ((m.start, x, 0.7), (m.start, y, 0.3), (x, x, 0.4), (x, y, 0.4), (x, m.end, 0.2), (y, z, 0.7), (y, y, 0.2),
                    (y, m.end, 0.1), (z, x, 0.3), (z, z, 0.3), (z, m.end, 0.4)):
        m.add_transition(s, t, p)
    m.bake()
    return m


def loop():
    """Finite: one emitting state that loops with probability 0.999."""
    m = Model("loop")
    a = State(NormalDistribution(0.0, 1.0), "a")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, a, 0.999)
    m.add_transition(a, m.end, 0.001)
    m.bake()
    return m


def dead_end():
    """Finite: a loops, ends, or enters b, an emitting state without out-edges."""
    m = Model("dead")
    a, b = State(NormalDistribution(0.0, 1.0), "a"), State(UniformDistribution(1.0, 2.0), "b")
    for s, t, p in ((m.start, a, 1.0), (a, a, 0.4), (a, b, 0.3), (a, m.end, 0.3)):
        m.add_transition(s, t, p)
    m.bake()
    return m


# name -> (builder, the `length` the exact-walk test samples with: 0 runs to `end`)
MODELS = {"chain4": (chain4, 0), "silent": (silent, 0), "ring": (ring, 12), "phi29": (phi29, 0),
          "phi29_all": (lambda: phi29("all"), 0), "kde": (kde, 0), "vector3": (vector3, 0)}
