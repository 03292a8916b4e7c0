"""Plain-Python restatement of HMM sampling (pypore_amd.hmm.Model.sample_batch, ps_hmm_sample), written from the
definition of the random stream and of the walk, not from the kernel: Philox4x32-10 on Python ints, the two uniforms of a
block, the sampling tables rebuilt from Distribution.parameters and Model.flat, and the walk itself on Python floats.

Stream: key (seed & 0xffffffff, seed >> 32); sequence Q = first + q owns the blocks j = 0, 1, 2, ... at counter
(j & 0xffffffff, j >> 32, Q & 0xffffffff, Q >> 32); a block r0..r3 gives u0 = ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53 and u1 the
same from r2, r3.  Blocks are taken in walk order: one per transition (the first out-edge e with u0 < cdf[e]), one per
component of an emission in ascending d, two for a kernel-density state (the point, then the normal)."""
import collections
import math

import numpy as np

from pypore_amd import hmm as H

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TWO_PI = 6.283185307179586


def philox(counter, key):
    """Philox4x32-10: four 32-bit counter words and two key words -> four 32-bit words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(r):
    """(u0, u1) of a block: 53 bits each, in [0, 1)."""
    return (((r[0] >> 5) * (1 << 26) + (r[1] >> 6)) * 2.0 ** -53, ((r[2] >> 5) * (1 << 26) + (r[3] >> 6)) * 2.0 ** -53)


def block(seed, Q, j):
    seed &= 0xFFFFFFFFFFFFFFFF
    return uniforms(philox((j & MASK, j >> 32, Q & MASK, Q >> 32), (seed & MASK, seed >> 32)))


def running(p, ptr):
    """Per CSR row the running sum of p, added one by one, exactly 1.0 from the row's last entry of positive probability on
    (a row without one: its last entry)."""
    out = [0.0] * len(p)
    for k in range(len(ptr) - 1):
        lo, hi = int(ptr[k]), int(ptr[k + 1])
        run = 0.0
        for e in range(lo, hi):
            run = run + float(p[e])
            out[e] = run
        positive = [e for e in range(lo, hi) if p[e] > 0]
        for e in range(positive[-1] if positive else max(hi - 1, lo), hi):
            out[e] = 1.0
    return out


def parts(distribution):
    """The univariate components of an emitting state's distribution."""
    return list(distribution.parameters[0]) if isinstance(distribution, H.MultivariateDistribution) else [distribution]


def emit_pair(d):
    a = d.parameters
    if isinstance(d, H.NormalDistribution) or isinstance(d, H.LogNormalDistribution):
        return float(a[0]), float(a[1])
    if isinstance(d, H.UniformDistribution):
        return float(a[0]), float(a[1]) - float(a[0])
    if isinstance(d, H.ExponentialDistribution):
        return 0.0, float(a[0])
    assert isinstance(d, H.GaussianKernelDensity), d
    return 0.0, float(a[1])


def tables(model):
    """dict(out_cdf, emit_param, kde_cdf) as lists of floats, from model.flat and the states' distributions."""
    f = model.flat
    emit = []
    for s in model.states[:f["n_emit"]]:
        for d in parts(s.distribution):
            emit.extend(emit_pair(d))
    return dict(out_cdf=running(np.exp(f["out_lp"]), f["out_ptr"]), emit_param=emit,
                kde_cdf=running(np.exp(f["kde_lw"]), f["kde_ptr"]))


def pick(cdf, lo, hi, u):
    for i in range(lo, hi):
        if u < cdf[i]:
            return i
    raise AssertionError("a cdf row must end in 1.0")


def normal(u0, u1):
    return math.sqrt(-2.0 * math.log(1.0 - u0)) * math.cos(TWO_PI * u1)


def draw(d, a, b, u0, u1):
    if isinstance(d, H.UniformDistribution):
        return a + u0 * b
    if isinstance(d, H.ExponentialDistribution):
        return -math.log(1.0 - u0) / b
    v = a + b * normal(u0, u1)
    return math.exp(v) if isinstance(d, H.LogNormalDistribution) else v


Walk = collections.namedtuple("Walk", "obs path flag exact")


def walk(model, T, seed, Q, length=0, max_length=1000000):
    """One walk: Walk(obs: a list of rows of n_dim floats, path: the state indices from start on, flag 0 / 1 / 2, exact: per
    row and component whether the value passed through no libm function -- a uniform draw)."""
    f = model.flat
    NE, end = f["n_emit"], f["end"]
    ptr, dst, kptr, kpt = f["out_ptr"], f["out_dst"], f["kde_ptr"], f["kde_pt"]
    k, j, flag = f["start"], 0, 1
    obs, exact, path = [], [], [k]
    bound = (max_length + 1) * (f["n_levels"] + 1) + 1
    for _ in range(bound):
        if k == end or (length > 0 and len(obs) >= length):
            flag = 0
            break
        if len(obs) >= max_length:
            break
        e0, e1 = int(ptr[k]), int(ptr[k + 1])
        if e0 == e1:
            flag = 2
            break
        u0, _ = block(seed, Q, j)
        j += 1
        k = int(dst[pick(T["out_cdf"], e0, e1, u0)])
        path.append(k)
        if k < NE:
            row, ex = [], []
            comps = parts(model.states[k].distribution)
            for c, d in enumerate(comps):
                i = k * len(comps) + c
                a, b = T["emit_param"][2 * i], T["emit_param"][2 * i + 1]
                u0, u1 = block(seed, Q, j)
                j += 1
                if isinstance(d, H.GaussianKernelDensity):
                    p = float(kpt[pick(T["kde_cdf"], int(kptr[k]), int(kptr[k + 1]), u0)])
                    u0, u1 = block(seed, Q, j)
                    j += 1
                    row.append(p + b * normal(u0, u1))
                else:
                    row.append(draw(d, a, b, u0, u1))
                ex.append(isinstance(d, H.UniformDistribution))
            obs.append(row)
            exact.append(ex)
    return Walk(obs, path, flag, exact)


def batch(model, n, seed, first=0, length=0, max_length=1000000):
    T = tables(model)
    return [walk(model, T, seed, first + q, length, max_length) for q in range(n)]
