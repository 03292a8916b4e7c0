"""Test-side oracle for posterior decoding (pypore_amd.hmm forward_backward / maximum_a_posteriori): plain numpy float64
on hmm_oracle's forward, backward and log probability, and a brute-force version that enumerates every complete state
path of a tiny model and weights its states and edges by the path's posterior.

Both take a `Compiled` view (hmm_oracle.Compiled, or profile_oracle.Compiled for kernel-density states: the dynamic
programmes read the emissions through it) and the edges [(from, to, p)] the counts are aligned with (default: the view's
model's `edges`, all of probability > 0 for a freshly baked model).

Definitions (pypore_amd/hmm.py module docstring), for a sequence of length n with f, b, logp:
  post[t][k]  = (f[t+1][k] + b[t+1][k]) - logp   for emitting k, -inf where either entry is -inf      (n x n_emit)
  state[t]    = the first index of the largest entry of post[t] (lowest index on a tie), -1 for an impossible sequence
  map_logp    = the sum over ascending t of post[t][state[t]], added one by one (0.0 for n = 0)
  counts[e]   = sum_t exp(f[t][k] + lp + e_l(x_t) + b[t+1][l] - logp) over t < n (l emitting) or
                sum_t exp(f[t][k] + lp + b[t][l] - logp) over t <= n (l silent), for edge e = k -> l
An impossible sequence: post all -inf, state all -1, map_logp -inf, counts 0."""
import collections
import math

import numpy as np

import hmm_oracle as O

NEG = -np.inf

Posterior = collections.namedtuple("Posterior", "logp post state map_logp counts gap")


def ordered_sum(values):
    """The sum in the order given, one addition at a time (np.sum adds pairwise)."""
    s = 0.0
    for v in values:
        s += float(v)
    return s


def top_two_gap(post):
    """Per row: the largest entry minus the second largest (inf with one state or a second of -inf; 0 on an exact tie)."""
    post = np.asarray(post, np.float64)
    if post.shape[1] < 2:
        return np.full(post.shape[0], np.inf)
    top = np.sort(post, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gap = top[:, 1] - top[:, 0]
    return np.where(np.isneginf(top[:, 0]), np.inf, gap)


def posterior(c, seq, edges=None):
    """Posterior(logp, post [n, NE], state int [n], map_logp, counts [len(edges)], gap [n]: top_two_gap of post)."""
    edges = c.model.edges if edges is None else edges
    seq = np.asarray(seq, np.float64)
    n, NE = seq.size, c.NE
    counts = np.zeros(len(edges))
    F = O.forward(c, seq)
    logp = O.final(c, F[n], False)[0]                                    # (= O.log_probability(c, seq), the matrix kept)
    if not logp > NEG:
        return Posterior(NEG, np.full((n, NE), NEG), np.full(n, -1, np.int64), NEG, counts, np.full(n, np.inf))
    B = O.backward(c, seq)
    both = np.isfinite(F[1:, :NE]) & np.isfinite(B[1:, :NE])
    with np.errstate(invalid="ignore"):
        post = np.where(both, (F[1:, :NE] + B[1:, :NE]) - logp, NEG)
    state = post.argmax(axis=1) if NE else np.zeros(0, np.int64)        # (argmax: the first of equal maxima)
    map_logp = ordered_sum(post[t, state[t]] for t in range(n))
    em = np.array([c.emissions(x) for x in seq]).reshape(n, NE)          # em[t, l] = e_l(x_t)
    for e, (k, l, p) in enumerate(edges):
        if not p > 0:
            continue
        lp = math.log(p)
        v = F[:n, k] + lp + em[:, l] + B[1:, l] - logp if l < NE else F[:, k] + lp + B[:, l] - logp
        counts[e] = np.exp(v[v > NEG]).sum() if v.size else 0.0
    return Posterior(logp, post, state.astype(np.int64), map_logp, counts, top_two_gap(post))


def posterior_brute_force(c, seq, edges=None):
    """(logp, post [n, NE], counts) by enumerating every complete path: a path of posterior w adds w to the posterior of
    the state that emitted observation t, for every t, and to the count of every edge it takes."""
    edges = c.model.edges if edges is None else edges
    seq = np.asarray(seq, np.float64)
    n, NE = seq.size, c.NE
    index = {(i, j): e for e, (i, j, _) in enumerate(edges)}
    paths = []

    def walk(k, t, lp, used, emitted):
        if t == n and (not c.finite or k == c.end):
            paths.append((lp, used, emitted))
        for l, w in c.outs[k]:
            if l < NE:
                if t < n:
                    e = c.emissions(seq[t])[l]
                    if e > NEG:
                        walk(l, t + 1, lp + w + e, used + [index[(k, l)]], emitted + [(t, l)])
            else:
                walk(l, t, lp + w, used + [index[(k, l)]], emitted)

    walk(c.start, 0, 0.0, [], [])
    counts = np.zeros(len(edges))
    if not paths:
        return NEG, np.full((n, NE), NEG), counts
    logp = O.lse_rows(np.array([p[0] for p in paths])[None, :])[0]
    prob = np.zeros((n, NE))
    for lp, used, emitted in paths:
        w = math.exp(lp - logp)
        for e in used:
            counts[e] += w
        for t, k in emitted:
            prob[t, k] += w
    with np.errstate(divide="ignore"):
        return logp, np.log(prob), counts
