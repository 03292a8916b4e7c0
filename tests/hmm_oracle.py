"""Test-side oracle for pypore_amd.hmm: a plain numpy log-space dynamic programme with the device's tie rule (in-edges
in ascending source index, a strictly greater score wins, so the lowest source wins a tie), and a brute-force enumerator
over every state path for tiny models.  Reads only a baked model's `states`, `edges`, `start`, `end` and `finite`, and
computes the emission densities from the distributions' parameters itself.  Beside it `viterbi_exact`, which restates the
device's Viterbi operation by operation on the uploaded arrays (model.flat) and so gives the device's bits: the yardstick
of tests/test_viterbi_exact_gpu.py, itself checked against the numpy programme in tests/test_viterbi_exact_host.py."""
import math

import numpy as np

from pypore_amd.hmm import GaussianKernelDensity, Model, NormalDistribution, State, UniformDistribution

NEG = -np.inf


def emission(state, x):
    """Log density of observation x in an emitting state (module formulas, written out again here)."""
    p = state.distribution.parameters
    if type(state.distribution).__name__ == "NormalDistribution":
        mean, std = p
        return -math.log(std * math.sqrt(2 * math.pi)) - (x - mean) ** 2 / (2 * std ** 2)
    low, high = p
    return -math.log(high - low) if low <= x <= high else NEG


class Compiled(object):
    """The DP's view of a baked model: padded in- and out-edge tables per group of states."""

    def __init__(self, model):
        self.model = model
        self.states = model.states
        self.S = len(model.states)
        self.NE = sum(1 for s in model.states if not s.is_silent())
        self.start = self.states.index(model.start)
        self.end = self.states.index(model.end)
        self.finite = bool(model.finite)
        ins = [[] for _ in range(self.S)]
        outs = [[] for _ in range(self.S)]
        for i, j, p in model.edges:
            ins[j].append((i, math.log(p)))
            outs[i].append((j, math.log(p)))
        self.ins = [sorted(e) for e in ins]
        self.outs = [sorted(e) for e in outs]
        # silent levels: longest chain of silent predecessors
        level = {}
        for k in range(self.NE, self.S):
            level[k] = 1 + max([level[i] for i, _ in self.ins[k] if i >= self.NE] or [-1])
        n_levels = max(level.values()) + 1 if level else 0
        self.levels = [[k for k in range(self.NE, self.S) if level[k] == L] for L in range(n_levels)]
        self.emit_group = self._group(list(range(self.NE)), self.ins)
        self.in_levels = [self._group(g, self.ins) for g in self.levels]
        self.out_levels = [self._group(g, self.outs) for g in self.levels]
        self.out_emit = self._group(list(range(self.NE)), self.outs)

    @staticmethod
    def _group(members, table):
        P = max([len(table[k]) for k in members] or [0]) or 1
        idx = np.zeros((len(members), P), np.int64)
        lp = np.full((len(members), P), NEG)
        for r, k in enumerate(members):
            for c, (o, w) in enumerate(table[k]):
                idx[r, c], lp[r, c] = o, w
        return np.array(members, np.int64), idx, lp

    def emissions(self, x):
        return np.array([emission(self.states[k], x) for k in range(self.NE)])


def lse_rows(v):
    """Log-sum-exp of every row: max + log1p(sum of exp(v - max) over the other terms); -inf rows stay -inf."""
    v = np.atleast_2d(v)
    m = v.max(axis=1)
    out = np.full(v.shape[0], NEG)
    ok = m > NEG
    if ok.any():
        w = v[ok]
        mm = m[ok]
        e = np.exp(w - mm[:, None])
        e[np.arange(w.shape[0]), w.argmax(axis=1)] = 0.0
        out[ok] = mm + np.log1p(e.sum(axis=1))
    return out


def _forward_like(c, seq, viterbi):
    seq = np.asarray(seq, dtype=np.float64)
    n, S = seq.size, c.S
    F = np.full((n + 1, S), NEG)
    bp = np.zeros((n + 1, S), np.int64)

    def combine(row, group, t, init_start):
        members, idx, lp = group
        if members.size == 0:
            return
        v = row[idx] + lp
        init = np.where((members == c.start) & init_start, 0.0, NEG)
        v = np.concatenate([init[:, None], v], axis=1)
        if viterbi:
            a = v.argmax(axis=1)
            row[members] = v[np.arange(v.shape[0]), a]
            bp[t, members] = np.maximum(a - 1, 0)
        else:
            row[members] = lse_rows(v)

    for t in range(n + 1):
        row = F[t]
        if t > 0:
            members, idx, lp = c.emit_group
            if members.size:
                v = F[t - 1][idx] + lp
                if viterbi:
                    a = v.argmax(axis=1)
                    best = v[np.arange(v.shape[0]), a]
                    bp[t, members] = a
                else:
                    best = lse_rows(v)
                with np.errstate(invalid="ignore"):
                    row[members] = np.where(best > NEG, best + c.emissions(seq[t - 1]), NEG)
        for g in c.in_levels:
            combine(row, g, t, t == 0)
    return F, bp


def forward(c, seq):
    return _forward_like(c, seq, False)[0]


def final(c, row, viterbi):
    if c.finite:
        return row[c.end], c.end
    if viterbi:
        k = int(np.argmax(row))
        return row[k], k
    return lse_rows(row[None, :])[0], None


def log_probability(c, seq):
    return final(c, forward(c, seq)[-1], False)[0]


def backward(c, seq):
    seq = np.asarray(seq, dtype=np.float64)
    n, S, NE = seq.size, c.S, c.NE
    B = np.full((n + 1, S), NEG)
    for t in range(n, -1, -1):
        comb = np.full(S, NEG)                      # [:NE] row t+1 plus emission of observation t, [NE:] row t
        if t < n:
            comb[:NE] = np.where(B[t + 1, :NE] > NEG, B[t + 1, :NE] + c.emissions(seq[t]), NEG)
        init = np.full(S, NEG)
        if t == n:
            if c.finite:
                init[c.end] = 0.0
            else:
                init[:] = 0.0
        for members, idx, lp in reversed(c.out_levels):
            v = np.concatenate([init[members][:, None], comb[idx] + lp], axis=1)
            comb[members] = lse_rows(v)
        B[t, NE:] = comb[NE:]
        members, idx, lp = c.out_emit
        if members.size:
            v = np.concatenate([init[members][:, None], comb[idx] + lp], axis=1)
            B[t, members] = lse_rows(v)
    return B


def viterbi_ties(c, seq, flip_near=False):
    """(logp, path as state indices or None, gap, ties, tied): the decisions on the winning path, told apart by kind.
    A decision is the choice among one state's in-edge candidates (or, for an infinite model, among the entries of the
    last row).  gap = the smallest NON-ZERO relative gap between a decision's winner and its best candidate that scores
    strictly less (inf when there is none); ties = the number of decisions where a second candidate equals the winner
    exactly; tied = those decisions as a sorted list of (t, state), the last row's as (n + 1, -1).
    flip_near: at every in-edge decision whose best lesser candidate lies within 1e-9 relative of the winner -- a near tie,
    which another arithmetic may decide the other way -- the traceback follows that candidate instead: the other path."""
    seq = np.asarray(seq, dtype=np.float64)
    F, bp = _forward_like(c, seq, True)
    n = seq.size
    logp, k = final(c, F[n], True)
    if not logp > NEG:
        return NEG, None, np.inf, 0, []
    gap, tied = np.inf, []

    def note(cands, where):
        """the ordinal of the best lesser candidate when it is a near tie, else None"""
        nonlocal gap
        best = max(cands)
        if sum(1 for v in cands if v == best) > 1:
            tied.append(where)
        below = [v for v in cands if NEG < v < best]
        if below:
            g = (best - max(below)) / max(1.0, abs(best))
            gap = min(gap, g)
            if g <= 1e-9:
                return cands.index(max(below))
        return None

    if not c.finite:
        note([float(v) for v in F[n]], (n + 1, -1))
    path, t = [k], n
    while not (t == 0 and k == c.start):
        src_t = t - 1 if k < c.NE else t
        near = note([float(F[src_t][i] + w) for i, w in c.ins[k]], (t, k))
        j = c.ins[k][near if (flip_near and near is not None) else bp[t, k]][0]
        t, k = src_t, j
        path.append(k)
    return logp, path[::-1], gap, len(tied), sorted(tied)


def viterbi(c, seq):
    """(logp, path as state indices or None, margin): margin = the smallest relative gap between the winner and the
    runner-up over the decisions on the winning path (inf when there was no alternative; 0.0 at an exact tie)."""
    logp, path, gap, ties, _ = viterbi_ties(c, seq)
    return logp, path, (0.0 if ties else gap)


def viterbi_exact(model, seq):
    """The device's Viterbi (csrc/seg_hmm.hpp hmm_fwd_kernel<HMM_VITERBI>, hmm_trace_kernel) restated operation by
    operation in plain Python floats, which are IEEE fp64 and never fuse a multiply-add, on the uploaded numbers themselves
    (model.flat: param, kind, in_ptr / in_src / in_lp, level_ptr, start, end, finite, and the kde_* tables).  Every
    operation is an fp64 addition, subtraction, multiplication or comparison in the device's order, so the results are the
    device's bit for bit:
      * an emitting state at step t >= 1 scans its in-edges over row t-1 in ordinal order from -inf, replacing on a
        strictly greater score, then takes  best + emission  where best > -inf, else -inf;
      * the silent states of row t go level by level over row t; `start` at t = 0 begins from 0.0;
      * emissions: normal  c - (d*d)*b;  uniform  c  inside [low, high], else -inf;  a kernel density of exactly one point
        c + (lw - (d*d)*b)  (HmmLse of one term returns  m + log1p(0) = m).  A kernel density of any other number of
        points raises ValueError: it goes through exp and log1p, which are not reproducible bit for bit;
      * the result is row[n][end] (finite) or the largest entry of row n, the lowest index on a tie (infinite).
    Returns (logp, path as state indices or None, the (n+1) x S score matrix, ties, other):  ties = the number of decisions
    on the winning path (final row included) where a second candidate equalled the winner;  other = the path under the
    opposite rule -- the LAST candidate wins a tie, the HIGHEST state wins in the final row -- which has the same scores."""
    f = model.flat
    S, NE, start, end = f["n_states"], f["n_emit"], f["start"], f["end"]
    param, kind = f["param"].tolist(), f["kind"].tolist()
    in_ptr, in_src, in_lp = f["in_ptr"].tolist(), f["in_src"].tolist(), f["in_lp"].tolist()
    level_ptr = f["level_ptr"].tolist()
    kde_ptr, kde_pt, kde_lw = f["kde_ptr"].tolist(), f["kde_pt"].tolist(), f["kde_lw"].tolist()
    for k in range(NE):
        if kind[k] == 3 and kde_ptr[k + 1] - kde_ptr[k] != 1:
            raise ValueError("state %d is a kernel density of %d points: only one point is exact" % (k, kde_ptr[k + 1] - kde_ptr[k]))
    xs = [float(v) for v in np.asarray(seq, dtype=np.float64).reshape(-1)]
    n = len(xs)
    ninf = float("-inf")

    def emit(k, x):
        a, b, c = param[3 * k], param[3 * k + 1], param[3 * k + 2]
        if kind[k] == 1:
            d = x - a
            return c - (d * d) * b
        if kind[k] == 2:
            return c if (x >= a and x <= b) else ninf
        d = x - kde_pt[kde_ptr[k]]
        return c + (kde_lw[kde_ptr[k]] - (d * d) * b)

    def scan(row, k, best):
        """(best, ordinal of the first candidate that reached it, of the last, how many reached it)"""
        first = last = 0
        cnt = 1 if best > ninf else 0
        e0 = in_ptr[k]
        for o in range(in_ptr[k + 1] - e0):
            v = row[in_src[e0 + o]] + in_lp[e0 + o]
            if v > best:
                best, first, last, cnt = v, o, o, 1
            elif v == best and v > ninf:
                last, cnt = o, cnt + 1
        return best, first, last, cnt

    F, first, last, count = [], [], [], []
    for t in range(n + 1):
        row, bf, bl, bc = [ninf] * S, [0] * S, [0] * S, [0] * S
        if t > 0:
            prev, x = F[t - 1], xs[t - 1]
            for k in range(NE):
                best, bf[k], bl[k], bc[k] = scan(prev, k, ninf)
                row[k] = best + emit(k, x) if best > ninf else ninf
        for L in range(len(level_ptr) - 1):
            for k in range(level_ptr[L], level_ptr[L + 1]):
                row[k], bf[k], bl[k], bc[k] = scan(row, k, 0.0 if (t == 0 and k == start) else ninf)
        F.append(row)
        first.append(bf)
        last.append(bl)
        count.append(bc)

    mat = np.array(F, np.float64).reshape(n + 1, S)
    if f["finite"]:
        logp, k_lo, k_hi, final_ties = F[n][end], end, end, 0
    else:
        logp = max(F[n])
        at = [k for k in range(S) if F[n][k] == logp]
        k_lo, k_hi, final_ties = at[0], at[-1], int(len(at) > 1)
    if not logp > ninf:
        return ninf, None, mat, 0, None

    def trace(bp, k):
        t, path, ties = n, [k], 0
        while not (t == 0 and k == start):
            ties += count[t][k] > 1
            e = in_ptr[k] + bp[t][k]
            if k < NE:
                t -= 1
            k = in_src[e]
            path.append(k)
        return path[::-1], ties

    path, ties = trace(first, k_lo)
    return logp, path, mat, ties + final_ties, trace(last, k_hi)[0]


def path_score(c, seq, path):
    """The log probability of one state path (None if it is not a valid path of the model for seq)."""
    seq = np.asarray(seq, dtype=np.float64)
    if not path or path[0] != c.start:
        return None
    w = {(i, j): lp for j in range(c.S) for i, lp in c.ins[j]}
    total, t = 0.0, 0
    for a, b in zip(path[:-1], path[1:]):
        if (a, b) not in w:
            return None
        total += w[(a, b)]
        if b < c.NE:
            if t >= seq.size:
                return None
            total += emission(c.states[b], seq[t])
            t += 1
    if t != seq.size or (c.finite and path[-1] != c.end):
        return None
    return total


def brute_force(c, seq):
    """Every state path, enumerated: (forward matrix from the enumeration, log_probability, best score, best path)."""
    seq = np.asarray(seq, dtype=np.float64)
    n = seq.size
    terms = {}
    ends = []

    def walk(k, t, lp, path):
        terms.setdefault((t, k), []).append(lp)
        if t == n and (not c.finite or k == c.end):
            ends.append((lp, path))
        for l, w in c.outs[k]:
            if l < c.NE:
                if t < n:
                    e = emission(c.states[l], seq[t])
                    if e > NEG:
                        walk(l, t + 1, lp + w + e, path + [l])
            else:
                walk(l, t, lp + w, path + [l])

    walk(c.start, 0, 0.0, [c.start])
    F = np.full((n + 1, c.S), NEG)
    for (t, k), v in terms.items():
        F[t, k] = lse_rows(np.array(v)[None, :])[0]
    if not ends:
        return F, NEG, NEG, None
    scores = np.array([e[0] for e in ends])
    best = int(np.argmax(scores))
    return F, lse_rows(scores[None, :])[0], scores[best], ends[best][1]


def merge_loop(segments, states, second):
    """The reference's HMM-guided merge (DataTypes.py:292-330), restated on plain tuples: segments = [(start in seconds,
    n)], states = the Viterbi path as [(index, state)].  Returns [(start in samples, end in samples, hidden_state)]."""
    i, j, n, out = 0, 0, len(segments), []
    while i < n - 1:
        if states[i][1].name != states[i + 1][1].name or i == n - 2:
            ledge = segments[j]
            redge = segments[i] if i < n - 2 else segments[-1]
            s, e = int(ledge[0] * second), int(redge[0] * second + redge[1])
            out.append((s, e, states[j + 1][1].name))
            j = i
        i += 1
    return out


# ---- model generators (tests and tools/bench_hmm.py) ---------------------------------------------------------------
def random_tiny(rng, finite, silent_chain):
    """At most 4 states besides start and end, some silent (a chain), some uniform."""
    m = Model("tiny")
    n_emit = int(rng.integers(1, 4))
    states = []
    for i in range(n_emit):
        if rng.random() < 0.3:
            lo = float(rng.uniform(-1, 0.5))
            states.append(State(UniformDistribution(lo, lo + float(rng.uniform(0.5, 2))), "e%d" % i))
        else:
            states.append(State(NormalDistribution(float(rng.normal()), float(rng.uniform(0.3, 2))), "e%d" % i))
    silents = [State(None, "s%d" % i) for i in range(silent_chain and max(0, 4 - n_emit))]
    for a, b in zip(silents[:-1], silents[1:]):
        m.add_transition(a, b, float(rng.uniform(0.2, 1)))
    allst = states + silents
    m.add_states(allst)
    for s in [m.start] + allst:
        for t in allst:
            if rng.random() < 0.5 and not (s.is_silent() and t.is_silent() and s in silents and t in silents
                                           and silents.index(t) <= silents.index(s)):
                m.add_transition(s, t, float(rng.uniform(0.05, 1)))
        if finite and s is not m.start and rng.random() < 0.5:
            m.add_transition(s, m.end, float(rng.uniform(0.05, 1)))
    m.add_transition(m.start, states[0], 0.3)
    if finite:
        m.add_transition(states[-1], m.end, 0.3)
    m.bake()
    return m


def random_model(rng, max_states=300, max_chain=60, finite=True):
    """Up to max_states states: emitting ones (normal, some uniform), a silent chain of up to max_chain states and a
    few loose silent states, random edges (silent -> silent only forward in a fixed order: acyclic)."""
    chain = int(rng.integers(0, max_chain + 1))
    loose = int(rng.integers(0, 4))
    n_emit = int(rng.integers(1, max(2, max_states - 2 - chain - loose)))
    m = Model("rand")
    emit = []
    for i in range(n_emit):
        if rng.random() < 0.15:
            lo = float(rng.uniform(-3, 1))
            emit.append(State(UniformDistribution(lo, lo + float(rng.uniform(1, 4))), "e%04d" % i))
        else:
            emit.append(State(NormalDistribution(float(rng.normal(0, 2)), float(rng.uniform(0.3, 3))), "e%04d" % i))
    silent = [State(None, "c%03d" % i) for i in range(chain)] + [State(None, "l%d" % i) for i in range(loose)]
    rng.shuffle(silent)
    order = {id(s): i for i, s in enumerate(silent)}
    chain_states = sorted([s for s in silent if s.name[0] == "c"], key=lambda s: order[id(s)])
    for a, b in zip(chain_states[:-1], chain_states[1:]):
        m.add_transition(a, b, float(rng.uniform(0.3, 1)))
    allst = emit + silent
    m.add_states(allst)
    m.add_transition(m.start, emit[0], 1.0)
    if chain_states:
        m.add_transition(m.start, chain_states[0], 0.5)
        m.add_transition(chain_states[-1], emit[int(rng.integers(n_emit))], 0.5)
    for s in allst:
        for _ in range(int(rng.integers(1, 5))):
            t = allst[int(rng.integers(len(allst)))]
            if s.is_silent() and t.is_silent() and order[id(t)] <= order[id(s)]:
                continue
            m.add_transition(s, t, float(rng.uniform(0.01, 1)))
        if not s.is_silent() and rng.random() < 0.3:
            t = silent[int(rng.integers(len(silent)))] if silent else emit[0]
            m.add_transition(s, t, float(rng.uniform(0.01, 1)))
        if finite and rng.random() < 0.2:
            m.add_transition(s, m.end, float(rng.uniform(0.01, 1)))
    if finite:
        m.add_transition(emit[-1], m.end, 0.1)
    m.bake()
    return m


def line_model(S):
    """S states: S - 2 emitting ones on a left-to-right line with self-loops and skips, start entering every 64th."""
    rng = np.random.default_rng(S)
    m = Model("line")
    st = [State(NormalDistribution(float(rng.normal(0, 3)), float(rng.uniform(0.5, 2))), "s%04d" % i) for i in range(S - 2)]
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


def profile_model(n=54, seed=0, name="profile", kde=False):
    """A global profile HMM like the reference tutorial's: per position a match (normal), an insert (uniform over the
    current range) and a silent delete; 3n + 1 + 2 states (n = 54: 165).  kde: every match state is the one-point kernel
    density GaussianKernelDensity([mean], std) instead, the same density through the kernel-density code."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(20, 60, n)
    m = Model(name)
    insert = lambda i: State(UniformDistribution(0, 90), "I:%d" % i)           # noqa: E731
    match = (lambda mean, std: GaussianKernelDensity([mean], std)) if kde else NormalDistribution
    M = [State(match(float(means[i]), float(rng.uniform(0.8, 2.0))), "M:%d" % (i + 1)) for i in range(n)]
    I = [insert(i) for i in range(n + 1)]                                      # noqa: E741
    D = [State(None, "D:%d" % (i + 1)) for i in range(n)]
    m.add_transition(m.start, M[0], 0.90)
    m.add_transition(m.start, I[0], 0.05)
    m.add_transition(m.start, D[0], 0.05)
    m.add_transition(I[0], I[0], 0.50)
    m.add_transition(I[0], M[0], 0.45)
    m.add_transition(I[0], D[0], 0.05)
    for i in range(n):
        last = i == n - 1
        nxt_m = m.end if last else M[i + 1]
        m.add_transition(M[i], M[i], 0.30)
        m.add_transition(M[i], nxt_m, 0.60)
        m.add_transition(M[i], I[i + 1], 0.05)
        m.add_transition(I[i + 1], I[i + 1], 0.50)
        m.add_transition(I[i + 1], nxt_m, 0.45)
        m.add_transition(D[i], I[i + 1], 0.10)
        m.add_transition(D[i], nxt_m, 0.50)
        if not last:
            m.add_transition(M[i], D[i + 1], 0.05)
            m.add_transition(I[i + 1], D[i + 1], 0.05)
            m.add_transition(D[i], D[i + 1], 0.40)
    m.bake()
    return m, means


def hub_model(n_in, shared=None):
    """A hub state h with n_in in-edges: from the emitting states e0000 .. (self-loop of h last, since the emitting
    states sort by name); `end` has n_in in-edges too.  start -> every e, e -> h or end, h -> h, any e or end.  The e
    levels lie 3 apart at std 0.5, h's far below, so an observation names its state and the Viterbi path its in-edges.
    shared = (lo, hi): e<hi> takes e<lo>'s distribution object, so the two hold the same bits wherever both are entered
    and h's in-edges of ordinals lo and hi tie.  Returns (model, h, [e states])."""
    m = Model("hub")
    h = State(NormalDistribution(-50.0, 1.0), "h")
    es = [State(NormalDistribution(3.0 * i, 0.5), "e%04d" % i) for i in range(n_in - 1)]
    if shared is not None:
        es[shared[1]].distribution = es[shared[0]].distribution
    for e in es:
        m.add_transition(m.start, e, 1.0)
        m.add_transition(e, h, 0.8)
        m.add_transition(e, m.end, 0.2)
        m.add_transition(h, e, 0.4 / len(es))
    m.add_transition(h, h, 0.4)
    m.add_transition(h, m.end, 0.2)
    m.bake()
    return m, h, es


def chain_model(n_chain):
    """An emitting state a whose only way back to itself is a chain of n_chain silent states: every observation after the
    first adds n_chain + 1 entries to the Viterbi path."""
    m = Model("loop")
    a = State(NormalDistribution(0.0, 1.0), "a")
    b = State(NormalDistribution(2.0, 1.0), "b")
    chain = [State(None, "c%02d" % i) for i in range(n_chain)]
    m.add_transition(m.start, a, 0.7)
    m.add_transition(m.start, b, 0.3)
    m.add_transition(a, chain[0], 0.8)
    m.add_transition(a, m.end, 0.2)
    for x, y in zip(chain[:-1], chain[1:]):
        m.add_transition(x, y, 1.0)
    m.add_transition(chain[-1], a, 1.0)
    m.add_transition(b, b, 0.5)
    m.add_transition(b, chain[0], 0.3)
    m.add_transition(b, m.end, 0.2)
    m.bake()
    return m


def profile_events(means, count, lo=50, hi=400, seed=1):
    """`count` sequences of lo..hi segment means walking through the profile (repeats, skips, noise)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L = int(rng.integers(lo, hi + 1))
        idx = np.minimum(np.cumsum(rng.choice([0, 1, 1, 2], L)) * len(means) // max(1, L), len(means) - 1)
        x = means[idx] + rng.normal(0, 1.2, L)
        x[rng.random(L) < 0.03] = rng.uniform(0, 90)
        out.append(x)
    return out
