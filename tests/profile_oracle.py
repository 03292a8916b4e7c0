"""Test-side oracle for kernel-density HMM states and the profile aligners (pypore_amd.hmm.GaussianKernelDensity,
pypore_amd.alignment PSSM / ProfileAligner / MultipleSequenceAligner).

hmm_oracle's dynamic programmes read a model through `Compiled.emissions`, so the subclass here gives them the new
distribution; the functions of hmm_oracle and hmm_train_oracle that call the module-level `emission` or build their own
`Compiled` (path_score, brute_force, estep_one, estep_brute_force) are written out again for it.  The second half is a
plain-Python restatement of the reference's profile code (PyPore/alignment.py:329-796) -- the PSSM, the three model
builders as edge tables, the two path-following loops and the multiple sequence aligner -- driven by the oracle's Viterbi,
never by the device."""
import math

import numpy as np

import hmm_oracle as O
import hmm_train_oracle as TO
from pypore_amd.hmm import GaussianKernelDensity, Model, State, UniformDistribution

NEG = -np.inf


# ---- the kernel-density emission -------------------------------------------------------------------------------------
def kde_logpdf(points, bandwidth, weights, x):
    """-log(h sqrt(2 pi)) + log sum_i w_i exp(-(x - p_i)^2 / (2 h^2)) as max + log1p(sum of the others); zero weights skipped."""
    p, w = np.asarray(points, np.float64), np.asarray(weights, np.float64)
    w = w / w.sum()
    keep = w > 0
    v = np.log(w[keep]) - (x - p[keep]) ** 2 / (2.0 * bandwidth ** 2)
    return -math.log(bandwidth * math.sqrt(2 * math.pi)) + O.lse_rows(v[None, :])[0]


def kde_logpdf_longdouble(points, bandwidth, weights, x):
    """The same density in np.longdouble (the yardstick for the float64 oracle's own error)."""
    L = np.longdouble
    p, w = np.asarray(points, L), np.asarray(weights, L)
    w = w / w.sum()
    keep = w > 0
    h = L(bandwidth)
    v = np.log(w[keep]) - (L(x) - p[keep]) ** 2 / (2 * h * h)
    m = v.max()
    return -np.log(h * np.sqrt(2 * L(np.pi))) + m + np.log(np.exp(v - m).sum())


PROBE_POINTS = (1, 2, 63, 64, 65, 200, 5000)
PROBE_BANDWIDTHS = (1e-3, 0.05, 1.0, 30.0, 1e3)
PROBE_ORDERS = ("random", "ascending", "descending", "equal")
PROBE_WEIGHTS = ("equal", "wide")


def kde_probe_grid(seed=1):
    """The emission probe's configurations, [(name, GaussianKernelDensity, observations)]: points per state x bandwidth x
    point order (random in [-50, 50], the same ascending -- HmmLse rescales on every term right of them --, descending,
    all equal to 7.25 -- log1p runs up to log N) x weights (equal, or 10 ** uniform(-300, 0) with one weight 0 when
    N > 2).  Seven observations each: the first point, the middle point + 0.3 h, -50 - 3 h, 50 + 40 h, 50 + 1e3 h, -1e4, 0.
    Every emission is finite in float64 (the largest exponent, at h = 1e-3 and x = -1e4, is about 5e13)."""
    rng = np.random.default_rng(seed)
    out = []
    for N in PROBE_POINTS:
        for h in PROBE_BANDWIDTHS:
            for order in PROBE_ORDERS:
                pts = rng.uniform(-50, 50, N)
                if order == "ascending":
                    pts = np.sort(pts)
                elif order == "descending":
                    pts = np.sort(pts)[::-1]
                elif order == "equal":
                    pts = np.full(N, 7.25)
                for wk in PROBE_WEIGHTS:
                    w = np.ones(N) if wk == "equal" else 10.0 ** rng.uniform(-300, 0, N)
                    if wk == "wide" and N > 2:
                        w[rng.integers(N)] = 0.0
                    xs = [pts[0], pts[N // 2] + 0.3 * h, -50 - 3 * h, 50 + 40 * h, 50 + 1e3 * h, -1e4, 0.0]
                    out.append(("k%04d_%g_%s_%s" % (N, h, order, wk), GaussianKernelDensity(pts, h, w), [float(x) for x in xs]))
    return out


def emission(state, x):
    d = state.distribution
    if type(d).__name__ == "GaussianKernelDensity":
        return kde_logpdf(d.parameters[0], d.parameters[1], d.parameters[2], x)
    return O.emission(state, x)


class Compiled(O.Compiled):
    """A view of the model as it is when made: the emissions of an observation are computed once per value and kept."""

    def emissions(self, x):
        memo = self.__dict__.setdefault("_emissions", {})
        key = float(x)
        if key not in memo:
            with np.errstate(over="ignore"):                  # (a distance whose square overflows: the emission is -inf)
                memo[key] = np.array([emission(self.states[k], x) for k in range(self.NE)])
        return memo[key].copy()


def path_score(c, seq, path):
    """hmm_oracle.path_score with this module's emission."""
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


def enumerate_paths(c, seq):
    """Every complete state path of seq: [(log probability, [states])], and the prefix terms {(t, k): [log probabilities]}."""
    seq = np.asarray(seq, dtype=np.float64)
    n, terms, ends = seq.size, {}, []

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
    return ends, terms


def brute_force(c, seq):
    """hmm_oracle.brute_force with this module's emission: (forward matrix, log probability, best score, best path)."""
    ends, terms = enumerate_paths(c, seq)
    F = np.full((len(seq) + 1, c.S), NEG)
    for (t, k), v in terms.items():
        F[t, k] = O.lse_rows(np.array(v)[None, :])[0]
    if not ends:
        return F, NEG, NEG, None
    scores = np.array([e[0] for e in ends])
    best = int(np.argmax(scores))
    return F, O.lse_rows(scores[None, :])[0], scores[best], ends[best][1]


# ---- the E-step (hmm_train_oracle's formulas, the shift of a kernel-density state = the weighted mean of its points) ------
def shifts(model):
    out = []
    for s in model.states[:TO.n_emit(model)]:
        p = s.distribution.parameters
        if type(s.distribution).__name__ == "GaussianKernelDensity":
            out.append(math.fsum(a * b for a, b in zip(p[0], p[2])))
        else:
            out.append(p[0])
    return np.array(out, np.float64)


def estep_one(model, seq, c=None, sh=None):
    """(counts aligned with model.edges, stats [NE, 3], logp) of one sequence; zeros when logp = -inf.  c, sh: a Compiled of
    TO.View(model, model.edges) and shifts(model) to use again (made here otherwise)."""
    edges = model.edges
    c = c if c is not None else Compiled(TO.View(model, edges))
    sh = sh if sh is not None else shifts(model)
    seq = np.asarray(seq, np.float64)
    n, NE = seq.size, c.NE
    counts, stats = np.zeros(len(edges)), np.zeros((NE, 3))
    F = O.forward(c, seq)
    logp = O.final(c, F[n], False)[0]
    if not logp > NEG:
        return counts, stats, logp
    B = O.backward(c, seq)
    em = np.array([c.emissions(x) for x in seq]).reshape(n, NE)
    # every edge k -> l at once: f[t][k] + log p + e_l(x_t) + b[t+1][l] - logp over t < n (l emitting), or
    # f[t][k] + log p + b[t][l] - logp over t <= n (l silent); a term of -inf (p = 0 included) adds exp(-inf) = 0
    src = np.array([e[0] for e in edges], np.int64).reshape(-1)
    dst = np.array([e[1] for e in edges], np.int64).reshape(-1)
    with np.errstate(divide="ignore"):
        lp = np.log(np.array([e[2] for e in edges], np.float64).reshape(-1))
    to_emit = dst < NE
    ke, le = src[to_emit], dst[to_emit]
    if n and ke.size:
        counts[to_emit] = np.exp(F[:n][:, ke] + lp[to_emit] + em[:, le] + B[1:][:, le] - logp).sum(axis=0)
    ks, ls = src[~to_emit], dst[~to_emit]
    if ks.size:
        counts[~to_emit] = np.exp(F[:, ks] + lp[~to_emit] + B[:, ls] - logp).sum(axis=0)
    if n:
        with np.errstate(invalid="ignore"):
            g = np.exp(F[1:, :NE] + B[1:, :NE] - logp)
        g = np.where(np.isfinite(F[1:, :NE]) & np.isfinite(B[1:, :NE]), g, 0.0)
        d = seq[:, None] - sh[None, :]
        stats[:, 0], stats[:, 1], stats[:, 2] = g.sum(axis=0), (g * d).sum(axis=0), (g * d * d).sum(axis=0)
    return counts, stats, logp


def estep(model, seqs):
    counts, stats, logp = np.zeros(len(model.edges)), np.zeros((TO.n_emit(model), 3)), []
    c, sh = Compiled(TO.View(model, model.edges)), shifts(model)
    for s in seqs:
        cc, st, lp = estep_one(model, s, c, sh)
        logp.append(lp)
        if lp > NEG:
            counts += cc
            stats += st
    logp = np.array(logp, np.float64)
    return counts, stats, logp, int(np.sum(~(logp > NEG)))


def estep_brute_force(model, seq):
    """The E-step by weighting every complete path's edges and emissions by the path's posterior."""
    c = Compiled(TO.View(model))
    seq = np.asarray(seq, np.float64)
    index = {(i, j): e for e, (i, j, _) in enumerate(model.edges)}
    counts, stats = np.zeros(len(model.edges)), np.zeros((c.NE, 3))
    ends, _ = enumerate_paths(c, seq)
    if not ends:
        return counts, stats, NEG
    logp = O.lse_rows(np.array([e[0] for e in ends])[None, :])[0]
    sh = shifts(model)
    for lp, path in ends:
        w, t = math.exp(lp - logp), 0
        for a, b in zip(path[:-1], path[1:]):
            counts[index[(a, b)]] += w
            if b < c.NE:
                d = seq[t] - sh[b]
                stats[b] += (w, w * d, w * d * d)
                t += 1
    return counts, stats, logp


# ---- random models with kernel-density states --------------------------------------------------------------------------------
def random_kde(rng, max_points=4, lo=-2.0, hi=2.0, zero_weights=True):
    n = int(rng.integers(1, max_points + 1))
    w = rng.uniform(0.1, 1.0, n)
    if zero_weights and n > 1:
        w[rng.random(n) < 0.2] = 0.0
        if not w.any():
            w[0] = 1.0
    return GaussianKernelDensity(rng.uniform(lo, hi, n), float(rng.uniform(0.2, 5.0)), w)


def with_kde(model_fn, rng, share=0.5, **kw):
    """A model from one of hmm_oracle's generators with about `share` of its emitting states turned into kernel densities
    (the same object graph, baked again)."""
    m = model_fn()
    emitting = [s for s in m._added if not s.is_silent()]
    chosen = [s for s in emitting if rng.random() < share] or emitting[:1]          # at least one
    for s in chosen:
        s.distribution = random_kde(rng, **kw)
    m.bake()
    return m


# ---- the reference's profile code, restated (PyPore/alignment.py line numbers) ---------------------------------------------------
def is_gap(x):
    return isinstance(x, str) and x == '-'


class Pssm(object):
    """alignment.py:340-369."""

    def __init__(self, msa):
        if isinstance(msa[0], str) or not hasattr(msa[0], '__iter__'):
            msa = [msa]
        self.msa, self.consensus, self.pssm = msa, [], []
        offset = 0
        for i, column in enumerate(list(zip(*msa))):
            vals = [x for x in column if not is_gap(x)]
            if not vals:
                for seq in self.msa:
                    del seq[i - offset]
                offset += 1
                continue
            self.pssm.append(vals)
            self.consensus.append(np.mean(vals))


def global_edges(n):
    """alignment.py:440-464 as a table of (from, to, probability as written)."""
    E = [("start", "I0", 0.15), ("I0", "I0", 0.20)]
    for i in range(1, n + 1):
        lm = "start" if i == 1 else "M%d" % (i - 1)
        E += [(lm, "M%d" % i, 0.60), (lm, "D%d" % i, 0.25), ("I%d" % (i - 1), "M%d" % i, 0.65), ("I%d" % (i - 1), "D%d" % i, 0.20),
              ("D%d" % i, "I%d" % i, 0.15), ("I%d" % i, "I%d" % i, 0.15), ("M%d" % i, "I%d" % i, 0.15)]
        if i > 1:
            E += [("D%d" % (i - 1), "M%d" % i, 0.65), ("D%d" % (i - 1), "D%d" % i, 0.20)]
    return E + [("D%d" % n, "end", 0.85), ("I%d" % n, "end", 0.85), ("M%d" % n, "end", 0.85)]


def repeat_core_edges(m):
    """alignment.py:494-536 (= :571-613): columns M0, M1 .. M(m-2) with inserts and deletes, the last match M(m-1)."""
    E = [("M0", "I0", 0.15), ("M0", "PE", 0.05), ("I0", "I0", 0.20), ("P0", "M0", 1. / m)]
    for i in range(1, m - 1):
        E += [("P0", "M%d" % i, 1. / m), ("M%d" % (i - 1), "M%d" % i, 0.65), ("M%d" % (i - 1), "D%d" % i, 0.15),
              ("I%d" % (i - 1), "D%d" % i, 0.20), ("I%d" % (i - 1), "M%d" % i, 0.65), ("I%d" % i, "I%d" % i, 0.15),
              ("D%d" % i, "I%d" % i, 0.15), ("M%d" % i, "I%d" % i, 0.15), ("M%d" % i, "PE", 0.05)]
        if i > 1:
            E += [("D%d" % (i - 1), "M%d" % i, 0.65), ("D%d" % (i - 1), "D%d" % i, 0.20)]
    z, last = m - 2, "M%d" % (m - 1)
    return E + [("P0", last, 1. / m), ("M%d" % z, last, 0.80), ("I%d" % z, last, 0.85), ("D%d" % z, last, 0.85), (last, "PE", 1.00)]


def local_edges(m):
    """alignment.py:484-487 and :538-541 around the core."""
    return ([("start", "Q0", 0.5), ("start", "P0", 0.5), ("Q0", "Q0", 0.75), ("Q0", "P0", 0.25)] + repeat_core_edges(m)
            + [("PE", "QE", 0.5), ("PE", "end", 0.5), ("QE", "QE", 0.75), ("QE", "end", 0.25)])


def repeat_edges(m):
    """alignment.py:563-569 around the core."""
    return [("start", "P0", 0.5), ("start", "Q", 0.5), ("Q", "Q", 0.50), ("Q", "P0", 0.25), ("Q", "end", 0.25),
            ("PE", "Q", 0.5), ("PE", "end", 0.5)] + repeat_core_edges(m)


def build(edges, columns, first_match, low, high, bandwidth, name="restated"):
    """A baked Model from an edge table: M<j> is the kernel density of columns[j - first_match], I* and Q* share one uniform
    distribution, D* and P* are silent."""
    model = Model(name)
    ins = UniformDistribution(low, high)
    states = {"start": model.start, "end": model.end}

    def state(nm):
        if nm not in states:
            if nm[0] == "M":
                states[nm] = State(GaussianKernelDensity(columns[int(nm[1:]) - first_match], bandwidth), nm)
            else:
                states[nm] = State(ins if nm[0] in "IQ" else None, nm)
        return states[nm]

    for a, b, p in edges:
        model.add_transition(state(a), state(b), p)
    model.bake()
    return model


def build_global(pssm, low=0, high=60, bandwidth=1):
    return build(global_edges(len(pssm.pssm)), pssm.pssm, 1, low, high, bandwidth, "Global Profile Aligner")


def build_local(pssm, low=0, high=60, bandwidth=1):
    return build(local_edges(len(pssm.pssm)), pssm.pssm, 0, low, high, bandwidth, "Local Profile Aligner")


def build_repeat(pssm, low=0, high=60, bandwidth=1):
    return build(repeat_edges(len(pssm.pssm)), pssm.pssm, 0, low, high, bandwidth, "Local Profile Aligner")


def follow_global(master, slave, names):
    """alignment.py:630-641; names = the whole path's state names."""
    for i, nm in enumerate(names[1:-1]):
        target = slave if nm[0] == 'D' else master if nm[0] == 'I' else None
        if target is not None:
            target.pssm.insert(i, '-')
            for seq in target.msa:
                seq.insert(i, '-')


def follow_local(master, slave, names):
    """alignment.py:658-690."""
    first, offset = True, 0
    inner = names[1:-1]
    for i, nm in enumerate(inner):
        if nm[0] == 'M' and first:
            first, offset = False, int(nm[1:])
            for seq in master.msa:
                del seq[:offset]
            del master.pssm[:offset]
            del master.consensus[:offset]
        if nm[0] == 'D':
            slave.pssm.insert(i, '-')
            for seq in slave.msa:
                seq.insert(i, '-')
        elif nm[0] == 'I':
            master.pssm.insert(i - offset, '-')
            for seq in master.msa:
                seq.insert(i - offset, '-')
        if nm == 'PE':
            cut = len(inner) - i - 1
            for seq in slave.msa:
                for _ in range(cut):
                    del seq[-1]
            break


class CompiledLongDouble(Compiled):
    """The same view with every kernel-density emission taken from kde_logpdf_longdouble and rounded to double: other bits
    than the float64 formula's wherever its exp / log1p rounded, so a tie that survives the change owes nothing to them."""

    def emissions(self, x):
        memo = self.__dict__.setdefault("_emissions", {})
        key = float(x)
        if key not in memo:
            out = []
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                for k in range(self.NE):
                    d = self.states[k].distribution
                    if type(d).__name__ == "GaussianKernelDensity":
                        v = float(kde_logpdf_longdouble(d.parameters[0], d.parameters[1], d.parameters[2], x))
                        out.append(v if v == v else NEG)
                    else:
                        out.append(O.emission(self.states[k], x))
            memo[key] = np.array(out)
        return memo[key].copy()


def viterbi_structural(model, seq, flip_near=False):
    """(logp, path, gap, ties, structural) of O.viterbi_ties on Compiled(model).  structural: every exact tie on the winning
    path has identical operands on both sides -- judged by running the same Viterbi again with the kernel-density
    emissions from long double (CompiledLongDouble): the winning path and the set of tied decisions are unchanged.  A
    device whose exp / log1p differ from numpy's by ulps then ties at the same decisions.  True when there is no tie.
    flip_near: the path that takes the other side of every near tie (O.viterbi_ties); structural is then not judged (None)."""
    logp, path, gap, ties, tied = O.viterbi_ties(Compiled(model), seq, flip_near)
    if flip_near:
        return logp, path, gap, ties, None
    if not ties:
        return logp, path, gap, ties, True
    _, path2, _, _, tied2 = O.viterbi_ties(CompiledLongDouble(model), seq)
    return logp, path, gap, ties, path2 == path and tied2 == tied


def align_ties(master, slave, mode="global", low=0, high=60, bandwidth=1, flip_near=False):
    """(prob, master Pssm, slave Pssm, gap, ties, structural) by the oracle's Viterbi (viterbi_structural);
    (-inf, None, None, inf, 0, True) when impossible.  master / slave: Pssm objects or what Pssm takes."""
    master = master if isinstance(master, Pssm) else Pssm(master)
    slave = slave if isinstance(slave, Pssm) else Pssm(slave)
    model = (build_global if mode == "global" else build_local)(master, low, high, bandwidth)
    prob, path, gap, ties, structural = viterbi_structural(model, slave.consensus, flip_near)
    if path is None:
        return NEG, None, None, np.inf, 0, True
    (follow_global if mode == "global" else follow_local)(master, slave, [model.states[k].name for k in path])
    return prob, master, slave, gap, ties, structural


def align(master, slave, mode="global", low=0, high=60, bandwidth=1):
    """(prob, master Pssm, slave Pssm, Viterbi margin): align_ties with the margin 0.0 at an exact tie."""
    prob, master, slave, gap, ties, _ = align_ties(master, slave, mode, low, high, bandwidth)
    return prob, master, slave, (0.0 if ties else gap)


def msa_score(msa):
    """alignment.py:729-731."""
    total = 0.0
    for col in zip(*msa):
        vals = [x for x in col if not is_gap(x)]
        h = 0.5 * math.log(2 * np.pi * np.e * np.std(vals) ** 2) if len(vals) > 1 and np.std(vals) > 0 else 0
        total += 1. / len(vals) ** 2 * h
    return total


def msa_iterative_ties(sequences, epsilon=1e-4, max_iterations=10, bandwidth=1, flip_near=False):
    """alignment.py:790-796 and :743-782: (score of the last trial, best msa, smallest non-zero Viterbi gap met, exact ties
    met, whether all of them were structural).  flip_near: every alignment takes the other side of its near ties
    (O.viterbi_ties), the outcome of an arithmetic that decides them the other way; structural is then None."""
    worst, ties, structural = np.inf, 0, (None if flip_near else True)

    def one(master, slave):
        nonlocal worst, ties, structural
        _, x, y, gap, t, s = align_ties(master, slave, bandwidth=bandwidth, flip_near=flip_near)
        worst, ties, structural = min(worst, gap), ties + t, (None if flip_near else structural and s)
        return x, y

    pssm = Pssm(sequences[0])
    for seq in sequences[1:]:
        master, slave = one(pssm, seq)
        pssm = Pssm(master.msa + slave.msa)
    score, msa = msa_score(pssm.msa), pssm.msa
    if score == 0:
        return 0, msa, worst, ties, structural
    n = len(msa)
    last_score, best_msa, best_score, iteration = float('inf'), msa, score, 0
    while abs(best_score - last_score) >= epsilon and iteration < max_iterations:
        iteration += 1
        last_score = best_score
        for i in range(n):
            slave = [x for x in best_msa[i] if not is_gap(x)]
            master = best_msa[:i] + best_msa[i + 1:]
            x, y = one(master, slave)
            msa = x.msa + y.msa
            score = msa_score(msa)
            if score < best_score:
                best_msa, best_score = msa, score
    m = max(len(s) for s in best_msa)
    for seq in best_msa:
        seq.extend(['-'] * (m - len(seq)))
    return score, best_msa, worst, ties, structural


def msa_iterative(sequences, epsilon=1e-4, max_iterations=10, bandwidth=1):
    """(score of the last trial, best msa, smallest Viterbi margin met: 0.0 at an exact tie)."""
    score, msa, worst, ties, _ = msa_iterative_ties(sequences, epsilon, max_iterations, bandwidth)
    return score, msa, (0.0 if ties else worst)


def derived_sequences(rng, columns, rows, noise=0.8, p_del=0.08, p_ins=0.08, lo=5.0, hi=55.0):
    """A template of `columns` means in [lo, hi] and `rows` sequences derived from it with deletions, insertions and noise,
    every value clipped into [0.5, 59.5] (inside the default insert range)."""
    template = rng.uniform(lo, hi, columns)
    out = []
    for _ in range(rows):
        seq = []
        for v in template:
            if rng.random() < p_ins:
                seq.append(float(rng.uniform(lo, hi)))
            if rng.random() >= p_del:
                seq.append(float(np.clip(v + rng.normal(0, noise), 0.5, 59.5)))
        out.append(seq if len(seq) >= 3 else [float(x) for x in np.clip(template[:3], 0.5, 59.5)])
    return template, out


def alignment_case(seed):
    """(master MSA rows with gaps, [slave sequences]) from one template: 5 to 60 columns, 1 to 30 master rows (noise and
    gaps), 4 slaves with deletions, insertions and noise."""
    rng = np.random.default_rng(seed)
    columns, rows = int(rng.integers(5, 61)), int(rng.integers(1, 31))
    template, slaves = derived_sequences(rng, columns, 4)
    msa = [[float(np.clip(v + rng.normal(0, 0.8), 0.5, 59.5)) if rng.random() >= 0.1 else '-' for v in template]
           for _ in range(rows)]
    return msa, slaves
