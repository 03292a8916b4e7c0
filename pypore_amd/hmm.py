"""Hidden Markov models with the surface the reference's HMM code uses (yahmm: Model, State, NormalDistribution,
UniformDistribution; add_state(s), add_transition, add_model, bake; viterbi, forward, backward, log_probability), decoded on
the MI355X (ps_hmm_batch, csrc/seg_hmm.hpp).

    model = Model("happy model")
    a = State(NormalDistribution(3, 4), 'a')
    b = State(NormalDistribution(10, 1), 'b')
    model.add_transition(model.start, a, 0.5)
    ...
    model.bake()
    logp, path = model.viterbi(means)                   # path: [(index into model.states, state), ...]
    results = model.viterbi_batch([means0, means1])     # many sequences in one launch

Semantics (the device and tests/hmm_oracle.py compute the same thing).  A path starts in `start` before the first
observation; an emitting state consumes one observation, a silent state none.  Row t of the forward matrix holds, per
state, the log probability of the first t observations with the path in that state after them: emitting states take their
in-edges from row t-1 and add their emission log density of observation t-1, silent states take their in-edges from row t
(silent predecessors come earlier in the topological order).  A model is finite when some edge goes into `end`; its paths
then end in `end` after the last observation, otherwise anywhere.  log_probability = f[n][end] (finite) or log-sum-exp of
f[n] over all states (infinite).  The backward matrix starts from log 1 at `end` (finite) or at every state (infinite) in
row n and runs the same recursion backwards; b[0][start] = log_probability.  Viterbi takes maxima instead of sums; it scans
in-edges in ascending source index and takes only a strictly greater score, so the lowest source index wins a tie, and an
infinite model's path ends in the best state of row n (lowest index on a tie).  An impossible sequence gives (-inf, None).

Deviations from yahmm, by design:
  * bake(merge=...) is accepted and ignored: no states are merged.  yahmm may merge chains of probability-1 silent edges
    and so drop those silent states from its paths; here every silent state visited appears in the path.
  * `end` is kept in model.states even when it cannot be reached (the model is then infinite).
  * Edges of probability 0 are dropped; negative probabilities raise ValueError.
There is no CPU fallback: inference runs on the GPU library or raises.
"""
import collections
import math

import numpy as np

NEG_INF = float("-inf")
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
KIND_SILENT, KIND_NORMAL, KIND_UNIFORM = 0, 1, 2      # include/poreseg.h ps_hmm_model.kind
MAX_STATES = 4096                                     # csrc/seg_hmm.hpp HMM_S_MAX


class Distribution(object):
    """Base class of the emission distributions: `parameters` is the list of their arguments."""
    kind = None

    def __init__(self, parameters):
        self.parameters = list(parameters)

    def log_probability(self, x):
        raise NotImplementedError

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join(repr(p) for p in self.parameters))


class NormalDistribution(Distribution):
    """log density -log(std sqrt(2 pi)) - (x - mean)^2 / (2 std^2)."""
    kind = KIND_NORMAL

    def __init__(self, mean, std):
        mean, std = float(mean), float(std)
        if not std > 0:
            raise ValueError("NormalDistribution needs std > 0, got %r" % std)
        Distribution.__init__(self, [mean, std])

    def log_probability(self, x):
        mean, std = self.parameters
        return -math.log(std) - _LOG_SQRT_2PI - (x - mean) ** 2 / (2 * std * std)

    def compiled(self):
        mean, std = self.parameters
        return mean, 1.0 / (2.0 * std * std), -(math.log(std) + _LOG_SQRT_2PI)


class UniformDistribution(Distribution):
    """log density -log(high - low) on [low, high], -inf outside."""
    kind = KIND_UNIFORM

    def __init__(self, low, high):
        low, high = float(low), float(high)
        if not high > low:
            raise ValueError("UniformDistribution needs high > low, got [%r, %r]" % (low, high))
        Distribution.__init__(self, [low, high])

    def log_probability(self, x):
        low, high = self.parameters
        return -math.log(high - low) if low <= x <= high else NEG_INF

    def compiled(self):
        low, high = self.parameters
        return low, high, -math.log(high - low)


class State(object):
    """A state of a Model: emitting with a Distribution, silent with None."""

    def __init__(self, distribution, name=None):
        if distribution is not None and not isinstance(distribution, Distribution):
            raise TypeError("a State takes a Distribution or None, got %r" % (distribution,))
        self.distribution = distribution
        self.name = name if name is not None else "s%x" % id(self)

    def is_silent(self):
        return self.distribution is None

    def __repr__(self):
        return "State(%r, %r)" % (self.distribution, self.name)


class Model(object):
    """A hidden Markov model: states, weighted edges, silent `start` and `end`.  bake() before inference."""

    def __init__(self, name=None):
        self.name = name if name is not None else "Model"
        self.start = State(None, name="%s-start" % self.name)
        self.end = State(None, name="%s-end" % self.name)
        self._added = []                                   # every state, in the order it joined
        self._known = set()
        self._edges = collections.OrderedDict()            # (from, to) -> probability as given
        self.states = None                                 # after bake()
        self._flat = None
        self._c = None                                     # the ctypes view of _flat, made on first use
        self.add_state(self.start)
        self.add_state(self.end)

    # ---- construction -----------------------------------------------------------------------------------------
    def add_state(self, state):
        if not isinstance(state, State):
            raise TypeError("add_state takes a State, got %r" % (state,))
        if id(state) not in self._known:
            self._known.add(id(state))
            self._added.append(state)
        self._flat = None

    def add_states(self, *states):
        """add_states(a, b, ...) or add_states([a, b, ...])."""
        if len(states) == 1 and isinstance(states[0], (list, tuple)):
            states = states[0]
        for s in states:
            self.add_state(s)

    def add_transition(self, a, b, probability):
        """An edge a -> b (states not yet in the model join it).  A second call for the same pair replaces the first."""
        p = float(probability)
        if p < 0 or math.isnan(p):
            raise ValueError("transition probability must be >= 0, got %r" % probability)
        self.add_state(a)
        self.add_state(b)
        self._edges[(a, b)] = p
        self._flat = None

    def add_model(self, other):
        """The other model's states and edges join this one; its start and end become ordinary silent states."""
        for s in other._added:
            self.add_state(s)
        for (a, b), p in other._edges.items():
            self._edges[(a, b)] = p
        self._flat = None

    # ---- bake ---------------------------------------------------------------------------------------------------
    def bake(self, verbose=False, merge=None):
        """Normalises each state's out-edges to sum to 1, drops the states `start` cannot reach (never `end`), rejects a
        cycle of silent states (ValueError), orders `states` -- emitting states by name (stable), then silent states in
        topological order (by level, then in the order they joined) -- and compiles the flat form the device reads.
        `merge` is accepted and ignored (module docstring)."""
        out = collections.OrderedDict((id(s), []) for s in self._added)
        for (a, b), p in self._edges.items():
            if p > 0:
                out[id(a)].append((b, p))
        # reachability from start
        seen = {id(self.start)}
        stack = [self.start]
        while stack:
            a = stack.pop()
            for b, _ in out[id(a)]:
                if id(b) not in seen:
                    seen.add(id(b))
                    stack.append(b)
        seen.add(id(self.end))
        kept = [s for s in self._added if id(s) in seen]
        # normalised edges among the kept states (an edge from a kept state never leaves them)
        edges = []
        for a in kept:
            total = sum(p for _, p in out[id(a)])
            edges.extend((a, b, p / total) for b, p in out[id(a)])
        # silent levels (Kahn); a silent state left over lies on a cycle
        silent = [s for s in kept if s.is_silent()]
        preds = {id(s): [] for s in silent}
        for a, b, _ in edges:
            if a.is_silent() and b.is_silent():
                preds[id(b)].append(a)
        level, remaining = {}, list(silent)
        while remaining:
            ready = [s for s in remaining if all(id(a) in level for a in preds[id(s)])]
            if not ready:
                raise ValueError("silent states form a cycle: %s" % ", ".join(sorted(s.name for s in remaining)))
            for s in ready:
                level[id(s)] = 1 + max([level[id(a)] for a in preds[id(s)]] or [-1])
            remaining = [s for s in remaining if id(s) not in level]
        emitting = sorted((s for s in kept if not s.is_silent()), key=lambda s: s.name)
        order = {id(s): i for i, s in enumerate(silent)}
        silent.sort(key=lambda s: (level[id(s)], order[id(s)]))
        self.states = emitting + silent
        index = {id(s): i for i, s in enumerate(self.states)}
        S, NE = len(self.states), len(emitting)
        self.edges = sorted((index[id(a)], index[id(b)], p) for a, b, p in edges)     # (from, to, probability)
        self.finite = any(j == index[id(self.end)] for _, j, _ in self.edges)
        if verbose:
            print("%s: %d states (%d silent), %d edges, %s" % (self.name, S, S - NE, len(self.edges),
                                                                 "finite" if self.finite else "infinite"))
        # the flat form (include/poreseg.h ps_hmm_model)
        kind = np.zeros(S, np.int32)
        param = np.zeros(3 * S, np.float64)
        for k, s in enumerate(emitting):
            kind[k] = s.distribution.kind
            param[3 * k:3 * k + 3] = s.distribution.compiled()
        lv = np.array([level[id(s)] for s in silent], np.int64)
        n_levels = int(lv.max()) + 1 if lv.size else 0
        level_ptr = (NE + np.searchsorted(lv, np.arange(n_levels + 1))).astype(np.int32)
        src = np.array([e[0] for e in self.edges], np.int32).reshape(-1)
        dst = np.array([e[1] for e in self.edges], np.int32).reshape(-1)
        with np.errstate(divide="ignore"):
            lp = np.log(np.array([e[2] for e in self.edges], np.float64).reshape(-1))
        by_dst = np.lexsort((src, dst))                 # in-edges: per target, source ascending
        by_src = np.lexsort((dst, src))                 # out-edges: per source, target ascending
        self._flat = dict(
            n_states=S, n_emit=NE, n_levels=n_levels, start=index[id(self.start)], end=index[id(self.end)],
            finite=int(self.finite), kind=kind, level_ptr=level_ptr, param=param,
            in_ptr=np.concatenate(([0], np.cumsum(np.bincount(dst, minlength=S)))).astype(np.int32),
            in_src=np.ascontiguousarray(src[by_dst]), in_lp=np.ascontiguousarray(lp[by_dst]),
            out_ptr=np.concatenate(([0], np.cumsum(np.bincount(src, minlength=S)))).astype(np.int32),
            out_dst=np.ascontiguousarray(dst[by_src]), out_lp=np.ascontiguousarray(lp[by_src]))
        self._c = None

    @property
    def flat(self):
        """The compiled arrays (bake()); raises ValueError before bake or after a change."""
        if self._flat is None:
            raise ValueError("model %r is not baked: call bake() after adding states and transitions" % self.name)
        return self._flat

    def _c_model(self):
        from . import _lib
        f = self.flat
        if self._c is None:
            m = _lib.HmmModel()
            for k in ("n_states", "n_emit", "n_levels", "start", "end", "finite"):
                setattr(m, k, f[k])
            for k in ("kind", "level_ptr", "in_ptr", "in_src", "out_ptr", "out_dst", "param", "in_lp", "out_lp"):
                setattr(m, k, f[k].ctypes.data if f[k].size else None)
            self._c = m
        return self._c

    # ---- inference on the device ---------------------------------------------------------------------------------
    def _run(self, sequences, mode, want_mat, device=None):
        import torch
        from . import engine
        f = self.flat
        seqs = [np.ascontiguousarray(s, dtype=np.float64) for s in sequences]
        for s in seqs:
            if s.ndim != 1:
                raise ValueError("an observation sequence must be 1-D, got shape %r" % (s.shape,))
        if f["n_states"] > MAX_STATES:
            raise ValueError("model %r has %d states: the device HMM kernels take at most %d" % (self.name, f["n_states"], MAX_STATES))
        ctx = engine.context(device)
        off = np.concatenate(([0], np.cumsum([s.size for s in seqs]))).astype(np.int64)
        obs = np.concatenate(seqs) if off[-1] else np.zeros(1, np.float64)
        obs = torch.from_numpy(obs).to(torch.device("cuda", ctx.device))
        return off, ctx.hmm_batch(self._c_model(), mode, obs, off, want_mat)

    def _matrices(self, sequences, mode, device):
        off, (logp, mat, _) = self._run(sequences, mode, True, device)
        mat = mat.cpu().numpy()
        return [mat[off[q] + q:off[q + 1] + q + 1] for q in range(off.size - 1)]

    def viterbi_batch(self, sequences, device=None):
        """[(logp, path) per sequence], one launch (more when the backpointers exceed the context's budget)."""
        from . import _lib
        off, (logp, _, (path, path_off, path_len)) = self._run(sequences, _lib.PS_HMM_VITERBI, False, device)
        logp, path, path_len = logp.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()
        out = []
        for q in range(off.size - 1):
            if not logp[q] > NEG_INF:
                out.append((NEG_INF, None))
                continue
            idx = path[path_off[q]:path_off[q] + path_len[q]]
            out.append((float(logp[q]), [(int(i), self.states[i]) for i in idx]))
        return out

    def forward_batch(self, sequences, device=None):
        """[(n+1) x len(states) log forward matrix per sequence]."""
        from . import _lib
        return self._matrices(sequences, _lib.PS_HMM_FORWARD, device)

    def backward_batch(self, sequences, device=None):
        """[(n+1) x len(states) log backward matrix per sequence]."""
        from . import _lib
        return self._matrices(sequences, _lib.PS_HMM_BACKWARD, device)

    def log_probability_batch(self, sequences, device=None):
        """float64 array: the log probability of every sequence (forward pass, no matrix kept)."""
        from . import _lib
        _, (logp, _, _) = self._run(sequences, _lib.PS_HMM_FORWARD, False, device)
        return logp.cpu().numpy()

    def viterbi(self, sequence):
        return self.viterbi_batch([sequence])[0]

    def forward(self, sequence):
        return self.forward_batch([sequence])[0]

    def backward(self, sequence):
        return self.backward_batch([sequence])[0]

    def log_probability(self, sequence):
        return float(self.log_probability_batch([sequence])[0])
