"""Hidden Markov models with the surface the reference's HMM code uses (yahmm: Model, State, NormalDistribution,
UniformDistribution, GaussianKernelDensity, MultivariateDistribution, LogNormalDistribution, ExponentialDistribution,
MixtureDistribution;
add_state(s), add_transition, add_model, bake; viterbi, forward, backward,
log_probability, forward_backward, maximum_a_posteriori) and the reference's profile HMM builders (HMMBoard, the three
board modules, ModularProfileModel, Phi29ProfileHMM, Hel308ProfileHMM: the end of this module), decoded on the MI355X
(ps_hmm_batch, ps_hmm_posterior, csrc/seg_hmm.hpp), and trained there (Model.train: Baum-Welch with its E-step in
ps_hmm_expect, or Viterbi training).

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

Emission log densities: NormalDistribution(mean, std) is -log(std sqrt(2 pi)) - (x - mean)^2 / (2 std^2);
UniformDistribution(low, high) is -log(high - low) on [low, high] and -inf outside; GaussianKernelDensity(points, bandwidth
h, weights w, normalised to sum to 1) is
    e(x) = -log(h sqrt(2 pi)) + log sum_i w_i exp(-(x - p_i)^2 / (2 h^2)),
the sum taken as a log-sum-exp over the points of non-zero weight in ascending index -- the largest term plus log1p of the
others' exp, the form the recursions use -- so an observation far from every point has a finite, accurate log density
instead of log(0).  With one point it is NormalDistribution(p, h).  On the device the lane that owns the state walks its
points (csrc/seg_hmm.hpp hmm_emit); the flat form holds them as CSR tables kde_ptr / kde_pt / kde_lw.

Mixture states.  MixtureDistribution(distributions, weights) is one state whose level is a weighted choice between J >= 1
univariate components -- Normal, Uniform, LogNormal or ExponentialDistribution -- with weights w_j, finite and >= 0 with a
sum > 0 (default: equal), normalised to sum to 1 as a kernel density's are.  Its log density is
    e(x) = log sum_j w_j p_j(x),
taken as a log-sum-exp in ascending j over the terms  log w_j + l_j(x)  that are > -inf -- the largest term so far plus
log1p of the others' exp, the form the recursions use (csrc/seg_hmm.hpp HmmLse) --, with l_j the component's own log
density above and below: -inf when no term is finite, never NaN, and one component of weight 1 gives that component's own
bits (log 1 = 0.0, 0.0 + l = l, l + log1p(0) = l).  A component of weight 0 keeps its slot -- component index equals table
index, always -- with log weight -inf, and is skipped.  responsibilities(x) are  exp((log w_j + l_j(x)) - e(x)),  0 for a
skipped term and all 0 where e(x) = -inf.  Mixture states stand in scalar models only: n_dim = 1, beside normal, uniform,
kernel-density and other mixture states; a mixture state in a vector model is a ValueError at bake() that names the state.
A log-normal or exponential COMPONENT of a mixture does not make the model a vector model: the mixture evaluates it
itself.  In `flat` a mixture state has kind 7 and param (0, 0, 0); `flat` gains no key.  The components live beside it in
Model._mix, built by bake() and again after every M-step: mix_ptr (int32, n_emit + 1: a CSR index, a kind-7 state has >= 1
entries and every other state none), mix_kind, mix_param (the component's compiled triple), mix_lw (log weights) and the
two sampling tables mix_cdf and mix_draw (Sampling, below); all empty for a model without mixture states, whose flat form,
upload, kernels and bits are what they were.  On the device the lane that owns the state walks its components
(csrc/seg_hmm.hpp HmmDevM, a fourth set of kernel instantiations, taken only when some state is kind 7).

Vector models (observations of more than one number: the reference's tutorial decodes
`[(s.mean, s.std, s.duration) for s in event.segments]`).  MultivariateDistribution(distributions, weights) is D >= 1
independent univariate components -- Normal, Uniform, LogNormal or ExponentialDistribution -- with weights w_d, finite and
> 0 (default 1); its log density of a length-D observation is  w_0 l_0(x_0) + w_1 l_1(x_1) + ...,  added in ascending d
from the first product (not from 0.0), so one component of weight 1 gives that component's own bits, and an impossible
component gives -inf, never NaN.  LogNormalDistribution(mu, sigma), with y = log x:
(-log(sigma sqrt(2 pi)) - (y - mu)^2 / (2 sigma^2)) - y  for x > 0, -inf otherwise; ExponentialDistribution(rate):
log(rate) - rate x  for x >= 0, -inf otherwise (a dwell time is not normal: a duration component takes one of the two).
Every emitting state of a model has the same dimension D = Model.n_dim (ValueError at bake() otherwise).  A model whose
emitting states are all normal, uniform or kernel density is compiled, uploaded and run as ever: the same flat arrays,
kernels and bits; n_dim = 1 and the flat entries comp_kind / comp_param / comp_w are empty.  Any model with a Multivariate,
LogNormal or ExponentialDistribution state is a vector model: every emitting state is compiled as D components (kind 4; a
plain normal or uniform state of a D = 1 model becomes one component of weight 1), the device reads the component tables
(csrc/seg_hmm.hpp HmmDevV: the lane that owns the state walks its components) and `param` is left 0.  A vector model takes
sequences of shape (n, D) -- anything np.asarray makes of that shape, a list of tuples as in the tutorial; [] is the empty
sequence; at D = 1 also 1-D -- in every method below, their _batch twins, expected_counts_batch and train; any other shape
is a ValueError that names D.  The device's log is not numpy's bit for bit, so results with log-normal components agree
with tests/multivariate_oracle.py to 1e-12, not to the bit; every other component does.

Deviations from yahmm, by design:
  * yahmm is not available to compare against.  What is assumed of its MultivariateDistribution is the constructor
    (distributions, weights), `parameters = [distributions, weights]`, and that a weight multiplies its component's log
    probability; of its LogNormalDistribution(mu, sigma) and ExponentialDistribution(rate) the argument order and the
    textbook densities above.  Nothing about its arithmetic or its training of these classes is assumed.
  * a GaussianKernelDensity cannot be a component, nor stand in a vector model (ValueError; the point loop inside the
    component loop is not built), and a MultivariateDistribution cannot be nested (ValueError).
  * what is assumed of yahmm's MixtureDistribution is the constructor (distributions, weights) and `parameters =
    [distributions, weights]`.  The mixture arithmetic -- the order of the log-sum-exp, the responsibilities, the M-step
    below -- is this package's own; nothing about yahmm's is assumed.  A kernel density, a multivariate or another mixture
    cannot be a component, and a mixture cannot be a component of a MultivariateDistribution (ValueError).
  * GaussianKernelDensity is normalised: it carries the 1/h factor above.  yahmm is not available to compare against; as
    far as is known its kernel density leaves 1/h out, which is the same density at bandwidth 1, the default and what
    every caller in the reference's alignment.py uses.  Nothing else about its arithmetic is assumed.
  * bake(merge=...) merges nothing by default (None, 'none'); as far as is known yahmm's default is 'all'.  The default
    differs so that a model baked without the argument keeps every silent state it was given, and its paths.  The rule,
    in this package's own terms (yahmm is not available to compare against): with merge='all', repeat until no state
    qualifies -- the first state a, in the order the states joined, that is silent, is neither start nor end, and has
    exactly one out-edge of positive probability, a -> b with b != a, leaves the model with that edge, and every in-edge
    x -> a becomes x -> b with its probability and pseudocount.  merge='partial' is the same with b silent as well.  Where
    x -> b exists already the two are parallel edges and are summed (probability and pseudocount): forward, backward,
    log_probability and the expected counts see the same total, so they stay as they were up to rounding, while Viterbi
    now scores the two ways as one, the sum, and may give a higher score or another path.  Without parallel edges the
    merged model's Viterbi path is the unmerged one with the removed states left out.  Merging rewrites the model's own
    construction graph: train() trains the merged structure and a later bake() starts from it.
  * `end` is kept in model.states even when it cannot be reached (the model is then infinite).
  * Edges of probability 0 are dropped; negative probabilities raise ValueError.

Posterior decoding (forward_backward, maximum_a_posteriori and their _batch twins; the device -- ps_hmm_posterior,
csrc/seg_hmm.hpp hmm_posterior_kernel -- and tests/posterior_oracle.py compute the same thing).  For one sequence x of
length n with f, b and logp as above:
  * the log posterior of emitting state k for observation t (0 <= t < n) is  (f[t+1][k] + b[t+1][k]) - logp,  -inf where
    either matrix entry is -inf: `emissions`, n rows of n_emit (the emitting states come first in `states`);
  * the MAP state of observation t is the emitting state with the largest entry of row t, the lowest index on a tie (the
    rule Viterbi uses for sources); the MAP log probability is the sum of those largest entries in ascending t, so it is
    bit for bit the sum one takes over `emissions`.  The MAP path need not be a path of the model: it maximises every
    observation's state on its own;
  * `transitions`[k][l] is the sequence's expected count of edge k -> l by the formula under Training below, per
    sequence instead of summed over the batch, 0 where the model has no such edge; expected_transitions(_batch) returns
    the same counts as one row per sequence in the order of `edges`, without the dense array;
  * an impossible sequence (logp = -inf) has emissions -inf, transitions 0 and MAP result (-inf, None); an empty one has
    no rows, MAP result (0.0, []), and its transitions hold the silent edges at t = 0.
Nothing is summed across sequences, so a batch gives the bits of the single calls however the library cuts it.

Deviations from yahmm, by design:
  * yahmm is not available to compare against.  What is assumed of its forward_backward is the shape of its result, a
    pair (transitions, emissions): expected transition counts NOT in log space, as a dense states x states array in
    the order of `states`, and emission weights IN log space, one row per observation.  Here emissions has a column per
    emitting state (the first n_emit of `states`), none for silent states.
  * maximum_a_posteriori returns (logp, path) in viterbi's element format, (index, state) per observation, and (-inf,
    None) for an impossible sequence; silent states never appear in it.

Training (Model.train; the device and tests/hmm_train_oracle.py compute the same thing).  For one sequence x of length n
with forward matrix f, backward matrix b and log probability logp (above):
  * the expected count of edge k -> l (log probability lp) is  sum_{t=0}^{n-1} exp(f[t][k] + lp + e_l(x_t) + b[t+1][l] - logp)
    for an emitting l and  sum_{t=0}^{n} exp(f[t][k] + lp + b[t][l] - logp)  for a silent l (finite and infinite models
    alike: b holds the end condition);
  * emitting state k's posterior for observation t is g_k(t) = exp(f[t+1][k] + b[t+1][k] - logp), and its statistics are
    W_k = sum g, A_k = sum g (x - c_k), B_k = sum g (x - c_k)^2 with the shift c_k = its current mean (param[3k]);
  * a sequence with logp = -inf is skipped (counted, contributes nothing); an empty one contributes its silent edges at
    t = 0; a batch's statistics are the sums over its sequences (Model.expected_counts_batch).
The M-step (host): count(k -> l) = expected count + the edge's pseudocount (use_pseudocount) + transition_pseudocount; the
new probability is count / (sum over k's out-edges), k keeps its old probabilities when that sum is 0, and then
p = edge_inertia p_old + (1 - edge_inertia) p_new.  A normal state with W > 0 gets mean = c + A/W, var = B/W - (A/W)^2,
std = max(sqrt(max(var, 0)), min_std), each mixed with its old value by distribution_inertia; W = 0 leaves it.  A
distribution shared by several states is updated once, from their pooled statistics.  Frozen distributions
(Distribution.freeze()) are never updated.  In a vector model state k's statistics are W_k and, per component d,
A_kd = sum g (y_d - c_kd), B_kd = sum g (y_d - c_kd)^2 with y_d = log x_d for a log-normal component and x_d otherwise,
and c_kd the component's shift (normal: mean; log-normal: mu; exponential: 0; uniform: low) -- `stats` is [n_emit, 1 + 2 D],
the (W, A, B) layout at D = 1.  The M-step updates COMPONENT distributions, pooled per distribution object over the
states and the component slots that hold it: a normal as above from (W, A_d, B_d); a log-normal by the same formulas on
log x, giving mu and sigma, with min_std the floor of sigma; an exponential  rate = W / A  (left as it is when A <= 0);
uniform components are untouched, and a frozen MultivariateDistribution freezes all its components.
In a model with mixture states `stats` is [n_emit + n_mix, 3]: the states' rows -- a mixture state's shift is 0, its row the
raw moments --, then one row per mixture component in the order of Model._mix.  Where mixture state k has posterior g for
observation x, component i with a term  v_i = log w_i + l_i(x) > -inf  has the responsibility  r = exp(v_i - e_k(x))  and
adds  W_i += g r,  A_i += g r d,  B_i += (g r d) d  with  d = y - c_i,  y = log x for a log-normal component and x
otherwise, c_i the component's shift as above.  In the M-step the components of a mixture join the pooling per distribution
object -- over plain states and mixture slots alike -- and take the formulas above from their own rows; a mixture's weights
are pooled per mixture object over the states that hold it:  w_j = W_j / sum_j W_j  when that sum is > 0, otherwise kept,
then mixed with the old weight by distribution_inertia.  A weight that becomes 0 keeps its slot (log weight -inf).  A
frozen mixture changes neither its weights nor, in its slots, its components.  Viterbi training gives each observation
weight 1 in its state and shares it out over the state's components by responsibilities(x), computed on the host.
The structure stays: `states`, their order and `edges` do not change, an edge
whose probability becomes 0 keeps its place (log -inf on the device), and the trained probabilities are written back to
the transitions, so a later bake() starts from them (and drops the zero edges, as always).  algorithm='viterbi' counts
each consecutive pair of states on every Viterbi path as one transition and gives each observation weight 1 in the
emitting state that consumed it (the shift and the M-step as above); its log probabilities are the Viterbi scores.

Deviations from yahmm, by design:
  * uniform distributions are not trained (their support decides which sequences are possible);
  * kernel-density distributions are not trained either: their points, bandwidth and weights stay as they are (bit for
    bit), while a model's edges and normal states train around them.  Their (W, A, B) are still reported, with the shift
    c_k = the weighted mean of the points;
  * Viterbi training runs the same stop loop as Baum-Welch, measured by the sum of the Viterbi scores.

Sampling (Model.sample, Model.sample_batch; the device -- ps_hmm_sample, csrc/seg_hmm.hpp hmm_sample_kernel -- and
tests/sample_oracle.py compute the same thing; Distribution.sample is one numpy draw on the host).  A walk starts in `start`
and, before every step, stops when it stands in `end` or has made `length` > 0 emissions (flag 0), has made max_length
emissions (flag 1) or stands in a state without out-edges (flag 2); otherwise it takes one transition and, when the new
state emits, draws one observation.  The random stream is counter-based, Philox4x32-10 with key (seed & 0xffffffff,
seed >> 32): sequence Q = first + q owns the blocks j = 0, 1, 2, ... at counter (j & 0xffffffff, j >> 32, Q & 0xffffffff,
Q >> 32), a block r0..r3 gives u0 = ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53 and u1 likewise from r2, r3, and blocks are taken in walk
order: one per transition -- the first out-edge e of the state with u0 < out_cdf[e] --, one per component of an emission in
ascending d, with z = sqrt(-2 log(1 - u0)) cos(2 pi u1): normal mean + std z, uniform low + u0 (high - low), log-normal
exp(mu + sigma z), exponential -log(1 - u0) / rate; a kernel-density state takes two: the first point i with u0 < kde_cdf[i],
then p_i + h z from the next block; a mixture state takes two as well: the first component i of the state with
u0 < mix_cdf[i], then that component's draw by its kind from the next block.  mix_cdf (Model._mix, aligned with mix_lw) is
per mixture state the running sum of the weights, added one by one, with the entry of the state's last component of positive
weight and every entry after it stored as exactly 1.0, so a component of weight 0 is never picked; mix_draw holds two
doubles per component by emit_param's rule, and emit_param (0, 0) for a mixture state.  The tables are built on the host in float64 (Model._sample_tables, not part of `flat`):
out_cdf, per state the running sum of np.exp(out_lp) in out-edge order, added one by one, with the entry of the state's last
out-edge of positive probability and every entry after it stored as exactly 1.0 (mix_cdf's rule: an edge that training left
at probability 0 is never taken, wherever it stands); kde_cdf the same over exp(kde_lw); emit_param, two doubles per
emitting state or component: normal (mean, std), uniform (low, high - low), log-normal (mu, sigma), exponential (0, rate), kernel density (0, bandwidth).  So a walk's path and
length depend on (seed, Q, out_cdf) alone, an integer seed reproduces a call bit for bit, and a batch cut in two with `first`
moved on gives the bits of the whole.  Values that pass through the device's log, cos and exp agree with the oracle to
1e-12, uniform draws to the bit.

Deviations from yahmm, by design:
  * yahmm is not available to compare against.  What is assumed of its Model.sample is the signature (length=0, path=False),
    that it returns a list, or (list, path) with path=True, and that an infinite model without a length is an error.
  * length > 0 on a finite model: the walk stops at `end` or after `length` emissions, whichever comes first, so the result
    is the prefix of a true sample.  As far as is known yahmm renormalises the walk away from `end` until the length is
    reached, which is not a sample of the model; that walk is not built.
  * a MultivariateDistribution's weights take no part in sampling, on the device or in Distribution.sample: a weight scales
    a log density and defines no distribution to draw from (yahmm ignores them as well).
There is no CPU fallback: inference, sampling and the Baum-Welch E-step run on the GPU library or raise.
"""
import collections
import math

import numpy as np

NEG_INF = float("-inf")
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
KIND_SILENT, KIND_NORMAL, KIND_UNIFORM, KIND_KDE = 0, 1, 2, 3     # include/poreseg.h ps_hmm_model.kind
KIND_VECTOR = 4                                       # ... kind: a state of n_dim components (a vector model)
KIND_LOGNORMAL, KIND_EXPONENTIAL = 5, 6               # ps_hmm_model.comp_kind, beside KIND_NORMAL and KIND_UNIFORM
COMPONENT_KINDS = (KIND_NORMAL, KIND_UNIFORM, KIND_LOGNORMAL, KIND_EXPONENTIAL)
KIND_MIXTURE = 7                                      # ... kind: a weighted choice between components (scalar models)
MAX_STATES = 4096                                     # csrc/seg_hmm.hpp HMM_S_MAX
MAX_DIM = 16                                          # csrc/seg_hmm.hpp HMM_D_MAX


def _rng(rng):
    return np.random.default_rng() if rng is None else rng


class Distribution(object):
    """Base class of the emission distributions: `parameters` is the list of their arguments."""
    kind = None

    def __init__(self, parameters):
        self.parameters = list(parameters)
        self.frozen = False

    def freeze(self):
        """Model.train leaves a frozen distribution as it is."""
        self.frozen = True

    def thaw(self):
        self.frozen = False

    def log_probability(self, x):
        raise NotImplementedError

    def sample(self, rng=None):
        """One draw on the host (numpy; rng: a np.random.Generator, default a fresh np.random.default_rng())."""
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

    def sample(self, rng=None):
        mean, std = self.parameters
        return float(_rng(rng).normal(mean, std))

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

    def sample(self, rng=None):
        low, high = self.parameters
        return low + float(_rng(rng).random()) * (high - low)

    def compiled(self):
        low, high = self.parameters
        return low, high, -math.log(high - low)


class GaussianKernelDensity(Distribution):
    """log density -log(h sqrt(2 pi)) + log sum_i w_i exp(-(x - p_i)^2 / (2 h^2)) (module docstring): `points` p,
    `bandwidth` h > 0, `weights` w >= 0 (default: equal), normalised to sum to 1.  parameters = [points, bandwidth,
    weights]."""
    kind = KIND_KDE

    def __init__(self, points, bandwidth=1, weights=None):
        points = [float(p) for p in np.asarray(points, dtype=np.float64).reshape(-1)]
        if not points:
            raise ValueError("GaussianKernelDensity needs at least one point")
        if not all(math.isfinite(p) for p in points):
            raise ValueError("GaussianKernelDensity needs finite points")
        bandwidth = float(bandwidth)
        if not bandwidth > 0 or not math.isfinite(bandwidth):
            raise ValueError("GaussianKernelDensity needs a finite bandwidth > 0, got %r" % bandwidth)
        if weights is None:
            weights = [1.0] * len(points)
        weights = [float(w) for w in np.asarray(weights, dtype=np.float64).reshape(-1)]
        if len(weights) != len(points):
            raise ValueError("GaussianKernelDensity got %d weights for %d points" % (len(weights), len(points)))
        if not all(math.isfinite(w) and w >= 0 for w in weights):
            raise ValueError("GaussianKernelDensity needs finite weights >= 0")
        total = math.fsum(weights)
        if not total > 0:
            raise ValueError("GaussianKernelDensity needs some weight > 0")
        Distribution.__init__(self, [points, bandwidth, [w / total for w in weights]])

    def tables(self):
        """(points, log weights) of the points with weight > 0, in order: what the flat form holds."""
        points, _, weights = self.parameters
        keep = [(p, math.log(w)) for p, w in zip(points, weights) if w > 0]
        return [p for p, _ in keep], [lw for _, lw in keep]

    def log_probability(self, x):
        _, h, _ = self.parameters
        b = 1.0 / (2.0 * h * h)
        m, r = NEG_INF, 0.0                     # the device's HmmLse: m the largest term so far, r the others' sum
        for p, lw in zip(*self.tables()):
            d = x - p
            v = lw - (d * d) * b
            if not v > NEG_INF:
                continue
            if v > m:
                r = (r + 1.0) * math.exp(m - v)
                m = v
            else:
                r += math.exp(v - m)
        if not m > NEG_INF:
            return NEG_INF
        return -(math.log(h) + _LOG_SQRT_2PI) + (m + math.log1p(r))

    def sample(self, rng=None):
        """A point chosen by its weight, then a normal of the bandwidth around it."""
        points, h, weights = self.parameters
        rng = _rng(rng)
        return float(rng.normal(points[int(rng.choice(len(points), p=np.asarray(weights) / math.fsum(weights)))], h))

    def compiled(self):
        points, h, weights = self.parameters
        return (math.fsum(p * w for p, w in zip(points, weights)), 1.0 / (2.0 * h * h), -(math.log(h) + _LOG_SQRT_2PI))


class LogNormalDistribution(Distribution):
    """log density, with y = log x:  (-log(sigma sqrt(2 pi)) - (y - mu)^2 / (2 sigma^2)) - y  for x > 0, -inf otherwise.
    A state with it makes its model a vector model (module docstring)."""
    kind = KIND_LOGNORMAL

    def __init__(self, mu, sigma):
        mu, sigma = float(mu), float(sigma)
        if not math.isfinite(mu):
            raise ValueError("LogNormalDistribution needs a finite mu, got %r" % mu)
        if not sigma > 0 or not math.isfinite(sigma):
            raise ValueError("LogNormalDistribution needs a finite sigma > 0, got %r" % sigma)
        Distribution.__init__(self, [mu, sigma])

    def log_probability(self, x):
        if not x > 0:
            return NEG_INF
        mu, sigma = self.parameters
        y = math.log(x)
        return (-math.log(sigma) - _LOG_SQRT_2PI - (y - mu) ** 2 / (2 * sigma * sigma)) - y

    def sample(self, rng=None):
        mu, sigma = self.parameters
        return float(_rng(rng).lognormal(mu, sigma))

    def compiled(self):
        mu, sigma = self.parameters
        return mu, 1.0 / (2.0 * sigma * sigma), -(math.log(sigma) + _LOG_SQRT_2PI)


class ExponentialDistribution(Distribution):
    """log density log(rate) - rate x for x >= 0, -inf otherwise.  A state with it makes its model a vector model."""
    kind = KIND_EXPONENTIAL

    def __init__(self, rate):
        rate = float(rate)
        if not rate > 0 or not math.isfinite(rate):
            raise ValueError("ExponentialDistribution needs a finite rate > 0, got %r" % rate)
        Distribution.__init__(self, [rate])

    def log_probability(self, x):
        rate, = self.parameters
        return math.log(rate) - rate * x if x >= 0 else NEG_INF

    def sample(self, rng=None):
        rate, = self.parameters
        return float(_rng(rng).exponential(1.0 / rate))

    def compiled(self):
        rate, = self.parameters
        return 0.0, rate, math.log(rate)


class MultivariateDistribution(Distribution):
    """D >= 1 independent univariate components (NormalDistribution, UniformDistribution, LogNormalDistribution or
    ExponentialDistribution), each with a weight w_d, finite and > 0 (default 1): the log density of a length-D observation
    is  w_0 l_0(x_0) + w_1 l_1(x_1) + ...,  added in ascending d from the first product, so one component of weight 1 gives
    that component's own bits.  parameters = [distributions, weights].  A GaussianKernelDensity or another
    MultivariateDistribution as a component raises ValueError.  freeze() freezes every component with it."""
    kind = KIND_VECTOR

    def __init__(self, distributions, weights=None):
        distributions = list(distributions)
        if not distributions:
            raise ValueError("MultivariateDistribution needs at least one component")
        for d in distributions:
            if isinstance(d, MultivariateDistribution):
                raise ValueError("a MultivariateDistribution cannot be a component of another")
            if isinstance(d, GaussianKernelDensity):
                raise ValueError("a GaussianKernelDensity cannot be a component of a MultivariateDistribution")
            if isinstance(d, MixtureDistribution):
                raise ValueError("a MixtureDistribution cannot be a component of a MultivariateDistribution: mixture "
                                 "states stand in scalar models only")
            if not isinstance(d, Distribution) or d.kind not in COMPONENT_KINDS:
                raise ValueError("a component must be a Normal, Uniform, LogNormal or ExponentialDistribution, got %r"
                                 % (d,))
        if weights is None:
            weights = [1.0] * len(distributions)
        weights = [float(w) for w in np.asarray(weights, dtype=np.float64).reshape(-1)]
        if len(weights) != len(distributions):
            raise ValueError("MultivariateDistribution got %d weights for %d components"
                             % (len(weights), len(distributions)))
        if not all(math.isfinite(w) and w > 0 for w in weights):
            raise ValueError("MultivariateDistribution needs finite weights > 0")
        Distribution.__init__(self, [distributions, weights])

    def log_probability(self, x):
        distributions, weights = self.parameters
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size != len(distributions):
            raise ValueError("an observation of %d values for %d components" % (x.size, len(distributions)))
        total = None
        for d, w, v in zip(distributions, weights, x.tolist()):
            term = w * d.log_probability(v)
            total = term if total is None else total + term
        return total

    def sample(self, rng=None):
        """One draw per component, independently, as a list; the weights are ignored, as in yahmm (a weight scales a log
        density and defines no distribution to draw from)."""
        rng = _rng(rng)
        return [d.sample(rng) for d in self.parameters[0]]


class MixtureDistribution(Distribution):
    """One state whose level is a weighted choice between J >= 1 univariate components (NormalDistribution,
    UniformDistribution, LogNormalDistribution or ExponentialDistribution) with `weights` w_j, finite and >= 0 with a sum
    > 0 (default: equal), normalised to sum to 1: log density  log sum_j w_j p_j(x)  (module docstring).  parameters =
    [distributions, weights].  A component of weight 0 keeps its slot -- component index equals table index -- and is
    skipped.  A GaussianKernelDensity, MultivariateDistribution or MixtureDistribution as a component raises ValueError.
    Scalar models only.  freeze() freezes the weights and, in this slot, every component; Model.train fits both."""
    kind = KIND_MIXTURE

    def __init__(self, distributions, weights=None):
        distributions = list(distributions)
        if not distributions:
            raise ValueError("MixtureDistribution needs at least one component")
        for d in distributions:
            if isinstance(d, MixtureDistribution):
                raise ValueError("a MixtureDistribution cannot be a component of another")
            if isinstance(d, (GaussianKernelDensity, MultivariateDistribution)):
                raise ValueError("a %s cannot be a component of a MixtureDistribution" % type(d).__name__)
            if not isinstance(d, Distribution) or d.kind not in COMPONENT_KINDS:
                raise ValueError("a component must be a Normal, Uniform, LogNormal or ExponentialDistribution, got %r"
                                 % (d,))
        if weights is None:
            weights = [1.0] * len(distributions)
        weights = [float(w) for w in np.asarray(weights, dtype=np.float64).reshape(-1)]
        if len(weights) != len(distributions):
            raise ValueError("MixtureDistribution got %d weights for %d components" % (len(weights), len(distributions)))
        if not all(math.isfinite(w) and w >= 0 for w in weights):
            raise ValueError("MixtureDistribution needs finite weights >= 0")
        total = math.fsum(weights)
        if not total > 0:
            raise ValueError("MixtureDistribution needs some weight > 0")
        Distribution.__init__(self, [distributions, [w / total for w in weights]])

    def log_weights(self):
        """log w_j per component, -inf for a weight of 0: the table mix_lw."""
        return [math.log(w) if w > 0 else NEG_INF for w in self.parameters[1]]

    def _terms(self, x):
        """log w_j + l_j(x) per component; -inf for a component of weight 0, whatever its density."""
        return [lw + d.log_probability(x) if lw > NEG_INF else NEG_INF
                for d, lw in zip(self.parameters[0], self.log_weights())]

    def log_probability(self, x):
        m, r = NEG_INF, 0.0                     # the device's HmmLse: m the largest term so far, r the others' sum
        for v in self._terms(x):
            if not v > NEG_INF:
                continue
            if v > m:
                r = (r + 1.0) * math.exp(m - v)
                m = v
            else:
                r += math.exp(v - m)
        if not m > NEG_INF:
            return NEG_INF
        return m + math.log1p(r)

    def responsibilities(self, x):
        """exp((log w_j + l_j(x)) - log_probability(x)) per component, 0 for a skipped term; all 0 where the density is
        -inf.  What Viterbi training shares an observation out by."""
        e = self.log_probability(x)
        if not e > NEG_INF:
            return [0.0] * len(self.parameters[0])
        return [math.exp(v - e) if v > NEG_INF else 0.0 for v in self._terms(x)]

    def sample(self, rng=None):
        """A component chosen by its weight, then that component's draw."""
        distributions, weights = self.parameters
        rng = _rng(rng)
        return distributions[int(rng.choice(len(distributions), p=np.asarray(weights) / math.fsum(weights)))].sample(rng)

    def compiled(self):
        return 0.0, 0.0, 0.0                    # (the state's triple is not read: the components' live in Model._mix)


def _mixture_slots(distribution):
    """[(component distribution, weight, frozen)] of a mixture state's distribution, [] for any other."""
    if distribution.kind != KIND_MIXTURE:
        return []
    return [(d, w, d.frozen or distribution.frozen) for d, w in zip(*distribution.parameters)]


def _components(distribution):
    """[(component distribution, weight, frozen)] of an emitting state's distribution: its own components, or itself."""
    if distribution.kind == KIND_VECTOR:
        return [(d, w, d.frozen or distribution.frozen) for d, w in zip(*distribution.parameters)]
    return [(distribution, 1.0, distribution.frozen)]


def _sample_param(d):
    """The two doubles ps_hmm_sample draws component d from (include/poreseg.h ps_hmm_sample_tables.emit_param)."""
    a = d.parameters
    if d.kind == KIND_UNIFORM:
        return a[0], a[1] - a[0]
    if d.kind == KIND_EXPONENTIAL:
        return 0.0, a[0]
    if d.kind == KIND_KDE:
        return 0.0, a[1]
    if d.kind == KIND_MIXTURE:
        return 0.0, 0.0                                   # (its components' pairs are Model._mix["mix_draw"])
    return a[0], a[1]                                     # normal (mean, std), log-normal (mu, sigma)


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
        self._pseudo = {}                                  # (from, to) -> pseudocount (train(use_pseudocount=True))
        self.states = None                                 # after bake()
        self.n_dim = None                                  # after bake(): values per observation
        self._flat = None
        self._mix = None                                   # after bake(): the mixture states' tables (_mixture_tables)
        self._c = None                                     # the ctypes view of _flat and _mix, made on first use
        self._s = None                                     # the sampling tables (_sample_tables), made on first use
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

    def add_transition(self, a, b, probability, pseudocount=None):
        """An edge a -> b (states not yet in the model join it).  A second call for the same pair replaces the first.
        pseudocount: what train(use_pseudocount=True) adds to the edge's expected count (default: `probability`)."""
        p = float(probability)
        if p < 0 or math.isnan(p):
            raise ValueError("transition probability must be >= 0, got %r" % probability)
        c = p if pseudocount is None else float(pseudocount)
        if c < 0 or math.isnan(c):
            raise ValueError("pseudocount must be >= 0, got %r" % pseudocount)
        self.add_state(a)
        self.add_state(b)
        self._edges[(a, b)] = p
        self._pseudo[(a, b)] = c
        self._flat = None

    def add_model(self, other):
        """The other model's states and edges join this one; its start and end become ordinary silent states."""
        for s in other._added:
            self.add_state(s)
        for (a, b), p in other._edges.items():
            self._edges[(a, b)] = p
            self._pseudo[(a, b)] = other._pseudo.get((a, b), p)
        self._flat = None

    # ---- bake ---------------------------------------------------------------------------------------------------
    def bake(self, verbose=False, merge=None):
        """Normalises each state's out-edges to sum to 1, drops the states `start` cannot reach (never `end`), rejects a
        cycle of silent states (ValueError), orders `states` -- emitting states by name (stable), then silent states in
        topological order (by level, then in the order they joined) -- and compiles the flat form the device reads.
        merge: None / 'none' (the default: nothing is merged), 'partial' or 'all' (any letter case): silent states with one
        way out are folded into their successor first (_merge_silent, module docstring); anything else raises ValueError."""
        mode = "none" if merge is None else str(merge).lower()
        if mode not in ("none", "partial", "all"):
            raise ValueError("merge must be None, 'none', 'partial' or 'all', got %r" % (merge,))
        if mode != "none":
            self._merge_silent(mode == "partial")
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
        self.n_dim, vector = self._dimension(emitting)
        kind = np.zeros(S, np.int32)
        for k, s in enumerate(emitting):
            kind[k] = KIND_VECTOR if vector else s.distribution.kind
        param, kde = self._emission_tables(emitting, S, self.n_dim if vector else 0)
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
            finite=int(self.finite), n_dim=self.n_dim, kind=kind, level_ptr=level_ptr, param=param,
            in_ptr=np.concatenate(([0], np.cumsum(np.bincount(dst, minlength=S)))).astype(np.int32),
            in_src=np.ascontiguousarray(src[by_dst]), in_lp=np.ascontiguousarray(lp[by_dst]),
            out_ptr=np.concatenate(([0], np.cumsum(np.bincount(src, minlength=S)))).astype(np.int32),
            out_dst=np.ascontiguousarray(dst[by_src]), out_lp=np.ascontiguousarray(lp[by_src]), **kde)
        self._mix = self._mixture_tables(emitting)
        self._in_order = by_dst                         # edges (= out-edge order) -> in-edge order
        self._c = self._s = None

    def _merge_silent(self, silent_only):
        """bake(merge='partial' | 'all'): rewrites the construction graph (_added, _edges, _pseudo).  Repeated until no
        state qualifies: the first state a, in joining order, that is silent, neither start nor end, and has exactly one
        out-edge of positive probability, a -> b with b != a (silent_only: b silent as well), leaves the model; every
        in-edge x -> a becomes x -> b, its probability and pseudocount added to an x -> b already there."""
        pos = {s: i for i, s in enumerate(self._added)}
        succ = {s: collections.OrderedDict() for s in self._added}      # out-edges, those of probability 0 too
        pred = {s: collections.OrderedDict() for s in self._added}
        for a, b in self._edges:
            succ[a][b] = pred[b][a] = None
        gone = set()
        i = 0
        while i < len(self._added):
            a = self._added[i]
            i += 1
            if a in gone or not a.is_silent() or a is self.start or a is self.end:
                continue
            live = [b for b in succ[a] if self._edges[(a, b)] > 0]
            if len(live) != 1 or live[0] is a or (silent_only and not live[0].is_silent()):
                continue
            b = live[0]
            for x in pred[a]:
                p, c = self._edges.pop((x, a)), self._pseudo.pop((x, a), None)
                del succ[x][a]
                if x is a:
                    continue
                c = p if c is None else c
                if (x, b) in self._edges:
                    c += self._pseudo.get((x, b), self._edges[(x, b)])
                    p += self._edges[(x, b)]
                self._edges[(x, b)], self._pseudo[(x, b)] = p, c
                succ[x][b] = pred[b][x] = None
                i = min(i, pos[x])                       # x may qualify now: the scan goes back to it
            for y in succ[a]:
                del self._edges[(a, y)], pred[y][a]
                self._pseudo.pop((a, y), None)
            gone.add(a)
        self._added = [s for s in self._added if s not in gone]
        self._known = {id(s) for s in self._added}

    def _dimension(self, emitting):
        """(n_dim, vector): the one dimension of the emitting states' distributions (ValueError when they differ; 1 without
        emitting states), and whether the model is a vector model -- some state is a MultivariateDistribution, log-normal or
        exponential -- which cannot hold a kernel-density state (ValueError)."""
        dims = sorted({len(_components(s.distribution)) for s in emitting}) or [1]
        if len(dims) > 1:
            raise ValueError("model %r: every emitting state must have the same dimension, got %s"
                             % (self.name, ", ".join(str(d) for d in dims)))
        vector = any(s.distribution.kind in (KIND_VECTOR, KIND_LOGNORMAL, KIND_EXPONENTIAL) for s in emitting)
        if vector and dims[0] > MAX_DIM:
            raise ValueError("model %r has %d components per state: the device HMM kernels take at most %d"
                             % (self.name, dims[0], MAX_DIM))
        for s in emitting:
            if vector and s.distribution.kind == KIND_MIXTURE:
                raise ValueError("model %r: mixture state %r cannot stand in a vector model (one with a Multivariate, "
                                 "LogNormal or ExponentialDistribution state)" % (self.name, s.name))
        if vector and any(s.distribution.kind == KIND_KDE for s in emitting):
            raise ValueError("model %r: a kernel-density state cannot stand in a vector model (one with a Multivariate, "
                             "LogNormal or ExponentialDistribution state)" % self.name)
        return dims[0], vector

    @staticmethod
    def _emission_tables(emitting, S, vector_dim=0):
        """param[3 S], the kernel-density CSR tables (kde_ptr[n_emit + 1] into kde_pt / kde_lw: the points and log
        weights of the kind-3 states, zero-weight points left out) and the component tables comp_kind / comp_param /
        comp_w (n_emit * vector_dim components; empty unless the model is a vector model, whose param stays 0)."""
        param = np.zeros(3 * S, np.float64)
        ptr, pts, lws = [0], [], []
        ckind, cparam, cw = [], [], []
        for k, s in enumerate(emitting):
            if vector_dim:
                for d, w, _ in _components(s.distribution):
                    ckind.append(d.kind)
                    cparam.extend(d.compiled())
                    cw.append(w)
            else:
                param[3 * k:3 * k + 3] = s.distribution.compiled()
                if s.distribution.kind == KIND_KDE:
                    p, lw = s.distribution.tables()
                    pts.extend(p)
                    lws.extend(lw)
            ptr.append(len(pts))
        return param, dict(kde_ptr=np.array(ptr, np.int32), kde_pt=np.array(pts, np.float64).reshape(-1),
                           kde_lw=np.array(lws, np.float64).reshape(-1), comp_kind=np.array(ckind, np.int32).reshape(-1),
                           comp_param=np.array(cparam, np.float64).reshape(-1), comp_w=np.array(cw, np.float64).reshape(-1))

    @staticmethod
    def _mixture_tables(emitting):
        """The tables of the mixture states (kind 7), kept beside `flat` (include/poreseg.h ps_hmm_model mix_*): mix_ptr
        [n_emit + 1], a CSR index into the others (a kind-7 state has >= 1 entries, every other state none); per component
        mix_kind, mix_param (its compiled() triple), mix_lw (log weight, -inf for weight 0) and the two sampling tables:
        mix_cdf, per state the running sum of the weights, added one by one, with the entry of the state's last component
        of positive weight and every entry after it stored as exactly 1.0, and mix_draw, the _sample_param pair.  All
        empty (mix_ptr all 0) without mixture states."""
        ptr, kinds, params, lws, cdf, draw = [0], [], [], [], [], []
        for s in emitting:
            slots = _mixture_slots(s.distribution)
            if slots:
                lws.extend(s.distribution.log_weights())
                last = max(j for j, (_, w, _) in enumerate(slots) if w > 0)
                run = 0.0
                for j, (d, w, _) in enumerate(slots):
                    kinds.append(d.kind)
                    params.extend(d.compiled())
                    draw.extend(_sample_param(d))
                    run = run + w
                    cdf.append(1.0 if j >= last else run)
            ptr.append(len(kinds))
        return dict(mix_ptr=np.array(ptr, np.int32), mix_kind=np.array(kinds, np.int32).reshape(-1),
                    mix_param=np.array(params, np.float64).reshape(-1), mix_lw=np.array(lws, np.float64).reshape(-1),
                    mix_cdf=np.array(cdf, np.float64).reshape(-1), mix_draw=np.array(draw, np.float64).reshape(-1))

    @property
    def _n_mix(self):
        """Mixture components of the baked model: the rows `stats` holds behind the states'."""
        self.flat
        return int(self._mix["mix_kind"].size)

    @property
    def _vector(self):
        """The baked model is a vector model: its emitting states are kind 4 and read the component tables."""
        return bool(self.flat["comp_kind"].size)

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
            if f["kde_pt"].size:                                # (read by the library only when some kind is 3)
                for k in ("kde_ptr", "kde_pt", "kde_lw"):
                    setattr(m, k, f[k].ctypes.data)
            m.n_dim = f["n_dim"]
            if f["comp_kind"].size:                             # (read by the library only when some kind is 4)
                for k in ("comp_kind", "comp_param", "comp_w"):
                    setattr(m, k, f[k].ctypes.data)
            if self._mix["mix_kind"].size:                      # (read by the library only when some kind is 7)
                for k, a in self._mix.items():
                    setattr(m, k, a.ctypes.data)
            self._c = m
        return self._c

    # ---- inference on the device ---------------------------------------------------------------------------------
    def _sequences(self, sequences):
        """The sequences as contiguous float64 arrays: 1-D for n_dim = 1, (n, n_dim) for a vector model of n_dim > 1 (a
        list of tuples; [] is the empty sequence).  A vector model of n_dim = 1 takes (n, 1) as well."""
        D = self.flat["n_dim"]
        seqs = [np.ascontiguousarray(s, dtype=np.float64) for s in sequences]
        for i, s in enumerate(seqs):
            if D == 1:
                if s.ndim == 2 and s.shape[1] == 1 and self._vector:
                    seqs[i] = s.reshape(-1)
                elif s.ndim != 1:
                    raise ValueError("an observation sequence must be 1-D, got shape %r" % (s.shape,))
            elif s.ndim == 1 and s.size == 0:
                seqs[i] = s.reshape(0, D)
            elif s.ndim != 2 or s.shape[1] != D:
                raise ValueError("an observation sequence of a model with n_dim = %d must have shape (n, %d), got %r"
                                 % (D, D, s.shape))
        return seqs

    def _upload(self, sequences, device):
        import torch
        from . import engine
        f = self.flat
        seqs = self._sequences(sequences)
        if f["n_states"] > MAX_STATES:
            raise ValueError("model %r has %d states: the device HMM kernels take at most %d" % (self.name, f["n_states"], MAX_STATES))
        ctx = engine.context(device)
        off = np.concatenate(([0], np.cumsum([s.shape[0] for s in seqs]))).astype(np.int64)
        obs = np.concatenate([s.reshape(-1) for s in seqs]) if off[-1] else np.zeros(1, np.float64)
        obs = torch.from_numpy(obs).to(torch.device("cuda", ctx.device))
        return ctx, off, obs

    def _run(self, sequences, mode, want_mat, device=None):
        ctx, off, obs = self._upload(sequences, device)
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

    # ---- sampling ---------------------------------------------------------------------------------------------------
    def _sample_tables(self):
        """What ps_hmm_sample reads beside the model (module docstring, Sampling), built in float64 from the distributions
        and `flat` and cached beside the ctypes view: dict(out_cdf, emit_param, kde_cdf, c: the _lib.HmmSampleTables)."""
        from . import _lib
        f = self.flat
        if self._s is None:
            def cdf(lw, ptr):
                p, out = np.exp(lw), np.zeros(lw.size, np.float64)
                for k in range(ptr.size - 1):
                    run, last = 0.0, int(ptr[k + 1]) - 1           # last: the row's last entry of positive probability
                    for e in range(int(ptr[k]), int(ptr[k + 1])):
                        run = run + float(p[e])                # (added one by one, in edge order)
                        out[e] = run
                    while last > ptr[k] and not p[last] > 0:
                        last -= 1
                    if ptr[k + 1] > ptr[k]:
                        out[last:ptr[k + 1]] = 1.0             # (an entry of probability 0 behind it is never picked)
                return out
            emit = []
            for s in self.states[:f["n_emit"]]:
                for d, _, _ in (_components(s.distribution) if self._vector else [(s.distribution, 1.0, False)]):
                    emit.extend(_sample_param(d))
            t = dict(out_cdf=cdf(f["out_lp"], f["out_ptr"]), emit_param=np.array(emit, np.float64).reshape(-1),
                     kde_cdf=cdf(f["kde_lw"], f["kde_ptr"]))
            c = _lib.HmmSampleTables()
            for k, count in (("out_cdf", "n_cdf"), ("emit_param", "n_param"), ("kde_cdf", "n_kde")):
                setattr(c, k, t[k].ctypes.data if t[k].size else None)
                setattr(c, count, t[k].size)
            t["c"] = c
            self._s = t
        return self._s

    def sample_batch(self, n, length=0, path=False, seed=0, first=0, max_length=1000000, device=None):
        """n sequences sampled from the model on the device (ps_hmm_sample, module docstring): a list of float64 arrays,
        (len,) for n_dim = 1 and (len, n_dim) for a vector model of n_dim > 1; with path=True also the list of their paths in
        viterbi's format, [(index into `states`, state)] from `start` to the last state visited, silent states included.
        length = 0: every walk runs until it enters `end` (ValueError for an infinite model); length > 0: until `end` or
        `length` emissions, whichever comes first.  seed: an integer (taken modulo 2^64) makes the call reproducible bit
        for bit; None draws one from os.urandom.  first: the index of the batch's first sequence in the random stream:
        sample_batch(a + b, seed=s) == sample_batch(a, seed=s) + sample_batch(b, seed=s, first=a).  A walk that has made
        max_length emissions without ending, or stands in a state without out-edges, stops there: one RuntimeWarning per
        call says how many."""
        import warnings
        from . import engine
        f = self.flat
        n, length, first, max_length = int(n), int(length), int(first), int(max_length)
        if n < 0 or length < 0 or first < 0:
            raise ValueError("n, length and first must be >= 0, got %d, %d, %d" % (n, length, first))
        if max_length < 1:
            raise ValueError("max_length must be >= 1, got %d" % max_length)
        if not f["finite"] and length == 0:
            raise ValueError("model %r is infinite (no edge into end): must specify a length" % self.name)
        if f["n_states"] > MAX_STATES:
            raise ValueError("model %r has %d states: the device HMM kernels take at most %d" % (self.name, f["n_states"], MAX_STATES))
        if seed is None:
            import os
            seed = int.from_bytes(os.urandom(8), "little")
        tables = self._sample_tables()
        ctx = engine.context(device)
        _, obs, off, lens, flags, paths = ctx.hmm_sample(self._c_model(), tables["c"], int(seed), first, n, length, max_length,
                                                         want_path=bool(path))
        obs, lens, flags = obs.cpu().numpy(), lens.cpu().numpy(), flags.cpu().numpy()
        if f["n_dim"] == 1:
            obs = obs.reshape(-1)
        seqs = [obs[off[q]:off[q] + lens[q]].copy() for q in range(n)]
        cut, dead = int(np.count_nonzero(flags == 1)), int(np.count_nonzero(flags == 2))
        if cut or dead:
            warnings.warn("model %r: %d of %d sampled sequences are truncated (%d stopped at max_length = %d, %d in a state "
                          "without out-edges)" % (self.name, cut + dead, n, cut, max_length, dead), RuntimeWarning, stacklevel=2)
        if not path:
            return seqs
        p, p_off, p_len = paths[0].cpu().numpy(), paths[1], paths[2].cpu().numpy()
        return seqs, [[(int(i), self.states[i]) for i in p[p_off[q]:p_off[q] + p_len[q]]] for q in range(n)]

    def sample(self, length=0, path=False, seed=None):
        """One sequence sampled from the model, as a plain list (of lists for a vector model of n_dim > 1), or (list, path)
        with path=True: sample_batch(1, ...)[0]."""
        out = self.sample_batch(1, length=length, path=path, seed=seed)
        return (out[0][0].tolist(), out[1][0]) if path else out[0].tolist()

    # ---- posterior decoding ---------------------------------------------------------------------------------------
    def maximum_a_posteriori_batch(self, sequences, device=None):
        """[(logp, path) per sequence] by posterior decoding on the device (ps_hmm_posterior, module docstring): path =
        [(index into `states`, state)] with one entry per observation -- the emitting state of the largest posterior, the
        lowest index on a tie; emitting states only -- and logp = the sum of those log posteriors.  An impossible
        sequence gives (-inf, None), an empty one (0.0, []).  Only the MAP states and their sums leave the device."""
        ctx, off, obs = self._upload(sequences, device)
        seq_logp, _, state, logp, _ = ctx.hmm_posterior(self._c_model(), obs, off, want_post=False, want_map=True)
        seq_logp, state, logp = seq_logp.cpu().numpy(), state.cpu().numpy(), logp.cpu().numpy()
        out = []
        for q in range(off.size - 1):
            if not seq_logp[q] > NEG_INF:
                out.append((NEG_INF, None))
                continue
            out.append((float(logp[q]), [(int(i), self.states[i]) for i in state[off[q]:off[q + 1]]]))
        return out

    def forward_backward_batch(self, sequences, device=None):
        """[(transitions, emissions) per sequence] (ps_hmm_posterior, module docstring): transitions = float64
        [len(states), len(states)], the expected count of every edge (from, to) in the sequence (not in log space; 0
        where there is no edge), scattered from the device's per-sequence row through `edges`; emissions = float64
        [n, n_emit], the log posterior of every emitting state per observation.  An impossible sequence has transitions
        0 and emissions -inf."""
        ctx, off, obs = self._upload(sequences, device)
        _, post, _, _, counts = ctx.hmm_posterior(self._c_model(), obs, off, want_post=True, want_map=False, want_counts=True)
        post, counts = post.cpu().numpy(), counts.cpu().numpy()
        S = len(self.states)
        src = np.array([e[0] for e in self.edges], np.int64).reshape(-1)
        dst = np.array([e[1] for e in self.edges], np.int64).reshape(-1)
        out = []
        for q in range(off.size - 1):
            transitions = np.zeros((S, S), np.float64)
            transitions[src, dst] = counts[q]
            out.append((transitions, post[off[q]:off[q + 1]]))
        return out

    def expected_transitions_batch(self, sequences, device=None):
        """float64 [n_seq, len(edges)]: every sequence's expected count of every edge, in the order of `edges` -- the
        numbers forward_backward_batch scatters into its dense arrays, from one ps_hmm_posterior call that asks for the
        counts alone (no posterior matrix on the device, no states x states array here).  An impossible sequence has a row
        of zeros."""
        ctx, off, obs = self._upload(sequences, device)
        _, _, _, _, counts = ctx.hmm_posterior(self._c_model(), obs, off, want_post=False, want_map=False, want_counts=True)
        return counts.cpu().numpy()

    def maximum_a_posteriori(self, sequence):
        return self.maximum_a_posteriori_batch([sequence])[0]

    def expected_transitions(self, sequence):
        return self.expected_transitions_batch([sequence])[0]

    def forward_backward(self, sequence):
        return self.forward_backward_batch([sequence])[0]

    # ---- training ------------------------------------------------------------------------------------------------
    def expected_counts_batch(self, sequences, device=None):
        """The Baum-Welch E-step on the device (ps_hmm_expect), summed over the sequences: Expectations(counts: float64
        per edge, aligned with `edges`; stats: float64 [n_emit, 3], (W, A, B) per emitting state -- for a vector model
        [n_emit, 1 + 2 n_dim]: W, then (A_d, B_d) per component; for a model with mixture states [n_emit + n_mix, 3]: the
        states' rows, then one (W, A, B) per mixture component in the order of _mix (module docstring);
        logp: float64 per sequence; skipped: the number of sequences with logp = -inf)."""
        ctx, off, obs = self._upload(sequences, device)
        width = self._stat_width
        logp, counts, stats, skipped = ctx.hmm_expect(self._c_model(), obs, off, width, mix_rows=self._n_mix)
        return Expectations(counts.cpu().numpy(), stats.cpu().numpy().reshape(-1, width), logp.cpu().numpy(), skipped)

    @property
    def _stat_width(self):
        """Statistics per emitting state: (W, A, B), or W and (A_d, B_d) per component of a vector model."""
        return 1 + 2 * self.flat["n_dim"] if self._vector else 3

    def _viterbi_counts(self, sequences, device=None):
        """Viterbi training's statistics (host counting on viterbi_batch's paths), as an Expectations."""
        f = self.flat
        S, NE = f["n_states"], f["n_emit"]
        src = np.array([e[0] for e in self.edges], np.int64)
        dst = np.array([e[1] for e in self.edges], np.int64)
        keys = src * S + dst                             # ascending: edges are sorted by (from, to)
        counts = np.zeros(len(self.edges))
        stats = np.zeros((NE + self._n_mix, self._stat_width))
        vector, D = self._vector, f["n_dim"]
        mixed = [k for k in range(NE) if f["kind"][k] == KIND_MIXTURE]
        if vector:                                       # per component: its shift, and whether it counts log x
            shift = f["comp_param"][0::3].reshape(NE, D)
            logs = f["comp_kind"].reshape(NE, D) == KIND_LOGNORMAL
            seqs = [x.reshape(-1, D) for x in self._sequences(sequences)]
        else:
            shift = f["param"][0:3 * NE:3]
            seqs = [np.asarray(x, dtype=np.float64) for x in sequences]
        res = self.viterbi_batch(seqs, device) if seqs else []
        logp = np.array([lp for lp, _ in res], np.float64)
        skipped = 0
        for (lp, path), x in zip(res, seqs):
            if path is None:
                skipped += 1
                continue
            idx = np.array([i for i, _ in path], np.int64)
            pk = idx[:-1] * S + idx[1:]
            np.add.at(counts, np.searchsorted(keys, pk), 1.0)
            em = idx[idx < NE]
            np.add.at(stats[:, 0], em, 1.0)
            if vector:
                with np.errstate(divide="ignore", invalid="ignore"):
                    y = np.where(logs[em], np.log(x), x)
                d = y - shift[em]
                for c in range(D):
                    np.add.at(stats[:, 1 + 2 * c], em, d[:, c])
                    np.add.at(stats[:, 2 + 2 * c], em, d[:, c] * d[:, c])
                continue
            d = x - shift[em]
            np.add.at(stats[:, 1], em, d)
            np.add.at(stats[:, 2], em, d * d)
            for k in mixed:                              # the component rows: each observation shared out on the host
                i0, dist = int(self._mix["mix_ptr"][k]), self.states[k].distribution
                for xv in x[em == k].tolist():
                    for j, r in enumerate(dist.responsibilities(xv)):
                        if r > 0:
                            i = i0 + j
                            y = math.log(xv) if self._mix["mix_kind"][i] == KIND_LOGNORMAL else xv
                            dv = y - float(self._mix["mix_param"][3 * i])
                            stats[NE + i] += (r, r * dv, (r * dv) * dv)
        return Expectations(counts, stats, logp, skipped)

    def _estep(self, sequences, algorithm, want_stats, device):
        """(logp per sequence, Expectations or None): the statistics only when want_stats (else a forward pass alone)."""
        if algorithm == "viterbi":
            est = self._viterbi_counts(sequences, device)
            return est.logp, est
        if want_stats:
            est = self.expected_counts_batch(sequences, device)
            return est.logp, est
        return (self.log_probability_batch(sequences, device) if len(sequences) else np.zeros(0)), None

    def _m_step(self, counts, stats, transition_pseudocount=0, use_pseudocount=False, edge_inertia=0.0,
                distribution_inertia=0.0, min_std=0.01):
        """New edge probabilities and distribution parameters from the E-step's statistics (module docstring); the flat
        arrays are derived again, so the next device call uploads the trained model."""
        f = self.flat
        S, NE = f["n_states"], f["n_emit"]
        counts = np.asarray(counts, np.float64).reshape(-1)
        width = self._stat_width
        stats = np.asarray(stats, np.float64)
        n_mix = self._n_mix
        if counts.size != len(self.edges) or stats.size != (NE + n_mix) * width:
            raise ValueError("statistics for %d edges and %d values of the emitting states, the model has %d edges and "
                             "%d emitting states and mixture components of %d values each"
                             % (counts.size, stats.size, len(self.edges), NE + n_mix, width))
        stats = stats.reshape(NE + n_mix, width)
        src = np.array([e[0] for e in self.edges], np.int64)
        old = np.array([e[2] for e in self.edges], np.float64)
        c = counts + float(transition_pseudocount)
        if use_pseudocount:
            c = c + np.array([self._pseudo.get((self.states[i], self.states[j]), self._edges.get((self.states[i], self.states[j]), 0.0))
                              for i, j, _ in self.edges], np.float64)
        total = np.bincount(src, weights=c, minlength=S) if src.size else np.zeros(S)
        tot = total[src]
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(tot > 0, c / np.where(tot > 0, tot, 1.0), old)
        new = edge_inertia * old + (1.0 - edge_inertia) * new
        self.edges = [(i, j, float(p)) for (i, j, _), p in zip(self.edges, new)]
        for i, j, p in self.edges:
            self._edges[(self.states[i], self.states[j])] = p
        # normal, log-normal and exponential distributions, pooled per distribution object over the states and component
        # slots that hold it (uniform and kernel-density distributions stay as they are)
        vector, D = self._vector, f["n_dim"]
        pooled = collections.OrderedDict()
        weights = collections.OrderedDict()              # per mixture object: [mixture, W_j pooled over its states]
        for k in range(NE):
            dist = self.states[k].distribution
            if dist.kind == KIND_MIXTURE:                # its slots' rows stand behind the states', in table order
                i0 = int(self._mix["mix_ptr"][k])
                rows = stats[NE + i0:NE + i0 + len(dist.parameters[0])]
                if not dist.frozen:
                    acc = weights.setdefault(id(dist), [dist, np.zeros(len(rows))])
                    acc[1] = acc[1] + rows[:, 0]
                for j, (d, _, frozen) in enumerate(_mixture_slots(dist)):
                    if d.kind not in (KIND_NORMAL, KIND_LOGNORMAL, KIND_EXPONENTIAL) or frozen:
                        continue
                    acc = pooled.setdefault(id(d), [d, self._mix["mix_param"][3 * (i0 + j)], 0.0, 0.0, 0.0])
                    acc[2:] = [acc[2] + rows[j, 0], acc[3] + rows[j, 1], acc[4] + rows[j, 2]]
                continue
            for c, (d, _, frozen) in enumerate(_components(dist)):
                if d.kind not in (KIND_NORMAL, KIND_LOGNORMAL, KIND_EXPONENTIAL) or frozen:
                    continue
                shift = f["comp_param"][3 * (k * D + c)] if vector else f["param"][3 * k]
                acc = pooled.setdefault(id(d), [d, shift, 0.0, 0.0, 0.0])
                acc[2:] = [acc[2] + stats[k, 0], acc[3] + stats[k, 1 + 2 * c], acc[4] + stats[k, 2 + 2 * c]]
        for dist, W in weights.values():                 # w_j = W_j / sum W, mixed with the old weight; a weight of 0 stays
            total = 0.0                                  # in its slot (log weight -inf)
            for w in W.tolist():
                total = total + w
            if total > 0:
                dist.parameters[1] = [min(distribution_inertia * old + (1.0 - distribution_inertia) * (w / total), 1.0)
                                      for old, w in zip(dist.parameters[1], W.tolist())]
        for d, shift, W, A, B in pooled.values():
            if not W > 0:
                continue
            if d.kind == KIND_EXPONENTIAL:               # (shift 0: A = sum g x)
                if A > 0:
                    d.parameters = [distribution_inertia * d.parameters[0] + (1.0 - distribution_inertia) * (W / A)]
                continue
            m = A / W                                    # (of log x for a log-normal: mu and sigma)
            mean = shift + m
            std = max(math.sqrt(max(B / W - m * m, 0.0)), min_std)
            om, os_ = d.parameters
            d.parameters = [distribution_inertia * om + (1.0 - distribution_inertia) * mean,
                            distribution_inertia * os_ + (1.0 - distribution_inertia) * std]
        self._recompile()

    def _recompile(self):
        """The flat arrays again from `edges` and the distributions (same structure: states, levels and CSR lists)."""
        f = dict(self.flat)
        with np.errstate(divide="ignore"):
            lp = np.log(np.array([e[2] for e in self.edges], np.float64).reshape(-1))
        f["out_lp"] = np.ascontiguousarray(lp)
        f["in_lp"] = np.ascontiguousarray(lp[self._in_order])
        f["param"], tables = self._emission_tables(self.states[:f["n_emit"]], f["n_states"],
                                                   f["n_dim"] if self._vector else 0)
        f.update(tables)
        self._flat = f
        self._mix = self._mixture_tables(self.states[:f["n_emit"]])
        self._c = self._s = None

    def train(self, sequences, stop_threshold=1e-9, min_iterations=0, max_iterations=None, algorithm='baum-welch',
              verbose=True, transition_pseudocount=0, use_pseudocount=False, edge_inertia=0.0, distribution_inertia=0.0,
              min_std=0.01, device=None):
        """Trains the baked model on `sequences` (each a 1-D array of observations; (n, n_dim) for a vector model) and
        returns the total improvement of the summed log probability.  Each iteration is an E-step ('baum-welch': ps_hmm_expect on the device; 'viterbi':
        counts on viterbi_batch's paths) and the M-step of the module docstring.  The loop (sequences impossible under
        the starting model are left out of every sum):

            initial = sum logp;  improvement = inf;  it = 0;  total = 0
            while improvement > stop_threshold or it < min_iterations:
                if max_iterations is not None and it >= max_iterations: break
                E-step (from the previous pass), M-step;  trained = sum logp under the new model
                improvement = trained - initial;  total += improvement;  initial = trained;  it += 1

        printing "Training improvement: ..." per iteration and "Total Training Improvement: ..." at the end when verbose.
        The pass that measures `trained` is the next iteration's E-step, so N iterations make N + 1 passes; the last is a
        forward pass alone when max_iterations ends the loop."""
        algorithm = str(algorithm).lower()
        if algorithm not in ("baum-welch", "viterbi"):
            raise ValueError("algorithm must be 'baum-welch' or 'viterbi', got %r" % algorithm)
        if max_iterations is not None and (int(max_iterations) != max_iterations or max_iterations < 0):
            raise ValueError("max_iterations must be None or an integer >= 0, got %r" % (max_iterations,))
        if int(min_iterations) != min_iterations or min_iterations < 0:
            raise ValueError("min_iterations must be an integer >= 0, got %r" % (min_iterations,))
        for name, v in (("edge_inertia", edge_inertia), ("distribution_inertia", distribution_inertia)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
        if not float(transition_pseudocount) >= 0:
            raise ValueError("transition_pseudocount must be >= 0, got %r" % (transition_pseudocount,))
        if not float(min_std) > 0:
            raise ValueError("min_std must be > 0, got %r" % (min_std,))
        if isinstance(sequences, np.ndarray) and sequences.ndim == 1:
            raise ValueError("train takes a list of sequences, not one sequence")
        self.flat                                              # raises before bake()
        seqs = self._sequences(sequences)
        mstep = dict(transition_pseudocount=float(transition_pseudocount), use_pseudocount=bool(use_pseudocount),
                     edge_inertia=float(edge_inertia), distribution_inertia=float(distribution_inertia),
                     min_std=float(min_std))

        def wants_stats(done):
            return max_iterations is None or done < max_iterations

        logp, est = self._estep(seqs, algorithm, wants_stats(0), device)
        logp = np.asarray(logp, np.float64)
        possible = logp > NEG_INF
        if not possible.all():
            seqs = [x for x, ok in zip(seqs, possible) if ok]
        initial = float(np.sum(logp[possible]))
        improvement, it, total = float("inf"), 0, 0.0
        while improvement > stop_threshold or it < min_iterations:
            if max_iterations is not None and it >= max_iterations:
                break
            self._m_step(est.counts, est.stats, **mstep)
            logp, est = self._estep(seqs, algorithm, wants_stats(it + 1), device)
            trained = float(np.sum(logp))
            improvement = trained - initial
            total += improvement
            initial = trained
            it += 1
            if verbose:
                print("Training improvement: {}".format(improvement))
        if verbose:
            print("Total Training Improvement: {}".format(total))
        return total


Expectations = collections.namedtuple("Expectations", "counts stats logp skipped")


# ---- the reference's profile HMM builders (PyPore/hmm.py) -------------------------------------------------------------
# A board is an unbaked Model with n lanes: silent ports s1..sn on its left and e1..en on its right.  A lane of direction
# '>' runs from the previous board's e port into this board's s port, a lane '<' from this board's s port back into the
# previous board's e port.  Each module below is a table of (from, to, probability) read by _wire; the keys name the
# board's ports and the module's own states.
class HMMBoard(Model):
    """A Model "Board {name}" with silent ports s1..sn and e1..en (attributes; named b{name}s{i} and b{name}e{i}),
    `n`, and `directions`, '>' for every lane until the module says otherwise."""

    def __init__(self, n, name=None):
        Model.__init__(self, name="Board {}".format(name))
        self.directions = ['>'] * n
        self.n = n
        for i in range(1, n + 1):
            for side in "se":
                port = State(None, name="b{}{}{}".format(name, side, i))
                setattr(self, "{}{}".format(side, i), port)
                self.add_state(port)


def _wire(board, states, table):
    """add_transition for every row of a module's table; a key is a port of the board or a key of `states`."""
    def find(key):
        return states[key] if key in states else getattr(board, key)
    for a, b, p in table:
        board.add_transition(find(a), find(b), p)
    return board


_GLOBAL_TABLE = (
    ("s1", "D", 1.00), ("s2", "M", 1.00),
    ("M", "e2", 0.90), ("M", "e1", 0.05), ("M", "I", 0.05),
    ("D", "I", 0.15), ("D", "e1", 0.15), ("D", "e2", 0.70),
    ("I", "I", 0.70), ("I", "e1", 0.15), ("I", "e2", 0.15))

_NANOPORE_TABLE = (
    ("s1", "D", 1.0), ("s2", "M", 1.0), ("e3", "B", 1.0),
    ("B", "M", 0.85), ("B", "s3", 0.15),
    ("D", "e1", 0.1), ("D", "e2", 0.8), ("D", "I", 0.1),
    ("M", "s3", 0.033), ("M", "M", 0.4), ("M", "e2", 0.5), ("M", "I", 0.033), ("M", "e1", 0.34),
    ("I", "I", 0.50), ("I", "M", 0.20), ("I", "e1", 0.05), ("I", "e2", 0.25))

_PHI29_MATCH_TABLE = (
    ("start", "M", 0.95), ("start", "MO", 0.05),
    ("M", "M", 0.10), ("M", "end", 0.90),
    ("MO", "MO", 0.80), ("MO", "end", 0.20))

_PHI29_TABLE = (
    ("s1", "D", 1.00), ("s2", "M.start", 1.00), ("e3", "ME", 1.00), ("s4", "MS", 1.00),
    ("e5", "M.start", 0.90), ("e5", "ME", 0.05), ("e5", "s5", 0.05),
    ("D", "e1", 0.1), ("D", "I", 0.1), ("D", "e2", 0.8),
    ("I", "M.start", 0.10), ("I", "I", 0.50), ("I", "e1", 0.05), ("I", "e2", 0.35),
    ("M.end", "I", 0.01), ("M.end", "e1", 0.01), ("M.end", "e2", 0.97), ("M.end", "s5", 0.01),
    ("MS", "s3", 0.80), ("MS", "MS", 0.20),
    ("ME", "e2", 0.10), ("ME", "ME", 0.10), ("ME", "e4", 0.80))


def GlobalAlignmentModule(distribution, name, insert):
    """The repeating unit of a global alignment profile: two lanes (1 delete, 2 match), states D:, I: and M:."""
    board = HMMBoard(2, name)
    states = collections.OrderedDict((("D", State(None, name="D:{}".format(name))),
                                      ("I", State(insert, name="I:{}".format(name))),
                                      ("M", State(distribution, name="M:{}".format(name)))))
    return _wire(board, states, _GLOBAL_TABLE)


def NanoporeGlobalAlignmentModule(distribution, name, insert):
    """The global alignment unit with a match self-loop, a way from the insert back to the match, and a third lane that
    runs backwards through the silent backslip state B:."""
    board = HMMBoard(3, name)
    board.directions = ['>', '>', '<']
    states = collections.OrderedDict((("I", State(insert, name="I:{}".format(name))),
                                      ("M", State(distribution, name="M:{}".format(name))),
                                      ("D", State(None, name="D:{}".format(name))),
                                      ("B", State(None, name="B:{}".format(name)))))
    return _wire(board, states, _NANOPORE_TABLE)


def Phi29GlobalAlignmentModule(distribution, name, insert=UniformDistribution(0, 90)):
    """One position of a Phi29 profile on five lanes: 1 delete and 2 match forwards, 3 and 5 backwards (backslips), 4
    forwards again after a backslip.  The match is a sub-model of M: and MO: (an oversegmented match: a long self-loop);
    MS: and ME: are the match entered on the way back and left on the way forward again; D: and I: as usual."""
    match = Model(name=str(name))
    inner = {"start": match.start, "end": match.end, "M": State(distribution, name="M:{}".format(name)),
             "MO": State(distribution, name="MO:{}".format(name))}
    match.add_states([inner["M"], inner["MO"]])
    _wire(match, inner, _PHI29_MATCH_TABLE)

    board = HMMBoard(n=5, name=str(name))
    board.directions = ['>', '>', '<', '>', '<']
    states = collections.OrderedDict((("D", State(None, name="D:{}".format(name))),
                                      ("I", State(insert, name="I:{}".format(name))),
                                      ("MS", State(distribution, name="MS:{}".format(name))),
                                      ("ME", State(distribution, name="ME:{}".format(name)))))
    board.add_model(match)
    board.add_states(list(states.values()))
    states["M.start"], states["M.end"] = match.start, match.end
    return _wire(board, states, _PHI29_TABLE)


def _join(model, left, right, forward, backward):
    """Lane by lane: '>' is left.e_j -> right.s_j with probability `forward`, '<' is right.s_j -> left.e_j with `backward`."""
    for j, d in zip(range(1, right.n + 1), right.directions):
        e, s = getattr(left, "e%d" % j), getattr(right, "s%d" % j)
        if d == '>':
            model.add_transition(e, s, forward)
        elif d == '<':
            model.add_transition(s, e, backward)


def ModularProfileModel(board_func, distributions, name, insert, merge=None):
    """A profile HMM of one board per entry of `distributions`, chained port to port and baked with bake(merge=merge).  An
    entry is a Distribution (board named by its 0-based position i) or a dict key -> Distribution, a fork: one board per
    key, named "{key}:{i+1}", side by side.  Into a fork of n branches the '>' lanes split 1/n each and the '<' lanes
    carry 1; out of it the '>' lanes carry 1 and the '<' lanes split 1/n; a fork after a fork joins equal keys.  Head:
    I:0 (`insert`, self-loop 0.70) -> s1 0.1, s2 0.2 of the first board; start -> I:0 0.02, s1 0.08, s2 0.90.  Tail: e1 and
    e2 of the last board -> end.  Every insert state shares the one `insert` object.  ValueError for an empty profile,
    a fork in the first or last position, and consecutive forks with different key lists."""
    distributions = list(distributions)
    if not distributions:
        raise ValueError("ModularProfileModel needs at least one distribution")
    if isinstance(distributions[0], dict) or isinstance(distributions[-1], dict):
        raise ValueError("a fork cannot be the first or the last position of a profile")
    model = Model(name)
    last = None                                            # the boards of the previous position
    for i, entry in enumerate(distributions):
        if isinstance(entry, Distribution):
            boards = [board_func(entry, name=i, insert=insert)]
        elif isinstance(entry, dict):
            if not entry:
                raise ValueError("position %d is a fork without branches" % i)
            if isinstance(distributions[i - 1], dict) and list(distributions[i - 1]) != list(entry):
                raise ValueError("consecutive forks need the same keys: %r at position %d, %r at %d"
                                 % (list(distributions[i - 1]), i - 1, list(entry), i))
            boards = [board_func(d, "{}:{}".format(key, i + 1), insert=insert) for key, d in entry.items()]
        else:
            raise TypeError("position %d holds neither a Distribution nor a dict: %r" % (i, entry))
        for b, board in enumerate(boards):
            model.add_model(board)
            if last is None:
                continue
            if len(last) == len(boards):                   # board to board, or branch to the branch of the same key
                _join(model, last[b], board, 1.00, 1.00)
            elif len(last) == 1:                           # into a fork
                _join(model, last[0], board, 1.00 / len(boards), 1.00)
            else:                                          # out of a fork
                for branch in last:
                    _join(model, branch, board, 1.00, 1.00 / len(last))
        last = boards
        if i == 0:
            first = boards[0]
    head = State(insert, name="I:0")
    model.add_state(head)
    for a, b, p in ((head, head, 0.70), (head, first.s1, 0.1), (head, first.s2, 0.2),
                    (model.start, head, 0.02), (model.start, first.s1, 0.08), (model.start, first.s2, 0.90),
                    (last[0].e1, model.end, 1.00), (last[0].e2, model.end, 1.00)):
        model.add_transition(a, b, p)
    model.bake(merge=merge)
    return model


def _linear_profile(distributions, name, low, high, sb_length, lb_length, match_p, sb_p, delete_p):
    """What Phi29ProfileHMM and Hel308ProfileHMM share, unbaked.  Per position i (named i + 1): a match sub-model M of two
    states of the same name (plain, and oversegmented with a long self-loop), an insert I (uniform on [low, high], one
    object for all), a silent delete D; from position sb_length on a silent short backslip S that goes back one match --
    directly, or through a pair of repeat states (named as the two matches) that flicker between the two levels -- or on to
    the S before it; from position lb_length on (lb_length not None) a silent long backslip L that goes lb_length matches
    back or on to the L before it.  match_p(i): previous match -> this match; sb_p = (S -> previous match with and
    without an S before it, S -> the repeat states); delete_p = (previous D -> this match, previous D -> this D)."""
    distributions = list(distributions)
    if not distributions:
        raise ValueError("a profile needs at least one distribution")
    if sb_length < 1 or (lb_length is not None and lb_length < 1):
        raise ValueError("backslip lengths must be at least 1, got sb_length=%r%s"
                         % (sb_length, "" if lb_length is None else ", lb_length=%r" % lb_length))
    model = Model("{}-{}".format(name, len(distributions)))
    insert_distribution = UniformDistribution(low, high)
    add = model.add_transition
    matches = []
    last_out, last_insert = model.start, State(insert_distribution, name="I0")    # last_out: the previous match's way out
    last_delete = last_sb = last_lb = None
    add(model.start, last_insert, 0.02)
    add(last_insert, last_insert, 0.70)
    for i, distribution in enumerate(distributions):
        label = "M" + str(i + 1)
        match = Model(name=label)
        plain, overseg = State(distribution, name=label), State(distribution, name=label)
        for a, b, p in ((match.start, plain, 0.75), (match.start, overseg, 0.25), (plain, plain, 0.10),
                        (plain, match.end, 0.90), (overseg, overseg, 0.80), (overseg, match.end, 0.20)):
            match.add_transition(a, b, p)
        insert = State(insert_distribution, name="I" + str(i + 1))
        delete = State(None, name="D" + str(i + 1))
        short = State(None, name="S" + str(i + 1)) if i >= sb_length else None
        long_ = State(None, name="L" + str(i + 1)) if lb_length is not None and i >= lb_length else None
        model.add_model(match)
        add(last_out, match.start, match_p(i))
        add(last_out, delete, 0.08 if i == 0 else 0.03)
        add(match.end, insert, 0.02)
        add(insert, insert, 0.75)
        add(insert, match.start, 0.10)
        add(last_insert, delete, 0.05)
        add(last_insert, match.start, 0.10)
        add(delete, insert, 0.10)
        if short is not None:
            previous = matches[-1]
            add(match.end, short, 0.03)
            add(short, previous.start, sb_p[0] if last_sb is not None else sb_p[1])
            repeat = State(distribution, name=label)
            repeat_previous = State(distributions[i - 1], name=previous.name)
            add(short, repeat_previous, sb_p[2])
            add(repeat_previous, repeat, 0.70)
            add(repeat_previous, match.start, 0.10)
            add(repeat_previous, repeat_previous, 0.20)
            add(repeat, repeat, 0.20)
            add(repeat, repeat_previous, 0.80)
            if last_sb is not None:
                add(short, last_sb, 0.15)
        if long_ is not None:
            add(match.end, long_, 0.02)
            add(long_, matches[-lb_length].start, 0.75 if last_lb is not None else 1.00)
            if last_lb is not None:
                add(long_, last_lb, 0.25)
        if last_delete is not None:
            add(last_delete, match.start, delete_p[0])
            add(last_delete, delete, delete_p[1])
        last_out, last_insert, last_delete, last_sb, last_lb = match.end, insert, delete, short, long_
        matches.append(match)
    add(last_delete, model.end, 0.95)
    add(last_insert, model.end, 0.70)
    add(last_out, model.end, 0.50)
    return model


def Phi29ProfileHMM(distributions, name="Phi29 Profile HMM", low=0, high=90, sb_length=1, verbose=True, merge='all'):
    """The reference's linear Phi29 profile: short backslips and their repeat states, oversegmentation through the
    two-state match (_linear_profile).  Baked with bake(verbose=verbose, merge=merge)."""
    model = _linear_profile(distributions, name, low, high, sb_length, None,
                            lambda i: 0.90 if i == 0 else 0.80 if i <= sb_length else 0.77,
                            (0.75, 0.90, 0.10), (0.80, 0.10))
    model.bake(verbose=verbose, merge=merge)
    return model


def Hel308ProfileHMM(distributions, name="Hel308 Profile HMM", low=0, high=90, sb_length=1, lb_length=9):
    """The reference's linear Hel308 profile: Phi29ProfileHMM's states with its own numbers, and long backslips of
    lb_length positions (_linear_profile).  Baked with the default bake()."""
    model = _linear_profile(distributions, name, low, high, sb_length, lb_length,
                            lambda i: 0.90 if i == 0 else 0.80 if i <= sb_length else 0.77 if i <= lb_length else 0.75,
                            (0.80, 0.95, 0.05), (0.70, 0.20))
    model.bake()
    return model
