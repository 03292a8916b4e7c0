"""`SegmentAligner` with the surface of PyPore/alignment.py:26-46: the wrapper DataTypes-level code uses around
cSegmentAligner.  align() returns (score, order) or (None, None) when the aligner raises ValueError
(alignment.py:43-46); other exceptions propagate as in the reference.  `transform` (alignment.py:48-107) is host
bookkeeping that reads `self.model`, which the reference never sets; it is not part of the accelerated path.

`PairwiseAligner` (PyPore/alignment.py:97-313) aligns two sequences of segment means on the GPU (ps_pairwise_batch /
ps_pairwise_scores, csrc/seg_pairwise.hpp); `pairwise_align_batch` and `pairwise_scores` do it for many pairs at once.

`PSSM`, `ProfileAligner` and `MultipleSequenceAligner` (PyPore/alignment.py:329-796) align sequences of segment means to
a profile -- a multiple sequence alignment whose columns become Gaussian kernel densities -- with profile HMMs decoded by
pypore_amd.hmm on the GPU; `profile_align_batch` aligns many sequences to one profile in a single Viterbi launch.

`NaiveTRF` (PyPore/alignment.py:799-893) finds the re-reads of an event in which the enzyme slipped back and lays them out
as a naive multiple alignment; its splitter runs on the GPU (ps_trf_split_batch, csrc/seg_trf.hpp), `naive_trf_batch` and
`naive_splits_batch` do it for many sequences in one call."""
import copy
import itertools as it
import math

import numpy as np

from . import _lib
from .calignment import cSegmentAligner
from .hmm import GaussianKernelDensity, Model, State, UniformDistribution


class SegmentAligner(object):
    def __init__(self, model_means, model_stds, model_durs, skip_penalty, backslip_penalty):
        self.aligner = cSegmentAligner(model_means, model_stds, model_durs, skip_penalty, backslip_penalty)

    def align(self, seq_means, seq_stds, seq_durs):
        try:
            return self.aligner.align(seq_means, seq_stds, seq_durs)
        except ValueError:
            return None, None

    def align_batch(self, seqs):
        """Many sequences in one launch; per sequence (score, order), (None, None) for a ValueError, or the
        exception instance the reference would have raised."""
        return [(None, None) if isinstance(r, ValueError) else r for r in self.aligner.align_batch(seqs)]


_MODES = {"global": 0, "local": 1, "local_repeated": 2, "repeated": 2}
_PW_INDEX_ERROR = "list index out of range"       # what the reference's IndexError says for an empty alignment


def _upload_values(seq):
    """A sequence as float64: the string '-' becomes the gap marker (NaN, scores 0); anything else must be a finite float."""
    out = np.empty(len(seq), dtype=np.float64)
    for k, v in enumerate(seq):
        if isinstance(v, str) and v == '-':
            out[k] = np.nan
            continue
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("element %d (%r) is neither a number nor the gap marker '-'" % (k, v))
        if not math.isfinite(f):
            raise ValueError("element %d is not finite: the maximum over NaN depends on the order in the reference" % k)
        out[k] = f
    return out


def _mode(mode):
    try:
        return _MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode %r: 'global', 'local' or 'local_repeated'" % (mode,))


def _penalty(penalty):
    p = float(penalty)
    if not math.isfinite(p):
        raise ValueError("the penalty must be finite")
    return p


def _pack(seqs):
    """Host side of an upload: the sequences checked and concatenated (float64, NaN markers), and their offsets."""
    vals = [_upload_values(s) for s in seqs]
    off = np.concatenate(([0], np.cumsum([v.size for v in vals]))).astype(np.int64)
    flat = np.concatenate(vals) if vals and off[-1] else np.zeros(1, np.float64)
    return flat, off


def _alignment(x, y, ci, cj):
    """Index columns in walk order -> the reference's (reversed(xalign), reversed(yalign)) over the caller's own objects."""
    xa = [x[i] if i >= 0 else '-' for i in ci]
    ya = [y[j] if j >= 0 else '-' for j in cj]
    return reversed(xa), reversed(ya)


def pairwise_align_batch_raw(pairs, mode='global', penalty=-1, min_length=2, device=None):
    """The arrays of engine.Context.pairwise_batch for `pairs` (a list of (x, y)); no exception for per-pair failures."""
    import torch
    from . import engine
    mode, penalty, min_length = _mode(mode), _penalty(penalty), int(min_length)
    a, a_off = _pack([p[0] for p in pairs])
    b, b_off = _pack([p[1] for p in pairs])
    ctx = engine.context(device)
    dev = torch.device("cuda", ctx.device)
    idx = np.arange(len(pairs), dtype=np.int32)
    return ctx.pairwise_batch(torch.from_numpy(a).to(dev), a_off, torch.from_numpy(b).to(dev), b_off, idx, idx, mode,
                              penalty, min_length)


def pairwise_align_batch(pairs, mode='global', penalty=-1, min_length=2, device=None):
    """Many pairs (x, y) in one call.  Per pair what the PairwiseAligner method of that mode returns -- (score, xalign,
    yalign) for 'global' and 'local', the list of such tuples for 'local_repeated' -- or the exception INSTANCE where the
    reference raises (IndexError); a repeated alignment that fails after it has yielded results is a list whose last
    entry is that instance."""
    pairs = [(p[0], p[1]) for p in pairs]
    mode_i = _mode(mode)
    (scores, status, ci, cj, col_off, aln_score, aln_start, aln_len, aln_off, aln_count) = pairwise_align_batch_raw(
        pairs, mode, penalty, min_length, device)
    out = []
    for q, (x, y) in enumerate(pairs):
        res = []
        for k in range(int(aln_count[q])):
            s = int(col_off[q]) + int(aln_start[aln_off[q] + k])
            e = s + int(aln_len[aln_off[q] + k])
            res.append((aln_score[aln_off[q] + k],) + _alignment(x, y, ci[s:e], cj[s:e]))
        if status[q]:
            res.append(IndexError(_PW_INDEX_ERROR))
        out.append(res if mode_i == 2 else res[0])
    return out


def pairwise_scores(seqs, others=None, mode='global', penalty=-1, device=None):
    """float64 [len(seqs), len(others)]: score[m][n] of the global alignment, or the maximum of the local matrix, of every
    pair -- on the score-only route, no traceback.  others=None: all-vs-all."""
    import torch
    from . import engine
    mode_i, penalty = _mode(mode), _penalty(penalty)
    if mode_i == 2:
        raise ValueError("pairwise_scores: mode 'global' or 'local'")
    a, a_off = _pack(seqs)
    b, b_off = (a, a_off) if others is None else _pack(others)
    ctx = engine.context(device)
    dev = torch.device("cuda", ctx.device)
    a = torch.from_numpy(a).to(dev)
    b = a if others is None else torch.from_numpy(b).to(dev)
    return ctx.pairwise_scores(a, a_off, b, b_off, mode_i, penalty)[0].cpu().numpy()


class PairwiseAligner(object):
    """PairwiseAligner of PyPore/alignment.py:97-313 on the GPU: two sequences of segment means (or '-'), aligned by
    Needleman-Wunsch, Smith-Waterman or the repeated local traceback, with the reference's return shapes and -- where it
    raises IndexError -- its exception.  Elements must be finite floats or the string '-' (ValueError otherwise: the
    reference's max over NaN depends on the order).  There is no CPU fallback in this package: the scoring function is the
    kernel's, and a subclass that overrides `_score` gets NotImplementedError from the alignment methods."""

    def __init__(self, x, y):
        self.x = x
        self.y = y
        self.m = len(self.x)
        self.n = len(self.y)

    def _score(self, x, y):
        if (isinstance(x, str) and x == '-') or (isinstance(y, str) and y == '-'):
            return 0
        d = abs(x - y)
        return 3 - d * d

    def dotplot(self):
        score = np.zeros((self.m + 1, self.n + 1))
        for i in range(1, self.m + 1):
            for j in range(1, self.n + 1):
                score[i, j] = self._score(self.x[i - 1], self.y[j - 1])
        return score

    def _run(self, mode, penalty, min_length=2):
        if type(self)._score is not PairwiseAligner._score:
            raise NotImplementedError("the device aligner scores with PairwiseAligner._score; there is no CPU fallback "
                                      "for a subclass's own _score")
        return pairwise_align_batch([(self.x, self.y)], mode, penalty, min_length)[0]

    def global_alignment(self, penalty=-1):
        return self._run('global', penalty)

    def local_alignment(self, penalty=-1):
        r = self._run('local', penalty)
        if isinstance(r, Exception):
            raise r
        return r

    def local_repeated_alignment(self, penalty=-1, min_length=2):
        # (a generator, as in the reference: nothing runs before the first next())
        for r in self._run('local_repeated', penalty, min_length):
            if isinstance(r, Exception):
                raise r
            yield r


# ---- profile alignment (PyPore/alignment.py:329-796) ---------------------------------------------------------------------
def _is_gap(x):
    return isinstance(x, str) and x == '-'


class PSSM(object):
    """A position specific scoring matrix over a multiple sequence alignment of segment means (rows of equal length, '-'
    for a gap): pssm[i] = the non-gap values of column i, consensus[i] = their mean.  A flat sequence is taken as a
    one-row alignment.  Columns that hold only gaps are deleted IN PLACE from the rows given (as in the reference)."""

    def __init__(self, msa):
        if not isinstance(msa, (list, PSSM)):
            msa = list(msa)
        if hasattr(msa, '__iter__') and (isinstance(msa[0], str) or not hasattr(msa[0], '__iter__')):
            msa = [msa]
        for profile in list(msa):
            if isinstance(profile, PSSM):
                msa = [seq for seq in it.chain(msa, profile.msa)]
        self.msa = msa
        self.consensus = []
        self.pssm = []
        offset = 0
        for i, column in enumerate(list(zip(*msa))):
            column = [x for x in column if not _is_gap(x)]
            if len(column) == 0:
                for seq in self.msa:
                    del seq[i - offset]
                offset += 1
                continue
            self.pssm.append([mean for mean in column])
            self.consensus.append(np.mean([mean for mean in column]))

    def __getitem__(self, slice):
        return self.pssm[slice]

    def __repr__(self):
        return '\n'.join("{}".format(mean) for mean in self.consensus)

    def __len__(self):
        return len(self.pssm)


def follow_global(master, slave, names):
    """The reference's path-following loop of global_alignment (alignment.py:630-641) on the state names of a Viterbi
    path, start and end included: a delete state puts a gap into the slave, an insert state one into the master, in
    `pssm` and in every row of `msa`, in place (`consensus` is left alone, as in the reference)."""
    for i, sname in enumerate(names[1:-1]):
        if sname.startswith('D'):
            slave.pssm.insert(i, '-')
            for seq in slave.msa:
                seq.insert(i, '-')
        elif sname.startswith('I'):
            master.pssm.insert(i, '-')
            for seq in master.msa:
                seq.insert(i, '-')
    return master, slave


def follow_local(master, slave, names):
    """The loop of local_alignment (alignment.py:658-690): at the first match state M<k> the first k columns of the
    master are dropped (msa, pssm and consensus), gaps go in as in follow_global with the master's position shifted by
    k, and at PE one element per remaining state is cut from the end of every slave row."""
    first_match = True
    offset = 0
    for i, sname in enumerate(names[1:-1]):
        if sname.startswith("M") and first_match:
            first_match = False
            offset = int(sname[1:])
            for j in range(offset):
                for seq in master.msa:
                    del seq[0]
                del master.pssm[0]
                del master.consensus[0]
        if sname.startswith('D'):
            slave.pssm.insert(i, '-')
            for seq in slave.msa:
                seq.insert(i, '-')
        elif sname.startswith('I'):
            master.pssm.insert(i - offset, '-')
            for seq in master.msa:
                seq.insert(i - offset, '-')
        if sname == 'PE':
            for _ in range(len(names) - i - 3):
                for seq in slave.msa:
                    del seq[-1]
            break
    return master, slave


class ProfileAligner(object):
    """Aligns a slave profile (its consensus) to a master profile with a profile HMM: match states are the kernel
    densities of the master's columns, insert states share one uniform distribution over [low, high], delete states are
    silent.  master and slave: a PSSM, a multiple sequence alignment (list of rows) or one flat sequence.  The state
    names and transition probabilities are the reference's (alignment.py:427-616); bake() normalises them."""

    def __init__(self, master, slave, bandwidth=1):
        self.bandwidth = bandwidth
        self.master = master if isinstance(master, PSSM) else PSSM(master)
        self.slave = slave if isinstance(slave, PSSM) else PSSM(slave)

    def _match(self, column, name):
        return State(GaussianKernelDensity(column, self.bandwidth), name=name)

    def _build_global(self, pssm, low, high):
        model = Model(name="Global Profile Aligner")
        insert_dist = UniformDistribution(low, high)
        last_match = model.start
        last_insert = State(insert_dist, name="I0")
        last_delete = None
        model.add_transition(model.start, last_insert, 0.15)
        model.add_transition(last_insert, last_insert, 0.20)
        for i, column in enumerate(pssm):
            match = self._match(column, "M" + str(i + 1))
            insert = State(insert_dist, name="I" + str(i + 1))
            delete = State(None, name="D" + str(i + 1))
            model.add_transition(last_match, match, 0.60)
            model.add_transition(last_match, delete, 0.25)
            model.add_transition(last_insert, match, 0.65)
            model.add_transition(last_insert, delete, 0.20)
            model.add_transition(delete, insert, 0.15)
            model.add_transition(insert, insert, 0.15)
            model.add_transition(match, insert, 0.15)
            if last_delete is not None:
                model.add_transition(last_delete, match, 0.65)
                model.add_transition(last_delete, delete, 0.20)
            last_match, last_insert, last_delete = match, insert, delete
        if last_delete is None:
            raise ValueError("a profile needs at least one column")
        model.add_transition(last_delete, model.end, 0.85)
        model.add_transition(last_insert, model.end, 0.85)
        model.add_transition(last_match, model.end, 0.85)
        model.bake()
        return model

    def _profile_repeat(self, model, pssm, insert_dist, start_delete, end_delete):
        """The columns shared by the local and the repeat model (alignment.py:494-536 and :571-613)."""
        m = len(pssm)
        if m < 3:
            raise ValueError("the local and repeat profile models need at least 3 columns, got %d" % m)
        last_match = self._match(pssm[0], "M0")
        last_insert = State(insert_dist, name="I0")
        last_delete = None
        model.add_transition(last_match, last_insert, 0.15)
        model.add_transition(last_match, end_delete, 0.05)
        model.add_transition(last_insert, last_insert, 0.20)
        model.add_transition(start_delete, last_match, 1. / m)
        for i, column in enumerate(pssm[1:-1]):
            match = self._match(column, "M" + str(i + 1))
            insert = State(insert_dist, name="I" + str(i + 1))
            delete = State(None, name="D" + str(i + 1))
            model.add_transition(start_delete, match, 1. / m)
            model.add_transition(last_match, match, 0.65)
            model.add_transition(last_match, delete, 0.15)
            model.add_transition(last_insert, delete, 0.20)
            model.add_transition(last_insert, match, 0.65)
            model.add_transition(insert, insert, 0.15)
            model.add_transition(delete, insert, 0.15)
            model.add_transition(match, insert, 0.15)
            model.add_transition(match, end_delete, 0.05)
            if last_delete is not None:
                model.add_transition(last_delete, match, 0.65)
                model.add_transition(last_delete, delete, 0.20)
            last_match, last_insert, last_delete = match, insert, delete
        match = self._match(pssm[-1], "M" + str(i + 2))
        model.add_transition(start_delete, match, 1. / m)
        model.add_transition(last_match, match, 0.80)
        model.add_transition(last_insert, match, 0.85)
        model.add_transition(last_delete, match, 0.85)
        model.add_transition(match, end_delete, 1.00)

    def _build_local(self, pssm, low, high):
        model = Model(name="Local Profile Aligner")
        insert_dist = UniformDistribution(low, high)
        start_insert = State(insert_dist, name="Q0")
        start_delete = State(None, name="P0")
        model.add_transition(model.start, start_insert, 0.5)
        model.add_transition(model.start, start_delete, 0.5)
        model.add_transition(start_insert, start_insert, 0.75)
        model.add_transition(start_insert, start_delete, 0.25)
        end_insert = State(insert_dist, name="QE")
        end_delete = State(None, name="PE")
        self._profile_repeat(model, pssm, insert_dist, start_delete, end_delete)
        model.add_transition(end_delete, end_insert, 0.5)
        model.add_transition(end_delete, model.end, 0.5)
        model.add_transition(end_insert, end_insert, 0.75)
        model.add_transition(end_insert, model.end, 0.25)
        model.bake()
        return model

    def _build_repeat(self, pssm, low, high):
        model = Model(name="Local Profile Aligner")
        insert_dist = UniformDistribution(low, high)
        intermediate_insert = State(insert_dist, name="Q")
        start_delete = State(None, name="P0")
        end_delete = State(None, name="PE")
        model.add_transition(model.start, start_delete, 0.5)
        model.add_transition(model.start, intermediate_insert, 0.5)
        model.add_transition(intermediate_insert, intermediate_insert, 0.50)
        model.add_transition(intermediate_insert, start_delete, 0.25)
        model.add_transition(intermediate_insert, model.end, 0.25)
        model.add_transition(end_delete, intermediate_insert, 0.5)
        model.add_transition(end_delete, model.end, 0.5)
        self._profile_repeat(model, pssm, insert_dist, start_delete, end_delete)
        model.bake()
        return model

    def _align(self, build, follow, low, high, device=None):
        profile = build(self.master, low, high)
        prob, states = profile.viterbi_batch([self.slave.consensus], device)[0]
        if states is None:
            return prob, None, None
        master, slave = follow(self.master, self.slave, [s.name for _, s in states])
        return prob, master, slave

    def global_alignment(self, low=0, high=60):
        """(log probability of the best path, master, slave) with the gaps of the alignment put into both profiles in
        place; (-inf, None, None) when the slave is impossible under the model (the reference would fail there)."""
        return self._align(self._build_global, follow_global, low, high)

    def local_alignment(self, low=0, high=60):
        """As global_alignment for the best local alignment: the master loses the columns before the first match, the
        slave's rows the tail after the profile."""
        return self._align(self._build_local, follow_local, low, high)

    def repeat_alignment(self, low=0, high=60):
        """The reference's repeat_alignment is marked incomplete and only prints the path's state names; this returns
        them: (log probability, [state names between start and end]), (-inf, None) for an impossible slave."""
        profile = self._build_repeat(self.master, low, high)
        prob, states = profile.viterbi(self.slave.consensus)
        return prob, (None if states is None else [s.name for _, s in states[1:-1]])


def profile_align_batch(master, slaves, mode='global', low=0, high=60, bandwidth=1, device=None):
    """Aligns every sequence (or alignment, or PSSM) of `slaves` to one master profile: one model, one viterbi_batch
    call.  Returns [(prob, master, slave)] -- per slave a deep copy of the master and the slave's PSSM with the
    alignment's gaps, what ProfileAligner(copy of master, slave, bandwidth).global_alignment(low, high) (mode 'local':
    local_alignment) returns, (-inf, None, None) for an impossible slave."""
    if mode not in ('global', 'local'):
        raise ValueError("mode must be 'global' or 'local', got %r" % (mode,))
    base = master if isinstance(master, PSSM) else PSSM(master)
    aligner = ProfileAligner(base, [0.0], bandwidth)
    model = (aligner._build_global if mode == 'global' else aligner._build_local)(base, low, high)
    follow = follow_global if mode == 'global' else follow_local
    pssms = [s if isinstance(s, PSSM) else PSSM(s) for s in slaves]
    results = model.viterbi_batch([p.consensus for p in pssms], device) if pssms else []
    out = []
    for (prob, states), slave in zip(results, pssms):
        if states is None:
            out.append((prob, None, None))
            continue
        m, s = follow(copy.deepcopy(base), slave, [st.name for _, st in states])
        out.append((prob, m, s))
    return out


class MultipleSequenceAligner(object):
    """Multiple sequence alignment by profile HMMs (alignment.py:712-796): an initial alignment built by adding one
    sequence at a time, then rounds that peel each row off and align it back to the profile of the others, scored by the
    columns' differential entropy.  Every step depends on the one before, so this is a chain of single-sequence Viterbi
    launches: bound by launch and transfer latency, not by the kernels."""

    def __init__(self, sequences, bandwidth=1):
        self.sequences = sequences
        self.bandwidth = bandwidth

    def _score(self, msa):
        """sum over columns of  entropy(non-gap values) / (non-gap count)^2,  entropy = 0.5 log(2 pi e std^2) for more
        than one value of non-zero spread, else 0 (lower is better)."""
        def entropy(col):
            return 0.5 * math.log(2 * np.pi * np.e * np.std(col) ** 2) if len(col) > 1 and np.std(col) > 0 else 0
        return sum(1. / (len(col) - sum(1 for x in col if _is_gap(x))) ** 2 * entropy([x for x in col if not _is_gap(x)])
                   for col in zip(*msa))

    @staticmethod
    def _global(master, slave, bandwidth):
        p, x, y = ProfileAligner(master=master, slave=slave, bandwidth=bandwidth).global_alignment()
        if x is None:
            raise ValueError("a sequence cannot be aligned to the profile: a value outside the insert range [0, 60]?")
        return p, x, y

    def iterative_alignment(self, epsilon=1e-4, max_iterations=10, bandwidth=1):
        """(score of the last trial alignment, best alignment found), as the reference returns them."""
        score, msa = self.iterative_initialization(bandwidth=bandwidth)
        if score == 0:
            return 0, msa
        n = len(msa)
        last_score = float('inf')
        best_msa, best_score = msa, score
        iteration = 0
        while abs(best_score - last_score) >= epsilon and iteration < max_iterations:
            iteration += 1
            last_score = best_score
            for i in range(n):
                slave = [x for x in best_msa[i] if not _is_gap(x)]
                master = best_msa[:i] + best_msa[i + 1:]
                p, x, y = self._global(master, slave, bandwidth)
                msa = [seq for seq in it.chain(x.msa, y.msa)]
                score = self._score(msa)
                if score < best_score:
                    best_msa, best_score = msa, score
        m = max(map(len, best_msa))
        for seq in best_msa:
            seq.extend(['-'] * (m - len(seq)))
        return score, best_msa

    def iterative_initialization(self, bandwidth=1):
        """(score, alignment) from adding the sequences one at a time to a growing profile."""
        pssm = PSSM(self.sequences[0])
        for seq in self.sequences[1:]:
            p, master, slave = self._global(pssm, seq, bandwidth)
            pssm = PSSM([seq for seq in it.chain(master.msa, slave.msa)])
        return self._score(pssm.msa), pssm.msa


# ---- tandem repeats (PyPore/alignment.py:799-893) --------------------------------------------------------------------------
def _trf_args(penalty, min_score, max_repeats):
    penalty, min_score = float(penalty), float(min_score)
    if not (math.isfinite(penalty) and penalty < 0):
        raise ValueError("NaiveTRF: the penalty must be finite and < 0 (with penalty >= 0 the reference's diagonal and lower "
                         "triangle, which the device does not compute, take part in the result)")
    if not (math.isfinite(min_score) and min_score >= 0):
        raise ValueError("NaiveTRF: min_score must be finite and >= 0 (the reference never ends for min_score < 0: it yields "
                         "the border cell (0, 0) for ever)")
    max_repeats = 0 if max_repeats is None else int(max_repeats)
    if max_repeats < 0:
        raise ValueError("max_repeats must be None or >= 0 (0: no cap)")
    return penalty, min_score, max_repeats


def _trf_values(seq, q):
    """(means, stds) of a sequence as float64 arrays, checked: a list of objects with .mean and .std, or a pair of arrays."""
    if isinstance(seq, tuple) and len(seq) == 2 and all(isinstance(v, (np.ndarray, list, tuple)) for v in seq):
        means, stds = (np.array(v, dtype=np.float64).reshape(-1) for v in seq)
        if means.size != stds.size:
            raise ValueError("sequence %d: %d means and %d stds" % (q, means.size, stds.size))
    else:
        means = np.array([s.mean for s in seq], dtype=np.float64).reshape(-1)
        stds = np.array([s.std for s in seq], dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(means)):
        raise ValueError("sequence %d: a mean is not finite" % q)
    if not np.all(np.isfinite(stds) & (stds > 0)):
        raise ValueError("sequence %d: a std is not finite and > 0 (the reference's score divides by std * std: inf or nan, "
                         "whose maximum depends on the order)" % q)
    if means.size > _lib.TRF_N_MAX:
        raise ValueError("sequence %d: %d segments, the device repeat splitter takes up to %d" % (q, means.size, _lib.TRF_N_MAX))
    return means, stds


def naive_splits_batch_raw(seqs, penalty=-1, min_score=2, max_repeats=None, device=None, slots=None, retry=True):
    """The arrays of engine.Context.trf_split_batch for `seqs`: (rc, score, length, i, j, slot_off, count, status).  Every
    argument is checked before the library is touched (ValueError)."""
    penalty, min_score, max_repeats = _trf_args(penalty, min_score, max_repeats)
    vals = [_trf_values(s, q) for q, s in enumerate(seqs)]
    off = np.concatenate(([0], np.cumsum([m.size for m, _ in vals]))).astype(np.int64)
    means = np.concatenate([m for m, _ in vals]) if vals and off[-1] else np.zeros(1, np.float64)
    stds = np.concatenate([s for _, s in vals]) if vals and off[-1] else np.ones(1, np.float64)
    import torch
    from . import engine
    ctx = engine.context(device)
    dev = torch.device("cuda", ctx.device)
    return ctx.trf_split_batch(torch.from_numpy(means).to(dev), torch.from_numpy(stds).to(dev), off, penalty, min_score,
                               max_repeats, slots, retry)


def naive_splits_batch(seqs, penalty=-1, min_score=2, max_repeats=None, device=None):
    """Per sequence the list of (score, length, start, end) that the reference's NaiveSplitter yields, in yield order, from
    one library call for the whole batch.  A sequence is a list of objects with .mean and .std, or a (means, stds) pair of
    arrays.  max_repeats: at most that many yields per sequence (None: all)."""
    seqs = list(seqs)
    _, score, length, i, j, slot_off, count, _ = naive_splits_batch_raw(seqs, penalty, min_score, max_repeats, device)
    return [[(float(score[k]), int(length[k]), int(i[k]), int(j[k])) for k in range(int(slot_off[q]), int(slot_off[q]) + int(count[q]))]
            for q in range(len(seqs))]


def _trf_stitch(seq, splits):
    """The stitching loop of alignment.py:873-893: the re-reads laid out under each other, padded with '-'."""
    last_end, last_start, offset, sequences = 0, 0, 0, []
    for score, length, start, end in sorted(splits, key=lambda x: x[3]):
        sequences.append(['-'] * offset + seq[last_end:end])
        offset = (len(sequences[-1]) - (end - start) if last_start != start else offset)
        last_end, last_start = end, start
    sequences.append(['-'] * offset + seq[last_end:])
    n = max(map(len, sequences))
    return [s + ['-'] * (n - len(s)) for s in sequences]


def naive_trf_batch(seqs, penalty=-1, min_score=2, max_repeats=None, device=None):
    """NaiveTRF for many sequences (lists of objects with .mean and .std) from one library call: per sequence the
    reference's list of rows, made of the caller's own objects and '-'."""
    seqs = [list(s) for s in seqs]
    return [_trf_stitch(s, sp) for s, sp in zip(seqs, naive_splits_batch(seqs, penalty, min_score, max_repeats, device))]


def NaiveTRF(seq, penalty=-1, min_score=2):
    """NaiveTRF of PyPore/alignment.py:799-893 on the GPU.  `seq`: the segments of an event in which the enzyme slipped back
    and re-read part of the strand (objects with .mean and .std, e.g. event.segments).  Step 1, on the device
    (ps_trf_split_batch, csrc/seg_trf.hpp): the local self-alignment matrix of the sequence is filled, its best off-diagonal
    path pulled out and masked, and the matrix filled again until nothing scores above min_score.  Step 2, on the host: the
    paths, sorted stably by their end, are stitched into a naive multiple alignment -- a list of rows of equal length made
    of the caller's own objects and '-'.

    Deliberate deviations from the reference, all ValueError before any library call: min_score < 0 (the reference never
    returns: it yields the border cell for ever); penalty >= 0 (the reference's diagonal and lower triangle, which the
    device does not compute, would take part); a mean that is not finite; a std that is not finite and > 0 (inf / nan
    scores whose maximum depends on the order of a tuple).  Sequences of up to 2048 segments.  The square of the
    reference's score, `** 2`, is taken as the product -- the correctly rounded value; the reference's is its host's
    libm pow, one ulp off for about 0.07 % of the operands.  There is no CPU fallback."""
    return naive_trf_batch([seq], penalty, min_score)[0]
