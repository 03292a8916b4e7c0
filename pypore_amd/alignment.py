"""`SegmentAligner` with the surface of PyPore/alignment.py:26-46: the wrapper DataTypes-level code uses around
cSegmentAligner.  align() returns (score, order) or (None, None) when the aligner raises ValueError
(alignment.py:43-46); other exceptions propagate as in the reference.  `transform` (alignment.py:48-107) is host
bookkeeping that reads `self.model`, which the reference never sets; it is not part of the accelerated path.

`PairwiseAligner` (PyPore/alignment.py:97-313) aligns two sequences of segment means on the GPU (ps_pairwise_batch /
ps_pairwise_scores, csrc/seg_pairwise.hpp); `pairwise_align_batch` and `pairwise_scores` do it for many pairs at once."""
import math

import numpy as np

from .calignment import cSegmentAligner


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
