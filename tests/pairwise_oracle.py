"""Plain numpy / Python restatement of PairwiseAligner (PyPore/alignment.py:97-313) as the device computes it: the
recurrences, tie rules and tracebacks of the reference cell for cell, with two stated differences -- the match score
squares by product (3.0 - d * d; the reference's `abs(x - y) ** 2` goes through the C library's pow, which differs from
the product by one unit in the last place for about one float in a thousand) and the penalty is a float.  The device
equals this file bit for bit; this file equals the recorded reference exactly on grid-valued goldens
(tests/test_pairwise_host.py).

Sequences are float64 arrays with NaN for the gap marker '-'.  Alignments are index columns in WALK order (the
alignment's last column first), -1 for a gap -- what ps_pairwise_batch writes."""
import numpy as np

NEGINF = -999999999.0
GLOBAL, LOCAL, REPEATED = 0, 1, 2
OK, INDEX_ERROR = 0, 1


def match(x, y):
    """_score (:112-115) of every cell: [m, n]."""
    x = np.asarray(x, dtype=np.float64)[:, None]
    y = np.asarray(y, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        d = np.abs(x - y)
        s = 3.0 - d * d
    return np.where(np.isnan(x) | np.isnan(y), 0.0, s)


def fill_loops(x, y, penalty, local):
    """The reference's doubly nested loops (:130-155, :194-212): (score [m+1, n+1], pointer [m+1, n+1])."""
    m, n = len(x), len(y)
    penalty = float(penalty)
    mt = match(x, y)
    score = np.zeros((m + 1, n + 1))
    pointer = np.zeros((m + 1, n + 1), dtype=np.int64)
    if not local:
        score[0, :] = np.arange(n + 1) * penalty
        score[:, 0] = np.arange(m + 1) * penalty
        pointer[0, :] = 1
        pointer[:, 0] = 2
        pointer[0, 0] = -1
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            cands = (score[i - 1, j - 1] + mt[i - 1, j - 1], score[i, j - 1] + penalty, score[i - 1, j] + penalty)
            if local:
                cands = (0.0,) + cands
            best = max(cands)
            score[i, j] = best
            pointer[i, j] = cands.index(best)
    return score, pointer


def fill(x, y, penalty, local):
    """The same matrices by anti-diagonals (every cell takes the same maximum over the same sums, first candidate
    winning: the cells of an anti-diagonal do not depend on each other)."""
    m, n = len(x), len(y)
    penalty = float(penalty)
    score = np.zeros((m + 1, n + 1))
    pointer = np.zeros((m + 1, n + 1), dtype=np.int64)
    if not local:
        score[0, :] = np.arange(n + 1) * penalty
        score[:, 0] = np.arange(m + 1) * penalty
        pointer[0, :] = 1
        pointer[:, 0] = 2
        pointer[0, 0] = -1
    if m == 0 or n == 0:
        return score, pointer
    mt = match(x, y)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        cands = [score[i - 1, j - 1] + mt[i - 1, j - 1], score[i, j - 1] + penalty, score[i - 1, j] + penalty]
        if local:
            cands.insert(0, np.zeros(i.size))
        best, ptr = cands[0].copy(), np.zeros(i.size, dtype=np.int64)
        for k in range(1, len(cands)):
            better = cands[k] > best
            best[better] = cands[k][better]
            ptr[better] = k
        score[i, j] = best
        pointer[i, j] = ptr
    return score, pointer


def global_alignment(x, y, penalty=-1.0):
    """(:157-181) -> (status, score, [(score, ci, cj)])."""
    score, pointer = fill(x, y, penalty, False)
    i, j = len(x), len(y)
    s = score[i, j]
    ci, cj = [], []
    while i > 0 and j > 0:
        p = pointer[i, j]
        if p == 0:
            ci.append(i - 1); cj.append(j - 1); i -= 1; j -= 1
        elif p == 1:
            ci.append(-1); cj.append(j - 1); j -= 1
        else:
            ci.append(i - 1); cj.append(-1); i -= 1
    return OK, s, [(s, ci, cj)]


def _walk(score, pointer, x, y, i, j):
    """One local walk from (i, j) (:226-244 / :268-286): (error, ci, cj, clean) -- clean = columns left once the
    alignment's start is trimmed while either side is '-' (:246-248), a gap or the caller's own marker."""
    m, n = len(x), len(y)
    ci, cj, clean = [], [], 0
    while pointer[i, j] != 0:
        p = pointer[i, j]
        pointer[i, j] = 0
        if j > m or i > n:                      # pointer[j, i]: IndexError
            return True, ci, cj, clean
        pointer[j, i] = 0
        score[i, j] = NEGINF
        score[j, i] = NEGINF
        if p == 1:
            ci.append(i - 1); cj.append(j - 1)
            if not (np.isnan(x[i - 1]) or np.isnan(y[j - 1])):
                clean = len(ci)
            i -= 1; j -= 1
        elif p == 2:
            ci.append(-1); cj.append(j - 1); j -= 1
        else:
            ci.append(i - 1); cj.append(-1); i -= 1
    return False, ci, cj, clean


def local_alignment(x, y, penalty=-1.0, repeated=False, min_length=2, matrices=None):
    """(:214-304) -> (status, score of the first maximum, [(score, ci, cj)] of the alignments completed).  `matrices`:
    a dict that receives the filled score matrix (before the walks mark it)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    score, pointer = fill(x, y, penalty, True)
    if matrices is not None:
        matrices["score"] = score.copy()
    n = len(y)
    out, first = [], None
    while True:
        am = int(np.argmax(score))
        i, j = am // (n + 1), am % (n + 1)
        if first is None:
            first = score[i, j]
        if pointer[i, j] == 0:
            if not repeated:
                return INDEX_ERROR, first, out  # xalign[-1] of an empty list
            break
        s = score[i, j]
        err, ci, cj, clean = _walk(score, pointer, x, y, i, j)
        if err:
            return INDEX_ERROR, first, out
        if repeated and len(ci) < min_length:
            continue
        if clean == 0:
            return INDEX_ERROR, first, out      # trimmed to nothing
        out.append((s, ci[:clean], cj[:clean]))
        if not repeated:
            break
    return OK, first, out


def align(x, y, mode, penalty=-1.0, min_length=2):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if mode == GLOBAL:
        return global_alignment(x, y, penalty)
    return local_alignment(x, y, penalty, mode == REPEATED, min_length)


def score_only(x, y, mode, penalty=-1.0):
    """What ps_pairwise_scores returns for the pair: (score, (i, j) of the local maximum)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    score, _ = fill(x, y, penalty, mode != GLOBAL)
    if mode == GLOBAL:
        return score[len(x), len(y)], (0, 0)
    am = int(np.argmax(score))
    return score.flat[am], (am // (len(y) + 1), am % (len(y) + 1))
