"""Inputs that put the pairwise aligner's tie rules to a decision, shared by test_pairwise_ties_host.py (which certifies
on the restatement that they do) and test_pairwise_ties_gpu.py: integer-valued alphabets (every match score and every
sum is a small integer, so candidates tie all the time), periodic pairs whose local maximum is held by many rows and
columns at once, and gap markers (NaN) at the seams of the 64-row stripes."""
import numpy as np

import pairwise_oracle as O

U = np.array([20.0, 23.0, 21.0, 22.0, 20.0, 20.0, 23.0])     # the period of the periodic pairs
STRIPE = 64                                                   # rows of a stripe, columns a lane strides over
SEAMS = (0, 62, 63, 64, 65, 127, 128)                         # marker positions, and the last element besides
PENALTIES = (-1, -0.5, 0, -3, 1)


def letters(rng, n, k):
    """n integer values from an alphabet of k letters, 20 .. 20 + k - 1."""
    return rng.integers(20, 20 + k, int(n)).astype(np.float64)


def periodic(m=200):
    """x = U repeated up to m elements, y = U: the local maximum 21 ends at every full period of x."""
    return np.tile(U, m // U.size + 1)[:m].copy(), U.copy()


def periodic_transposed(n=200):
    x, y = periodic(n)
    return y, x


def periodic_square(m):
    """U repeated on both sides, y one period behind: the off-diagonals a period apart hold equal scores."""
    t = np.tile(U, m // U.size + 2)
    return t[:m].copy(), t[U.size:U.size + m].copy()


def candidates(x, y, penalty, local):
    """(score, pointer, a, b, c): the filled matrices and the three candidates of every interior cell."""
    score, pointer = O.fill(x, y, penalty, local)
    a = score[:-1, :-1] + O.match(x, y)
    b = score[1:, :-1] + float(penalty)
    c = score[:-1, 1:] + float(penalty)
    return score, pointer, a, b, c


def diagonal_tie_share(x, y, penalty, local):
    """Share of the interior cells in which the diagonal candidate equals a gap candidate and is the one taken."""
    _, pointer, a, b, c = candidates(x, y, penalty, local)
    won = pointer[1:, 1:] == (1 if local else 0)
    return float(np.mean(won & ((a == b) | (a == c))))


def maximum_cells(x, y, penalty=-1.0):
    """(maximum, rows, columns) of the local matrix: 1-based coordinates of every cell that holds the maximum."""
    score, _ = O.fill(x, y, penalty, True)
    i, j = np.nonzero(score == score.max())
    return score.max(), i, j


def with_markers(v, positions, run=1):
    """A copy of v with NaN at every position p .. p + run - 1 that lies within it."""
    v = np.array(v, dtype=np.float64)
    for p in positions:
        v[[q for q in range(p, p + run) if 0 <= q < v.size]] = np.nan
    return v


def related(rng, m, n, k=4):
    """x of m letters and y: its first n elements (further letters beyond m) with every fifth one drawn again."""
    x = letters(rng, m, k)
    y = x[:n].copy() if n <= m else np.concatenate((x, letters(rng, n - m, k)))
    flip = rng.random(y.size) < 0.2
    y[flip] = letters(rng, int(flip.sum()), k)
    return x, y


def marker_all_seams(rng, m=130, n=130, run=1):
    """A related pair with a marker (a run of them) at every seam and at the last element of both sequences."""
    x, y = related(rng, m, n)
    return with_markers(x, SEAMS + (m - 1,), run), with_markers(y, SEAMS + (n - 1,), run)


def marker_pairs(rng, m=130, n=130):
    """Pairs over one related base pair of m x n: a marker (and a run of three) in x at every seam row and at m - 1, the
    same in y at the seam columns within it and at n - 1, and both sides at once."""
    x, y = related(rng, m, n)
    pairs = []
    for run in (1, 3):
        for p in SEAMS + (m - 1,):
            pairs.append((with_markers(x, [p], run), y.copy()))
        for p in [s for s in SEAMS if s < n] + [n - 1]:
            pairs.append((x.copy(), with_markers(y, [p], run)))
        pairs.append((with_markers(x, SEAMS + (m - 1,), run), with_markers(y, SEAMS + (n - 1,), run)))
    return pairs


def trim_cases():
    """(name, x, y, mode, penalty, min_length) of the cases in which the trim of a local alignment's start decides the
    result; test_pairwise_ties_host.py certifies what each of them does."""
    nan = np.nan
    far = np.arange(8, dtype=np.float64) * 10.0
    return [
        # the second walk of a repeated alignment starts in a marker cell and ends at the cell the first one cleared
        ("repeated_trimmed_to_nothing", np.array([20.0, nan]), np.array([20.0, 21.0]), O.REPEATED, -1, 1),
        # a positive penalty: every border cell starts a gap, so the alignment's start is a run of gap columns
        ("positive_partial_trim", np.array([nan, 21.0, 22.0, nan, 23.0]), np.array([22.0, nan, 21.0, 22.0, 20.0]),
         O.LOCAL, 1, 2),
        # nothing matches: the walk from the corner is gaps only
        ("positive_trimmed_to_nothing", far, far + 300.0, O.LOCAL, 1, 2),
        ("positive_markers_trimmed_to_nothing", np.full(6, nan), np.full(6, nan), O.LOCAL, 1, 2),
        ("positive_repeated_yields_then_nothing", np.array([20.0, 21.0, 22.0, 20.0, 23.0, 21.0]),
         np.array([22.0, 20.0, 21.0, 22.0, 20.0, 23.0]), O.REPEATED, 1, 1),
    ]


def walks(x, y, penalty, repeated, min_length=2):
    """The local modes walk by walk, as O.local_alignment runs them: (status, [(error, columns walked, columns kept)])."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    score, pointer = O.fill(x, y, penalty, True)
    n, out = len(y), []
    while True:
        am = int(np.argmax(score))
        i, j = am // (n + 1), am % (n + 1)
        if pointer[i, j] == 0:
            return (O.OK if repeated else O.INDEX_ERROR), out
        err, ci, _, clean = O._walk(score, pointer, x, y, i, j)
        out.append((err, len(ci), clean))
        if err:
            return O.INDEX_ERROR, out
        if repeated and len(ci) < min_length:
            continue
        if clean == 0:
            return O.INDEX_ERROR, out
        if not repeated:
            return O.OK, out
