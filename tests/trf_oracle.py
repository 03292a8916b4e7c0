"""numpy / Python restatement of the reference's NaiveTRF (PyPore/alignment.py:799-893), the oracle of the device repeat
splitter (csrc/seg_trf.hpp).  A sequence is a pair of float64 arrays (means, stds).

splits_full     NaiveSplitter exactly as the reference runs it: the full (n + 1)^2 score, pointer and mask matrices, the
                diagonal cells computed, both triangles written, np.argmax over everything, the literal -999.
splits_upper    the form the device computes: the strict upper triangle only, row 0 as a zero border whose mask bits count,
                a masked source left out instead of scored -999, the arg-max as the row-major-first cell of the triangle.
stitch          the loop of alignment.py:873-893 on indices: rows of element indices, -1 for '-'.

Both splitters return (yields, info): yields = [(score, length, i, j)], info the facts tests/test_trf_host.py asserts
(every walked cell, whether a diagonal cell was ever the arg-max or a source, whether a masked candidate ever won)."""
import numpy as np

MASKED = -999


def match(mi, si, mj, sj):
    d = abs(mi - mj)
    return 2 - d * d / (si * sj)        # (d ** 2 of the reference: the product)


def splits_full(means, stds, penalty=-1, min_score=2, max_repeats=None):
    means = np.asarray(means, dtype=np.float64)
    stds = np.asarray(stds, dtype=np.float64)
    n = len(means)
    score = np.zeros((n + 1, n + 1))
    pointer = np.zeros((n + 1, n + 1))
    mask = np.identity(n + 1)
    yields = []
    info = {"walked": [], "diag_argmax": False, "masked_won": False, "left_upper": False, "new_cells": []}
    while max_repeats is None or len(yields) < max_repeats:
        for i in range(1, n + 1):
            for j in range(i, n + 1):
                scores = (0,
                          score[i - 1, j - 1] + match(means[i - 1], stds[i - 1], means[j - 1], stds[j - 1]) if not mask[i - 1, j - 1] else MASKED,
                          score[i, j - 1] + penalty if not mask[i, j - 1] else MASKED,
                          score[i - 1, j] + penalty if not mask[i - 1, j] else MASKED)
                score[i, j] = max(scores)
                score[j, i] = score[i, j]
                pointer[i, j] = scores.index(score[i, j])
                pointer[j, i] = pointer[i, j]
                p = int(pointer[i, j])
                if p and mask[(i - 1, i, i - 1)[p - 1], (j - 1, j - 1, j)[p - 1]]:
                    info["masked_won"] = True
        argmax = np.argmax(score)
        i, j = argmax // (n + 1), argmax % (n + 1)
        alignment_score = score[i, j]
        if alignment_score <= min_score:
            info["stop_score"] = float(alignment_score)
            break
        if i == j:
            info["diag_argmax"] = True
        length = 0
        before = int(mask.sum())
        cells = []
        while pointer[i, j] != 0:
            length += 1
            mask[i, j] = mask[j, i] = 1
            cells.append((int(i), int(j)))
            if not i < j:
                info["left_upper"] = True
            p = pointer[i, j]
            if p == 1:
                i -= 1
                j -= 1
            elif p == 2:
                j -= 1
            elif p == 3:
                i -= 1
        mask[i, j] = 1
        if not i < j:
            info["left_upper"] = True
        info["walked"].append(cells)
        info["new_cells"].append(int(mask.sum()) - before)
        yields.append((float(alignment_score), int(length), int(i), int(j)))
    return yields, info


def splits_upper(means, stds, penalty=-1, min_score=2, max_repeats=None):
    means = np.asarray(means, dtype=np.float64)
    stds = np.asarray(stds, dtype=np.float64)
    n = len(means)
    score = np.zeros((n + 1, n + 1))
    pointer = np.zeros((n + 1, n + 1), dtype=np.int8)
    mask = np.zeros((n + 1, n + 1), dtype=bool)     # strict upper triangle and row 0; (i, i) counts as masked, never stored
    yields = []
    info = {"walked": []}
    while max_repeats is None or len(yields) < max_repeats:
        best = (0.0, 0, 0)
        for i in range(1, n + 1):
            for j in range(i + 1, n + 1):
                v, p = 0.0, 0
                if not mask[i - 1, j - 1]:
                    a = score[i - 1, j - 1] + match(means[i - 1], stds[i - 1], means[j - 1], stds[j - 1])
                    if a > v:
                        v, p = a, 1
                if j - 1 > i and not mask[i, j - 1]:
                    b = score[i, j - 1] + penalty
                    if b > v:
                        v, p = b, 2
                if not mask[i - 1, j]:
                    c = score[i - 1, j] + penalty
                    if c > v:
                        v, p = c, 3
                score[i, j] = v
                pointer[i, j] = p
                if v > best[0]:
                    best = (v, i, j)
        v, i, j = best
        if not v > min_score:
            break
        length = 0
        cells = []
        while i >= 1 and pointer[i, j] != 0:
            length += 1
            mask[i, j] = True
            cells.append((i, j))
            p = pointer[i, j]
            if p == 1:
                i -= 1
                j -= 1
            elif p == 2:
                j -= 1
            else:
                i -= 1
        mask[i, j] = True
        info["walked"].append(cells)
        yields.append((float(v), int(length), int(i), int(j)))
    return yields, info


def stitch(n, yields):
    """Rows of indices into a sequence of n elements, -1 for '-' (alignment.py:873-893)."""
    last_end, last_start, offset, sequences = 0, 0, 0, []
    for score, length, start, end in sorted(yields, key=lambda x: x[3]):
        sequences.append([-1] * offset + list(range(n))[last_end:end])
        offset = (len(sequences[-1]) - (end - start) if last_start != start else offset)
        last_end, last_start = end, start
    sequences.append([-1] * offset + list(range(n))[last_end:])
    m = max(map(len, sequences))
    return [s + [-1] * (m - len(s)) for s in sequences]
