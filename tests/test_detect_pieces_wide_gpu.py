"""ps_detect_pieces refuses a float32 trace whose counts lie so far from their piece's first sample that the int64 sum of squares
could overflow ("counts too wide"): the bound is floor(sqrt((2^63 - 1) / n)) counts for a trace of n samples
(pypore_amd/csrc/piece_plan.hpp: piece_span_max).  At n = 200 000 that is 6 790 939 counts; float32 on the grid holds |count| <
2^23 = 8 388 608, so two levels at -4e6 and +4e6 counts inside ONE piece (both on one side of the threshold) are 8e6 apart: on
the grid, and past the bound.  The same levels in a trace of 1 000 samples (bound 2^24 - 2) are accepted and exact."""
import math

import numpy as np
import pytest

from pypore_amd import synth

pytestmark = pytest.mark.gpu

Q = synth.QUANTUM
LEVEL = 4_000_000


def levels(n):
    k = np.full(n, -LEVEL, dtype=np.int64)
    k[n // 2:] = LEVEL
    k[::7] += 3
    return k


def f32(k):
    import torch
    a = (k * Q).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), k * Q)          # on the grid, exactly
    return torch.from_numpy(a).cuda()


def test_float32_counts_too_wide_are_refused_and_the_context_stays_usable():
    from pypore_amd import engine
    ctx = engine.context(0)
    n = 200_000
    bound = math.isqrt((2 ** 63 - 1) // n)
    assert bound == 6_790_939 and 2 * LEVEL > bound and LEVEL + 3 < 2 ** 23
    thr = (LEVEL + 100) * Q                                      # everything below: one piece
    with pytest.raises(ValueError, match=r"counts too wide: a float32 sample lies more than %d counts" % bound):
        ctx.detect_pieces(f32(levels(n)), Q, thr)
    # the context is usable, and the same levels in a short trace -- no restriction up to 2^15 samples -- give exact rows
    k = levels(1_000)
    edges, stats = ctx.detect_pieces(f32(k), Q, thr)
    assert edges.tolist() == [0, 1_000]
    y = [int(v) - int(k[0]) for v in k]
    s1, s2 = sum(y), sum(v * v for v in y)
    my = float(s1) / 1000.0
    var = max(0.0, float(s2) / 1000.0 - my * my)
    want = np.array([[(float(int(k[0])) + my) * Q, math.sqrt(var) * Q, float(int(k.min())) * Q, float(int(k.max())) * Q]])
    assert np.array_equal(stats.view(np.int64), want.view(np.int64))
    # with the threshold between the levels each piece stays near its first sample: the long trace is accepted
    edges, _ = ctx.detect_pieces(f32(levels(n)), Q, 0.0)
    assert edges.tolist() == [0, n // 2, n]
