"""ps_range_stats (engine.Context.range_stats): mean / std / min / max of caller-given ranges of one device buffer.

The oracle is written out here in Python integers: k0 = the count of the range's first sample, S1 = sum(count - k0) and S2 =
sum((count - k0)^2) exactly, then the library's final expressions in float64, none fused --
    my = S1 / n,  var = max(0, S2 / n - my * my),  mean = (k0 + my) q,  std = sqrt(var) q,  min / max = (k0 + min y) q, (k0 + max y) q
-- and every comparison is == on all four columns: the device sums integers, so there is no tolerance anywhere in this file.

One seeded int16 buffer of 70 000 samples: dwells with noise, a stretch alternating between -32768 and 32767, a constant stretch.
Option range_tile is set to 512 so that ranges of a few thousand samples are cut into several units and the seams are hit."""
import contextlib
import math

import numpy as np
import pytest

from pypore_amd import synth

pytestmark = pytest.mark.gpu

N = 70_000
T = 512
Q = synth.QUANTUM
HEADER_Q = 10.0 / 0.0005 / 20.0 / 32768.0 * 1.0001        # an .abf header's scale: not a power of two
ALT = (20_000, 21_001)                                     # counts alternating -32768 / 32767
FLAT = (30_003, 30_600)                                    # one count throughout
LENGTHS = (1, 2, 7, 8, 9, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3)
BAD_ARG = r"status -1"


def context():
    from pypore_amd import engine
    return engine.context(0)


@contextlib.contextmanager
def tile(ctx, samples):
    before = ctx.get_option("range_tile")
    try:
        ctx.set_option("range_tile", int(samples))
        yield ctx
    finally:
        ctx.set_option("range_tile", before)


_BUF = {}


def counts():
    """The buffer's counts as int64 (built once, left unchanged)."""
    if "k" not in _BUF:
        rng = np.random.default_rng(20241021)
        k = np.empty(N, dtype=np.int64)
        at = 0
        while at < N:
            n = int(rng.integers(150, 2500))
            k[at:at + n] = int(rng.integers(-20000, 20000))
            at += n
        k += np.rint(rng.normal(0.0, 300.0, N)).astype(np.int64)
        k[ALT[0]:ALT[1]] = np.where(np.arange(ALT[1] - ALT[0]) % 2 == 0, -32768, 32767)
        k[FLAT[0]:FLAT[1]] = 12345
        assert k.min() >= -32768 and k.max() <= 32767
        _BUF["k"] = k
    return _BUF["k"]


def buffer(dtype):
    """The buffer as a CUDA tensor: int16 counts, or float32 on the 2^-5 pA grid (counts cut to +-2^15 there, far inside 2^23)."""
    import torch
    if dtype not in _BUF:
        k = counts()
        t = torch.from_numpy(k.astype(np.int16)) if dtype == "i16" else torch.from_numpy((k * Q).astype(np.float32))
        _BUF[dtype] = t.cuda()
        assert _BUF[dtype].data_ptr() % 16 == 0
    return _BUF[dtype]


def oracle(starts, ends, q, offset_counts=0):
    k = counts()
    out = np.empty((len(starts), 4), dtype=np.float64)
    for r, (a, z) in enumerate(zip(starts, ends)):
        k0 = int(k[a]) + offset_counts
        y = k[a:z] + offset_counts - k0
        n, s1, s2 = int(z - a), int(y.sum()), int((y * y).sum())         # (|y| <= 65535, n <= 70 000: inside int64)
        assert abs(s1) < 2 ** 53
        my = float(s1) / float(n)
        var = float(s2) / float(n) - my * my
        var = 0.0 if var < 0 else var
        out[r] = ((float(k0) + my) * q, math.sqrt(var) * q, float(k0 + int(y.min())) * q, float(k0 + int(y.max())) * q)
    return out


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (bad[:5], got[bad[:5, 0]], want[bad[:5, 0]])


def aligned_ranges(alignments):
    starts = [1000 + 4096 * i + a for i, _ in enumerate(LENGTHS) for a in alignments]
    ends = [1000 + 4096 * i + a + n for i, n in enumerate(LENGTHS) for a in alignments]
    return starts, ends


def special_ranges():
    """Overlapping, identical, nested and descending ranges; the whole buffer; its first and its last sample alone; the
    alternating stretch (inside it, across its ends, from an odd start); the constant stretch."""
    r = [(5000, 9000), (5000, 9000), (6000, 8000), (8999, 9001), (4000, 6000), (3000, 3700), (100, 1500), (0, N), (0, 1), (N - 1, N),
         (N - 2 * T - 3, N), (0, 2 * T + 3), ALT, (ALT[0] + 1, ALT[1] - 1), (ALT[0] - 700, ALT[1] + 700), (ALT[0] + 3, ALT[0] + 4),
         FLAT, (FLAT[0] + 5, FLAT[0] + 6), (FLAT[0] - 1, FLAT[1]), (5000, 9000)]
    return [a for a, _ in r], [z for _, z in r]


@pytest.mark.parametrize("dtype, alignments", [("i16", tuple(range(8))), ("f32", (3,))])
def test_lengths_alignments_and_special_ranges(dtype, alignments):
    """Range lengths 1 .. 2 T + 3 at every start alignment (int16; float32 at one), then overlapping, identical, descending
    ranges, the whole buffer, its two end samples, the rails alternating and a constant stretch -- at range_tile 512 and at
    the default, == against the oracle, and so the same bits however the tile cuts."""
    ctx = context()
    x = buffer(dtype)
    for starts, ends in (aligned_ranges(alignments), special_ranges()):
        want = oracle(starts, ends, Q)
        with tile(ctx, T):
            cut = ctx.range_stats(x, starts, ends, Q)
        whole = ctx.range_stats(x, starts, ends, Q)
        same_bits(cut, want)
        same_bits(whole, want)
    # the constant stretch: no spread at all; the rails: min and max are the rails
    st, en = special_ranges()
    got = ctx.range_stats(x, st, en, Q)
    flat, alt = st.index(FLAT[0]), st.index(ALT[0])
    assert got[flat, 1] == 0.0 and got[flat, 0] == got[flat, 2] == got[flat, 3] == 12345 * Q
    assert got[alt, 2] == -32768 * Q and got[alt, 3] == 32767 * Q and got[alt, 1] > 32767 * Q


def test_offset_counts_and_a_header_scale_quantum():
    ctx = context()
    x = buffer("i16")
    starts, ends = special_ranges()
    a2, e2 = aligned_ranges((0, 5))
    starts, ends = starts + a2, ends + e2
    for q, off in ((Q, 37), (HEADER_Q, 0), (HEADER_Q, -1234), (0.0305, 32767)):
        with tile(ctx, T):
            same_bits(ctx.range_stats(x, starts, ends, q, offset_counts=off), oracle(starts, ends, q, off))
    # float32 samples are absolute values: offset_counts is not added to them
    same_bits(ctx.range_stats(buffer("f32"), starts, ends, Q, offset_counts=37), oracle(starts, ends, Q, 0))


def test_seventy_thousand_one_sample_ranges_in_one_call():
    ctx = context()
    k = counts()
    starts = np.arange(N, dtype=np.int64)[::-1].copy()                 # (descending)
    for dtype in ("i16", "f32"):
        got = ctx.range_stats(buffer(dtype), starts, starts + 1, Q)
        level = k[starts].astype(np.float64) * Q
        assert got.shape == (N, 4)
        assert np.array_equal(got[:, 0], level) and np.array_equal(got[:, 2], level) and np.array_equal(got[:, 3], level)
        assert not got[:, 1].any()
    same_bits(got[:300], oracle(starts[:300], starts[:300] + 1, Q))


def test_refusals_name_the_range_and_leave_the_context_usable():
    import torch
    ctx = context()
    x = buffer("i16")
    ok_s, ok_e = [10, 20, 30], [15, 2000, 31]
    for starts, ends, index in (([10, -1, 30], [15, 5, 31], 1), ([10, 20, 69_999], [15, 25, N + 1], 2), ([10, 20], [15, 20], 1),
                                ([10, 20, 30], [15, 19, 31], 1), ([-5], [N + 5], 0), ([N], [N + 1], 0),
                                ([0, -2 ** 63], [1, 2 ** 63 - 1], 1), ([0, 2 ** 63 - 1], [1, -2 ** 63], 1)):
        with pytest.raises(ValueError, match=BAD_ARG) as err:
            ctx.range_stats(x, starts, ends, Q)
        assert "range %d:" % index in str(err.value)
        same_bits(ctx.range_stats(x, ok_s, ok_e, Q), oracle(ok_s, ok_e, Q))
    with pytest.raises(ValueError, match="one length"):
        ctx.range_stats(x, [1, 2], [3], Q)
    # float64 samples are not served; an off-grid float32 sample is reported as everywhere
    with pytest.raises(ValueError, match="float64"):
        ctx.range_stats(torch.zeros(100, dtype=torch.float64, device="cuda"), [0], [10], Q)
    off_grid = buffer("f32").clone()
    off_grid[1234] += Q / 4
    with pytest.raises(ValueError, match=r"status -6"):
        ctx.range_stats(off_grid, [1000], [2000], Q)
    same_bits(ctx.range_stats(off_grid, [0], [1234], Q), oracle([0], [1234], Q))
    # option range_tile: 64 .. 2^20
    for bad in (0, 63, (1 << 20) + 1, -512):
        with pytest.raises(ValueError):
            ctx.set_option("range_tile", bad)
    assert ctx.get_option("range_tile") == 16384
    # no ranges: nothing to do
    got = ctx.range_stats(x, [], [], Q)
    assert got.shape == (0, 4) and got.dtype == np.float64


def test_scratch_belongs_to_the_context():
    from pypore_amd import engine
    x = buffer("i16")
    starts, ends = aligned_ranges((1,))
    base = engine.live_bytes()
    cx = engine.Context(0)
    try:
        created = engine.live_bytes()
        cx.set_option("range_tile", T)
        first = cx.range_stats(x, starts, ends, Q)
        held = engine.live_bytes()
        assert held > created
        again = cx.range_stats(x, starts, ends, Q)
        assert engine.live_bytes() == held                  # a repeated call of the same size allocates nothing
        same_bits(first, again)
        cx.range_stats(x, starts[:5], ends[:5], Q)
        assert engine.live_bytes() == held
    finally:
        cx.close()
    assert engine.live_bytes() == base
