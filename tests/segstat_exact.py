"""Exact per-segment statistics and the checker for the device's K2 rows (Segment.mean / std / min / max).

The device works on integer counts k (int16 raw + offset_counts, or float32 / quantum, which lies on the grid), so the
statistics of a segment [a, b) have an exact form: S1 = sum k and S2 = sum k^2 as integers (Python ints here -- numpy
int64 only where the bound below says it cannot overflow), n = b - a, and

    mean = q S1 / n,    var = (n S2 - S1^2) / n^2 (in counts^2, population),    min / max = k_min q, k_max q.

No float accumulates anywhere; the only floats are the device's rows, compared as exact rationals (fractions.Fraction).

Where the device's bounds come from.  Both K2 kernels centre their sums on an integer count c -- segstat_bs_kernel on its
digest's centre m (the event's first count in the two calls, the trace's first count in the single pass), segstat_kernel
on the event's first count -- and form, with y = k - c, s1 = sum y and s2 = sum y^2 held EXACTLY in fp64 (true while
sum y^2 < 2^53; check_rows refuses a row for which neither centre satisfies it), with u = eps / 2 the unit roundoff:

    my = s1 / n                      |my - mu| <= u |mu|,            mu = S1 / n - c
    mean = (c + my) * q              |mean - q S1/n| <= |q| u (|mu| + 2 |S1/n|) + O(u^2) <= 1.5 eps (|S1/n| + |c|) |q|
    var = s2 / n - my * my           |var - V| <= u (V + mu^2) + 3 u mu^2 + u V = 2 u V + 4 u mu^2 + O(u^2)
    std = sqrt(var) * q              (std / q)^2 = var (1 + d), |d| <= 4 u (two roundings, squared)
                                     => |(std / q)^2 - V| <= 6 u V + 4 u mu^2 + O(u^2) <= 3 eps (V + mu^2)

(V the exact variance; a fused multiply-add only removes roundings, a clamp of var < 0 to 0 only moves var towards V >= 0).
The checker takes C = max(|k_ev0|, |k_tr0|) and D = max(|S1/n - k_ev0|, |S1/n - k_tr0|) so that either centre passes, and
allows 8 eps (|S1/n| + C) |q| on the mean and 16 eps (V + D^2) on the variance: five times the leading terms, which leaves
room for the O(u^2) terms and for a device sqrt or division that is off by a couple of ulps instead of half of one.  A
count missed or counted twice moves V by about V / n and the mean by (k - mean) / n: far beyond both bars for every n the
suite uses.  A formula about count 0 (c = 0, the old segstat_kernel) loses about eps S2 / n = eps (V + (S1/n)^2) to
cancellation, which the bar rejects as soon as (S1/n)^2 >> 16 (V + D^2): a quiet segment at a high level.

min and max must be bit-equal to float(k_min) * q and float(k_max) * q, the std of a constant segment exactly 0, and an
empty segment NaN in all four fields.
"""
from fractions import Fraction
import math

import numpy as np

EPS = Fraction(2) ** -52                       # np.finfo(np.float64).eps, exactly
MEAN_EPS = 8                                   # the bars of the docstring, in eps
VAR_EPS = 16
EXACT_LIMIT = 2 ** 53                          # the centred sum of squares must stay below this for the bound to hold
CHUNK = 1024                                   # samples per digest chunk (128 blocks of 8: seg_bs.hpp BS_CHUNK)


def counts_of(samples, q, offset_counts=0):
    """The integer counts the device sees: int16 raw + offset_counts, or float32 / q (asserted to lie on the grid)."""
    a = np.asarray(samples)
    if a.dtype == np.int16:
        return a.astype(np.int64) + int(offset_counts)
    k = a.astype(np.float64) / q
    kr = np.rint(k)
    assert np.array_equal(kr, k) and np.abs(kr).max(initial=0) < 2 ** 23, "float samples off the grid of q"
    return kr.astype(np.int64) + int(offset_counts)


def ranges_of(edges):
    """[(a, b)] of consecutive edges (0, boundaries..., n)."""
    e = np.asarray(edges, dtype=np.int64)
    return np.stack([e[:-1], e[1:]], axis=1)


class Exact(object):
    """Exact integer statistics of ranges [a, b) of the counts k: n, S1, S2 (Python ints), k_min, k_max."""

    def __init__(self, k, ranges, q):
        k = np.asarray(k, dtype=np.int64)
        assert k.size == 0 or np.abs(k).max() < 2 ** 31
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        self.q = float(q)
        self.a, self.b = r[:, 0], r[:, 1]
        self.n = [int(v) for v in self.b - self.a]
        # prefix sums: S1 in int64 (|k| < 2^31, n < 2^32); k^2 < 2^62 split into 31-bit halves, each prefix below 2^63
        c1 = np.concatenate(([0], np.cumsum(k)))
        sq = k * k
        lo, hi = sq & ((1 << 31) - 1), sq >> 31
        cl, ch = np.concatenate(([0], np.cumsum(lo))), np.concatenate(([0], np.cumsum(hi)))
        self.s1 = [int(v) for v in c1[self.b] - c1[self.a]]
        self.s2 = [(int(h) << 31) + int(l) for h, l in zip(ch[self.b] - ch[self.a], cl[self.b] - cl[self.a])]
        self.kmin, self.kmax = [], []
        for a, b in zip(self.a, self.b):
            self.kmin.append(int(k[a:b].min()) if b > a else None)
            self.kmax.append(int(k[a:b].max()) if b > a else None)

    def __len__(self):
        return len(self.n)

    def mean(self, i):
        return Fraction(self.s1[i], self.n[i]) * Fraction(self.q)

    def var(self, i):
        """Exact population variance in counts^2."""
        n, s1, s2 = self.n[i], self.s1[i], self.s2[i]
        return Fraction(n * s2 - s1 * s1, n * n)

    def floats(self):
        """(n, 4) float64: the exact statistics rounded once (mean, std, min, max) -- for comparisons at a loose bar."""
        out = np.full((len(self), 4), np.nan)
        for i in range(len(self)):
            if self.n[i]:
                out[i] = [float(self.mean(i)), math.sqrt(float(self.var(i))) * abs(self.q),
                          float(self.kmin[i]) * self.q, float(self.kmax[i]) * self.q]
        return out


def _centres(centres, m):
    c = np.asarray(centres, dtype=np.int64)
    if c.ndim == 1:
        c = np.broadcast_to(c.reshape(1, 2), (m, 2))
    assert c.shape == (m, 2)
    return c


def row_errors(rows, ref, centres):
    """Per row, None when the row passes the checks of the module docstring, else a short reason.  centres: (k_ev0, k_tr0)
    for all rows, or one such pair per row: the event's and the trace's first count."""
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.shape == (len(ref), 4), (rows.shape, len(ref))
    cen = _centres(centres, len(ref))
    q = ref.q
    qf = Fraction(q)
    out = []
    for i in range(len(ref)):
        mean, std, mn, mx = (float(v) for v in rows[i])
        n = ref.n[i]
        if n == 0:
            out.append(None if all(math.isnan(v) for v in (mean, std, mn, mx)) else "n = 0 but not NaN")
            continue
        if not all(math.isfinite(v) for v in (mean, std, mn, mx)):
            out.append("non-finite row %r" % (rows[i].tolist(),))
            continue
        s1, s2 = ref.s1[i], ref.s2[i]
        c_ev, c_tr = int(cen[i, 0]), int(cen[i, 1])
        if min(s2 - 2 * c * s1 + n * c * c for c in (c_ev, c_tr)) >= EXACT_LIMIT:
            raise ValueError("segment %d: the centred sums of squares leave 2^53 about both centres; the bound does not apply" % i)
        if mn != float(ref.kmin[i]) * q or mx != float(ref.kmax[i]) * q:
            out.append("min/max %r %r, want %r %r" % (mn, mx, float(ref.kmin[i]) * q, float(ref.kmax[i]) * q))
            continue
        mu = Fraction(s1, n)
        C = max(abs(c_ev), abs(c_tr))
        err = abs(Fraction(mean) - qf * mu)
        if err > MEAN_EPS * EPS * (abs(mu) + C) * abs(qf):
            out.append("mean off by %.3g eps (|S1/n| + C) |q|" % float(err / (EPS * (abs(mu) + C) * abs(qf))))
            continue
        V = Fraction(n * s2 - s1 * s1, n * n)
        if ref.kmin[i] == ref.kmax[i]:
            out.append(None if std == 0.0 else "constant segment with std %r" % std)
            continue
        D = max(abs(mu - c_ev), abs(mu - c_tr))
        s = Fraction(std) / qf
        err = abs(s * s - V)
        if err > VAR_EPS * EPS * (V + D * D):
            out.append("var off by %.3g eps (V + D^2)" % float(err / (EPS * (V + D * D))))
            continue
        out.append(None)
    return out


def check_rows(rows, ref, centres):
    """Boolean mask: which rows pass (row_errors)."""
    return np.array([e is None for e in row_errors(rows, ref, centres)], dtype=bool)


def assert_rows(rows, ref, centres, what=""):
    errs = row_errors(rows, ref, centres)
    bad = [(i, e) for i, e in enumerate(errs) if e is not None]
    if bad:
        shown = "; ".join("segment %d [%d, %d): %s" % (i, ref.a[i], ref.b[i], e) for i, e in bad[:6])
        raise AssertionError("%s: %d of %d rows fail the exact-statistics bar: %s" % (what, len(bad), len(errs), shown))


# ---- fp64 emulations of the two kernel formulas (CPU tests of the checker) ------------------------------------------
def emulate_rows(k, ranges, q, centre=None):
    """Rows as a K2 kernel forms them, in fp64 with exact sums: centred on `centre` (one int per range, or one for all)
    in the kernels' operation order (my = s1/n, var = s2/n - my*my, mean = (c + my) q), or about count 0 when centre is
    None -- the formula segstat_kernel used before it was centred (m = S1/n, var = S2/n - m*m, mean = m q)."""
    k = np.asarray(k, dtype=np.int64)
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    cs = np.zeros(len(r), dtype=np.int64) if centre is None else np.broadcast_to(np.asarray(centre, dtype=np.int64), (len(r),))
    out = np.full((len(r), 4), np.nan)
    for i, (a, b) in enumerate(r):
        n = int(b - a)
        if n <= 0:
            continue
        c = int(cs[i])
        y = k[a:b] - c
        s1 = float(int(y.sum()))
        s2 = float(Exact(y, [(0, n)], 1.0).s2[0])
        dn = float(n)
        my = s1 / dn
        var = s2 / dn - my * my
        if var < 0:
            var = 0.0
        mean = (float(c) + my) * q if centre is not None else my * q
        out[i] = [mean, math.sqrt(var) * q, float(int(k[a:b].min())) * q, float(int(k[a:b].max())) * q]
    return out


# ---- designed traces ---------------------------------------------------------------------------------------------
def step_counts(rng, lengths, levels, sigma):
    """Counts of consecutive segments of the given lengths and levels plus rounded normal noise of `sigma` counts
    (0: constant segments)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    k = np.repeat(np.asarray(levels, dtype=np.int64), lengths)
    if sigma > 0:
        k = k + np.rint(rng.normal(0.0, sigma, k.size)).astype(np.int64)
    return k


def geometry_lengths(rng, n_short=700):
    """Segment lengths for the narrow-route sweep: short ones (8..40, every residue pair mod 8), segments that end exactly
    on a 1024-sample chunk boundary (so the next starts on one), and long ones across one and across many chunks."""
    out, pos = [], 0

    def add(n):
        nonlocal pos
        out.append(int(n)); pos += int(n)

    for j in range(n_short):
        add(8 + (j * 7 + int(rng.integers(0, 33))) % 33)
        if j % 50 == 49:                        # up to the next chunk boundary, then across one and across several
            to_edge = -pos % CHUNK
            add(to_edge if to_edge >= 64 else to_edge + CHUNK)
            add(int(rng.integers(1100, 1900)))
            add(int(rng.integers(4000, 12000)))
    return out


def alternating_levels(rng, m, centre, step_lo, step_hi):
    """m levels about `centre`: each differs from the one before by step_lo..step_hi counts, alternating in sign."""
    lv = [int(centre)]
    for j in range(1, m):
        d = int(rng.integers(step_lo, step_hi + 1))
        lv.append(lv[-1] + (d if j % 2 else -d))
    return np.array(lv, dtype=np.int64)


def narrow_trace(seed, centre=1500, sigma=12.0):
    """The narrow-route geometry sweep: geometry_lengths at levels 150..400 counts apart, noise of `sigma` counts."""
    rng = np.random.default_rng(seed)
    ln = geometry_lengths(rng)
    return step_counts(rng, ln, alternating_levels(rng, len(ln), centre, 150, 400), sigma)


def quiet_trace(seed, n_seg=12, centre=30000, sigma=0.5):
    """Quiet segments at a high level: thousands of samples each, levels 3..6 counts apart, noise below one count."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(3000, 20000, n_seg)
    return step_counts(rng, ln, alternating_levels(rng, n_seg, centre, 3, 6), sigma)


def coverage(ranges, digest_start=0):
    """What a set of segments [a, b) covers, in the coordinates of their digest (block 0 of the digest at `digest_start`):
    residue pairs (a mod 8, b mod 8), lengths, and the chunk classes of segstat_bs_kernel."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2) - digest_start
    a, b = r[:, 0], r[:, 1]
    n = b - a
    ca, cb = a // CHUNK, np.maximum(b - 1, a) // CHUNK
    return dict(pairs={(int(x) % 8, int(y) % 8) for x, y in zip(a, b)},
                lengths={int(v) for v in n},
                in_one_chunk=bool(np.any((ca == cb) & (n >= 32))),
                across_one=bool(np.any(cb - ca == 1)),
                across_many=bool(np.any(cb - ca >= 3)),
                starts_on_chunk=bool(np.any((a % CHUNK == 0) & (a > 0) & (n >= 32))),
                ends_on_chunk=bool(np.any((b % CHUNK == 0) & (n >= 32))))


# ---- the public surface: Segment statistics of a float64 current x = fl(fl(k q) + offset) ----------------------------
def public_errors(segs, x, k, q, offset, centres):
    """Per Segment (of an event whose float64 current is x and whose counts are k), None or a reason.  The device row
    passes check_rows' bars; the host then adds `offset` to mean / min / max (one rounding, u |mean|), and x itself differs
    from k q + offset by at most E = u (|k q| + 2 |x|) per sample (the product and the sum each rounded), which moves the
    exact mean of x and its std (a seminorm: |std(a + e) - std(a)| <= max |e|) by at most E.  So:
    |mean - mean(x)| <= u |mean| + 8 eps (|S1/n| + C) |q| + E,  |std - std(x)| <= |q| sqrt(16 eps (V + D^2)) + E,
    min / max bit-equal to those of x (rounding is monotone)."""
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(k, dtype=np.int64)
    ranges = [(int(s.start), int(s.end)) for s in segs]
    ref = Exact(k, ranges, q)
    cen = _centres(centres, len(ref))
    qf, u = abs(Fraction(q)), EPS / 2
    out = []
    for i, s in enumerate(segs):
        a, b = ranges[i]
        n = b - a
        xs = x[a:b]
        if n == 0:
            out.append(None)
            continue
        if float(s.min) != xs.min() or float(s.max) != xs.max():
            out.append("min/max %r %r, x has %r %r" % (s.min, s.max, xs.min(), xs.max()))
            continue
        vals, cnt = np.unique(xs, return_counts=True)
        sx = sum(Fraction(float(v)) * int(c) for v, c in zip(vals, cnt))
        sxx = sum(Fraction(float(v)) ** 2 * int(c) for v, c in zip(vals, cnt))
        mean_x = sx / n
        var_x = sxx / n - mean_x * mean_x
        E = u * (int(np.abs(k[a:b]).max()) * qf + 2 * Fraction(float(np.abs(xs).max())))
        mu = Fraction(ref.s1[i], n)
        c_ev, c_tr = int(cen[i, 0]), int(cen[i, 1])
        C = max(abs(c_ev), abs(c_tr))
        tol = u * abs(Fraction(float(s.mean))) + MEAN_EPS * EPS * (abs(mu) + C) * qf + E
        if abs(Fraction(float(s.mean)) - mean_x) > tol:
            out.append("mean %r off by %.3g of its bound" % (s.mean, float(abs(Fraction(float(s.mean)) - mean_x) / tol)))
            continue
        V = ref.var(i)
        D = max(abs(mu - c_ev), abs(mu - c_tr))
        T = qf * Fraction(math.sqrt(float(VAR_EPS * EPS * (V + D * D)))) * (1 + EPS) + E
        sd = Fraction(float(s.std))
        lo = max(sd - T, Fraction(0))
        if not lo * lo <= var_x <= (sd + T) ** 2:
            out.append("std %r off beyond %.3g" % (s.std, float(T)))
            continue
        out.append(None)
    return out
