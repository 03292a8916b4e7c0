"""StatSplit's arithmetic restated on the host (test infrastructure): numpy float64 scalars, a Python recursion.

What is computed, in this order (include/poreseg.h: ps_statsplit_f64):
* c = cumsum(x), c2 = cumsum(x * x), ct = cumsum(x * t) with t = 0, 1, ... -- numpy's sequential chains;
* mean(P, a, b) = 0 if a == b, P[b-1] / b if a == 0, else (P[b-1] - P[a-1]) / (b - a);
* stepwise var(a, b) = mean(c2) - mean(c) * mean(c);
* slanted var(a, b) = the mean square residual of the least-squares line through samples a .. b-1, from y_bar, y2_bar,
  xy_bar, x_bar = a + (b - a - 1) / 2 and x2_bar = N / 6 with the exact integer N = 2b^2 + b(2a - 3) + 2a^2 - 3a + 1;
* gain(i) = (pe - ps) f(var(ps, pe)) - ((i - ps) f(var(ps, i)) + (pe - i) f(var(i, pe))), f = log or the identity;
* a window [ps, pe) of at least 2 mw samples splits at the candidate ps + mw .. pe - mw with the largest gain above
  min_gain_per_sample * window_width (strict), the lowest index among equal gains;
* windows start at start, start + W // 2, ... while ps < end - 2 mw; a window that starts beyond start + max_width forces
  a split at min(start + max_width, end - mw) and only the right part goes on; when no window splits, an interval longer
  than max_width is split there too and both parts go on.
"""
import numpy as np

F = np.float64


class Oracle(object):
    def __init__(self, x, min_width, max_width, window_width, min_gain_per_sample, use_log, splitter):
        x = np.asarray(x, dtype=np.float64)
        self.mw, self.maxw, self.W = int(min_width), int(max_width), int(window_width)
        self.thresh = min_gain_per_sample * window_width
        self.use_log = bool(use_log)
        self.slanted = splitter == "slanted"
        self.c = np.cumsum(x)
        self.c2 = np.cumsum(x * x)
        self.ct = np.cumsum(x * np.arange(x.size, dtype=np.float64)) if self.slanted else None
        self.windows = []          # (ps, pe, split or -1) of every window scanned

    @staticmethod
    def mean(P, a, b):
        if a == b:
            return F(0.0)
        if a == 0:
            return P[b - 1] / F(b)
        return (P[b - 1] - P[a - 1]) / F(b - a)

    def var(self, a, b):
        y_bar, y2_bar = self.mean(self.c, a, b), self.mean(self.c2, a, b)
        if not self.slanted:
            return y2_bar - y_bar * y_bar
        xy_bar = self.mean(self.ct, a, b)
        x_bar = F(a) + F(b - a - 1) / F(2.0)
        x2_bar = F(float(2 * b * b + b * (2 * a - 3) + 2 * a * a - 3 * a + 1)) / F(6.0)
        beta = (xy_bar - x_bar * y_bar) / (x2_bar - x_bar * x_bar)
        alpha = y_bar - beta * x_bar
        v = y2_bar - (F(2.0) * alpha) * y_bar
        v = v - (F(2.0) * beta) * xy_bar
        v = v + alpha * alpha
        v = v + ((F(2.0) * alpha) * beta) * x_bar
        return v + (beta * beta) * x2_bar

    def cost(self, a, b):
        v = self.var(a, b)
        return F(b - a) * (np.log(v) if self.use_log else v)

    def gains(self, ps, pe):
        """(candidates, gains) of the window [ps, pe)."""
        tot = self.cost(ps, pe)
        cand = range(ps + self.mw, pe + 1 - self.mw)
        return cand, [tot - (self.cost(ps, i) + self.cost(i, pe)) for i in cand]

    def best_split(self, ps, pe):
        if pe - ps < 2 * self.mw:
            return None
        with np.errstate(all="ignore"):
            cand, g = self.gains(ps, pe)
        best, x = self.thresh, None
        for i, gi in zip(cand, g):
            if gi > best:
                best, x = gi, i
        self.windows.append((ps, pe, -1 if x is None else x))
        return x

    def segment(self, start, end):
        mw, maxw = self.mw, self.maxw
        split = None
        for ps in range(start, end - 2 * mw, self.W // 2):
            if ps > start + maxw:
                at = min(start + maxw, end - mw)
                return [at] + self.segment(at, end)
            split = self.best_split(ps, min(end, ps + self.W))
            if split is not None:
                break
        if split is None:
            if end - start <= maxw:
                return []
            split = min(start + maxw, end - mw)
        return self.segment(start, split) + [split] + self.segment(split, end)


def segment(x, min_width, max_width, window_width, min_gain_per_sample, use_log, splitter, start=0, end=None):
    """The boundaries StatSplit(...).parse(x, start, end) places, as int32 positions in x."""
    o = Oracle(x, min_width, max_width, window_width, min_gain_per_sample, use_log, splitter)
    return np.array(o.segment(start, len(x) if end is None else end), dtype=np.int32)
