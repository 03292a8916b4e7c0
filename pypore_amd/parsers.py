"""Parser plug-ins: the objects File.parse / Event.parse accept (`parse(current) -> list[Segment]`).

Surface kept from the reference (PyPore/parsers.py; SURVEY.md 8 a7, a11, b): `SpeedyStatSplit` with its eight
constructor keywords stored as attributes of the same names (:505-534) -- they are also its JSON schema --,
`lambda_event_parser(threshold, rules)` (:124-155), `MemoryParse(starts, ends)` (:110-122) and the base `parser`
with `to_dict` / `to_json` / `from_json` / `parse` (:34-107); beside them `StatSplit` (:220-503) and the two state
parsers, `snakebase_parser` (:572-607) and `FilterDerivativeSegmenter` (:609-679).  The Qt GUI hooks are UI and out of scope.

How it is built here: every subclass of `parser` registers itself by name (that is what `from_json` resolves),
a parser's JSON is its public scalar attributes, and the two parsers that compute -- SpeedyStatSplit and the
event detector with its default rules -- hand the samples to the HIP kernels through pypore_amd.engine.
"""
import numbers

import numpy as np

from .core import Segment, dump_json, load_json, plain
from .cparsers import FastStatSplit

__all__ = ["parser", "MemoryParse", "lambda_event_parser", "PieceTable", "SpeedyStatSplit", "StatSplit", "snakebase_parser",
           "FilterDerivativeSegmenter", "FastStatSplit", "Segment"]

_REGISTRY = {}


class parser(object):
    """Base of the plug-ins.  Its own parse() returns the whole array as one segment."""

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        _REGISTRY[cls.__name__] = cls

    def __repr__(self):
        return self.to_json()

    def to_dict(self):
        """Public attributes that are plain scalars (numbers, strings, None), plus the class name: what the reference
        writes for the parsers in scope (rule lambdas and GUI widgets never reach its JSON either)."""
        d = {k: plain(v) for k, v in vars(self).items()
             if not k.startswith('_') and k != 'param_dict'
             and (v is None or isinstance(plain(v), (numbers.Number, str)))}
        d['name'] = type(self).__name__
        return d

    def to_json(self, filename=False):
        return dump_json(self.to_dict(), filename or None)

    def parse(self, current):
        return [Segment(current=current, start=0, duration=current.shape[0] / 100000)]

    @classmethod
    def from_json(cls, _json):
        """Parser of the class named in the JSON (text or *.json path), built from the remaining keys."""
        d = dict(load_json(_json))
        kind = _REGISTRY.get(d.pop('name'))
        if kind is None:
            raise AttributeError("no parser of that name in pypore_amd.parsers")
        return kind(**d)


_REGISTRY['parser'] = parser


class MemoryParse(object):
    """Replays stored split points: one Segment (copy of the samples) per (start, end) pair, in samples."""

    def __init__(self, starts, ends):
        self.starts = starts
        self.ends = ends

    def parse(self, current):
        spans = ((int(s), int(e), s, e) for s, e in zip(self.starts, self.ends))
        return [Segment(current=np.array(current[i:j], copy=True), start=s, duration=e - s) for i, j, s, e in spans]


class PieceTable(object):
    """Every piece a threshold cuts a trace into, as arrays (lambda_event_parser.pieces): `start`, `end`, `duration`, `n`
    (int64, in samples) and `min`, `max`, `mean`, `std` (float64, in pA), in the order of the trace.  `edges` are the P + 1
    cut positions and `stats` the (P, 4) rows in core.STAT_COLUMNS order; `offset` (the pA at count 0 of the upload) is added
    to mean, min and max -- the device's statistics are those of count * quantum -- and not to std."""

    def __init__(self, edges, stats, offset=0.0):
        self.edges = np.ascontiguousarray(edges, dtype=np.int64)
        stats = np.asarray(stats, dtype=np.float64).reshape(-1, 4)
        if self.edges.ndim != 1 or self.edges.size != stats.shape[0] + 1:
            raise ValueError("a table of P pieces has P + 1 edges")
        if offset:
            stats = stats + np.array([offset, 0.0, offset, offset])
        self.stats = stats
        self.start, self.end = self.edges[:-1], self.edges[1:]
        self.duration = self.n = self.end - self.start
        self.mean, self.std, self.min, self.max = (stats[:, j] for j in range(4))

    def __len__(self):
        return self.start.size

    def segments(self, current, mask=None):
        """The pieces (mask: those it selects) as Segments of `current`: slices of the caller's array, not copies, with the
        table's rows as their statistics (core.segments_from_edges)."""
        from .core import segments_from_edges
        if mask is None:
            return segments_from_edges(current, self.edges, self.stats)
        out = []
        for p in np.flatnonzero(np.asarray(mask, dtype=bool)).tolist():
            out.extend(segments_from_edges(current, self.edges[p:p + 2], self.stats[p:p + 1]))
        return out


def _host_table(x, threshold):
    """The PieceTable of a host array by numpy (where no count-space threshold reproduces x < threshold)."""
    x = np.asarray(x, dtype=np.float64)
    if not x.size:
        return PieceTable([0], np.zeros((0, 4)))
    below = x < threshold
    edges = np.concatenate(([0], np.flatnonzero(below[1:] != below[:-1]) + 1, [x.size]))
    n = np.diff(edges)
    mean = np.add.reduceat(x, edges[:-1]) / n
    dev = x - np.repeat(mean, n)
    std = np.sqrt(np.add.reduceat(dev * dev, edges[:-1]) / n)
    return PieceTable(edges, np.stack([mean, std, np.minimum.reduceat(x, edges[:-1]), np.maximum.reduceat(x, edges[:-1])], axis=1))


def _apply_rules(pieces, rules):
    """The pieces every rule accepts, in their order; each rule is called per piece, as the reference calls it."""
    from .core import gc_paused
    with gc_paused():
        return [piece for piece in pieces if all(rule(piece) for rule in rules)]


class lambda_event_parser(parser):
    """Threshold event detector.  The trace is cut wherever it crosses `threshold`; a piece is an event when every
    rule accepts it -- by default: longer than 100 000 samples, minimum above -0.5 pA, maximum below the threshold
    (the blockade side of the cut).  Start and duration of the returned Segments are in samples.

    on_device=True (an extension; it stays out of the JSON) runs rules of the caller's own on the GPU's piece table: one device
    call cuts the trace and computes every piece's statistics (ps_detect_pieces), the rules are then called per piece on
    Segments that carry those rows and slices of the caller's current.  Same pieces, order, start, duration and current as
    the host route and the same min and max; mean and std come from the device's exact integer sums (numpy's differ in the
    last bits).  With rules=None the flag changes nothing."""
    MIN_DURATION = 100000
    MIN_CURRENT = -0.5

    def __init__(self, threshold=90, rules=None, on_device=False):
        self.threshold = threshold
        self._builtin = rules is None
        self._on_device = bool(on_device)
        self.rules = rules or [lambda event: event.duration > self.MIN_DURATION,
                               lambda event: event.min > self.MIN_CURRENT,
                               lambda event: event.max < self.threshold]

    @property
    def _device_route(self):
        """parse() takes the samples to the GPU itself: hand it a file's counts, not its float64 current."""
        return self._builtin or self._on_device

    def parse(self, current, quantum=None, device=None, offset=None):
        """Built-in rules: one streaming pass on the GPU (ps_detect_events: crossings, then min / max of the long
        pieces).  Custom rules are Python callables on Segment objects: over numpy pieces on the host, or -- on_device=True --
        over the device's piece table."""
        if self._builtin:
            return self._parse_device(current, quantum, device, offset)
        if self._on_device and len(current):
            table, host = self._pieces(current, quantum, device, offset, fallback=False)
            if table is not None:
                return _apply_rules(table.segments(host), self.rules)
            return self._parse_host(np.asarray(host))
        return self._parse_host(np.asarray(current))

    def pieces(self, current, quantum=None, device=None, offset=None):
        """Every piece `threshold` cuts `current` into, as a PieceTable computed on the GPU -- whatever the parser's rules
        are; for callers who would rather filter with numpy than with lambdas."""
        return self._pieces(current, quantum, device, offset, fallback=True)[0]

    def _pieces(self, current, quantum, device, offset, fallback):
        """(PieceTable, the host values the Segments are cut from).  Float samples whose counts are not monotone across the
        threshold (detector_thresholds returns None) have no device table: numpy's with fallback, else None."""
        from . import engine
        if not len(current):
            return PieceTable([0], np.zeros((0, 4))), current
        s, thr, values, counts, on_device = self._stage(current, quantum, device, offset)
        if thr is None:
            return (_host_table(values, self.threshold) if fallback else None), values
        edges, stats = engine.context(device).detect_pieces(s.tensor, s.quantum, thr[0])
        return PieceTable(edges, stats, s.offset), self._host_values(current, s, values, counts, on_device)

    def _parse_host(self, x):
        below = x < self.threshold
        cuts = np.flatnonzero(below[1:] != below[:-1]) + 1
        edges = np.concatenate(([0], cuts, [x.shape[0]]))
        pieces = (Segment(current=np.array(x[a:b]), start=a, duration=b - a) for a, b in zip(edges[:-1], edges[1:]))
        return [piece for piece in pieces if all(rule(piece) for rule in self.rules)]

    def _stage(self, current, quantum, device, offset):
        """The upload both device routes take: (Samples, the thresholds in count space or None, the caller's values, the
        counts float samples went up as or None, whether the caller's samples were on the device)."""
        from . import engine
        s, counts = engine.to_device_with_counts(current, quantum, offset, device)
        # the kernel compares count * quantum with its arguments: the rules on the caller's pA values become thresholds in
        # count space (engine.detector_thresholds) -- from the formula the values came from (a file's counts, int16, a device
        # tensor, float samples on a power-of-two grid), or, for float samples that went up as the counts of another grid or
        # with an offset, from the samples and those counts
        on_device = hasattr(current, "is_cuda")
        values = current
        if on_device and counts is not None:        # a float64 tensor that went up as recovered counts: its own values, once
            values = current.detach().cpu().numpy()
        if counts is None:
            thr = engine.detector_thresholds(s.quantum, self.threshold, self.MIN_CURRENT, offset=s.offset)
        else:                                        # (None: not monotone in the counts at a threshold -- the rules on the host)
            thr = engine.detector_thresholds(s.quantum, self.threshold, self.MIN_CURRENT, values=values, counts=counts)
        return s, thr, values, counts, on_device

    @staticmethod
    def _host_values(current, s, values, counts, on_device):
        """What the returned Segments are cut from."""
        if on_device and counts is not None:        # (the events hold the caller's values, not count * quantum + offset again)
            return values
        if on_device:                               # device tensor in: the events' values come back as pA
            host = s.tensor.cpu().numpy().astype(np.float64)
            if not s.tensor.dtype.is_floating_point:
                host = host * s.quantum
            return host + s.offset
        from .grid import Deferred
        return current if isinstance(current, (np.ndarray, Deferred)) else np.asarray(current)

    def _parse_device(self, current, quantum, device, offset):
        from . import engine
        s, thr, values, counts, on_device = self._stage(current, quantum, device, offset)
        if thr is None:
            return self._parse_host(np.asarray(values))
        starts, lens = engine.context(device).detect_events(
            s.tensor, s.quantum, threshold=thr[0], min_duration=self.MIN_DURATION, min_current=thr[1])
        host = self._host_values(current, s, values, counts, on_device)
        # (slices, not copies: a GridArray -- or a current that has not been written out -- keeps its counts that way
        #  and Event.parse stays on the int16 route)
        return [Segment(current=host[a:a + n], start=a, duration=n) for a, n in zip(starts.tolist(), lens.tolist())]


class SpeedyStatSplit(parser):
    """The drop-in segmenter: stores the reference's eight parameters under the reference's names and runs
    FastStatSplit -- here the HIP kernels -- on parse().  Extra keywords (kept out of the JSON): `quantum` / `offset`
    describe the ADC grid of float input (pA per count, pA at count 0; found automatically when omitted), `device`
    picks the GPU, `off_grid` says what happens to float input that lies on NO grid (the reference takes any float64
    buffer, cparsers.pyx:53): "raise" (default) ValueError -- nothing is rounded silently --, "requantise" rounds it
    on the device to the finest power-of-two grid that keeps the counts below 2**22, "exact" segments it with
    the reference's own arithmetic -- its sequential fp64 cumsums and var_c expressions, on the device: the reference's
    boundaries on the same input by construction, tens of milliseconds per 1e6 samples --, "exact_on_near_tie" takes the fast
    route and the exact one only where that counted a near tie.  The last two also apply to FILTERED events (Event.parse,
    File.parse_events), whose current lies on no grid either."""

    def __init__(self, min_width=100, max_width=1000000, window_width=10000,
                 min_gain_per_sample=None, false_positive_rate=None,
                 prior_segments_per_second=None, sampling_freq=1.e5, cutoff_freq=None,
                 quantum=None, device=None, offset=None, off_grid="raise"):
        self.min_width = min_width
        self.max_width = max_width
        self.min_gain_per_sample = min_gain_per_sample
        self.window_width = window_width
        self.prior_segments_per_second = prior_segments_per_second
        self.false_positive_rate = false_positive_rate
        self.sampling_freq = sampling_freq
        self.cutoff_freq = cutoff_freq
        from .cparsers import OFF_GRID_MODES
        if off_grid not in OFF_GRID_MODES:
            raise ValueError("off_grid must be one of %s" % ", ".join(repr(m) for m in OFF_GRID_MODES))
        self._grid = dict(quantum=quantum, device=device, offset=offset, off_grid=off_grid)

    def _fast(self, cutoff=True):
        return FastStatSplit(self.min_width, self.max_width, self.window_width, self.min_gain_per_sample,
                             self.false_positive_rate, self.prior_segments_per_second, self.sampling_freq,
                             self.cutoff_freq if cutoff else None, **self._grid)

    def parse(self, current):
        return self._fast().parse(current)

    def parse_batch(self, currents, levels=None, near_ties_out=None, exact_from=None):
        """All events of a file in one device call (extension; same result as [parse(c) for c in currents]).  levels: the
        level in pA that was subtracted from each event upstream (Event.parse of a filtered event), or None.
        near_ties_out / exact_from: see cparsers.FastStatSplit.parse_batch."""
        return self._fast().parse_batch(currents, levels, near_ties_out=near_ties_out, exact_from=exact_from)

    def parse_exact(self, current):
        """The exact route for one float64 current (extension; cparsers.FastStatSplit.parse_exact_batch)."""
        return self._fast().parse_exact_batch([current])[0]

    @property
    def off_grid(self):
        return self._grid["off_grid"]

    def parse_filtered_batch(self, currents, order=1, cutoff=2000., sampling_freq=None, near_ties_out=None):
        """event.filter(order, cutoff); event.parse(self) for many events, on the device from end to end (extension).
        near_ties_out: a list that receives every event's near-tie sites (cparsers.FastStatSplit.parse_filtered_batch)."""
        return self._fast().parse_filtered_batch(currents, order, cutoff, self.sampling_freq if sampling_freq is None else sampling_freq,
                                                 near_ties_out=near_ties_out)

    def best_single_split(self, current):
        """(gain, index) of the best single split; like the reference wrapper, without cutoff_freq (:530-534)."""
        return self._fast(cutoff=False).best_single_split(current)


def _stage_f64(currents, dev):
    """Currents (numpy arrays, anything numpy.asarray takes -- a grid-backed current gives its float64 values --, or CUDA
    tensors) as float64 tensors on `dev`, with the host arrays the Segments are cut from."""
    import torch
    ts, srcs = [], []
    for cur in currents:
        if isinstance(cur, torch.Tensor):
            t = cur.to(dev, torch.float64).contiguous()
            src = cur.detach().cpu().numpy()
        else:
            src = cur if isinstance(cur, np.ndarray) else np.asarray(cur)
            a = np.ascontiguousarray(src, dtype=np.float64)
            if a.ndim != 1:
                raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
            t = torch.from_numpy(a).to(dev)
        ts.append(t)
        srcs.append(src)
    return ts, srcs


class StatSplit(parser):
    """The reference's older segmenter (parsers.py:220-503; "DEPRECATED: USE SPEEDYSTATSPLIT" there, but the only one that
    splits on the variance itself and the only one with a slanted model), on the GPU (ps_statsplit_f64, include/poreseg.h).

    It is not SpeedyStatSplit under another name: a window is scanned when it holds at least 2 * min_width samples (so one
    of exactly 2 * min_width has a single candidate; cparsers.pyx:164 refuses it), the threshold is min_gain_per_sample *
    window_width (not doubled), `use_log=False` compares variances instead of their logarithms, and `splitter="slanted"`
    models each side of a split as a straight line plus noise -- ramps and drifting levels.  The prefix sums are numpy's
    sequential cumsums and every expression is the reference's, operation for operation in float64: the reference's
    boundaries by construction, up to the last bit of the logarithm when use_log is set.

    Attributes carry the reference's names (they are the JSON schema).  Deliberate deviations from the reference:
    * splitter="slanted" with use_log=True works (the reference calls an undefined `log`: NameError);
    * a parser stays what it was built as: the reference's parse() overwrites `splitter` with a bound method, so that a
      second parse() of a slanted parser silently runs stepwise;
    * splitter="slanted" with an `end` short of len(current) raises ValueError, as the reference's broadcast of
      current * linspace(0, end, num=end) does;
    * a callable splitter raises NotImplementedError (the reference would call it; nothing on the device can);
    * no RecursionError on long traces: the recursion runs on an explicit stack on the device.
    Input: numpy arrays or float64 CUDA tensors (what SpeedyStatSplit.parse_exact_batch takes), converted to float64."""

    def __init__(self, min_width=1000, max_width=1000000, min_gain_per_sample=0.03, window_width=10000, use_log=True,
                 splitter="stepwise"):
        self.min_width = max(min_width, 1)
        self.max_width = max_width or 100 * min_width
        self.min_gain_per_sample = min_gain_per_sample
        self.window_width = window_width or 10 * min_width
        assert self.max_width >= self.min_width
        assert self.window_width >= 2 * self.min_width
        self.use_log = use_log
        self.splitter = splitter

    def _params(self):
        from . import _lib
        if callable(self.splitter):
            raise NotImplementedError("StatSplit: a callable splitter cannot run on the device; use 'stepwise' or 'slanted'")
        slanted = self.splitter == "slanted"
        return _lib.StatSplitParams(int(self.min_width), int(self.max_width), int(self.window_width),
                                    float(self.min_gain_per_sample * self.window_width), 1 if self.use_log else 0,
                                    _lib.PS_STATSPLIT_SLANTED if slanted else _lib.PS_STATSPLIT_STEPWISE)

    @staticmethod
    def _normalise(n, start, end):
        """start / end as subscripts of a current of n samples (parsers.py:263-268)."""
        if start < 0:
            start += n + 1
        if end < 0:
            end += n + 1
        return min(start, n), min(end, n)

    def _bounds(self, currents, ranges):
        """Boundaries (int32 numpy, positions in the current) per current, all in one device call; ranges: (start, end)
        per current, normalised.  Returns them with the host arrays the Segments are cut from."""
        import torch
        from . import engine
        params = self._params()
        ctx = engine.context(None)
        dev = torch.device("cuda", ctx.device)
        ts, srcs = _stage_f64(currents, dev)
        lens = np.array([t.numel() for t in ts], dtype=np.int64)
        lo = np.array([r[0] for r in ranges], dtype=np.int64)
        hi = np.array([r[1] for r in ranges], dtype=np.int64)
        if self.splitter == "slanted" and np.any(hi != lens):
            raise ValueError("operands could not be broadcast together: splitter='slanted' needs end == len(current)")
        if lo.size and (lo.min() < 0 or hi.min() < 0):
            raise ValueError("start / end before the first sample")
        if not lens.sum():
            return [np.zeros(0, dtype=np.int32) for _ in ts], srcs
        allt = ts[0] if len(ts) == 1 else torch.cat(ts)
        bounds, boff = ctx.statsplit_f64(allt, np.concatenate(([0], np.cumsum(lens)))[:-1], lens, params, lo=lo, hi=hi)
        b = bounds.cpu().numpy()
        return [b[boff[e]:boff[e + 1]] for e in range(len(ts))], srcs

    @staticmethod
    def _segments(src, b, start, end):
        edges = [start] + b.tolist() + [end]
        return [Segment(current=src[a:z_], start=a, duration=z_ - a) for a, z_ in zip(edges, edges[1:])]

    def parse(self, current, start=0, end=-1):
        """Segments current[start:end] (negative start / end count from len + 1, as in the reference).  Returns Segments
        with absolute `start` and `duration` in samples; their `current` is a view of the input."""
        start, end = self._normalise(len(current), start, end)
        (b,), (src,) = self._bounds([current], [(start, end)])
        return self._segments(src, b, start, end)

    def parse_batch(self, currents):
        """Many currents in one device call (extension): [parse(c) for c in currents]."""
        ranges = [(0, len(c)) for c in currents]
        bs, srcs = self._bounds(currents, ranges)
        return [self._segments(src, b, a, z_) for src, b, (a, z_) in zip(srcs, bs, ranges)]


class _SpanParser(parser):
    """What the two state parsers share: the currents of a call go to the device as one float64 array, the device returns
    (start, end) spans per current, and the Segments are cut on the host with the keywords the reference passes."""

    def _call(self, ctx, allt, starts, lens):
        raise NotImplementedError

    def _check(self, lens):
        pass

    def _spans(self, currents):
        lens = np.array([len(c) for c in currents], dtype=np.int64)
        self._check(lens)                                  # (before anything touches the device)
        import torch
        from . import engine
        ctx = engine.context(None)
        ts, srcs = _stage_f64(currents, torch.device("cuda", ctx.device))
        if not lens.sum():
            return [np.zeros((0, 2), dtype=np.int32) for _ in ts], srcs
        allt = ts[0] if len(ts) == 1 else torch.cat(ts)
        spans, soff = self._call(ctx, allt, np.concatenate(([0], np.cumsum(lens)))[:-1], lens)
        sp = spans.cpu().numpy()
        return [sp[soff[e]:soff[e + 1]] for e in range(len(ts))], srcs

    @staticmethod
    def _segments(src, spans):
        return [Segment(current=src[a:z_], start=a) for a, z_ in spans.tolist()]

    def parse(self, current):
        (sp,), (src,) = self._spans([current])
        return self._segments(src, sp)

    def parse_batch(self, currents):
        """Many currents in one device call (extension): [parse(c) for c in currents]."""
        sps, srcs = self._spans(currents)
        return [self._segments(src, sp) for src, sp in zip(srcs, sps)]


class snakebase_parser(_SpanParser):
    """The reference's snakebase_parser (parsers.py:572-607) on the GPU (ps_snakebase_f64, include/poreseg.h): what its
    parse() RETURNS.  With low = the positions j where |current[j + 1] - current[j]| < 1e-3, the segments are
    current[low[0]:low[1]], current[low[2]:low[3]], ... and, when low has an odd number of entries, current[low[-1]:n - 1];
    `start` is the left end, in samples.  The reference also forms a piecewise cumulative sum and the points where it
    passes `threshold` and then uses neither: the threshold has no influence on the result.  The attribute is kept (it is
    the parser's JSON); the cumulative sum is not computed."""

    def __init__(self, threshold=1.5):
        self.threshold = threshold

    def _call(self, ctx, allt, starts, lens):
        return ctx.snakebase_f64(allt, starts, lens)


class FilterDerivativeSegmenter(_SpanParser):
    """The reference's FilterDerivativeSegmenter (parsers.py:609-679) on the GPU (ps_filter_derivative_f64): a first-order
    Bessel low-pass at cutoff_freq run forward and backward, the absolute derivative of the result, blocks where it exceeds
    low_threshold, and the states between the blocks that are kept.  What parse() RETURNS, quirks included:
    * the edges of the blocks are paired in order, so when the derivative starts above low_threshold the pairs are the gaps
      between the blocks; an unpaired last edge is dropped;
    * a pair is kept when np.argmax(deriv[start:end]) > high_threshold: the INDEX of the maximum within the pair, not its
      value, is compared with the threshold.
    A current of 6 samples or fewer raises ValueError, as scipy's filtfilt does.  The device filter agrees with scipy to
    1e-11 of max|y|: a decision closer than that to its threshold may fall the other way.  Non-finite samples: undefined."""

    def __init__(self, low_threshold=1, high_threshold=2, cutoff_freq=1000., sampling_freq=1.e5):
        self.low_threshold = low_threshold
        self.high_threshold = high_threshold
        self.cutoff_freq = cutoff_freq
        self.sampling_freq = sampling_freq

    def _check(self, lens):
        if lens.size and lens.min() <= 6:
            raise ValueError("The length of the input vector x must be greater than padlen, which is 6.")

    def _params(self, prefiltered=False):
        from . import _lib
        return _lib.FilterDerivativeParams(float(self.low_threshold), float(self.high_threshold), float(self.cutoff_freq),
                                           float(self.sampling_freq), 1 if prefiltered else 0)

    def _call(self, ctx, allt, starts, lens):
        return ctx.filter_derivative_f64(allt, starts, lens, self._params())
