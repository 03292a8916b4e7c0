"""File / Event: the containers on either side of the segmenter.

Call contract kept from the reference (PyPore/DataTypes.py):
  File(filename) | File(current=, timestep=)   .second = 1000 / timestep, .events, .parse(parser)        (:567-602)
  Event(current, start, end, duration, second, file)   .filter(order, cutoff), .parse(parser), .segments   (:239-333)
  to_dict / to_json / from_json / to_meta on both, MetaEvent, Event.from_segments                         (:480-545, :683-796)
  Experiment(filenames).parse(event_detector, segmenter, filter_params), .files / .events / .segments; Sample   (:938-1049)
and the JSON schema of README.md:346-391 (tests/golden/readme_file.json); apply_hmm on Event / MetaEvent / Experiment
and HMM-guided parsing (:62-68, :276-333, :349-355, :990-995) with pypore_amd.hmm models decoded on the device.
Plotting and MySQL are out of scope.

Built here around three pieces: `encode()` turns any tree of records into JSON-able dicts (one recursive walk
instead of per-class loops), `_rebuild_event()` is the inverse for one event, and a File read from an .abf keeps
the int16 counts next to the float64 current (pypore_amd.grid), so that parsing stays on the 2 B/sample device route.
"""
import numpy as np

from .core import MetaSegment, Segment, SEGMENT_FIELDS, dump_json, fields_of, gc_paused, ignored, load_json, plain, raw_current
from .parsers import SpeedyStatSplit, StatSplit, lambda_event_parser, parser as _parser_base  # noqa: F401 (StatSplit: re-export)

EVENT_FIELDS = SEGMENT_FIELDS + ('filtered', 'filter_order', 'filter_cutoff', 'n', 'state_parser', 'segments')
FILE_FIELDS = ('filename', 'n', 'event_parser', 'mean', 'std', 'duration', 'start', 'end', 'events')


def encode(value):
    """Records (anything with to_dict) -> dicts, sequences -> lists, numpy scalars -> numbers, recursively."""
    if hasattr(value, 'to_dict'):
        value = value.to_dict()
    if isinstance(value, dict):
        return {k: encode(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [encode(v) for v in value]
    return plain(value)


def _parser_from(d):
    return _parser_base.from_json(dump_json(d)) if d is not None else None


def _observations(event, hmm, features):
    """What an HMM is handed for one event.  features None: the segment means as a 1-D array (the reference's call); a
    tuple of segment attribute names, e.g. ('mean', 'std', 'duration'): the (n, len(features)) array of those attributes
    as they stand now.  A pypore_amd.hmm.Model of n_dim > 1 needs `features`, as many as its n_dim (ValueError); any
    other object is not asked about its dimension."""
    from .hmm import Model
    n_dim = hmm.n_dim if isinstance(hmm, Model) else None
    if features is None:
        if n_dim is not None and n_dim > 1:
            raise ValueError("the model takes %d values per observation: pass features=, a tuple of %d segment attribute "
                             "names such as ('mean', 'std', 'duration')" % (n_dim, n_dim))
        return np.array([seg.mean for seg in event.segments], dtype=np.float64)
    if isinstance(features, str):
        raise ValueError("features must be a tuple of segment attribute names, got the string %r" % features)
    features = tuple(features)
    if n_dim is not None and len(features) != n_dim:
        raise ValueError("%d features for a model of n_dim = %d" % (len(features), n_dim))
    return np.array([[getattr(seg, name) for name in features] for seg in event.segments],
                    dtype=np.float64).reshape(-1, len(features))


def _apply_hmm(event, hmm, algorithm, features=None):
    """getattr(hmm, algorithm)(segment means), as the reference calls it (DataTypes.py:62-68, :349-355); with `features`
    the (n, D) array of those segment attributes instead (_observations)."""
    return getattr(hmm, algorithm)(_observations(event, hmm, features))


class MetaEvent(MetaSegment):
    """An event reduced to its numbers (and its MetaSegments)."""
    json_fields = EVENT_FIELDS

    def apply_hmm(self, hmm, algorithm='viterbi', features=None):
        """The HMM's `algorithm` ('viterbi', 'forward', 'backward', 'log_probability', 'forward_backward',
        'maximum_a_posteriori') on the segment means: for a pypore_amd.hmm.Model, (logp, path) / a log matrix / a float /
        (transitions, emissions) / (logp, path of one emitting state per segment), computed on the device.  features: a
        tuple of segment attribute names, e.g. ('mean', 'std', 'duration') -- the model is handed the (n, D) array of
        those instead of the means (a vector model, pypore_amd.hmm, of n_dim = D)."""
        return _apply_hmm(self, hmm, algorithm, features)

    def delete(self):
        for segment in self.__dict__.get('segments', []):
            segment.delete()
        self.__dict__.clear()


class Event(Segment):
    """A blockade event: its current, and after parse() its segments."""
    json_fields = EVENT_FIELDS
    # after a parse on the device: the near-tie sites of its segmentation, [(window_start, window_end, split)] in samples of
    # the event (engine.consistent_sites); None: not counted, or not segmented on the device.  Not persisted.
    near_ties = None

    def __init__(self, current, segments=(), **kwargs):
        segments = list(segments)
        if segments:                                     # an event assembled from segments owns their concatenation
            try:
                current = np.concatenate([seg.current for seg in segments])
            except (AttributeError, ValueError):
                current = []
        Segment.__init__(self, current, filtered=False, segments=segments, **kwargs)

    @property
    def n(self):
        return len(self.__dict__.get('segments') or ())

    # ---- Event.filter (DataTypes.py:258-274) ----------------------------------------------------------------
    def filter(self, order=1, cutoff=2000., quantum=None):
        """Bessel low-pass, cutoff relative to the Nyquist frequency of the file's sampling rate, run forward and
        backward (scipy.signal.filtfilt semantics) on the device; `current` becomes the float64 result.  Orders 1..8
        run on the device (1, the reference's default, by scans; 2..8 by segments with halos); higher orders raise
        ValueError.  The result no longer lies on the ADC grid: see parse.  Like the reference, this filters whatever
        `current` holds: a current on an ADC grid (what a file reader returns) goes up as counts, anything else -- an
        event that was filtered before (Experiment.parse twice on the same files), float64 data on no grid -- as float64."""
        if type(self) is not Event:
            raise TypeError("Cannot filter a metaevent. Must have the current.")
        import torch
        from . import engine
        cur = raw_current(self)
        s = None
        if not self.__dict__.get("filtered") or quantum is not None:
            try:
                s = engine.to_device(cur, quantum)
            except ValueError:
                if quantum is not None:
                    raise                                # the caller named a grid the data does not lie on
        if s is not None:
            ctx = engine.context(s.tensor.device.index)
            out = ctx.filter_bessel(s.tensor, s.quantum, cutoff=cutoff, sampling_freq=float(self.second), order=order)
            # (a DC offset passes a unit-gain low-pass unchanged: filter the counts, put the offset back)
            self.current = out.cpu().numpy() + s.offset if s.offset else out.cpu().numpy()
        else:
            # no grid: the float64 values themselves (a current still parked on the device stays there)
            t = getattr(cur, "tensor", None)
            off = 0.0
            if t is None or not t.is_cuda:
                a = np.ascontiguousarray(np.asarray(self.current), dtype=np.float64)
                if a.ndim != 1:
                    raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
                t = torch.from_numpy(a).cuda()
            else:
                # a parked tensor holds the current WITHOUT the file's offset (grid.Deferred.from_tensor(y, off), what
                # parse_events leaves behind): a unit-gain low-pass passes a constant unchanged, so it goes back on afterwards
                off = float(getattr(cur, "offset", 0.0) or 0.0)
            ctx = engine.context(t.device.index)
            out = ctx.filter_bessel(t.contiguous(), 1.0, cutoff=cutoff, sampling_freq=float(self.second), order=order).cpu().numpy()
            self.current = out + off if off else out
        self.filtered, self.filter_order, self.filter_cutoff = True, order, cutoff

    # ---- Event.parse (DataTypes.py:276-289, :333) -----------------------------------------------------------
    def parse(self, parser=None, hmm=None, features=None):
        """segments = parser.parse(current); every segment learns its event and is rescaled from samples to seconds
        with the file's sampling rate.

        With `hmm` (HMM-guided segmentation, DataTypes.py:292-330): the segment means go through hmm.viterbi, and runs of
        consecutive segments in the same hidden state are merged into one Segment.  The reference's loop is restated
        behaviour for behaviour, quirks included:
          * path entry i is compared with entry i+1; the path starts with the model's start state (and holds every
            silent state visited), so the comparisons are offset against the segments;
          * after a group closes, j = i (not i + 1): consecutive merged segments share their boundary segment;
          * the last group closes at i == n-2 and takes segments[-1] as its right edge;
          * a new segment starts at int(ledge.start * second) and ends at int(redge.start * second + redge.n), with
            `start` in SAMPLES (the scaling to seconds ran before the merge); `second` is the event's;
          * its hidden_state is the name of path entry j+1's state;
          * an event with fewer than two segments ends with no segments.
        A pypore_amd.hmm.Model is decoded on the device; any other object with a `viterbi` method is called the same
        way (duck typing; the reference accepts yahmm models only).  An impossible sequence (viterbi returns
        (-inf, None)) raises ValueError where the reference would fail on indexing None.  features: as for apply_hmm --
        the segment attributes hmm.viterbi is handed instead of the means; the merge is the same."""
        if parser is None:
            parser = SpeedyStatSplit(prior_segments_per_second=10)
        if hmm and not callable(getattr(hmm, "viterbi", None)):
            raise TypeError("hmm must be a pypore_amd.hmm.Model or have a viterbi method")
        self._segment(parser)
        if hmm:
            self.segments = self._merge_by_hmm(hmm, features)
        self.state_parser = parser

    def _merge_by_hmm(self, hmm, features=None):
        _, states = self.apply_hmm(hmm, features=features)
        second = self.second
        i, j, n, segments = 0, 0, len(self.segments), []
        if states is None and n >= 2:
            raise ValueError("the HMM gives the segment means probability zero: there is no Viterbi path to merge by")
        while i < n - 1:
            if states[i][1].name != states[i + 1][1].name or i == n - 2:
                ledge = self.segments[j]
                redge = self.segments[i] if i < n - 2 else self.segments[-1]
                s, e = int(ledge.start * second), int(redge.start * second + redge.n)
                segments.append(Segment(start=s, current=self.current[s:e], event=self, second=self.second,
                                        hidden_state=states[j + 1][1].name))
                j = i
            i += 1
        return segments

    def apply_hmm(self, hmm, algorithm='viterbi', features=None):
        """The HMM's `algorithm` ('viterbi', 'forward', 'backward', 'log_probability', 'forward_backward',
        'maximum_a_posteriori') on the segment means: for a pypore_amd.hmm.Model, (logp, path) / a log matrix / a float /
        (transitions, emissions) / (logp, path of one emitting state per segment), computed on the device.  features: a
        tuple of segment attribute names, e.g. ('mean', 'std', 'duration') -- the model is handed the (n, D) array of
        those instead of the means (a vector model, pypore_amd.hmm, of n_dim = D)."""
        return _apply_hmm(self, hmm, algorithm, features)

    def _segment(self, parser):
        if self.__dict__.get("filtered"):
            self.segments = self._parse_filtered(parser)
        else:
            # (our own segmenter takes the counts behind a current that has not been written out; any other parser gets
            #  the float64 array)
            if isinstance(parser, SpeedyStatSplit):
                nt = []
                self.segments = parser.parse_batch([raw_current(self)], near_ties_out=nt)[0]
                self.near_ties = nt[0]
            else:
                self.segments = parser.parse(self.current)
        rate = float(self.file.second)
        for segment in self.segments:
            segment.event = self
            segment.scale(rate)

    def _on_fine_grid(self):
        """A filtered current is float64 off every ADC grid, and the device segmenter works on exact integer sums.
        The current is centred on its mean (the gains are shift invariant) and rounded to the finest power-of-two grid
        that keeps every count below 2**22 (2**-18 pA for a 100 pA range): on the golden vectors recorded from the
        reference that reproduces every boundary the reference finds on the unrounded float64 current
        (tests/test_filter.py); coarser grids do not -- a heavily smoothed current has almost no variance left.
        Returns (rounded current, grid step, the level that was subtracted)."""
        cur = np.asarray(self.current, dtype=np.float64)
        centre = float(np.mean(cur)) if cur.size else 0.0
        span = float(np.max(np.abs(cur - centre))) if cur.size else 0.0
        step = 2.0 ** (int(np.ceil(np.log2(span * 1.01))) - 22) if span > 0 else 1.0
        centre = np.rint(centre / step) * step
        return np.rint((cur - centre) / step) * step, step, float(centre)

    def _adopt_filtered(self, segments):
        """Segments found on the rounded current keep views of the unrounded one and take their statistics from those."""
        for segment in segments:
            # (a state parser's segments carry the reference's keywords, `current` and `start`, and no `end`: snakebase_parser)
            start = int(segment.start)
            end = int(segment.end) if 'end' in segment.__dict__ else start + len(raw_current(segment))
            segment.current = self.current[start:end]
            segment.__dict__.pop('_gpu_stats', None)
        return segments

    def _parse_filtered(self, parser):
        return _segment_filtered([self], parser)[0]

    # ---- persistence ----------------------------------------------------------------------------------------
    def to_dict(self):
        return fields_of(self, self.json_fields)

    def to_json(self, filename=None):
        return dump_json(encode(self), filename)

    def to_meta(self):
        for segment in self.segments:
            segment.to_meta()
        self.freeze(SEGMENT_FIELDS + ('n',))
        self.__class__ = MetaEvent

    def delete(self):
        for segment in self.__dict__.get('segments', []):
            segment.delete()
        self.__dict__.clear()

    @classmethod
    def from_json(cls, _json):
        """Event from JSON text or a *.json path.  Without a `current` entry (what to_json writes) the result is a
        MetaEvent holding the stored numbers, its segments as MetaSegments and its parser rebuilt."""
        d = dict(load_json(_json))
        d.pop('name', None)
        if 'current' in d:
            return cls(np.asarray(d['current'], dtype=np.float64), start=d.get('start', 0))
        d['segments'] = [MetaSegment(**{k: v for k, v in sj.items() if k != 'name'}) for sj in d.get('segments', [])]
        if isinstance(d.get('state_parser'), dict):
            d['state_parser'] = _parser_from(d['state_parser'])
        return MetaEvent(**d)

    @classmethod
    def from_segments(cls, segments):
        """Event spanning `segments`.  With their currents at hand: the concatenation.  From metadata alone: a
        MetaEvent whose duration is the sum, whose mean is the duration-weighted mean and whose std pools the
        segment variances about their own means (what the reference's formulas at :538-545 are after; its own result
        there is an Event with an empty current)."""
        segments = list(segments)
        if all(hasattr(seg, 'current') for seg in segments):
            return cls(current=None, start=0, segments=segments)
        dur = float(sum(seg.duration for seg in segments))
        mean = sum(seg.mean * seg.duration for seg in segments) / dur
        std = float(np.sqrt(sum(seg.std ** 2 * seg.duration for seg in segments) / dur))
        return MetaEvent(start=0, duration=dur, mean=mean, std=std, n=len(segments), segments=segments, filtered=False)


def filter_events(events, order=1, cutoff=2000.):
    """`event.filter(order, cutoff)` for every Event of `events`, in as few device calls as their currents allow
    (engine.Context.filter_bessel_batch: one launch for a batch on the order-1 route): every event ends as Event.filter would
    leave it -- the same float64 `current`, bit for bit, `filtered`, `filter_order`, `filter_cutoff`.  The events are routed
    as Event.filter routes one:
      * a current on an ADC grid goes up as counts.  Events cut from one file are stretches of the file's one device tensor
        and take one call per file tensor, nothing is copied; counts of any other origin (a GridArray, float samples whose
        grid is found) are packed into one tensor per grid and sampling rate; the offset is put back afterwards;
      * everything else -- an event that was filtered before, float64 data on no grid -- is packed into one float64 tensor
        per sampling rate.
    One download per group.  A MetaEvent raises Event.filter's TypeError, before anything is filtered."""
    import torch
    from . import engine
    from .grid import grid_of
    events = list(events)
    for ev in events:
        if type(ev) is not Event:
            raise TypeError("Cannot filter a metaevent. Must have the current.")
    dev = torch.device("cuda", torch.cuda.current_device())
    # group key -> [(event, tensor or (first sample, length) of the group's base tensor, offset to put back)]
    stretched, packed = {}, {}
    for ev in events:
        cur = raw_current(ev)
        rate = float(ev.second)
        s = None
        if not ev.__dict__.get("filtered"):
            stretch = getattr(cur, "device_stretch", None)
            g = grid_of(cur) if stretch is not None else None
            where = stretch(dev, engine._int_counts_tensor) if g is not None else None
            if where is not None:
                base, a0, n0 = where
                stretched.setdefault((base.data_ptr(), float(g[1]), rate), [base]).append((ev, a0, n0, float(g[2])))
                continue
            try:
                s = engine.to_device(cur, None)
            except ValueError:
                s = None
        if s is not None:
            packed.setdefault((s.tensor.dtype, float(s.quantum), rate, s.tensor.device.index), []).append((ev, s.tensor, float(s.offset or 0.0)))
            continue
        t = getattr(cur, "tensor", None)
        off = 0.0
        if t is None or not t.is_cuda:
            a = np.ascontiguousarray(np.asarray(ev.current), dtype=np.float64)
            if a.ndim != 1:
                raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
            t = torch.from_numpy(a)
        else:
            # (a parked tensor holds the current WITHOUT the file's offset: Event.filter)
            off = float(getattr(cur, "offset", 0.0) or 0.0)
        packed.setdefault((torch.float64, 1.0, rate, t.device.index if t.is_cuda else dev.index), []).append((ev, t, off))

    def finish(members, y, offsets):
        y = y.cpu().numpy()                              # (one download per group)
        for k, (ev, off) in enumerate(members):
            out = y[int(offsets[k]):int(offsets[k + 1])]
            # (a DC offset passes a unit-gain low-pass unchanged: filter the counts, put the offset back)
            ev.current = out + off if off else out
            ev.filtered, ev.filter_order, ev.filter_cutoff = True, order, cutoff

    for (_, quantum, rate), group in stretched.items():
        base, members = group[0], group[1:]
        y, offsets = engine.context(base.device.index).filter_bessel_batch(
            base, [a0 for _, a0, _, _ in members], [n0 for _, _, n0, _ in members], quantum, cutoff=cutoff, sampling_freq=rate, order=order)
        finish([(ev, o) for ev, _, _, o in members], y, offsets)
    for (dtype, quantum, rate, index), members in packed.items():
        where = torch.device("cuda", index)
        # (a host array goes up on its own: one pinned staging copy of the whole group would cost a second pass over it)
        ts = [t.to(where).contiguous() for _, t, _ in members]
        lens = np.array([t.numel() for t in ts], dtype=np.int64)
        allt = ts[0] if len(ts) == 1 else torch.cat(ts)
        y, offsets = engine.context(index).filter_bessel_batch(allt, np.concatenate(([0], np.cumsum(lens)))[:-1], lens, quantum, cutoff=cutoff,
                                                               sampling_freq=rate, order=order)
        finish([(ev, o) for ev, _, o in members], y, offsets)


def state_name_ids(states):
    """(ids, names) of a model's states: ids[k] = the index into `names` of states[k].name, so equal names share an id (the
    reference's merge compares path entries by state NAME: two states that share one do not end a group)."""
    seen, ids = {}, np.empty(len(states), dtype=np.int64)
    for k, state in enumerate(states):
        ids[k] = seen.setdefault(state.name, len(seen))
    return ids, list(seen)


def merge_ranges(seg_start, seg_n, path, name_ids, second):
    """The reference's HMM-guided merge (DataTypes.py:292-330; Event._merge_by_hmm restates it as a loop) for one event, in
    numpy and without a loop over the segments.  seg_start: the segments' starts in SECONDS, seg_n: their sample counts, path:
    the Viterbi path as state indices (start state first, silent states included: at least as many entries as segments),
    name_ids: state index -> name id (state_name_ids).  Returns (s, e, hidden) int64 arrays, one entry per merged segment:
    first and end sample in the event, name id of its hidden state.  Quirks kept: entry i is compared with entry i + 1 by name;
    after a group closes j = i, so consecutive merged segments share their boundary segment and overlap; the last group
    closes at i == n - 2 and ends with the last segment; the hidden state is entry j + 1's; fewer than two segments give
    nothing; s = int(start_j * second) and e = int(start_r * second + n_r) are these two float64 expressions, truncated --
    (a / second) * second falls just below a for about 8 % of the sample indices, and then s = a - 1."""
    n = len(seg_n)
    none = np.zeros(0, dtype=np.int64)
    if n < 2:
        return none, none, none
    start = np.asarray(seg_start, dtype=np.float64)
    count = np.asarray(seg_n).astype(np.float64)
    nid = np.asarray(name_ids, dtype=np.int64)[np.asarray(path, dtype=np.int64)[:n]]
    close = nid[:n - 2] != nid[1:n - 1]                      # i = 0 .. n - 3: path entry i against entry i + 1
    i = np.concatenate((np.flatnonzero(close), [n - 2]))     # ... and i = n - 2 always closes
    j = np.concatenate(([0], i[:-1]))
    r = i.copy()
    r[-1] = n - 1                                            # (i < n - 2: segments[i]; the last group: segments[-1])
    second = float(second)
    s = np.trunc(start[j] * second).astype(np.int64)
    e = np.trunc(start[r] * second + count[r]).astype(np.int64)
    return s, e, nid[j + 1]


def _viterbi_paths(events, hmm, features):
    """[path or None per event] from ONE hmm.viterbi_batch call when the object has one, else hmm.viterbi per event."""
    obs = [_observations(ev, hmm, features) for ev in events]
    batch = getattr(hmm, "viterbi_batch", None)
    results = batch(obs) if callable(batch) else [hmm.viterbi(o) for o in obs]
    return [path for _, path in results]


def merge_by_hmm(events, hmm, features=None):
    """`ev.segments = ev._merge_by_hmm(hmm, features)` for every Event of `events` (HMM-guided segmentation, DataTypes.py:
    292-330, of events that are segmented already), in as few device calls as their currents allow:
      * one hmm.viterbi_batch call for all events (a pypore_amd.hmm.Model: one launch); an object with `viterbi` only is
        called per event, duck-typed as Event.parse takes it;
      * the merge itself in numpy (merge_ranges);
      * unfiltered events that are stretches of one file tensor (the grouping of filter_events) take their merged segments'
        mean / std / min / max from ONE engine.Context.range_stats call per file tensor: a merged Segment holds the same
        deferred stretch of the file's counts that parse_events' segments hold, and the file's float64 current is not written
        out.  Filtered events and events whose current is a host array keep what Event.parse does: a view of ev.current, lazy
        numpy statistics.
    Every merged segment has start (in samples, as the reference leaves it), event, second and hidden_state as _merge_by_hmm
    sets them.  Raised before any event is changed: TypeError for a MetaEvent and for an hmm without `viterbi`; ValueError,
    naming the event's index, for an event of two or more segments that the model gives probability zero."""
    if not hmm or not callable(getattr(hmm, "viterbi", None)):
        raise TypeError("hmm must be a pypore_amd.hmm.Model or have a viterbi method")
    events = list(events)
    for ev in events:
        if type(ev) is not Event:
            raise TypeError("Cannot merge the segments of a metaevent. Must have the current.")
    paths = _viterbi_paths(events, hmm, features)
    for k, (ev, path) in enumerate(zip(events, paths)):
        if path is None and len(ev.segments) >= 2:
            raise ValueError("event %d: the HMM gives the segment means probability zero: there is no Viterbi path to merge by" % k)
    states = getattr(hmm, "states", None)
    if states is not None:
        ids, names = state_name_ids(states)
    else:
        ids, names, seen = None, [], {}                  # (a model that shows no state list: the names the paths hold)
    merged = []
    for ev, path in zip(events, paths):
        n = len(ev.segments)
        if n < 2:
            merged.append(merge_ranges((), (), (), (), ev.second))
            continue
        if ids is not None:
            idx, table = [entry[0] for entry in path[:n]], ids
        else:
            idx = [seen.setdefault(entry[1].name, len(seen)) for entry in path[:n]]
            table = np.arange(len(seen), dtype=np.int64)
        merged.append(merge_ranges([seg.start for seg in ev.segments], [seg.n for seg in ev.segments], idx, table, ev.second))
    if ids is None:
        names = list(seen)
    # the events whose counts are parked on the device as stretches of one tensor: one range_stats call per tensor
    rows = [None] * len(events)
    stretched = {}
    if any(len(m[0]) for m in merged):
        stretched = _device_stretches([(k, ev) for k, ev in enumerate(events) if len(merged[k][0]) and not ev.__dict__.get("filtered")])
    for (_, quantum, offset), group in stretched.items():
        base, members = group[0], group[1:]
        lo = np.concatenate([a0 + np.clip(merged[k][0], 0, n0) for k, a0, n0 in members])
        hi = np.concatenate([a0 + np.clip(merged[k][1], 0, n0) for k, a0, n0 in members])
        ok = hi > lo                                         # (an empty slice has no statistics: numpy's nan, as in the loop)
        from . import engine
        stats = engine.context(base.device.index).range_stats(base, lo[ok], hi[ok], quantum)
        if offset:
            stats[:, [0, 2, 3]] += offset
        at = np.concatenate(([0], np.cumsum(ok)))
        pos = 0
        for k, _, _ in members:
            m = len(merged[k][0])
            rows[k] = [stats[at[pos + q]] if ok[pos + q] else None for q in range(m)]
            pos += m
    with gc_paused():
        for k, ev in enumerate(events):
            s, e, hid = merged[k]
            # (an event that ends with no segments is not asked for its current: that would write a file's out)
            cur = None if not len(s) else raw_current(ev) if rows[k] is not None else ev.current
            out = []
            for q in range(len(s)):
                seg = Segment(start=int(s[q]), current=cur[int(s[q]):int(e[q])], event=ev, second=ev.second, hidden_state=names[hid[q]])
                if rows[k] is not None and rows[k][q] is not None:
                    seg.__dict__['_gpu_stats'] = rows[k][q]
                out.append(seg)
            ev.segments = out


def _device_stretches(members):
    """{(base tensor's address, quantum, offset): [base tensor, (key, first sample, length) ...]} for the (key, event) pairs
    whose current is a stretch of a file's counts parked on the current device -- the grouping of filter_events; the pairs
    whose current is anything else are left out."""
    import torch
    from . import engine
    from .grid import grid_of
    out = {}
    dev = None
    for key, ev in members:
        cur = raw_current(ev)
        stretch = getattr(cur, "device_stretch", None)
        if stretch is None or getattr(cur, "counts", None) is None:
            continue
        g = grid_of(cur)
        if g is None:
            continue
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        where = stretch(dev, engine._int_counts_tensor)
        if where is not None:
            base, a0, n0 = where
            out.setdefault((base.data_ptr(), float(g[1]), float(g[2])), [base]).append((key, a0, n0))
    return out


def _segment_filtered(events, parser):
    """Segments of already-filtered events (float64 currents on no ADC grid) with `parser`, in event order.  Every current
    is centred and rounded onto a fine grid (Event._on_fine_grid), and the events that share a grid step are segmented
    together.  A SpeedyStatSplit also gets the unrounded currents, for its off_grid policy (cparsers.FastStatSplit.
    _fast_or_exact), and sets each event's near_ties; when that policy makes no fast call nothing is rounded and all
    events go to its exact route in one call.  Any other parser gets the rounded currents.  The segments hold views of the unrounded
    currents and take their statistics from those (Event._adopt_filtered)."""
    if not events:
        return []
    ours = isinstance(parser, SpeedyStatSplit)
    values = [np.asarray(ev.current, dtype=np.float64) for ev in events] if ours else None
    if ours and not parser._fast()._fast_call:
        for ev in events:
            ev.near_ties = None
        return [ev._adopt_filtered(segs) for ev, segs in zip(events, parser._fast().parse_exact_batch(values))]
    by_step = {}
    for k, ev in enumerate(events):
        rounded, step, centre = ev._on_fine_grid()
        by_step.setdefault(step, []).append((k, rounded, centre))
    found = [None] * len(events)
    for group in by_step.values():
        ks = [k for k, _, _ in group]
        currents = [r for _, r, _ in group]
        if ours:
            # (the level goes along: the device judges near ties against the noise of the reference's cumsums, which run on
            #  the uncentred current -- include/poreseg.h, ps_sample_format)
            nt = []
            segs = parser.parse_batch(currents, [c for _, _, c in group], near_ties_out=nt, exact_from=[values[k] for k in ks])
            for k, sites in zip(ks, nt):
                events[k].near_ties = sites
        elif hasattr(parser, "parse_batch"):
            segs = parser.parse_batch(currents)          # a user's parser with the one-argument parse_batch of earlier rounds
        else:
            segs = [parser.parse(c) for c in currents]
        for k, sg in zip(ks, segs):
            found[k] = events[k]._adopt_filtered(sg)
    return found


class File(Segment):
    """One recording: the current of an .abf file (or an array with its time step in ms) and the events found in it."""
    json_fields = FILE_FIELDS

    def __init__(self, filename=None, current=None, timestep=None, **kwargs):
        if current is not None and timestep is not None:
            filename = ""
        elif filename and current is None and timestep is None:
            from .abf import read_abf_counts
            from .grid import Deferred
            # The reference's reader returns float64 pA (read_abf.py:208-212).  Here the array is written out when
            # somebody reads `file.current` (a GridArray then, as from abf.read_abf); detection and segmentation take
            # the file's int16 counts and never ask for it: 0.10 s of an 0.21 s Experiment.parse on a 1e8-sample file.
            timestep, counts, scale, offset = read_abf_counts(filename)
            current = Deferred.from_counts(counts, scale, offset)
            filename = filename.split("\\")[-1]
            filename = filename[:-4] if filename.endswith(".abf") else filename
        else:
            raise SyntaxError("Must provide current and timestep, or filename corresponding to a valid abf file.")
        Segment.__init__(self, current=current, filename=filename, second=1000. / timestep, events=[], sample=None)

    def __getitem__(self, index):
        return self.events[index]

    @property
    def n(self):
        return len(self.events)

    def parse(self, parser=None):
        """Event detection: one Event per Segment the parser returns, its start / end / duration in seconds."""
        if parser is None:
            parser = lambda_event_parser(threshold=90)
        rate = self.second
        device_route = isinstance(parser, lambda_event_parser) and parser._device_route
        self.events = [Event(current=raw_current(seg), start=seg.start / rate, end=(seg.start + seg.duration) / rate,
                             duration=seg.duration / rate, second=rate, file=self)
                       for seg in parser.parse(raw_current(self) if device_route else self.current)]
        self.event_parser = parser

    def filter_events(self, order=1, cutoff=2000.):
        """`event.filter(order, cutoff)` for every event of the file, batched on the device (DataTypes.filter_events): the
        filtered currents of a file's events without segmenting them, in one call per file tensor."""
        filter_events(self.events, order=order, cutoff=cutoff)

    def parse_events(self, parser=None, filter_params=None, hmm=None, features=None):
        """The inner loop of Experiment.parse (DataTypes.py:975-984) for this file: every event is filtered when
        `filter_params` = (order, cutoff) is given, then all events are segmented in as few device calls as their
        representations allow -- one for unfiltered events, one per grid step for filtered ones (events of one file span
        similar ranges and mostly share a step).  Same result as `event.filter(...); event.parse(parser)` per event.
        With a SpeedyStatSplit the filtered currents never leave the device between the two steps
        (parse_filtered_batch: filter, re-quantisation and segmentation on the device, one copy of the float64 result
        back for Event.current).

        hmm (HMM-guided segmentation, as Event.parse(parser, hmm=model)): after the segmentation the segment means of ALL events
        go through the model in one viterbi_batch call and runs of segments in one hidden state are merged (merge_by_hmm; the
        statistics of the merged segments of unfiltered events come from one device call, the file's current stays unwritten).
        features: the segment attributes a vector model is handed instead of the means.  Same result as
        `event.parse(parser, hmm=hmm, features=features)` per event."""
        if hmm and not callable(getattr(hmm, "viterbi", None)):
            raise TypeError("hmm must be a pypore_amd.hmm.Model or have a viterbi method")
        with gc_paused():                                # (one pause for the file: re-enabling after every event costs a
            self._parse_events(parser, filter_params)    #  collection each time, 0.5 ms x the number of events)
            if hmm:
                merge_by_hmm(self.events, hmm, features)

    def _parse_events(self, parser, filter_params):
        if parser is None:
            parser = SpeedyStatSplit(prior_segments_per_second=10)
        rate = float(self.second)
        if filter_params is not None and hasattr(parser, "parse_filtered_batch") and all(type(ev) is Event for ev in self.events):
            # filter -> grid -> segments without leaving the device: only the filtered float64 currents come back
            order, cutoff = (tuple(filter_params) + (2000.,))[:2] if len(tuple(filter_params)) else (1, 2000.)
            sites = []
            if isinstance(parser, SpeedyStatSplit):
                done = parser.parse_filtered_batch([raw_current(ev) for ev in self.events], order, cutoff, rate, near_ties_out=sites)
            else:
                done = parser.parse_filtered_batch([raw_current(ev) for ev in self.events], order, cutoff, rate)
            for k, ev in enumerate(self.events):
                if sites:
                    ev.near_ties = sites[k]
            for ev, (cur, segs) in zip(self.events, done):
                ev.current = cur
                ev.filtered, ev.filter_order, ev.filter_cutoff = True, order, cutoff
                ev.segments = segs
                for segment in segs:
                    segment.event = ev
                    segment.scale(rate)
                ev.state_parser = parser
            return
        if filter_params is not None:
            if all(type(ev) is Event for ev in self.events) and len(tuple(filter_params)) <= 2:
                filter_events(self.events, *filter_params)
            else:                                        # (a MetaEvent raises where the loop reaches it; a third entry names a grid)
                for ev in self.events:
                    ev.filter(*filter_params)
        batched = hasattr(parser, "parse_batch")
        results = [None] * len(self.events)
        plain_idx = [i for i, ev in enumerate(self.events) if not ev.__dict__.get("filtered")]
        currents = [raw_current(self.events[i]) if batched else self.events[i].current for i in plain_idx]
        ours = isinstance(parser, SpeedyStatSplit)
        nt = []
        for i, segs in zip(plain_idx, parser.parse_batch(currents, near_ties_out=nt) if ours else
                           parser.parse_batch(currents) if batched else [parser.parse(c) for c in currents]):
            results[i] = segs
        for i, sites in zip(plain_idx, nt):
            self.events[i].near_ties = sites
        filtered_idx = [i for i, ev in enumerate(self.events) if ev.__dict__.get("filtered")]
        for i, segs in zip(filtered_idx, _segment_filtered([self.events[i] for i in filtered_idx], parser)):
            results[i] = segs
        for ev, segs in zip(self.events, results):
            ev.segments = segs
            for segment in segs:
                segment.event = ev
                segment.scale(rate)
            ev.state_parser = parser

    # ---- persistence ----------------------------------------------------------------------------------------
    def to_dict(self):
        if 'end' not in self.__dict__ and 'start' in self.__dict__ and 'duration' in self.__dict__:
            self.end = self.start + self.duration
        return fields_of(self, self.json_fields)

    def to_json(self, filename=None):
        """The file, its event parser, and every event with its segments and state parser (README.md:346-391)."""
        return dump_json(encode(self), filename)

    def to_meta(self):
        self.__dict__.pop('current', None)
        for event in self.events:
            event.to_meta()

    def delete(self):
        for event in self.__dict__.get('events', []):
            event.delete()
        self.__dict__.clear()

    @classmethod
    def from_json(cls, _json):
        """Rebuilds a stored analysis (JSON text or *.json path).  If `<filename>.abf` can be read, events and segments
        get views of its current again and filtered events are filtered again; otherwise everything comes back as
        MetaEvent / MetaSegment."""
        d = load_json(_json)
        if d.get('name') != "File":
            raise TypeError("JSON does not encode a file")
        try:
            file = cls(filename=d['filename'] + ".abf")
            meta = False
        except Exception:
            file = cls(current=[], timestep=1)
            file.filename = d.get('filename', "")
            del file.current                            # nothing to take statistics of: the stored numbers are all there is
            meta = True
        if 'event_parser' in d:
            file.event_parser = _parser_from(d['event_parser'])
        file.events = [_rebuild_event(file, ej, meta) for ej in d.get('events', [])]
        return file


def _rebuild_event(file, ej, meta):
    """One event of a stored analysis: MetaEvent from the numbers, or Event on views of the file's current."""
    segs = ej.get('segments', [])
    filtered = bool(ej.get('filtered', False))
    state_parser = _parser_from(ej.get('state_parser'))
    if meta:
        event = MetaEvent(**{k: v for k, v in ej.items() if k not in ('name', 'segments', 'state_parser')})
        event.segments = [MetaSegment(**{k: v for k, v in sj.items() if k != 'name'}) for sj in segs]
    else:
        rate = file.second
        a, b = int(ej['start'] * rate), int(ej['end'] * rate)
        event = Event(current=file.current[a:b], start=a / rate, end=b / rate, duration=(b - a) / rate,
                      second=rate, file=file)
        if filtered:
            event.filter(order=ej['filter_order'], cutoff=ej['filter_cutoff'])
        event.segments = [Segment(current=event.current[int(sj['start'] * rate):int(sj['end'] * rate)], second=rate,
                                  event=event, **{k: v for k, v in sj.items() if k != 'name'}) for sj in segs]
    event.filtered = filtered
    if state_parser is not None:
        event.state_parser = state_parser
    return event


class Experiment(object):
    """Several recordings analysed together (DataTypes.py:938-1037): `parse` opens one file after the other, detects its
    events, filters and segments them, and keeps the files; `.events` / `.segments` run over all of them.

    `filenames` may also hold File objects (e.g. built from arrays), which are taken as they are.  Per file the events
    go to the device together (File.parse_events) instead of one by one."""

    def __init__(self, filenames, name=None):
        self.filenames = filenames
        self.name = name or "Experiment"
        self.files = []

    _DEFAULT = object()

    def parse(self, event_detector=None, segmenter=_DEFAULT, filter_params=(1, 2000), verbose=True, meta=False, workers=None,
              hmm=None, features=None):
        """Defaults as in the reference (:956-960): lambda_event_parser(threshold=90), SpeedyStatSplit with
        prior_segments_per_second=10 and cutoff_freq=2000, a first-order 2 kHz Bessel filter.  segmenter=None: events
        are detected (and filtered) only; filter_params=None: no filter; meta=True: the currents are dropped afterwards.
        hmm, features: HMM-guided segmentation of every file's events (File.parse_events); ignored without a segmenter.

        The reference takes one file after the other (:968-984).  Files are independent, so here up to `workers` of them
        are in flight (default: 2 when detector and segmenter are this package's own device classes, else 1): while file
        k is segmented, file k+1 is read, uploaded and searched for events on another host thread -- every thread has
        its own device context (engine.context), its kernels overlap with the others' like the contexts of a StreamPool.
        `files`, and the lines printed with verbose=True, keep the order of `filenames` whatever finishes first."""
        if event_detector is None:
            event_detector = lambda_event_parser(threshold=90)
        if segmenter is Experiment._DEFAULT:
            segmenter = SpeedyStatSplit(prior_segments_per_second=10, cutoff_freq=2000.)
        entries = list(self.filenames)
        if workers is None:
            ours = isinstance(event_detector, lambda_event_parser) and getattr(event_detector, "_device_route", False) and \
                (segmenter is None or isinstance(segmenter, SpeedyStatSplit))
            workers = 2 if ours else 1
        workers = max(1, min(int(workers), len(entries)))

        def one(entry, say=None):
            lines = []
            say = say or lines.append                    # (one file at a time: the lines appear as the reference prints them)
            file = entry if isinstance(entry, File) else File(entry)
            say("Opening {}".format(file.filename))
            file.parse(parser=event_detector)
            say("\tDetected {} Events".format(file.n))
            if segmenter is not None:
                file.parse_events(segmenter, filter_params, hmm=hmm, features=features)
                for i, event in enumerate(file.events):
                    say("\t\tEvent {} has {} segments".format(i + 1, event.n))
            elif filter_params is not None:
                for event in file.events:
                    event.filter(*filter_params)
            if meta:
                file.to_meta()
            return file, lines

        def take(done):
            file, lines = done
            if verbose:
                for line in lines:
                    print(line)
            self.files.append(file)

        if workers == 1:
            for entry in entries:
                take(one(entry, print if verbose else (lambda line: None)))
            return
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="pypore-file") as pool:
            for fut in [pool.submit(one, entry) for entry in entries]:
                take(fut.result())

    def apply_hmm(self, hmm, filter=None, indices=None, features=None):
        """The Viterbi paths of the events' segment means, concatenated (what DataTypes.py:990-995 intends; as written
        there it cannot run).  Events: `indices` of self.events (all when None), then those for which `filter(event)`
        is true.  A pypore_amd.hmm.Model decodes them all in ONE viterbi_batch call; another object with a `viterbi`
        method is called per event.  Returns the list of (index, state) entries of every path in event order (an
        impossible event contributes nothing).  hmm=None or an object without `viterbi`: NotImplementedError.  features:
        as for Event.apply_hmm -- a tuple of segment attribute names instead of the means, for a vector model."""
        if hmm is None or not callable(getattr(hmm, "viterbi", None)):
            raise NotImplementedError("apply_hmm needs a model with a viterbi method (pypore_amd.hmm.Model)")
        events = self.events
        if indices is not None:
            events = [events[i] for i in indices]
        if filter is not None:
            events = [event for event in events if filter(event)]
        means = [_observations(event, hmm, features) for event in events]
        batch = getattr(hmm, "viterbi_batch", None)
        results = batch(means) if callable(batch) else [hmm.viterbi(m) for m in means]
        return [entry for _, path in results if path is not None for entry in path]

    def delete(self):
        for file in self.files:
            file.delete()
        self.__dict__.clear()

    @property
    def n(self):
        return len(self.files)

    @property
    def events(self):
        """All events of all files, in file order."""
        return [event for file in self.files for event in file.events]

    @property
    def segments(self):
        """All segments of all events."""
        return [segment for event in self.events for segment in event.segments]


class Sample(object):
    """Events (and the files they came from) attributed to one substrate (DataTypes.py:1039-1049)."""

    def __init__(self, events=None, files=None, label=None):
        self.events = list(events) if events is not None else []
        self.files = list(files) if files is not None else []
        self.label = label

    def delete(self):
        with ignored(AttributeError):
            for file in self.files:
                file.delete()
        for event in self.events:
            event.delete()
        del self.events
        del self.files
