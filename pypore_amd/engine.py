"""Device-side plumbing between Python and libporeseg.so: one Context per GPU (a ps_ctx handle
plus torch-allocated HBM buffers).  torch is used for device memory and streams only; all
compute is in the HIP kernels behind the C ABI.
"""
import collections
import ctypes
import os
import threading
import warnings

import numpy as np
import torch

from . import _lib

_contexts = {}

# Options every new Context of this process gets (ps_set_option name -> value) and its tiling (ps_set_tiling).  EMPTY in
# the product: neither this package nor libporeseg.so reads a PORESEG_* variable on its own (round 6; the one exception is
# PORESEG_LIB / PORESEG_COMM_LIB, the path of the library to load).  tests/conftest.py and the scripts under tools/ fill
# them from the environment through apply_env_defaults(), so that `PORESEG_MODE=2 pytest -m gpu` still runs the whole
# suite in verify mode on the product library.
DEFAULT_OPTIONS = {}
DEFAULT_TILING = [0, 0]
# options a StreamPool applies to its contexts on top of "shared_device" while it runs (experiments: tools/)
POOL_OVERRIDES = {}

PIECE_CAP = 1 << 16      # pieces Context.detect_pieces has room for at first (2 MB of rows; a trace with more takes a second call)
EVENT_CAP = 1 << 16      # events the detector's host arrays hold at first (Context.detect_events / detect_segment_trace grow them when a trace has more)

# variable -> option, the integer-valued ones: the same list as the table of pypore_amd/csrc/ctx_options.hpp has (kept here as well because
# the package works without a compiler; tests/test_ctx_options_host.py compares the two).  PORESEG_NOISE_K, a fraction, is read below.
_ENV_OPTIONS = {
    "PORESEG_MODE": "mode", "PORESEG_SPINE_NT": "spine_nt", "PORESEG_TREE_NT": "tree_nt", "PORESEG_PRUNE": "prune",
    "PORESEG_SCAN_BS": "scan_bs", "PORESEG_GROUPS": "groups", "PORESEG_TREE_PAR": "tree_par", "PORESEG_K0_WAVES": "k0_waves",
    "PORESEG_K0_SHARED": "k0_shared", "PORESEG_K0_MAX": "k0_admit", "PORESEG_K0_SETS": "k0_sets", "PORESEG_WIDE_BS": "wide_bs",
    "PORESEG_BRIDGE_SINGLE": "bridge_single", "PORESEG_TREE_TAIL": "tree_tail_pct", "PORESEG_FILTER_FUSED": "filter_fused",
    "PORESEG_UPLOAD": "upload_by_kernel", "PORESEG_TIMING": "timing", "PORESEG_TREE_MW": "tree_mw",
    "PORESEG_TREE_JPW": "tree_jobs_per_wave", "PORESEG_TREE_SCREEN": "tree_screen", "PORESEG_SLOTS_PCT": "slots_pct", "PORESEG_BRIDGE_EXT": "bridge_ext",
    "PORESEG_LAT_HELP": "lat_help", "PORESEG_BRIDGE_BUDGET": "bridge_budget", "PORESEG_DEBUG": "debug",
    "PORESEG_SHORT_CHAIN": "short_chain", "PORESEG_BRIDGE_PATIENCE": "bridge_patience",
    "PORESEG_GATHER_FUSED": "gather_fused", "PORESEG_SINGLE_PASS": "single_pass", "PORESEG_DOWNLOAD": "download_by_kernel", "PORESEG_K0_UNALIGNED": "k0_unaligned",
    # libporeseg_diag.so only (PORESEG_LIB=.../libporeseg_diag.so): stale or partial results, never the product
    "PORESEG_DBG_PHASE": "dbg_phase", "PORESEG_DBG_K0_NOGRP": "dbg_k0_nogrp", "PORESEG_SCAN_LDS_PAD": "scan_lds_pad",
    "PORESEG_REP_EVAL": "rep_eval", "PORESEG_REP_STAGE": "rep_stage", "PORESEG_REP_SUM": "rep_sum",
}


def options_from_env(environ=None):
    """(options, tiling, pool overrides) named by PORESEG_* variables -- for tests and tools, which call it explicitly."""
    env = os.environ if environ is None else environ
    opts = {}
    for var, name in _ENV_OPTIONS.items():
        if var in env and env[var] != "":
            opts[name] = int(env[var])
    if env.get("PORESEG_STITCH"):
        opts["stitch_host"] = 1 if env["PORESEG_STITCH"] == "host" else 0
    if "PORESEG_NOISE_K" in env:
        opts["noise_k_ppm"] = int(round(float(env["PORESEG_NOISE_K"]) * 1e6))
    tiling = [int(env.get("PORESEG_TILE", "0") or 0), int(env.get("PORESEG_HALO", "0") or 0)]
    pool = {}
    if "PORESEG_POOL_K0_WAVES" in env:
        pool["k0_waves"] = int(env["PORESEG_POOL_K0_WAVES"])
    if "PORESEG_POOL_K0_MAX" in env:
        pool["k0_admit"] = int(env["PORESEG_POOL_K0_MAX"])
    if env.get("PORESEG_POOL_SHARED", "0") == "1":
        pool["k0_shared"] = 1
    return opts, tiling, pool


def apply_env_defaults(environ=None):
    """Contexts created from now on start with the settings the PORESEG_* variables name (tests/conftest.py, tools/)."""
    opts, tiling, pool = options_from_env(environ)
    DEFAULT_OPTIONS.update(opts)
    if tiling[0] or tiling[1]:
        DEFAULT_TILING[:] = tiling
    POOL_OVERRIDES.update(pool)
    return opts, tiling, pool


def _ptr(t):
    """The device address of a CUDA tensor as the C ABI takes it (None or an empty tensor: null)."""
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _addr(t):
    """The address of a CUDA tensor as torch gives it: an empty view of a live tensor keeps its own (the library refuses NULL
    where it must have samples, so _ptr is for the arguments that may be absent)."""
    return ctypes.c_void_p(t.data_ptr())


_HOST_POINTER = {np.int64: ctypes.POINTER(ctypes.c_int64), np.int32: ctypes.POINTER(ctypes.c_int32),
                 np.float64: ctypes.POINTER(ctypes.c_double)}


def _host(a, dtype=np.int64):
    """A host array for the C ABI: (contiguous array of int64, int32 or float64, the pointer to it -- valid while the array lives)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(_HOST_POINTER[dtype])


_offsets = _host


def _slot_offsets(slots):
    """Per-sequence slot sizes as the offsets the C ABI takes: ([0, s0, s0 + s1, ...], the pointer to them)."""
    return _host(np.concatenate(([0], np.cumsum(slots))))


def _device_input(*tensors, dtype=None, one_dim=True):
    """What a device input must be (asserted): a contiguous CUDA tensor, one-dimensional and of `dtype` where the caller
    says so.  Returns the device."""
    for t in tensors:
        assert t.is_cuda and t.is_contiguous() and (not one_dim or t.dim() == 1) and (dtype is None or t.dtype == dtype)
    return tensors[0].device


def _fmt(samples, quantum, offset_counts, f64=False):
    """The ps_sample_format of a tensor: float32 on the grid `quantum`, int16 counts, and -- only for a call that takes it,
    f64=True -- float64 on no grid (quantum and offset are ignored then)."""
    if samples.dtype == torch.float32:
        return _lib.SampleFormat(_lib.PS_DTYPE_F32, int(offset_counts), float(quantum))
    if samples.dtype == torch.int16:
        return _lib.SampleFormat(_lib.PS_DTYPE_I16, int(offset_counts), float(quantum))
    if f64 and samples.dtype == torch.float64:
        return _lib.SampleFormat(_lib.PS_DTYPE_F64, 0, 1.0)
    raise ValueError("samples must be float32 or int16, got %s" % samples.dtype)


def _call_rc(dev, fn, handle, *args):
    """The one path of a library call: what torch's current stream of `dev` was given is finished (inputs produced there are
    ready; dev None: the call reads no device memory), then fn(handle, *args).  Returns the status for a caller that
    interprets it itself."""
    if dev is not None:
        torch.cuda.current_stream(dev).synchronize()
    return fn(handle, *args)


def _call(dev, fn, handle, *args):
    """_call_rc with the status checked: any but PS_OK raises (_lib.check)."""
    _lib.check(_call_rc(dev, fn, handle, *args), handle)


def _retry_capacity(handle, attempt, cap, fixed=False):
    """A call whose output has ONE capacity.  attempt(cap) makes it with room for cap entries and returns (status, the size
    the library reported, result).  PS_ERR_CAPACITY with a reported size above cap: CapacityError when the caller fixed cap,
    else one more attempt with the reported size.  Whatever status stands then is checked; returns the result."""
    rc, need, out = attempt(cap)
    if rc == _lib.PS_ERR_CAPACITY and fixed:
        raise CapacityError(need, cap)
    if rc == _lib.PS_ERR_CAPACITY and need > cap:
        rc, need, out = attempt(int(need))
    _lib.check(rc, handle)
    return out


def _retry_slots(handle, attempt, reported, slots, retry=True):
    """A call whose output has a slot PER SEQUENCE.  attempt(*slots) makes it with the given slot sizes and returns (status,
    result); reported() reads the exact sizes the call counted, as a tuple like slots.  PS_ERR_CAPACITY: with retry one more
    attempt with the reported sizes, and whatever status stands then is checked; without, the status is returned as it is
    with whatever fitted.  Any other status is checked.  Returns (status, result)."""
    rc, out = attempt(*slots)
    if rc == _lib.PS_ERR_CAPACITY and retry:
        rc, out = attempt(*reported())
    if rc != _lib.PS_ERR_CAPACITY or retry:
        _lib.check(rc, handle)
    return rc, out


def _int64_host(counts, n):
    """The first n of a device tensor of counts as an int64 numpy array (the exact sizes for _retry_slots)."""
    return counts[:n].cpu().numpy().astype(np.int64)


def live_bytes():
    """ps_live_bytes: device + pinned host bytes that the library's contexts of this process hold right now (a diagnostic)."""
    return int(_lib.lib().ps_live_bytes())


def _serialised(method):
    """The method runs under its Context's lock."""
    import functools

    @functools.wraps(method)
    def call(self, *a, **kw):
        with self.lock:
            return method(self, *a, **kw)
    return call


class Context(object):
    """Owns a ps_ctx bound to GPU `device` (one process per GPU; one host thread at a time)."""

    def __init__(self, device=0):
        L = _lib.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("pypore_amd: no GPU visible to torch -- the segmenter has no CPU fallback")
        self.device = int(device)
        h = ctypes.c_void_p()
        _lib.check(L.ps_create(self.device, None, ctypes.byref(h)))
        self.handle = h
        self.L = L
        self.lock = threading.RLock()                   # one call at a time per ps_ctx (see engine.context)
        if DEFAULT_TILING[0] or DEFAULT_TILING[1]:
            self.set_tiling(*DEFAULT_TILING)
        for name, value in DEFAULT_OPTIONS.items():
            self.set_option(name, value)

    def close(self):
        if self.handle:
            self.L.ps_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tiling(self, tile_len=0, halo=0):
        with self.lock:
            _call(None, self.L.ps_set_tiling, self.handle, int(tile_len), int(halo))

    def set_option(self, name, value):
        """ps_set_option, under the context's lock: an option never changes in the middle of another thread's call."""
        with self.lock:
            _call(None, self.L.ps_set_option, self.handle, name.encode(), int(value))

    def get_option(self, name):
        """ps_get_option: any option set_option knows, as it stands -- its default, what was last set (a switch as 0 / 1), what
        "shared_device" planned for "k0_waves", "k0_admit" and "lat_help"; "k0_unaligned" is what the device's probe granted."""
        out = ctypes.c_int64()
        with self.lock:
            _call(None, self.L.ps_get_option, self.handle, name.encode(), ctypes.byref(out))
        return int(out.value)

    def seq_ms(self):
        """Device time of the most recent segment call (HIP events, first upload .. last result copy), in ms: the
        light accessor for timed loops (timings() builds a dict of everything)."""
        if not hasattr(self, "_tm"):
            self._tm = ((ctypes.c_double * 8)(), (ctypes.c_int64 * 8)())
        self.L.ps_get_timings(self.handle, self._tm[0], 8, self._tm[1], 8)
        return self._tm[0][_lib.MS_NAMES.index("seq")]

    def timings(self):
        """ps_get_timings as a dict: "<name>_ms" for _lib.MS_NAMES, the counters by their _lib.COUNTER_NAMES."""
        ms = (ctypes.c_double * len(_lib.MS_NAMES))()
        cnt = (ctypes.c_int64 * len(_lib.COUNTER_NAMES))()
        _call(None, self.L.ps_get_timings, self.handle, ms, len(ms), cnt, len(cnt))
        out = {name + "_ms": ms[i] for i, name in enumerate(_lib.MS_NAMES)}
        out.update({name: cnt[i] for i, name in enumerate(_lib.COUNTER_NAMES) if name})
        return out

    def near_ties(self):
        """Windows of the most recent segment call that were decided among fp64 contenders with a margin inside the
        noise of the device logarithm against glibc's (1e-9 relative): the reference could have decided
        them the other way.  0 in every golden vector except the constructed exact tie.  -1: the call ran on the LDS-window
        kernels, which do not count them (callers that redo near ties on the exact route treat it as "some")."""
        if not hasattr(self, "_cnt"):
            self._cnt = self.L.ps_counters(self.handle)      # the context's counters in place: no call per look
        return int(self._cnt[_lib.COUNTER_NAMES.index("near_ties")])

    def near_tie_sites(self):
        """Where the near ties of the most recent segment call lie (ps_get_near_ties): a numpy structured array of
        NEAR_TIE_DTYPE -- (event, window_start, window_end, split) in samples of the event, split -1: none -- sorted by
        (event, window_start), speculative scans included (consistent_sites removes those).  None when the sites are not
        counted (LDS-window kernels, option near_tie_log 0) or incomplete (the log overflowed): treat every event as flagged."""
        n = ctypes.c_int64()

        def attempt(cap):
            buf = (_lib.NearTie * cap)()
            return _call_rc(None, self.L.ps_get_near_ties, self.handle, buf, cap, ctypes.byref(n)), n.value, buf

        with self.lock:
            buf = _retry_capacity(self.handle, attempt, 64)
        if n.value < 0:
            return None
        return np.frombuffer(buf, dtype=NEAR_TIE_DTYPE, count=int(n.value)).copy()

    # ---- the hot path ---------------------------------------------------------------------------
    @_serialised
    def segment_batch(self, samples, ev_off, params, quantum, offset_counts=0, want_stats=True, cap=None,
                      want_spine=False, lead=0, out=None, near_tie_warning=True):
        """ps_segment_batch on device-resident `samples` (torch float32 or int16 CUDA tensor).
        Returns (bounds int32 CUDA tensor [total], bounds_off int64 numpy [n_ev+1],
        stats float64 CUDA tensor [total+n_ev, 4] or None).  lead > 0: the boundaries are a view that starts `lead`
        elements into their buffer (dist.BoundaryGather puts its header there and sends the buffer as it is).
        out: int32 CUDA tensor to receive the boundaries (its size is the capacity; ValueError if they do not fit).
        near_tie_warning=False: no NearTieWarning from this call (its caller acts on the near ties itself)."""
        assert samples.is_cuda and samples.is_contiguous() and samples.dim() == 1
        if samples.dtype == torch.float32:
            dtype = _lib.PS_DTYPE_F32
        elif samples.dtype == torch.int16:
            dtype = _lib.PS_DTYPE_I16
        else:
            raise ValueError("samples must be float32 or int16, got %s" % samples.dtype)
        ev_off = np.ascontiguousarray(ev_off, dtype=np.int64)
        n_ev = ev_off.size - 1
        fmt = _lib.SampleFormat(dtype, int(offset_counts), float(quantum))
        off_p = ev_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        if cap is None and out is None:
            cap = int(self.L.ps_bounds_capacity(off_p, n_ev, int(params.min_width)))
            if cap < 0:
                raise ValueError("min_width must be >= 1")
        dev = samples.device
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and out.dim() == 1
            bounds, cap = out, int(out.numel())
        else:
            bounds = torch.empty(max(cap, 1) + lead, dtype=torch.int32, device=dev)[lead:]
        stats = torch.empty((max(cap, 1) + n_ev, 4), dtype=torch.float64, device=dev) if want_stats else None
        boff = np.zeros(n_ev + 1, dtype=np.int64)
        torch.cuda.current_stream(dev).synchronize()      # inputs produced on torch's stream are ready
        spine = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev) if want_spine else None
        rc = self.L.ps_segment_batch_ex(self.handle, ctypes.c_void_p(samples.data_ptr()), ctypes.byref(fmt), off_p,
                                        n_ev, ctypes.byref(params), ctypes.c_void_p(bounds.data_ptr()), cap,
                                        boff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        ctypes.c_void_p(stats.data_ptr()) if want_stats else None,
                                        ctypes.c_void_p(spine.data_ptr()) if want_spine else None)
        _lib.check(rc, self.handle)
        if NEAR_TIE_WARNING and near_tie_warning:
            nt = self.near_ties()
            if nt > 0:
                import warnings
                warnings.warn("%d window(s) were decided by a margin inside the reference's own rounding noise (near tie: below 1e-9 "
                              "relative on grid data -- the logarithm's last bit; on re-quantised float64 data, e.g. a filtered event, "
                              "within the noise of the reference's cumsums): the reference could place such a boundary elsewhere, "
                              "typically one sample beside it" % nt, NearTieWarning, stacklevel=2)
        total = int(boff[-1])
        if want_spine:
            return bounds[:total], boff, (stats[:total + n_ev] if want_stats else None), spine[:total]
        return bounds[:total], boff, (stats[:total + n_ev] if want_stats else None)

    _fmt = staticmethod(_fmt)        # (tools/ build a format for their own ctx.L calls)

    @_serialised
    def detect_events(self, samples, quantum, threshold=90.0, min_duration=100000, min_current=-0.5,
                      offset_counts=0):
        """ps_detect_events on a device-resident trace: (starts, lengths) int64 numpy arrays of the
        events lambda_event_parser(threshold) keeps with its default rules (parsers.py:124-155)."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        n = samples.numel()
        cnt = ctypes.c_int64()

        def attempt(cap):
            (st, st_p), (ln, ln_p) = _host(np.zeros(cap, dtype=np.int64)), _host(np.zeros(cap, dtype=np.int64))
            rc = _call_rc(dev, self.L.ps_detect_events, self.handle, _addr(samples), ctypes.byref(fmt), n, float(threshold),
                          int(min_duration), float(min_current), st_p, ln_p, cap, ctypes.byref(cnt))
            return rc, cnt.value, (st, ln)

        # (room for every event the rules can keep is n / min_duration + 2 -- gigabytes of host memory for a long trace and a
        #  small min_duration; a file has a few hundred: start with EVENT_CAP and take the count the library reports if it is more)
        st, ln = _retry_capacity(self.handle, attempt, min(n // max(1, int(min_duration)) + 2, EVENT_CAP))
        return st[:cnt.value].copy(), ln[:cnt.value].copy()

    @_serialised
    def detect_pieces(self, samples, quantum, threshold, offset_counts=0):
        """ps_detect_pieces on a device-resident trace: EVERY piece the threshold cuts it into -- (edges int64 [P + 1], stats
        float64 [P, 4] in core.STAT_COLUMNS order), numpy arrays; piece p is [edges[p], edges[p + 1]).  The statistics are those
        of count * quantum, from exact integer sums: range_stats on the same pieces gives the same bits.  Starts with room for
        PIECE_CAP pieces and takes the count the library reports if a trace has more (one more call)."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        n = samples.numel()
        cnt = ctypes.c_int64()

        def attempt(cap):
            edges = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            stats = torch.empty((max(cap, 1), 4), dtype=torch.float64, device=dev)
            rc = _call_rc(dev, self.L.ps_detect_pieces, self.handle, _addr(samples), ctypes.byref(fmt), n, float(threshold),
                          _addr(edges), _addr(stats), cap, ctypes.byref(cnt))
            return rc, cnt.value, (edges, stats)

        edges, stats = _retry_capacity(self.handle, attempt, min(n, PIECE_CAP))
        return edges[:cnt.value + 1].cpu().numpy(), stats[:cnt.value].cpu().numpy()

    @_serialised
    def detect_segment_trace(self, samples, quantum, params, threshold=90.0, min_duration=100000, min_current=-0.5,
                             offset_counts=0, want_stats=False):
        """ps_detect_segment_trace: detect_events + segment_events of a device-resident file trace in one call and one pass
        over its samples (include/poreseg.h).  Returns (starts, lengths, bounds, bounds_off, stats or None)."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        n = samples.numel()
        cnt = ctypes.c_int64()
        cap = n // int(params.min_width) + 1     # (every event holds at most length / min_width boundaries, all of them together n / min_width)

        def attempt(ev_cap):
            st, ln, boff = np.zeros(ev_cap, dtype=np.int64), np.zeros(ev_cap, dtype=np.int64), np.zeros(ev_cap + 1, dtype=np.int64)
            bounds = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            stats = torch.empty((max(cap, 1) + ev_cap, 4), dtype=torch.float64, device=dev) if want_stats else None
            rc = _call_rc(dev, self.L.ps_detect_segment_trace, self.handle, _addr(samples), ctypes.byref(fmt), n, float(threshold),
                          int(min_duration), float(min_current), ctypes.byref(params), _host(st)[1], _host(ln)[1], ev_cap,
                          ctypes.byref(cnt), _addr(bounds), cap, _host(boff)[1], _ptr(stats))
            return rc, cnt.value, (st, ln, boff, bounds, stats)

        # (more events than EVENT_CAP: once more with room for all; see detect_events)
        st, ln, boff, bounds, stats = _retry_capacity(self.handle, attempt, min(n // max(1, int(min_duration)) + 2, EVENT_CAP))
        n_ev = int(cnt.value)
        total = int(boff[n_ev])
        return st[:n_ev].copy(), ln[:n_ev].copy(), bounds[:total], boff[:n_ev + 1].copy(), (stats[:total + n_ev] if want_stats else None)

    @_serialised
    def segment_events(self, samples, ev_start, ev_len, params, quantum, offset_counts=0, want_stats=False):
        """ps_segment_events: events are sub-ranges [start, start+len) of one device-resident trace."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        n_ev = ev_start.size
        cap = int(np.sum(ev_len // int(params.min_width) + 1)) if n_ev else 0
        bounds = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        stats = torch.empty((max(cap, 1) + n_ev, 4), dtype=torch.float64, device=dev) if want_stats else None
        boff, boff_p = _host(np.zeros(n_ev + 1, dtype=np.int64))
        _call(dev, self.L.ps_segment_events, self.handle, _addr(samples), ctypes.byref(fmt), st_p, ln_p, n_ev, ctypes.byref(params),
              _addr(bounds), cap, boff_p, _ptr(stats), None)
        total = int(boff[-1])
        return bounds[:total], boff, (stats[:total + n_ev] if want_stats else None)

    @_serialised
    def segment_exact_f64(self, current, ev_start, ev_len, params):
        """ps_segment_exact_f64: events [start, start + len) of a float64 CUDA tensor (pA, on no grid) segmented from the
        reference's own sequential prefix sums (include/poreseg.h).  Returns (bounds int32 CUDA tensor, bounds_off)."""
        dev = _device_input(current, dtype=torch.float64)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        n_ev = ev_start.size
        cap = int(np.sum(ev_len // int(params.min_width) + 1)) if n_ev else 0
        bounds = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        boff, boff_p = _host(np.zeros(n_ev + 1, dtype=np.int64))
        _call(dev, self.L.ps_segment_exact_f64, self.handle, _addr(current), st_p, ln_p, n_ev, ctypes.byref(params), _addr(bounds),
              cap, boff_p)
        return bounds[:int(boff[-1])], boff

    @_serialised
    def statsplit_f64(self, current, ev_start, ev_len, params, lo=None, hi=None, cap=None):
        """ps_statsplit_f64: events [start, start + len) of a float64 CUDA tensor segmented as the reference's StatSplit does
        (include/poreseg.h); params: _lib.StatSplitParams.  lo / hi: per event the range [lo, hi) that is segmented, in
        samples from its start (None: all of it).  cap: boundaries the output may hold (None: what the model allows); when
        it is too small, CapacityError names the size required.  Returns (bounds int32 CUDA tensor, bounds_off)."""
        dev = _device_input(current, dtype=torch.float64)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        n_ev = ev_start.size
        lo, lo_p = (None, None) if lo is None else _host(lo)
        hi, hi_p = (None, None) if hi is None else _host(hi)
        if cap is None:
            span = np.maximum((ev_len if hi is None else hi) - (0 if lo is None else lo), 0)
            cap = int(np.sum(2 * (span // max(int(params.min_width), 1)) + 2)) if n_ev else 0
        bounds = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        boff, boff_p = _host(np.zeros(n_ev + 1, dtype=np.int64))

        def attempt(cap):
            rc = _call_rc(dev, self.L.ps_statsplit_f64, self.handle, _ptr(current), st_p, ln_p, n_ev, lo_p, hi_p, ctypes.byref(params),
                          _addr(bounds), cap, boff_p)
            return rc, int(boff[-1]), bounds

        return _retry_capacity(self.handle, attempt, cap, fixed=True)[:int(boff[-1])], boff

    def _spans_f64(self, fn, current, ev_start, ev_len, cap, guess, *params):
        """The state parsers' common call fn(handle, current, starts, lengths, n_ev, *params, spans, cap, span_off): spans (n, 2)
        int32 CUDA tensor and span_off.  cap None: a first call sized by guess(ev_len), repeated once with the size the library
        reports when that is too small."""
        dev = _device_input(current, dtype=torch.float64)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        n_ev = ev_start.size
        soff, soff_p = _host(np.zeros(n_ev + 1, dtype=np.int64))

        def attempt(cap):
            spans = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)
            rc = _call_rc(dev, fn, self.handle, _ptr(current), st_p, ln_p, n_ev, *params, _addr(spans), cap, soff_p)
            return rc, int(soff[-1]), spans

        spans = _retry_capacity(self.handle, attempt, int(guess(ev_len)) if cap is None else cap, fixed=cap is not None)
        return spans[:int(soff[-1])], soff

    @_serialised
    def snakebase_f64(self, current, ev_start, ev_len, cap=None):
        """ps_snakebase_f64: the spans snakebase_parser.parse returns for events [start, start + len) of a float64 CUDA
        tensor (include/poreseg.h).  cap: spans the output may hold -- CapacityError names the size required when it is
        too small; None: the most an event can have, a span per two samples (the normal case on ADC-grid data is not far
        from it).  Returns (spans (n, 2) int32 CUDA tensor of (start, end), span_off)."""
        return self._spans_f64(self.L.ps_snakebase_f64, current, ev_start, ev_len, cap, lambda ln: (ln // 2).sum())

    @_serialised
    def filter_derivative_f64(self, current, ev_start, ev_len, params, cap=None):
        """ps_filter_derivative_f64: the spans FilterDerivativeSegmenter.parse returns; params: _lib.FilterDerivativeParams
        (prefiltered 1: `current` is the filtered current).  cap and the result as for snakebase_f64; None: a span per 64
        samples, and one more call with the size the library reports when that is too small."""
        return self._spans_f64(self.L.ps_filter_derivative_f64, current, ev_start, ev_len, cap, lambda ln: ln.sum() // 64 + ln.size + 1,
                               ctypes.byref(params))

    @_serialised
    def statsplit_prefix_f64(self, current, want_ct=True):
        """ps_statsplit_prefix_f64 (diagnostics): the prefix sums StatSplit forms of one float64 CUDA tensor -- (c, c2, ct) as
        CUDA tensors, ct None unless asked for."""
        dev = _device_input(current, dtype=torch.float64)
        c, c2 = torch.empty_like(current), torch.empty_like(current)
        ct = torch.empty_like(current) if want_ct else None
        _call(dev, self.L.ps_statsplit_prefix_f64, self.handle, _ptr(current), current.numel(), _ptr(c), _ptr(c2), _ptr(ct))
        return c, c2, ct

    @_serialised
    def best_single_split(self, samples, quantum, offset_counts=0):
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        g = ctypes.c_double()
        i = ctypes.c_int32()
        _call(dev, self.L.ps_best_single_split, self.handle, _addr(samples), ctypes.byref(fmt), samples.numel(), ctypes.byref(g),
              ctypes.byref(i))
        return g.value, i.value

    @_serialised
    def audit_bounds(self, samples, quantum, params, windows, offset_counts=0):
        """ps_audit_bounds (diagnostic): the pruning bounds of the block-sum scan -- corner, two-boundary, group -- against
        the gains they cover, evaluated on the device from the raw samples, for the given windows [(ps, pe), ...] of the
        trace taken as one event.  Returns a dict of counts, violations and smallest margins per kind."""
        fmt = _fmt(samples, quantum, offset_counts)
        w, w_p = _host(np.asarray(windows, dtype=np.int32).reshape(-1, 2), np.int32)
        out = (ctypes.c_double * 12)()
        _call(samples.device, self.L.ps_audit_bounds, self.handle, _addr(samples), ctypes.byref(fmt), samples.numel(),
              ctypes.byref(params), w_p, int(w.shape[0]), out)
        o = list(out)
        return {"corner": {"blocks": int(o[0]), "violations": int(o[1]), "min_margin": o[6]},
                "two_boundary": {"blocks": int(o[2]), "violations": int(o[3]), "min_margin": o[7]},
                "group": {"groups": int(o[4]), "violations": int(o[5]), "min_margin": o[8]},
                "windows_with_coarse_pass": int(o[9])}

    @_serialised
    def score_window(self, samples, quantum, min_width, min_gain, offset_counts=0):
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts)
        scores = torch.empty(max(1, samples.numel()), dtype=torch.float64, device=dev)
        i = ctypes.c_int32()
        _call(dev, self.L.ps_score_window, self.handle, _addr(samples), ctypes.byref(fmt), samples.numel(), int(min_width),
              float(min_gain), _addr(scores), ctypes.byref(i))
        return i.value, scores[:samples.numel()]

    @_serialised
    def filter_bessel(self, samples, quantum, cutoff=2000., sampling_freq=1.e5, order=1, offset_counts=0):
        """ps_filter_bessel: Event.filter (DataTypes.py:258-274) -- Bessel low-pass of order 1..8, forward and backward
        (scipy filtfilt semantics); returns the filtered current in pA as a float64 CUDA tensor.  `samples`: float32 pA on
        the grid `quantum` / int16 counts (what a file holds), or a float64 tensor of pA on no grid at all -- the current
        of an event that was filtered before (quantum is ignored then)."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts, f64=True)
        out = torch.empty(max(1, samples.numel()), dtype=torch.float64, device=dev)
        _call(dev, self.L.ps_filter_bessel, self.handle, _addr(samples), ctypes.byref(fmt), samples.numel(), int(order), float(cutoff),
              float(sampling_freq), _addr(out))
        return out[:samples.numel()]

    @_serialised
    def filter_requantise_batch(self, samples, ev_start, ev_len, quantum, cutoff=2000., sampling_freq=1.e5, order=1, offset_counts=0):
        """ps_filter_requantise_batch: Event.filter + the re-quantisation for many events of ONE device-resident trace in one
        call (two host synchronisations for the batch instead of three per event).  Returns (filtered float64 CUDA tensor,
        rounded float32 CUDA tensor -- both the events back to back --, offsets int64 numpy [n_ev + 1], centres, steps)."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts, f64=True)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        n_ev = ev_start.size
        off = _slot_offsets(ev_len)[0]
        total = int(off[-1])
        filtered = torch.empty(max(1, total), dtype=torch.float64, device=dev)
        rounded = torch.empty(max(1, total), dtype=torch.float32, device=dev)
        centre, centre_p = _host(np.zeros(max(1, n_ev), dtype=np.float64), np.float64)
        step, step_p = _host(np.zeros(max(1, n_ev), dtype=np.float64), np.float64)
        _call(dev, self.L.ps_filter_requantise_batch, self.handle, _addr(samples), ctypes.byref(fmt), st_p, ln_p, n_ev, int(order),
              float(cutoff), float(sampling_freq), _addr(filtered), _addr(rounded), centre_p, step_p)
        return filtered[:total], rounded[:total], off, centre[:n_ev], step[:n_ev]

    @_serialised
    def filter_bessel_batch(self, samples, ev_start, ev_len, quantum, cutoff=2000., sampling_freq=1.e5, order=1, offset_counts=0):
        """ps_filter_bessel_batch: Event.filter for many events of ONE device-resident tensor in one call -- event e is
        samples[ev_start[e] : ev_start[e] + ev_len[e]]; events may overlap and come in any order.  `samples` as for filter_bessel
        (float32 on the grid `quantum`, int16 counts, or float64 on no grid).  Returns (float64 CUDA tensor, the filtered
        events back to back, each bit for bit what filter_bessel returns for it alone; offsets int64 numpy [n_ev + 1]).  One
        launch on the fused order-1 route, one host synchronisation for the batch."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts, f64=True)
        (ev_start, st_p), (ev_len, ln_p) = _host(ev_start), _host(ev_len)
        if ev_start.shape != ev_len.shape or ev_start.ndim != 1:
            raise ValueError("ev_start and ev_len must be one-dimensional and of one length")
        n_ev = ev_start.size
        if n_ev and (int(ev_start.min()) < 0 or int(ev_len.min()) < 0 or int((ev_start + ev_len).max()) > samples.numel()):
            raise ValueError("an event lies outside the samples")
        off = _slot_offsets(ev_len)[0]
        total = int(off[-1])
        out = torch.empty(max(1, total), dtype=torch.float64, device=dev)
        _call(dev, self.L.ps_filter_bessel_batch, self.handle, _addr(samples), ctypes.byref(fmt), st_p, ln_p, n_ev, int(order),
              float(cutoff), float(sampling_freq), _addr(out))
        return out[:total], off

    @_serialised
    def range_stats(self, samples, starts, ends, quantum, offset_counts=0):
        """ps_range_stats: mean / std / min / max of the sample ranges [starts[r], ends[r]) of ONE device-resident tensor (int16
        counts, or float32 on the grid `quantum`) as an (n_ranges, 4) float64 numpy array in core.STAT_COLUMNS order.  The
        ranges may overlap, repeat and come in any order (the merged segments of DataTypes.merge_by_hmm do); two launches
        whatever their number, one download.  Exact integer sums: the same ranges give the same bits however option
        "range_tile" cuts them.  An empty or reversed range, one that leaves the samples, or float64 samples: ValueError,
        nothing is launched."""
        dev = _device_input(samples)
        fmt = _fmt(samples, quantum, offset_counts, f64=True)        # (float64: passed on for the library to refuse in its own words)
        (starts, starts_p), (ends, ends_p) = _host(starts), _host(ends)
        if starts.shape != ends.shape or starts.ndim != 1:
            raise ValueError("starts and ends must be one-dimensional and of one length")
        n_ranges = starts.size
        out = torch.empty((max(1, n_ranges), 4), dtype=torch.float64, device=dev)
        _call(dev, self.L.ps_range_stats, self.handle, _addr(samples), ctypes.byref(fmt), samples.numel(), starts_p, ends_p, n_ranges,
              _addr(out))
        return out[:n_ranges].cpu().numpy()

    @_serialised
    def requantise(self, current):
        """ps_requantise: a filtered current (float64 CUDA tensor, pA) centred and rounded to the finest power-of-two
        grid that keeps its counts below 2**22.  Returns (float32 CUDA tensor on that grid, centre, step): segment it
        with quantum = step."""
        dev = _device_input(current, dtype=torch.float64)
        out = torch.empty(max(1, current.numel()), dtype=torch.float32, device=dev)
        centre, step = ctypes.c_double(), ctypes.c_double()
        _call(dev, self.L.ps_requantise, self.handle, _addr(current), current.numel(), _addr(out), ctypes.byref(centre), ctypes.byref(step))
        return out[:current.numel()], centre.value, step.value

    @_serialised
    def grid_check(self, current, origin, quantum, tol=1e-6):
        """ps_grid_check_f64: a candidate grid origin + k * quantum tried on every sample of a float64 CUDA tensor.  Returns
        _lib.GridReport (max |k - rint k|, the smallest one above tol, min and max rint k, non-finite samples)."""
        dev = _device_input(current, dtype=torch.float64)
        r = _lib.GridReport()
        _call(dev, self.L.ps_grid_check_f64, self.handle, _addr(current), current.numel(), float(origin), float(quantum), float(tol),
              ctypes.byref(r))
        return r

    @_serialised
    def grid_counts(self, current, origin, quantum, centre):
        """ps_grid_counts_f64: int16 CUDA tensor of rint((x - origin) / quantum) - centre, for a grid that grid_check
        confirmed and whose re-centred range the caller found inside int16."""
        dev = _device_input(current, dtype=torch.float64)
        out = torch.empty(current.numel(), dtype=torch.int16, device=dev)
        _call(dev, self.L.ps_grid_counts_f64, self.handle, _addr(current), current.numel(), float(origin), float(quantum), int(centre),
              _addr(out))
        return out

    @_serialised
    def narrow_f64(self, current):
        """ps_narrow_f64: (float32 CUDA tensor of a float64 one, the number of samples the conversion changed)."""
        dev = _device_input(current, dtype=torch.float64)
        out = torch.empty(current.numel(), dtype=torch.float32, device=dev)
        bad = ctypes.c_int64()
        _call(dev, self.L.ps_narrow_f64, self.handle, _addr(current), current.numel(), _addr(out), ctypes.byref(bad))
        return out, bad.value

    @_serialised
    def align_batch(self, model_means, model_stds, model_durs, skip_penalty, backslip_penalty,
                    seq_means, seq_stds, seq_durs, seq_off):
        """ps_align_batch: cSegmentAligner.align (calignment.pyx:20-100) for a batch of sequences.  Model arrays: host
        (numpy); sequence arrays: float64 CUDA tensors, sequence q = [seq_off[q], seq_off[q+1]).  Returns CUDA tensors
        (scores float64 [n_seq] = score[s-1][m-1], paths uint32-as-int64 view avoided: int32 bits of the reference's
        unsigned j [total], status int32 [n_seq])."""
        (mm, mm_p), (ms, ms_p), (md, md_p) = (_host(a, np.float64) for a in (model_means, model_stds, model_durs))
        assert mm.size == ms.size == md.size
        off, off_p = _host(seq_off)
        n_seq = off.size - 1
        assert min(t.numel() for t in (seq_means, seq_stds, seq_durs)) >= int(off[-1])
        dev = _device_input(seq_means, seq_stds, seq_durs, dtype=torch.float64, one_dim=False)
        scores = torch.zeros(max(n_seq, 1), dtype=torch.float64, device=dev)
        paths = torch.zeros(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n_seq, 1), dtype=torch.int32, device=dev)
        _call(dev, self.L.ps_align_batch, self.handle, mm_p, ms_p, md_p, mm.size, float(skip_penalty), float(backslip_penalty),
              _ptr(seq_means), _ptr(seq_stds), _ptr(seq_durs), off_p, n_seq, _ptr(scores), _ptr(paths), _ptr(status))
        return scores[:n_seq], paths[:int(off[-1])], status[:n_seq]

    @_serialised
    def pairwise_scores(self, a, a_off, b, b_off, mode, penalty, want_pos=False):
        """ps_pairwise_scores: every pair of the sequence sets A x B on the score-only route.  a, b: float64 CUDA tensors
        (NaN: the gap marker), set k of A = a[a_off[k]:a_off[k+1]].  Returns (scores float64 [n_a, n_b], positions int32
        [n_a, n_b, 2] of the local maximum or None)."""
        (a_off, a_off_p), (b_off, b_off_p) = _host(a_off), _host(b_off)
        n_a, n_b = a_off.size - 1, b_off.size - 1
        dev = _device_input(a, b, dtype=torch.float64, one_dim=False)
        scores = torch.zeros((n_a, n_b), dtype=torch.float64, device=dev)
        pos = torch.zeros((n_a, n_b, 2), dtype=torch.int32, device=dev) if want_pos else None
        _call(dev, self.L.ps_pairwise_scores, self.handle, _ptr(a), a_off_p, n_a, _ptr(b), b_off_p, n_b, int(mode), float(penalty),
              _ptr(scores), _ptr(pos))
        return scores, pos

    @_serialised
    def pairwise_batch(self, a, a_off, b, b_off, pair_a, pair_b, mode, penalty, min_length=2, col_slots=None,
                       aln_slots=None):
        """ps_pairwise_batch: pair q = (A[pair_a[q]], B[pair_b[q]]) with traceback.  Returns numpy arrays: (scores [n],
        status [n], cols_i, cols_j (index columns in walk order, -1 a gap), col_off [n + 1], aln_score, aln_start, aln_len,
        aln_off [n + 1], aln_count [n]).  Slots that turn out too small (PS_ERR_CAPACITY) make the call run again with
        the sizes the first run reported."""
        (a_off, a_off_p), (b_off, b_off_p) = _host(a_off), _host(b_off)
        (pair_a, pair_a_p), (pair_b, pair_b_p) = _host(pair_a, np.int32), _host(pair_b, np.int32)
        n = pair_a.size
        assert pair_b.size == n
        dev = _device_input(a, b, dtype=torch.float64, one_dim=False)
        if n and (pair_a.min() < 0 or pair_a.max() >= a_off.size - 1 or pair_b.min() < 0 or pair_b.max() >= b_off.size - 1):
            raise ValueError("a pair names a sequence that is not there")
        m_len = np.diff(a_off)[pair_a] if n else np.zeros(0, np.int64)
        n_len = np.diff(b_off)[pair_b] if n else np.zeros(0, np.int64)
        if col_slots is None:       # global and local alignments have at most m + n columns; repeated ones are re-run if they need more
            col_slots = (m_len + n_len) * (1 if mode != _lib.PS_PW_LOCAL_REPEATED else 2)
        if aln_slots is None:
            aln_slots = np.ones(n, np.int64) if mode != _lib.PS_PW_LOCAL_REPEATED else np.minimum(m_len, n_len) + 1
        scores = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
        status, col_need, aln_count = (torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3))

        def attempt(col_slots, aln_slots):
            (col_off, col_off_p), (aln_off, aln_off_p) = _slot_offsets(col_slots), _slot_offsets(aln_slots)
            cols = torch.zeros((2, max(int(col_off[-1]), 1)), dtype=torch.int32, device=dev)
            aln_score = torch.zeros(max(int(aln_off[-1]), 1), dtype=torch.float64, device=dev)
            aln_il = torch.zeros((2, max(int(aln_off[-1]), 1)), dtype=torch.int32, device=dev)
            rc = _call_rc(dev, self.L.ps_pairwise_batch, self.handle, _ptr(a), a_off_p, a_off.size - 1, _ptr(b), b_off_p, b_off.size - 1,
                          pair_a_p, pair_b_p, n, int(mode), float(penalty), int(min_length), _ptr(scores), _ptr(status), col_off_p,
                          _ptr(cols[0]), _ptr(cols[1]), _ptr(col_need), aln_off_p, _ptr(aln_score), _ptr(aln_il[0]), _ptr(aln_il[1]),
                          _ptr(aln_count))
            return rc, (col_off, cols, aln_off, aln_score, aln_il)

        _, (col_off, cols, aln_off, aln_score, aln_il) = _retry_slots(
            self.handle, attempt, lambda: (_int64_host(col_need, n), _int64_host(aln_count, n)), (col_slots, aln_slots))
        cols, aln_il = cols.cpu().numpy(), aln_il.cpu().numpy()
        return (scores[:n].cpu().numpy(), status[:n].cpu().numpy(), cols[0], cols[1], col_off, aln_score.cpu().numpy(),
                aln_il[0], aln_il[1], aln_off, aln_count[:n].cpu().numpy())

    @_serialised
    def trf_split_batch(self, mean, std, off, penalty, min_score, max_repeats=0, slots=None, retry=True):
        """ps_trf_split_batch: the repeats of every sequence q = (mean, std)[off[q]:off[q+1]] (float64 CUDA tensors), the
        reference's NaiveSplitter.  Returns (rc, score float64, length, i, j int32 -- numpy, sequence q's yields at
        slot_off[q] .. slot_off[q] + count[q] in yield order --, slot_off [n + 1], count int32 [n], status int32 [n]).
        slots: entries per sequence (default: its segments, what random levels yield about twice over).  Yields beyond a
        slot are counted, not stored (PS_ERR_CAPACITY); with retry the call then runs again with slots of the exact counts
        and rc is PS_OK; without, rc is returned as it is (PS_OK or PS_ERR_CAPACITY) with whatever fitted and the true
        counts.  Any other status raises."""
        off, off_p = _host(off)
        n = off.size - 1
        dev = _device_input(mean, std, dtype=torch.float64, one_dim=False)
        if slots is None:
            slots = np.diff(off)
        slots = np.asarray(slots, np.int64).reshape(-1)
        assert slots.size == n
        count, status = (torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(2))

        def attempt(slots):
            slot_off, slot_off_p = _slot_offsets(slots)
            score = torch.zeros(max(int(slot_off[-1]), 1), dtype=torch.float64, device=dev)
            lij = torch.zeros((3, max(int(slot_off[-1]), 1)), dtype=torch.int32, device=dev)
            rc = _call_rc(dev, self.L.ps_trf_split_batch, self.handle, _ptr(mean), _ptr(std), off_p, n, float(penalty), float(min_score),
                          int(max_repeats), _ptr(score), _ptr(lij[0]), _ptr(lij[1]), _ptr(lij[2]), slot_off_p, _ptr(count), _ptr(status))
            return rc, (slot_off, score, lij)

        rc, (slot_off, score, lij) = _retry_slots(self.handle, attempt, lambda: (_int64_host(count, n),), (slots,), retry)
        lij = lij.cpu().numpy()
        return rc, score.cpu().numpy(), lij[0], lij[1], lij[2], slot_off, count[:n].cpu().numpy(), status[:n].cpu().numpy()

    @_serialised
    def hmm_batch(self, model, mode, obs, off, want_mat=False, path_slots=None):
        """ps_hmm_batch: one HMM pass over a batch of sequences.  model: a _lib.HmmModel (its arrays kept alive by the caller);
        obs: float64 CUDA tensor, sequence q = obs[off[q]:off[q+1]].  Returns (logp float64 [n_seq], matrix float64
        [off[-1] + n_seq, n_states] or None, and for Viterbi: (path int32 tensor, path offsets, path lengths int32 tensor)
        -- else None).  A Viterbi path longer than its slot (path_slots[q] entries, default 2 (n + 1) + the silent states + 1)
        makes the call run again with slots of the exact lengths (PS_ERR_CAPACITY)."""
        off, off_p = _host(off)
        n_seq = off.size - 1
        dev = _device_input(obs, dtype=torch.float64, one_dim=False)
        S = model.n_states
        logp = torch.empty(max(n_seq, 1), dtype=torch.float64, device=dev)
        mat = torch.empty((int(off[-1]) + n_seq, S), dtype=torch.float64, device=dev) if want_mat else None
        args = (self.L.ps_hmm_batch, self.handle, ctypes.byref(model), int(mode), _ptr(obs), off_p, n_seq, _ptr(logp), _ptr(mat))
        if mode != _lib.PS_HMM_VITERBI:
            _call(dev, *args, None, None, None)
            return logp[:n_seq], mat, None
        if path_slots is None:
            path_slots = 2 * (np.diff(off) + 1) + (S - model.n_emit) + 1
        path_len = torch.empty(max(n_seq, 1), dtype=torch.int32, device=dev)

        def attempt(path_slots):
            path_off, path_off_p = _slot_offsets(path_slots)
            path = torch.empty(max(int(path_off[-1]), 1), dtype=torch.int32, device=dev)
            return _call_rc(dev, *args, _ptr(path), path_off_p, _ptr(path_len)), (path, path_off)

        _, (path, path_off) = _retry_slots(self.handle, attempt, lambda: (_int64_host(path_len, n_seq),), (path_slots,))
        return logp[:n_seq], mat, (path, path_off, path_len[:n_seq])

    @_serialised
    def hmm_expect(self, model, obs, off, stat_width=3, mix_rows=0):
        """ps_hmm_expect: the Baum-Welch E-step over a batch.  model: a _lib.HmmModel (its arrays kept alive by the caller);
        obs: float64 CUDA tensor, sequence q = obs[off[q]:off[q+1]].  Returns (logp float64 [n_seq], edge counts float64
        [n_edges] in out-edge order, statistics float64 [n_emit, stat_width], the number of sequences skipped for
        logp = -inf).  stat_width: the doubles per emitting state the library writes -- 3, (W, A, B), or 1 + 2 n_dim for a
        vector model (kind 4), whose obs holds n_dim doubles per observation; the caller, who built the model, says which
        (pypore_amd.hmm.Model._stat_width).  mix_rows: the mixture components of a model with kind-7 states (mix_ptr[n_emit]):
        the statistics are then [n_emit + mix_rows, 3], the states' rows followed by one row per component."""
        off, off_p = _host(off)
        n_seq = off.size - 1
        dev = _device_input(obs, dtype=torch.float64, one_dim=False)
        n_edges = int(ctypes.cast(model.out_ptr, ctypes.POINTER(ctypes.c_int32))[model.n_states])
        logp = torch.empty(max(n_seq, 1), dtype=torch.float64, device=dev)
        counts = torch.empty(max(n_edges, 1), dtype=torch.float64, device=dev)
        rows = model.n_emit + int(mix_rows)
        stats = torch.empty((max(rows, 1), int(stat_width)), dtype=torch.float64, device=dev)
        skipped = ctypes.c_int32(0)
        _call(dev, self.L.ps_hmm_expect, self.handle, ctypes.byref(model), _ptr(obs), off_p, n_seq, _ptr(logp), _ptr(counts), _ptr(stats),
              ctypes.byref(skipped))
        return logp[:n_seq], counts[:n_edges], stats[:rows], int(skipped.value)

    @_serialised
    def hmm_posterior(self, model, obs, off, want_post=False, want_map=True, want_counts=False):
        """ps_hmm_posterior: posterior decoding over a batch, nothing summed over the sequences.  model: a _lib.HmmModel
        (its arrays kept alive by the caller); obs: float64 CUDA tensor, sequence q = obs[off[q]:off[q+1]].  Returns (logp
        float64 [n_seq]; log posteriors float64 [off[-1], n_emit] when want_post; MAP states int32 [off[-1]] and MAP log
        probabilities float64 [n_seq] when want_map; per-sequence edge counts float64 [n_seq, n_edges] in out-edge order
        when want_counts), None for what was not asked for: only the outputs asked for are allocated."""
        off, off_p = _host(off)
        n_seq, total = off.size - 1, int(off[-1])
        dev = _device_input(obs, dtype=torch.float64, one_dim=False)
        n_edges = int(ctypes.cast(model.out_ptr, ctypes.POINTER(ctypes.c_int32))[model.n_states])
        logp = torch.empty(max(n_seq, 1), dtype=torch.float64, device=dev)
        post = torch.empty((total, model.n_emit), dtype=torch.float64, device=dev) if want_post else None
        map_state = torch.empty(total, dtype=torch.int32, device=dev) if want_map else None
        map_logp = torch.empty(max(n_seq, 1), dtype=torch.float64, device=dev) if want_map else None
        counts = torch.empty((n_seq, n_edges), dtype=torch.float64, device=dev) if want_counts else None
        _call(dev, self.L.ps_hmm_posterior, self.handle, ctypes.byref(model), _ptr(obs), off_p, n_seq, _ptr(logp), _ptr(post),
              _ptr(map_state), _ptr(map_logp), _ptr(counts))
        return logp[:n_seq], post, map_state, map_logp[:n_seq] if want_map else None, counts

    @_serialised
    def hmm_sample(self, model, tables, seed, first, n_seq, length=0, max_length=1000000, want_path=False, obs_slots=None,
                   path_slots=None, retry=True):
        """ps_hmm_sample: n_seq walks of the model, sequence q on the random stream of (seed, first + q).  model: a
        _lib.HmmModel, tables: a _lib.HmmSampleTables (their arrays kept alive by the caller).  Returns (rc, obs float64
        tensor [slots, n_dim], off, lengths int32 [n_seq], flags int32 [n_seq], and (path int32 tensor, path offsets, path
        lengths int32 [n_seq]) or None): sequence q is obs[off[q]:off[q] + lengths[q]].  obs_slots / path_slots: entries per
        sequence (default: `length`, or 2 n_emit observations when it is 0; 2 (slot + 1) + the silent states + 1 path
        entries).  A walk longer than its slot is counted, not written (PS_ERR_CAPACITY); with retry the call then runs
        again with slots of the exact lengths -- the walks are the same -- and rc is PS_OK; without, rc is returned as it
        is (PS_OK or PS_ERR_CAPACITY) with whatever fitted.  Any other status raises."""
        n_seq = int(n_seq)
        dev = torch.device("cuda", self.device)
        D = model.n_dim if model.n_dim > 1 else 1
        if obs_slots is None:
            obs_slots = np.full(max(n_seq, 0), int(length) if length > 0 else 2 * model.n_emit, np.int64)
        obs_slots = np.asarray(obs_slots, np.int64).reshape(-1)
        if want_path and path_slots is None:
            path_slots = 2 * (obs_slots + 1) + (model.n_states - model.n_emit) + 1
        lens = torch.empty(max(n_seq, 1), dtype=torch.int32, device=dev)
        flags = torch.empty(max(n_seq, 1), dtype=torch.int32, device=dev)
        path_len = torch.empty(max(n_seq, 1), dtype=torch.int32, device=dev) if want_path else None

        def attempt(obs_slots, path_slots):
            off, off_p = _slot_offsets(obs_slots)
            obs = torch.empty((max(int(off[-1]), 1), D), dtype=torch.float64, device=dev)
            path = path_off = path_off_p = None
            if want_path:
                path_off, path_off_p = _slot_offsets(np.asarray(path_slots, np.int64).reshape(-1))
                path = torch.empty(max(int(path_off[-1]), 1), dtype=torch.int32, device=dev)
            rc = _call_rc(dev, self.L.ps_hmm_sample, self.handle, ctypes.byref(model), ctypes.byref(tables),
                          ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(first), n_seq, int(length), int(max_length), _addr(obs),
                          off_p, _ptr(lens), _ptr(flags), _ptr(path), path_off_p, _ptr(path_len))
            return rc, (obs, off, path, path_off)

        rc, (obs, off, path, path_off) = _retry_slots(
            self.handle, attempt, lambda: (_int64_host(lens, n_seq), _int64_host(path_len, n_seq) if want_path else None),
            (obs_slots, path_slots), retry)
        return rc, obs, off, lens[:n_seq], flags[:n_seq], ((path, path_off, path_len[:n_seq]) if want_path else None)

    @_serialised
    def synth_trace(self, n, seed, seg_end, level_counts, dtype=torch.float32, start=0):
        """Synthetic step trace generated directly in HBM (csrc synth_kernel == pypore_amd.synth).  start > 0: the
        samples [start, start + n) of the trace the table describes (a rank's piece of one long trace): the noise hash
        of sample i is splitmix64(seed + (i + 1) * GOLDEN), so the piece is the same generator with a shifted seed and a
        table cut at `start`."""
        out = torch.empty(n, dtype=dtype, device="cuda:%d" % self.device)
        seg_end = np.asarray(seg_end, dtype=np.int64)
        level_counts = np.asarray(level_counts, dtype=np.int32)
        if start:
            first = int(np.searchsorted(seg_end, start, side="right"))
            seg_end, level_counts = seg_end[first:] - start, level_counts[first:]
            seed = (int(seed) + int(start) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        (seg_end, seg_end_p), (level_counts, level_counts_p) = _host(seg_end), _host(level_counts, np.int32)
        _call(out.device, self.L.ps_synth_trace, self.handle, _addr(out), _lib.PS_DTYPE_F32 if dtype == torch.float32 else _lib.PS_DTYPE_I16,
              n, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), seg_end_p, level_counts_p, seg_end.size)
        return out


NEAR_TIE_DTYPE = np.dtype([("event", np.int32), ("window_start", np.int32), ("window_end", np.int32), ("split", np.int32)])


def consistent_sites(sites, bounds, bounds_off, lengths, window_width):
    """The near-tie sites of a call (Context.near_tie_sites) that belong to its final recursion.  The log also holds
    speculative scans (tile spines, look-ahead helpers, bridges); by DESIGN.md 3 every window the final recursion scans
    starts at s + k * (window_width // 2) for some s in B = {0} u boundaries u {n} other than n, ends at
    min(e, window_start + window_width) for some range end e in B beyond its start, and splits, if at all, at a returned
    boundary.  A site is kept when all three hold.  bounds / bounds_off: the call's boundaries (flat, per-event offsets),
    lengths: the events' lengths.  None stays None."""
    if sites is None:
        return None
    W = int(window_width)
    half = max(1, W // 2)
    arr = sites if isinstance(sites, np.ndarray) else np.array([tuple(x) for x in sites], dtype=NEAR_TIE_DTYPE)
    keep = np.zeros(len(arr), dtype=bool)
    bounds = np.asarray(bounds, dtype=np.int64)
    ev = arr["event"].astype(np.int64)
    for e in np.unique(ev):                                 # (vectorised per event: sites x range starts)
        rows = np.nonzero(ev == e)[0]
        ws = arr["window_start"][rows].astype(np.int64)
        we = arr["window_end"][rows].astype(np.int64)
        sp = arr["split"][rows].astype(np.int64)
        n = int(lengths[e])
        b = bounds[int(bounds_off[e]):int(bounds_off[e + 1])]
        starts = np.concatenate(([0], b))                   # B without n
        d = ws[:, None] - starts[None, :]
        on_grid = np.any((d >= 0) & (d % half == 0), axis=1)
        ends = np.concatenate((b, [n]))                     # range ends beyond 0
        end_ok = ((we == ws + W) & (n >= ws + W)) | ((we < ws + W) & (we > ws) & np.isin(we, ends))
        split_ok = (sp == -1) | np.isin(sp, b)
        keep[rows] = on_grid & end_ok & split_ok
    return sites[keep] if isinstance(sites, np.ndarray) else [x for x, kk in zip(sites, keep) if kk]


def events_to_redo(sites, n_ev):
    """Events of a call that the exact route must redo under off_grid="exact_on_near_tie": those with a site, or all of
    them when the sites are None (not counted, or the log overflowed)."""
    if sites is None:
        return list(range(int(n_ev)))
    return sorted({int(e) for e in np.asarray(sites["event"] if isinstance(sites, np.ndarray) else [s[0] for s in sites])})


class NearTieWarning(UserWarning):
    """A segment call decided at least one window by a margin inside the reference's own rounding noise: the logarithm's last
    bit on grid data, the noise of its uncentred cumsums on re-quantised float64 data (Context.near_ties)."""


class CapacityError(RuntimeError):
    """The caller's output capacity was too small (PS_ERR_CAPACITY): `required` is the size that fits."""

    def __init__(self, required, cap):
        RuntimeError.__init__(self, "poreseg: output capacity %d < required %d" % (cap, required))
        self.required, self.cap = int(required), int(cap)


NEAR_TIE_WARNING = True      # set False to skip the counter read after every call (one ps_get_timings, ~1 us)


class StreamPool(object):
    """T contexts on one GPU (each a ps_ctx with its own HIP stream and scratch) fed by T host threads.

    One call of the path is a chain of kernels with idle stretches -- the tails of the spine and subtree kernels, the
    single-workgroup stitch kernels, the seam bridges that occupy a fraction of the chip.  Batches are independent
    (events and files are the reference's own unit of work, DataTypes.py:968-984), so the kernels of one batch fill the
    idle stretches of another when they are submitted on different streams: two streams deliver 1.4x the batches per
    second of one on the 1e8-sample bench trace, with bit-identical results.  ctypes drops the GIL for the duration of a
    call, so plain Python threads are enough.  Every call still ends with its own stream synchronisation.

    A host that keeps the pool busy for long should take CPython's cyclic collector out of the way (`gc.collect();
    gc.freeze()` once everything is set up): a full collection holds the GIL for tens of milliseconds and every worker
    then waits for it on its way out of the C call -- 0.33 instead of 0.35-0.43 ms per 1e8-sample batch over runs of
    400-2000 batches (tools/pool_stalls.py).

    HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue run their
    kernels one after the other: of T contexts min(T, queues) calls execute at a time.  The library plans each pooled call
    for that many ("shared_device", ps_pool_plan: DESIGN.md section 6 has the table), so the pool needs nothing set; a host
    that wants sixteen calls in flight exports GPU_MAX_HW_QUEUES=16 before the runtime starts.  Round 4, 1e8-sample trace,
    as many queues as contexts: 4 / 8 / 16 contexts in flight deliver a batch every 0.216 / 0.202 / 0.189 ms."""

    def __init__(self, device=None, streams=2, overrides=None):
        """overrides: ps_set_option name -> value applied to the pool's contexts while it runs, on top of "shared_device"
        (default: engine.POOL_OVERRIDES, empty in the product)."""
        import queue
        import threading
        base = context(device)
        self.contexts = [base] + [Context(base.device) for _ in range(max(1, int(streams)) - 1)]
        self.overrides = dict(POOL_OVERRIDES if overrides is None else overrides)
        self._shared_now = {}                            # id(context) -> the "shared_device" value it was last given
        # persistent workers for contexts 1 .. T-1 (the caller's thread drives context 0): a run() costs a queue
        # hand-over per worker, not a thread start
        self._inbox = [queue.SimpleQueue() for _ in self.contexts]
        self._done = queue.SimpleQueue()
        self._threads = []
        for t in range(1, len(self.contexts)):
            th = threading.Thread(target=self._worker, args=(t,), daemon=True)
            th.start()
            self._threads.append(th)

    def __len__(self):
        return len(self.contexts)

    def _share(self, t, n_jobs, job, results, errors, ticket=None):
        try:
            if ticket is None:                         # fixed shares: job k on context k % T
                for k in range(t, n_jobs, len(self.contexts)):
                    results[k] = job(self.contexts[t], k, t)
            else:                                      # whoever is free takes the next job
                while True:
                    k = next(ticket)                   # (itertools.count: one C call, atomic under the GIL)
                    if k >= n_jobs:
                        break
                    results[k] = job(self.contexts[t], k, t)
        except BaseException as e:                     # noqa: B036 -- re-raised on the submitting thread
            errors.append(e)

    def _worker(self, t):
        while True:
            task = self._inbox[t].get()
            if task is None:
                return
            self._share(t, *task)
            self._done.put(t)

    def close(self):
        for t in range(1, len(self.contexts)):
            self._inbox[t].put(None)
        self._threads = []

    # What a context that shares the chip wants is decided in the library (ps_set_option "shared_device" n -> ps_pool_plan for
    # min(n, hardware queues) calls executing at a time, include/poreseg.h).  With sixteen calls in flight (measured in round 5):
    #   * K0 as a persistent kernel at one wave per SIMD: beside the scan waves of other calls a K0 that takes every wave slot
    #     it can get is in the way (sixteen in flight: 0.193 -> 0.170 ms per step); a lone call is faster with the one-shot K0;
    #   * no look-ahead helpers: with sixteen calls in flight the other calls are the better use of an idle workgroup (a trace
    #     without steps 1.2 -> 8.6 ms per step with them on); for a lone call they are worth 2 x on sparse traces;
    #   * more than three contexts: at most three K0s in flight (K0 is bound by HBM; sixteen of them at once finish late together,
    #     with every call's scan kernels behind them: 0.188 -> 0.175 ms per step).
    # The front stream ("k0_shared") lost (0.26-0.30 ms per step) and is set by nothing; overrides can name it for the record.
    def _configure(self, cx, n):
        """context `cx` shares its device with n - 1 others (n <= 1: a lone context again)"""
        if not hasattr(cx, "set_option") or self._shared_now.get(id(cx)) == n:
            return
        cx.set_option("shared_device", n)
        if n > 1:
            for name, value in self.overrides.items():
                cx.set_option(name, value)
        else:
            if "k0_shared" in self.overrides:
                cx.set_option("k0_shared", 0)
            if _device_shared(getattr(cx, "device", None), cx):
                cx.set_option("lat_help", 0)             # (other threads' contexts are alive on the device: see _note_live)
        # (what the process was started with -- tests / tools through engine.DEFAULT_OPTIONS -- stays in force)
        for name in ("k0_waves", "lat_help", "k0_admit"):
            if name in DEFAULT_OPTIONS:
                cx.set_option(name, DEFAULT_OPTIONS[name])
        self._shared_now[id(cx)] = n

    def run(self, n_jobs, job, dynamic=False):
        """Runs job(ctx, k, t) for k = 0 .. n_jobs-1 and returns the results in job order.  Job k runs on context
        t = k % T, or -- dynamic=True -- on whichever context is free next (jobs of unequal length).  While more than one
        job is in flight the contexts are configured for a shared device; afterwards the caller's own context
        (contexts[0], the one SpeedyStatSplit.parse uses on this thread) is a lone context again, whatever happened."""
        import itertools
        T = len(self.contexts)
        results = [None] * n_jobs
        errors = []
        n_shared = T if (T > 1 and n_jobs > 1) else 1
        try:
            for cx in (self.contexts if n_shared > 1 else self.contexts[:1]):
                self._configure(cx, n_shared)
            ticket = itertools.count() if dynamic else None
            busy = [t for t in range(1, T) if t < n_jobs]
            for t in busy:
                self._inbox[t].put((n_jobs, job, results, errors, ticket))
            self._share(0, n_jobs, job, results, errors, ticket)
            for _ in busy:
                self._done.get()
        finally:
            self._configure(self.contexts[0], 1)         # (every option the run changed, k0_admit included)
        if errors:
            raise errors[0]
        return results

    def segment_many(self, batches, params, quantum, offset_counts=0, want_stats=False):
        """batches: list of (samples CUDA tensor, ev_off); one ps_segment_batch each, spread over the streams.  Returns
        the list of (bounds, bounds_off, stats) in batch order."""
        return self.run(len(batches), lambda ctx, k, t: ctx.segment_batch(batches[k][0], batches[k][1], params, quantum,
                                                                          offset_counts=offset_counts, want_stats=want_stats))


_thread_contexts = threading.local()
_contexts_lock = threading.Lock()


def context(device=None):
    """The Context of `device` (default: torch's current device) that belongs to the CALLING THREAD.

    A ps_ctx serves one call at a time (its stream, its scratch, its status block).  The reference is safe under the GIL
    (a new FastStatSplit per parse()); here ctypes drops the GIL for the duration of a call, so two threads that call
    SpeedyStatSplit.parse at once must not meet in one ps_ctx.  The main thread keeps the process-wide context of the
    device; every other thread gets one of its own on first use (its own HIP stream and scratch: calls of different threads
    overlap on the GPU like the contexts of a StreamPool) and gives it back when the thread ends.  Each Context also
    carries a lock that its calls take, for code that hands ONE Context to several threads."""
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    device = int(device)
    if threading.current_thread() is threading.main_thread():
        with _contexts_lock:
            fresh = device not in _contexts
            if fresh:
                _contexts[device] = Context(device)
            cx = _contexts[device]
        if fresh:
            _note_live(device, cx)
        return cx
    mine = getattr(_thread_contexts, "by_device", None)
    if mine is None:
        mine = _thread_contexts.by_device = {}
    if device not in mine:
        mine[device] = Context(device)
        _note_live(device, mine[device])
    return mine[device]


_live = {}                                              # device -> weak set of the contexts engine.context() handed out


def _device_shared(device, cx):
    with _contexts_lock:
        return any(c is not cx and getattr(c, "handle", None) for c in _live.get(device, ()))


def _note_live(device, cx):
    """The look-ahead kernel's helpers are for a call that has the chip to itself.  Whether a context is alone is a matter of
    how many contexts are alive on its device -- not of which thread made it: a program that does all its work on ONE worker
    thread (a notebook kernel, a server) keeps the helpers; once a second context appears on the device, all of them run
    without (the sharing may end when a thread does; the helpers then stay off for the survivors, which is the safe side)."""
    import weakref
    with _contexts_lock:
        live = _live.setdefault(device, weakref.WeakSet())
        live.add(cx)
        others = [c for c in live if c is not cx and getattr(c, "handle", None)]
    if others and "lat_help" not in DEFAULT_OPTIONS:
        for c in others + [cx]:
            if hasattr(c, "set_option"):
                c.set_option("lat_help", 0)


# ---- host-side input normalisation -------------------------------------------------------------
class GridRefusal(ValueError):
    """The values are not what a road takes -- on no power-of-two grid (detect_quantum), or not exact in float32 -- so the
    caller may try the next road.  Every other ValueError of the upload is an error and goes through to the caller."""


def detect_quantum(x, max_bits=24, full=True):
    """Largest power of two q = 2**-k (0 <= k <= max_bits) such that every sample of the numpy
    array `x` is an integer multiple of q; ValueError if there is none (off-grid data).
    Real traces are int16 ADC counts times a scale (read_abf.py:202-210), so such a q exists
    whenever the scale is a power of two; pass quantum= explicitly to skip this host pass.
    The candidate is found on a strided subset (<= 65 536 samples) and then confirmed on the whole
    array, so a large trace costs two passes instead of one per bit.  With full=False the confirmation
    is left to the device, which checks every sample anyway (PS_ERR_OFF_GRID -> ValueError)."""
    x = np.asarray(x)
    if x.size == 0:
        return 1.0

    def integral(a, k):
        y = a * (2.0 ** k)
        return bool(np.all(y == np.rint(y)))

    def smallest_k(a):
        for k in (5,) + tuple(i for i in range(0, max_bits + 1) if i != 5):
            if integral(a, k):
                while k > 0 and integral(a, k - 1):        # coarsest grid that still holds
                    k -= 1
                return k
        return None

    sub = x[::max(1, x.size // 65536)]
    k = smallest_k(sub)
    if k is None:
        raise GridRefusal("samples are not on a power-of-two ADC grid; pass quantum= (pA per count)")
    if not full or sub.size == x.size or integral(x, k):
        return 2.0 ** -k
    k = smallest_k(x)                                      # the subset was too coarse a witness: full search
    if k is None:
        raise GridRefusal("samples are not on a power-of-two ADC grid; pass quantum= (pA per count)")
    return 2.0 ** -k


Samples = collections.namedtuple("Samples", "tensor quantum offset")      # pA = count * quantum + offset


COUNTS_BEYOND_INT16 = "ADC counts beyond int16 on a grid that is not a power of two: not supported"
NOT_FLOAT32 = "samples are not exactly representable in float32; pass int16 counts or a coarser grid"


def _int_counts_tensor(counts, dev):
    """int16 CUDA tensor of integer counts; ValueError when they leave the int16 range."""
    counts = np.asarray(counts)
    if counts.dtype != np.int16:
        if counts.size and (counts.min() < -32768 or counts.max() > 32767):
            raise ValueError(COUNTS_BEYOND_INT16)
        counts = counts.astype(np.int16)
    if counts.size >= _STAGE_MIN:
        return _staged_upload(counts, dev)
    with warnings.catch_warnings():                     # (a read-only memmap of an .abf: the tensor is only copied from)
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.ascontiguousarray(counts)).to(dev)


_STAGE_MIN = 1 << 22                                    # samples: below this one pageable copy is as fast
_STAGE_CHUNK = 1 << 24                                  # int16 samples per staging buffer (32 MB)
_STAGE_F64_MIN = _STAGE_MIN                             # numpy float64 of at least this many samples goes up raw and finds its grid
                                                        # on the device (_float64_on_device); None: always the host passes
_STAGE_CHUNK_F64 = 1 << 22                              # float64 samples per staging buffer (32 MB)
INGEST_PASS = 2048                                      # samples per workgroup pass of the ingest kernels (csrc/seg_ingest.hpp ING_T)
INGEST_GRID_MAX = 2048                                  # ... and their workgroups at most (ING_GRID_MAX): longer buffers stride
_stage = {}
_stage_lock = threading.Lock()                          # the staging buffers of a device are shared: one upload at a time


def _staged_upload(counts, dev):
    """A long int16 array (the data section of an .abf, usually a memmap of the page cache) -> CUDA tensor through two
    pinned staging buffers: the host's copy of chunk k+1 out of the page cache runs while chunk k crosses PCIe.  One
    `np.ascontiguousarray` of the whole file plus a pageable copy of it is 2-3 x slower (tools/bench_experiment.py).
    A float64 array (a caller's pA values on their way to the device's grid recovery) goes the same way through
    buffers of its own."""
    f64 = counts.dtype == np.float64
    dtype, chunk = (torch.float64, _STAGE_CHUNK_F64) if f64 else (torch.int16, _STAGE_CHUNK)
    key = (dev.index, dtype)
    with _stage_lock:                                    # (two host threads uploading to one device would overwrite each other's chunks)
        if key not in _stage or _stage[key][0][0].numel() != chunk:
            _stage[key] = ([torch.empty(chunk, dtype=dtype, pin_memory=True) for _ in range(2)],
                           [torch.cuda.Event() for _ in range(2)], torch.cuda.Stream(device=dev))
        bufs, events, stream = _stage[key]
        out = torch.empty(counts.size, dtype=dtype, device=dev)
        # `out` comes from the caching allocator on the CURRENT stream: work still queued there on a recycled block must
        # be finished before the side stream writes into it
        stream.wait_stream(torch.cuda.current_stream(dev))
        used = [False, False]
        with torch.cuda.stream(stream):
            for k, a in enumerate(range(0, counts.size, chunk)):
                b = min(counts.size, a + chunk)
                i = k & 1
                if used[i]:
                    events[i].synchronize()              # the copy that last read this buffer is done
                np.copyto(bufs[i].numpy()[:b - a], counts[a:b])
                out[a:b].copy_(bufs[i][:b - a], non_blocking=True)
                events[i].record(stream)
                used[i] = True
        stream.synchronize()
    return out


def _recovered(x, dev, want_counts):
    """A float64 CUDA tensor on no power-of-two grid -> (Samples(int16 counts, quantum, offset), the counts on the host as
    int64 when asked for: 2 B/sample come down) by grid.affine_grid_device; ValueError as grid.affine_grid raises it."""
    from .grid import affine_grid_device
    q, o, k = affine_grid_device(x, dev)
    return Samples(k, q, o), (k.cpu().numpy().astype(np.int64) if want_counts else None)


def _float64_on_device(a, dev, want_counts):
    """to_device_with_counts for a long numpy float64 array without quantum= / offset=: the raw values go up once through
    pinned staging and the full-array passes run there.  The decisions are the host road's, in its order: the power-of-two
    grid of the subset (detect_quantum) and an exact float32 copy (ps_narrow_f64 for astype / astype / array_equal) give
    the float32 tensor; a refusal of either leads to the affine grid (grid.affine_grid_device for grid.affine_grid)."""
    x = _staged_upload(a, dev)
    try:
        q = detect_quantum(a, full=False)
        t, bad = context(dev.index).narrow_f64(x)
        if bad:
            raise GridRefusal(NOT_FLOAT32)
        return Samples(t, q, 0.0), None
    except GridRefusal:
        return _recovered(x, dev, want_counts)


def to_device(current, quantum=None, offset=None, device=None, full_detect=False):
    """Anything a caller of the parser API may hand over -> Samples(CUDA tensor, quantum, offset).

    * a GridArray (what abf.read_abf returns; slices of it): its int16 counts, 2 B/sample;
    * numpy int16: ADC counts, quantum as given (default 1);
    * numpy float64 / float32 pA: with `quantum` a power of two (or none given and a power-of-two grid found) the
      values go up as float32, exactly; otherwise the counts are recovered -- rint((x - offset) / quantum) when the
      grid is given, grid.affine_grid(x) when it is not -- and go up as int16.  Data that lies on no grid at all
      raises ValueError: nothing is ever rounded silently.  A float64 array of _STAGE_F64_MIN samples or more without
      quantum= / offset= goes up raw and takes these decisions on the device (_float64_on_device): same tensors;
    * torch tensors (float32 / float64 / int16, host or device) are taken as they are; a float64 CUDA tensor that is not
      exact in float32 finds its grid on the device (grid.affine_grid_device) and becomes int16 counts there.
    """
    return _to_device(current, quantum, offset, device, full_detect, False)[0]


def to_device_with_counts(current, quantum=None, offset=None, device=None, full_detect=False):
    """to_device, and how the caller's pA values x relate to the counts k the kernels read: None when x = fl(fl(k * quantum)
    + offset) by construction (a file's counts, int16, a tensor, float samples on a power-of-two grid without an offset);
    otherwise the counts (int64 numpy, on the host) that float samples went up as -- the caller's values are then their own
    rounding of the grid, and only they can say which count a threshold falls on (detector_thresholds).  Counts that were
    recovered on the device come down as int16 for this (to_device leaves them there)."""
    return _to_device(current, quantum, offset, device, full_detect, True)


def _to_device(current, quantum, offset, device, full_detect, want_counts):
    from .grid import affine_grid, grid_of
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    g = grid_of(current) if quantum is None else None
    if g is not None:
        from .grid import Deferred
        if isinstance(current, Deferred) and current.counts is not None:
            # (a file's counts go up once: events cut from the file are stretches of the same device tensor)
            return Samples(current.device_counts(dev, _int_counts_tensor), g[1], g[2]), None
        return Samples(_int_counts_tensor(g[0], dev), g[1], g[2]), None
    if (isinstance(current, torch.Tensor) and current.is_cuda and current.dtype == torch.float64 and current.dim() == 1
            and quantum is None and offset is None):
        try:                                        # exact in float32 on a power-of-two grid: as it always went up
            t, q = to_device_samples(current, quantum, device, full_detect)
            return Samples(t, q, 0.0), None
        except GridRefusal:                         # not float32, or float32 on no power-of-two grid (numpy input goes on to the
                                                    # affine grid after either): any scale and offset, the counts found on the device
            return _recovered(current.detach().to(dev), dev, want_counts)
    if isinstance(current, torch.Tensor) or np.asarray(current).dtype == np.int16:
        t, q = to_device_samples(current, quantum, device, full_detect)
        return Samples(t, q, 0.0 if offset is None else float(offset)), None
    a = np.asarray(current)
    if a.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
    if a.dtype not in (np.float64, np.float32):
        raise ValueError("Buffer dtype mismatch, expected 'double' but got %s" % a.dtype)
    if (a.dtype == np.float64 and quantum is None and offset is None and not full_detect
            and _STAGE_F64_MIN is not None and a.size >= _STAGE_F64_MIN):
        return _float64_on_device(a, dev, want_counts)
    off = 0.0 if offset is None else float(offset)
    pow2 = quantum is not None and quantum > 0 and np.log2(quantum) == np.rint(np.log2(quantum))
    if quantum is None or pow2:
        try:
            shifted = a - off if off else a
            t, q = to_device_samples(shifted, quantum, device, full_detect)
            return Samples(t, q, off), (np.rint(shifted / q).astype(np.int64) if off else None)
        except ValueError:
            if quantum is not None:
                raise
    if quantum is None:                             # no power-of-two grid: any scale and offset (a real .abf header)
        q, o, k = affine_grid(a)
        return Samples(_int_counts_tensor(k, dev), q, o), k
    k = (a.astype(np.float64) - off) / float(quantum)
    kr = np.rint(k)
    if a.size and np.max(np.abs(k - kr)) > 1e-6:
        raise ValueError("samples are not integer multiples of quantum=%r above offset=%r" % (quantum, off))
    kr = kr.astype(np.int64)
    return Samples(_int_counts_tensor(kr, dev), float(quantum), off), kr


def _first_count(pred, guess):
    """The smallest integer k (within +-2^31) with pred(k), for a predicate that is monotone in k, found by a walk from guess."""
    lim = 2147483000
    k = max(-lim, min(lim, guess))
    while k > -lim and pred(k - 1):
        k -= 1
    while k < lim and not pred(k):
        k += 1
    return k


def _count_threshold(q, t, offset, strict):
    """(first - 0.5) * q, first the smallest count k with fl(fl(k q) + offset) >= t (strict: > t); t - offset where there
    is nothing to round (offset 0: fl(k q) itself is the caller's value) or no count to find (t or q not finite, q <= 0)."""
    if offset == 0.0 or not (np.isfinite(t) and np.isfinite(q) and q > 0.0):
        return t - offset
    g = max(-2.0 ** 31, min(2.0 ** 31, (t - offset) / q))      # (a huge t: the walk starts, and stays, at the clamp)
    if strict:
        first = _first_count(lambda k: float(k) * q + offset > t, int(np.floor(g)) + 1)
    else:
        first = _first_count(lambda k: float(k) * q + offset >= t, int(np.ceil(g)))
    return (first - 0.5) * q


def detector_thresholds(quantum, threshold, min_current, offset=0.0, values=None, counts=None):
    """The detector's thresholds as the library must receive them.  The kernels test double(k) * quantum < threshold and
    > min_current on the counts k; the caller's rule is x < threshold and x > min_current on the pA values x it holds.
    Both are monotone in k, so each rule is k < kthr (k > kmin) for one integer, and the library is handed
    (kthr - 0.5) * quantum and (kmin + 0.5) * quantum: half a count from every count, the test is exact for |k| < 2^31.

    values / counts None: x = fl(fl(k * quantum) + offset), as GridArray.from_counts and abf.read_abf compute it (a file, a
    device tensor, int16 counts); with offset 0 the kernel's own product is x and the thresholds go through unchanged, and
    a threshold that is not finite (min_current=-inf: the rule off) moves by the offset as it is.  Otherwise the caller's
    samples and the counts they went up as (to_device_with_counts): the thresholds are read off the data, and None is
    returned when the data are not monotone in k across a threshold (no count-space threshold reproduces x < threshold)."""
    threshold, min_current, q = float(threshold), float(min_current), float(quantum)
    if values is None:
        offset = float(offset)
        return _count_threshold(q, threshold, offset, False), _count_threshold(q, min_current, offset, True)
    x = np.asarray(values)
    k = np.asarray(counts, dtype=np.int64)
    out = []
    for hit in (x >= threshold, x > min_current):          # k_thr: first count at or above the threshold; k_min + 1: first above min_current
        if hit.all():
            first = int(k.min()) if k.size else 0
        elif not hit.any():
            first = int(k.max()) + 1
        else:
            first = int(k[hit].min())
            if int(k[~hit].max()) >= first:                # the same count on both sides of the rule
                return None
        out.append((first - 0.5) * q)
    return tuple(out)


def to_device_samples(current, quantum=None, device=None, full_detect=False):
    """numpy float64/float32 (pA), numpy int16 (ADC counts) or torch tensor -> (CUDA tensor, quantum).
    Without `quantum` the grid is detected on a subset of the samples (full_detect=True: on all of them); a
    finer grid that only shows elsewhere makes the device call fail with ValueError (off grid)."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    if isinstance(current, torch.Tensor):
        t = current
        if t.dtype == torch.float64:
            t32 = t.to(torch.float32)
            if not torch.equal(t32.to(torch.float64), t):
                raise GridRefusal(NOT_FLOAT32)
            t = t32
        if t.dtype not in (torch.float32, torch.int16):
            raise ValueError("Buffer dtype mismatch, expected float64/float32 pA or int16 counts")
        if quantum is None:
            quantum = 1.0 if t.dtype == torch.int16 else detect_quantum(t.detach().cpu().numpy())
        return t.to(dev).contiguous(), quantum
    a = np.asarray(current)
    if a.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % a.ndim)
    if a.dtype == np.int16:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev), (1.0 if quantum is None else quantum)
    if a.dtype not in (np.float64, np.float32):
        raise ValueError("Buffer dtype mismatch, expected 'double' but got %s" % a.dtype)
    if quantum is None:
        quantum = detect_quantum(a, full=full_detect)
    a32 = a.astype(np.float32)
    if a.dtype == np.float64 and not np.array_equal(a32.astype(np.float64), a):
        raise GridRefusal(NOT_FLOAT32)
    return torch.from_numpy(np.ascontiguousarray(a32)).to(dev), quantum
