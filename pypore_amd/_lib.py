"""ctypes binding of libporeseg.so (include/poreseg.h) -- the thin shim between the Python
class surface and the HIP kernels.  There is NO CPU fallback: if the shared library is missing
or a compute entry point is called without a GPU, this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PORESEG_LIB") or os.path.join(_HERE, "libporeseg.so")   # PORESEG_LIB: diagnostic builds

PS_OK = 0
PS_ERR_ARG, PS_ERR_ASSERT_WIDTH, PS_ERR_ASSERT_WINDOW, PS_ERR_ASSERT_CUTOFF = -1, -2, -3, -4
PS_ERR_CAPACITY, PS_ERR_OFF_GRID, PS_ERR_HIP, PS_ERR_NO_DEVICE, PS_ERR_INTERNAL = -5, -6, -7, -8, -9
PS_DTYPE_F32, PS_DTYPE_I16 = 0, 1
PS_DTYPE_F64 = 2          # float64 pA on no grid: ps_filter_bessel input only
PS_ALIGN_OK, PS_ALIGN_VALUE_ERROR, PS_ALIGN_INDEX_ERROR, PS_ALIGN_ZERO_DIVISION, PS_ALIGN_UNDEFINED = 0, 1, 2, 3, 4

PS_STATSPLIT_STEPWISE, PS_STATSPLIT_SLANTED = 0, 1
PS_HMM_VITERBI, PS_HMM_FORWARD, PS_HMM_BACKWARD = 0, 1, 2
PS_PW_GLOBAL, PS_PW_LOCAL, PS_PW_LOCAL_REPEATED = 0, 1, 2
PS_PW_OK, PS_PW_INDEX_ERROR = 0, 1
PS_TRF_DONE, PS_TRF_MAX_REPEATS = 0, 1
TRF_N_MAX = 2048          # segments per sequence of ps_trf_split_batch
PS_NT_NOT_COUNTED, PS_NT_INCOMPLETE = -1, -2     # ps_get_near_ties: *n_out when the sites are not counted / the log overflowed
# What ps_get_timings returns, in index order (include/poreseg.h: PS_MS_<NAME>, PS_CNT_<NAME>; None: reserved)
MS_NAMES = ("spine", "tree", "gather", "total", "stitch", "bridge", "blocksum", "seq")
COUNTER_NAMES = ("windows", "candidates", "tiles", "tree_jobs", "repairs", "exact_rescans", "full_exact_scans", "wide_redo", "windows_spine",
                 "windows_bridge", "windows_tree", "near_ties", "helper_chunks_published", "helper_chunks_taken", "tree_deferred", "windows_screen",
                 "lookahead_skipped", "upload_skipped", "seams_resumed", None)


class SplitParams(ctypes.Structure):
    _fields_ = [("min_width", ctypes.c_int32), ("max_width", ctypes.c_int32), ("window_width", ctypes.c_int32),
                ("min_gain_per_sample", ctypes.c_double), ("false_positive_rate", ctypes.c_double),
                ("prior_segments_per_second", ctypes.c_double), ("sampling_freq", ctypes.c_double),
                ("cutoff_freq", ctypes.c_double)]


class StatSplitParams(ctypes.Structure):
    """ps_statsplit_params: StatSplit's widths, its threshold min_gain_per_sample * window_width, use_log and the splitter."""
    _fields_ = [("min_width", ctypes.c_int32), ("max_width", ctypes.c_int32), ("window_width", ctypes.c_int32),
                ("threshold", ctypes.c_double), ("use_log", ctypes.c_int32), ("splitter", ctypes.c_int32)]


class FilterDerivativeParams(ctypes.Structure):
    """ps_filter_derivative_params: FilterDerivativeSegmenter's four attributes; prefiltered 1: the input is the filtered
    current itself."""
    _fields_ = [("low_threshold", ctypes.c_double), ("high_threshold", ctypes.c_double), ("cutoff_freq", ctypes.c_double),
                ("sampling_freq", ctypes.c_double), ("prefiltered", ctypes.c_int32)]


class SampleFormat(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("offset_counts", ctypes.c_int32), ("quantum", ctypes.c_double)]


class NearTie(ctypes.Structure):
    """ps_near_tie: one near-tie window of the last segment call, in samples of its event (split -1: none)."""
    _fields_ = [("event", ctypes.c_int32), ("window_start", ctypes.c_int32), ("window_end", ctypes.c_int32),
                ("split", ctypes.c_int32)]


class HmmModel(ctypes.Structure):
    """ps_hmm_model: a baked HMM as host arrays (pypore_amd.hmm.Model.bake)."""
    _fields_ = [("n_states", ctypes.c_int32), ("n_emit", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("start", ctypes.c_int32), ("end", ctypes.c_int32), ("finite", ctypes.c_int32)] + \
               [(f, ctypes.c_void_p) for f in ("kind", "level_ptr", "in_ptr", "in_src", "out_ptr", "out_dst",
                                                "param", "in_lp", "out_lp", "kde_ptr", "kde_pt", "kde_lw")] + \
               [("n_dim", ctypes.c_int32)] + [(f, ctypes.c_void_p) for f in ("comp_kind", "comp_param", "comp_w")] + \
               [(f, ctypes.c_void_p) for f in ("mix_ptr", "mix_kind", "mix_param", "mix_lw", "mix_cdf", "mix_draw")]


class HmmSampleTables(ctypes.Structure):
    """ps_hmm_sample_tables: what ps_hmm_sample reads beside the model (pypore_amd.hmm.Model._sample_tables)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("out_cdf", "emit_param", "kde_cdf")] + \
               [(f, ctypes.c_int64) for f in ("n_cdf", "n_param", "n_kde")]


class PoolPlan(ctypes.Structure):
    """ps_pool_plan_t: what option "shared_device" n sets on a process with a given number of hardware queues."""
    _fields_ = [("n_eff", ctypes.c_int32), ("k0_waves", ctypes.c_int32), ("k0_admit", ctypes.c_int32), ("lat_help", ctypes.c_int32)]


class GridReport(ctypes.Structure):
    """ps_grid_report: what ps_grid_check_f64 found on a float64 current for one candidate grid."""
    _fields_ = [("max_frac", ctypes.c_double), ("min_frac_above", ctypes.c_double), ("min_count", ctypes.c_double),
                ("max_count", ctypes.c_double), ("n_nonfinite", ctypes.c_int64), ("n_undefined", ctypes.c_int64)]


vp, i32, i64, u64, dbl, cint, cstr, P = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_int,
                                         ctypes.c_char_p, ctypes.POINTER)
# The C ABI, declared once: every function of include/poreseg.h -> (restype, argtypes).  lib() applies the table when it loads
# the library; tests/test_host_logic.py compares every row with the header's prototype.
_ABI = {
    "ps_version": (cstr, []),
    "ps_device_count": (cint, []),
    "ps_create": (cint, [cint, vp, P(vp)]),
    "ps_destroy": (None, [vp]),
    "ps_live_bytes": (i64, []),
    "ps_last_error": (cstr, [vp]),
    "ps_set_tiling": (cint, [vp, i64, i64]),
    "ps_set_option": (cint, [vp, cstr, i64]),
    "ps_get_option": (cint, [vp, cstr, P(i64)]),
    "ps_pool_plan": (cint, [i32, i32, P(PoolPlan)]),
    "ps_hw_queues": (cint, []),
    "ps_gate_stats": (cint, [cint, P(i64), i32, cint]),
    "ps_synchronize": (cint, [vp]),
    "ps_min_gain": (cint, [P(SplitParams), P(dbl)]),
    "ps_segment_batch": (cint, [vp, vp, P(SampleFormat), P(i64), i32, P(SplitParams), vp, i64, P(i64), vp]),
    "ps_segment_batch_ex": (cint, [vp, vp, P(SampleFormat), P(i64), i32, P(SplitParams), vp, i64, P(i64), vp, vp]),
    "ps_segment_events": (cint, [vp, vp, P(SampleFormat), P(i64), P(i64), i32, P(SplitParams), vp, i64, P(i64), vp, vp]),
    "ps_segment_exact_f64": (cint, [vp, vp, P(i64), P(i64), i32, P(SplitParams), vp, i64, P(i64)]),
    "ps_statsplit_f64": (cint, [vp, vp, P(i64), P(i64), i32, P(i64), P(i64), P(StatSplitParams), vp, i64, P(i64)]),
    "ps_statsplit_prefix_f64": (cint, [vp, vp, i64, vp, vp, vp]),
    "ps_bounds_capacity": (i64, [P(i64), i32, i32]),
    "ps_best_single_split": (cint, [vp, vp, P(SampleFormat), i64, P(dbl), P(i32)]),
    "ps_score_window": (cint, [vp, vp, P(SampleFormat), i64, i32, dbl, vp, P(i32)]),
    "ps_audit_bounds": (cint, [vp, vp, P(SampleFormat), i64, P(SplitParams), P(i32), i32, P(dbl)]),
    "ps_detect_events": (cint, [vp, vp, P(SampleFormat), i64, dbl, i64, dbl, P(i64), P(i64), i64, P(i64)]),
    "ps_detect_segment_trace": (cint, [vp, vp, P(SampleFormat), i64, dbl, i64, dbl, P(SplitParams), P(i64), P(i64), i64, P(i64),
                                       vp, i64, P(i64), vp]),
    "ps_filter_bessel": (cint, [vp, vp, P(SampleFormat), i64, i32, dbl, dbl, vp]),
    "ps_requantise": (cint, [vp, vp, i64, vp, P(dbl), P(dbl)]),
    "ps_grid_check_f64": (cint, [vp, vp, i64, dbl, dbl, dbl, P(GridReport)]),
    "ps_grid_counts_f64": (cint, [vp, vp, i64, dbl, dbl, i64, vp]),
    "ps_narrow_f64": (cint, [vp, vp, i64, vp, P(i64)]),
    "ps_filter_bessel_batch": (cint, [vp, vp, P(SampleFormat), P(i64), P(i64), i32, i32, dbl, dbl, vp]),
    "ps_filter_requantise_batch": (cint, [vp, vp, P(SampleFormat), P(i64), P(i64), i32, i32, dbl, dbl, vp, vp, P(dbl), P(dbl)]),
    "ps_range_stats": (cint, [vp, vp, P(SampleFormat), i64, P(i64), P(i64), i64, vp]),
    "ps_align_batch": (cint, [vp, P(dbl), P(dbl), P(dbl), i32, dbl, dbl, vp, vp, vp, P(i64), i32, vp, vp, vp]),
    "ps_pairwise_scores": (cint, [vp, vp, P(i64), i32, vp, P(i64), i32, i32, dbl, vp, vp]),
    "ps_pairwise_batch": (cint, [vp, vp, P(i64), i32, vp, P(i64), i32, P(i32), P(i32), i32, i32, dbl, i32, vp, vp,
                                 P(i64), vp, vp, vp, P(i64), vp, vp, vp, vp]),
    "ps_trf_split_batch": (cint, [vp, vp, vp, P(i64), i32, dbl, dbl, i64, vp, vp, vp, vp, P(i64), vp, vp]),
    "ps_hmm_batch": (cint, [vp, P(HmmModel), i32, vp, P(i64), i32, vp, vp, vp, P(i64), vp]),
    "ps_hmm_expect": (cint, [vp, P(HmmModel), vp, P(i64), i32, vp, vp, vp, P(i32)]),
    "ps_hmm_posterior": (cint, [vp, P(HmmModel), vp, P(i64), i32, vp, vp, vp, vp, vp]),
    "ps_hmm_sample": (cint, [vp, P(HmmModel), P(HmmSampleTables), u64, i64, i32, i32, i32, vp, P(i64), vp, vp, vp, P(i64), vp]),
    "ps_get_timings": (cint, [vp, P(dbl), i32, P(i64), i32]),
    "ps_counters": (P(i64), [vp]),
    "ps_get_near_ties": (cint, [vp, P(NearTie), i32, P(i64)]),
    "ps_synth_trace": (cint, [vp, vp, i32, i64, u64, P(i64), P(i32), i64]),
    "ps_snakebase_f64": (cint, [vp, vp, P(i64), P(i64), i32, vp, i64, P(i64)]),
    "ps_filter_derivative_f64": (cint, [vp, vp, P(i64), P(i64), i32, P(FilterDerivativeParams), vp, i64, P(i64)]),
}
EXPORTS = list(_ABI)
# include/poreseg_pieces.h, the extension header beside poreseg.h (same library; declared by the same loop in lib())
_ABI_PIECES = {
    "ps_detect_pieces": (cint, [vp, vp, P(SampleFormat), i64, dbl, vp, vp, i64, P(i64)]),
}
PIECES_EXPORTS = list(_ABI_PIECES)

_lib = None


def lib():
    """Loads libporeseg.so and declares every function of _ABI and _ABI_PIECES; raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "pypore_amd: %s not found -- build it with `make -C pypore_amd/csrc` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): import it FIRST so the
    # process has exactly one HIP runtime, shared by torch's allocator and our kernels.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(_ABI.items()) + list(_ABI_PIECES.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def split_params(min_width=100, max_width=1000000, window_width=10000, min_gain_per_sample=None,
                 false_positive_rate=None, prior_segments_per_second=None, sampling_freq=1.e5,
                 cutoff_freq=None):
    """The eight FastStatSplit constructor arguments (cparsers.pyx:55-57) as a C struct;
    None and 0 both mean "not given", as in the reference (`if not x`)."""
    return SplitParams(int(min_width), int(max_width), int(window_width),
                       float(min_gain_per_sample or 0.0), float(false_positive_rate or 0.0),
                       float(prior_segments_per_second or 0.0), float(sampling_freq),
                       float(cutoff_freq or 0.0))


_ASSERT_MSG = {
    PS_ERR_ASSERT_WIDTH: "Maximum width must be greater than minimum width.",
    PS_ERR_ASSERT_WINDOW: "Window width must be greater than twice the minimum width.",
    PS_ERR_ASSERT_CUTOFF: "Cutoff freq must be less than half the sampling frequency.",
}


def check(rc, ctx=None):
    """Maps a status code to the exception the reference would raise (AssertionError for the
    three constructor assertions, ValueError for bad buffers) or RuntimeError."""
    if rc == PS_OK:
        return
    msg = ""
    if ctx is not None:
        m = lib().ps_last_error(ctx)
        msg = m.decode() if m else ""
    if rc in _ASSERT_MSG:
        raise AssertionError(_ASSERT_MSG[rc])
    if rc in (PS_ERR_ARG, PS_ERR_OFF_GRID):
        raise ValueError("poreseg: %s (status %d)" % (msg or "invalid argument", rc))
    if rc == PS_ERR_NO_DEVICE:
        raise RuntimeError("poreseg: no MI355X (gfx950) device available -- there is no CPU fallback")
    raise RuntimeError("poreseg: %s (status %d)" % (msg or "error", rc))


def min_gain(**kw):
    out = ctypes.c_double()
    p = split_params(**kw)
    check(lib().ps_min_gain(ctypes.byref(p), ctypes.byref(out)))
    return out.value


def pool_plan(n_contexts, hw_queues=0):
    """ps_pool_plan (no GPU): the options "shared_device" n_contexts sets with hw_queues hardware queues (0: HIP's default of 4),
    as a dict with n_eff = min(n_contexts, hw_queues)."""
    p = PoolPlan()
    check(lib().ps_pool_plan(int(n_contexts), int(hw_queues), ctypes.byref(p)))
    return {f: int(getattr(p, f)) for f, _ in PoolPlan._fields_}


def hw_queues():
    """ps_hw_queues (no GPU): the hardware queues of this process as the library read them from GPU_MAX_HW_QUEUES."""
    return int(lib().ps_hw_queues())


def gate_stats(device=0, reset=False):
    """ps_gate_stats (host bookkeeping of the K0 gate): tickets, open now, most open at a time, host waits, waits given up."""
    out = (ctypes.c_int64 * 5)()
    check(lib().ps_gate_stats(int(device), out, 5, 1 if reset else 0))
    return dict(zip(("tickets", "open", "open_max", "host_waits", "gave_up"), (int(v) for v in out)))
