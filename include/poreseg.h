/*
 * poreseg.h -- C ABI of libporeseg.so, the MI355X (gfx950) implementation of PyPore's
 * SpeedyStatSplit / FastStatSplit change-point segmenter.
 *
 * Every entry point below replaces one piece of the reference interface (file:line under
 * the reference tree, PyPore/...).  The reference has no FFI of its own (the hot path is a
 * Cython cdef class called from Python); the binding a maintainer would add is a ctypes
 * stub, shown in INTEGRATION.md, which is exactly what pypore_amd/_lib.py does.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns a status
 * (PS_OK == 0, negative on error); ps_last_error() returns a human-readable message for the
 * most recent failure on that context.  Pointers prefixed d_ are DEVICE pointers (HBM of the
 * context's GPU), h_ are host pointers.  Outputs are caller-allocated with an explicit
 * capacity; when a capacity is too small the call fails with PS_ERR_CAPACITY and reports
 * the required size through the corresponding out-parameter.  A context is bound to one
 * GPU and one HIP stream and may be used by one host thread at a time.
 *
 * Sample model.  The reference consumes float64 current in pA (cparsers.pyx:53,103).  Real
 * traces are int16 ADC counts times a scale (read_abf.py:202-210), so the device consumes
 * either fp32 pA values that lie on an ADC grid (x = k * quantum, k integer, |k| < 2^23) or
 * the raw int16 counts; prefix sums are then exact integers and window variances are
 * evaluated in fp64 with the reference's operation order.  Off-grid fp32 input is rejected
 * with PS_ERR_OFF_GRID (never silently rounded).
 */
#ifndef PORESEG_H
#define PORESEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_OK                 0
#define PS_ERR_ARG           -1   /* invalid argument (null pointer, negative size ...) */
#define PS_ERR_ASSERT_WIDTH  -2   /* reference assertion max_width >= min_width        (cparsers.pyx:69) */
#define PS_ERR_ASSERT_WINDOW -3   /* reference assertion window_width >= 2*min_width   (cparsers.pyx:71) */
#define PS_ERR_ASSERT_CUTOFF -4   /* reference assertion cutoff_freq <= sampling_freq/2 (cparsers.pyx:74) */
#define PS_ERR_CAPACITY      -5   /* caller buffer too small; required size reported */
#define PS_ERR_OFF_GRID      -6   /* fp32 sample is not an integer multiple of quantum */
#define PS_ERR_HIP           -7   /* HIP runtime error (message in ps_last_error) */
#define PS_ERR_NO_DEVICE     -8   /* no gfx950 device / code object missing */
#define PS_ERR_INTERNAL      -9   /* device-side stack or scratch overflow */

#define PS_DTYPE_F32 0            /* float pA on the grid k*quantum */
#define PS_DTYPE_I16 1            /* raw int16 ADC counts (read_abf.py:208) */
#define PS_DTYPE_F64 2   /* float64 pA on no grid: accepted by ps_filter_bessel ONLY (the current of an event that was
                            filtered before, DataTypes.py:258-274); quantum and offset_counts are ignored */

typedef struct ps_ctx ps_ctx;

/* The eight constructor arguments of FastStatSplit / SpeedyStatSplit
 * (cparsers.pyx:55-57, parsers.py:511-513).  "Not given" (Python None) is encoded as 0,
 * which the reference also treats as not given (`if not false_positive_rate`). */
typedef struct ps_split_params {
    int32_t min_width;                   /* default 100      */
    int32_t max_width;                   /* default 1000000  */
    int32_t window_width;                /* default 10000    */
    double  min_gain_per_sample;         /* 0 = None         */
    double  false_positive_rate;         /* 0 = None         */
    double  prior_segments_per_second;   /* 0 = None         */
    double  sampling_freq;               /* default 1e5      */
    double  cutoff_freq;                 /* 0 = None         */
} ps_split_params;

/* How samples map to pA: pA = (count + offset_counts) * quantum for PS_DTYPE_I16; PS_DTYPE_F32 samples are the pA
 * values themselves, count = x/quantum, and offset_counts is NOT added to them: non-zero, it names the level (in counts
 * of quantum) that the caller subtracted upstream -- ps_requantise's centre, for a filtered event -- and is used only to
 * judge near ties against the reference's own rounding noise (its cumsums run on the uncentred values; counters[11] of
 * ps_get_timings).  quantum should be a power of two for bit-exact parity with the reference (read_abf.py:202-205
 * scale/offset). */
typedef struct ps_sample_format {
    int32_t dtype;                       /* PS_DTYPE_* */
    int32_t offset_counts;
    double  quantum;
} ps_sample_format;

/* Per-segment statistics: Segment.mean/std/min/max (core.py:209-223), std = population. */
typedef struct ps_segstat {
    double mean, std, min, max;
} ps_segstat;

/* Library / device ------------------------------------------------------------------------ */
const char *ps_version(void);
/* Number of visible gfx950 GPUs (0 if none; never fails). */
int ps_device_count(void);
/* Creates a context on GPU `device`; stream = an existing hipStream_t to launch on, or NULL
 * to let the context create its own. */
int ps_create(int device, void *stream, ps_ctx **out);
/* Waits for the context's stream, then frees every buffer, event and stream the context made (never a caller's stream). */
void ps_destroy(ps_ctx *ctx);
/* Diagnostic: bytes of device memory plus pinned host memory that the contexts of this process hold right now (the library's
 * own bookkeeping, not the device's free memory).  Back at its earlier value once the contexts made since are destroyed. */
int64_t ps_live_bytes(void);
const char *ps_last_error(const ps_ctx *ctx);
/* Tiling of long traces: a trace longer than tile_len + halo samples is cut into tiles whose
 * spines are computed speculatively and stitched.  0 keeps the default. */
int ps_set_tiling(ps_ctx *ctx, int64_t tile_len, int64_t halo);
/* Diagnostic / tuning options (none changes a result): "mode" 0 screen+exact (default), 1 exact fp64
 * scans only, 2 verify (screen and exact must agree); "scan_bs" 1 (default) block-sum scan with
 * single-wave workgroups behind the block-prefix kernel, 0 LDS-window scan; "prune" 0 switches the
 * block pruning of the LDS-window scan off; "stitch_host" 1 forces the host-stitch pipeline (halo
 * tiles + seam repairs, otherwise only the fallback); "timing" 0/1/2 (see ps_get_timings); "upload_by_kernel" 1
 * (default) the call's host tables are fetched by a kernel reading the pinned blob, 0 hipMemcpyAsync; "filter_fused" 1
 * (default) fast filters run both directions in one kernel over tiles with halos, 0 always the exact three-pass
 * scan; "tree_mw" 0 (default) subtree jobs of the block-sum scan run on single-wave workgroups, one per wave slot,
 * striding over the job list, 1 two-wave workgroups whose waves share the workgroup's job list through an LDS counter
 * (round 2's default; slower at four waves per SIMD); "groups" 1 (default) K0 writes one record per 256 samples and
 * every window scan starts with the coarse pass over them (whole groups of 32 blocks are bounded, rows of the sweep
 * that lie in pruned groups are skipped), 0 every row is swept; "wide_bs" 1 (default) counts too wide for the 32-bit
 * digest are retried on the 64-bit one, 0 straight to the LDS-window scan; "spine_nt" 256/512/1024, "tree_nt" 256/512
 * workgroup sizes of the LDS-window kernels; "tree_par" 1 (default) the deep subtree jobs of a call on the 64-bit digest
 * (a filtered event) are shared by the four waves of a workgroup when the call has few jobs, 0 one wave per job;
 * "k0_waves" n > 0: the block-prefix kernel K0 is persistent -- n waves per SIMD (twice that for int16 samples) stride
 * over the call, each with its next wave block's samples in flight: what a context that shares the chip with other calls
 * wants (engine.StreamPool sets 1) --, 0 (default): one wave per 2 048 samples, as many as fit the chip: faster for a
 * call that has the chip to itself;
 * "k0_shared" 1: this context queues its upload + K0 launches on the device's shared front stream, where the K0
 * kernels of all such contexts run back to back (they are bound by HBM: side by side they only share it) and the
 * context's own stream takes over behind an event; 0 (default) everything on the context's stream -- a host that keeps
 * several contexts busy (engine.StreamPool) sets it for the duration of its runs (measured slower: nothing sets it);
 * "k0_admit" M > 0: at most M calls of this device have their K0 in flight at a time -- enforced on the device (round 6): a
 * call queues a wait for the K0 of the call M tickets before it in front of its own K0 (hipStreamWaitEvent); the host thread
 * never waits for the device, only -- for the length of a kernel launch -- for the thread that holds that ticket and has
 * not queued its K0 yet (ps_gate_stats) --, 0 (default) no limit; "shared_device" sets what ps_pool_plan says;
 * "bridge_ext" 1 (default): seams whose bridge ran out of anchors (256 without meeting a downstream tile's chain:
 * densely stepped data) and open tiles entered exactly at their start are continued on the device -- up to four rounds,
 * 16 384 more anchors per seam -- before the call falls back to the host stitch, 0 straight to the host stitch;
 * "lat_help" 1 (default): in the look-ahead kernel, workgroups that are through with their own seams scan chunks of 16
 * windows ahead of the seams that walk long stretches without splits and publish what they find; the seam's owner takes a
 * published chunk instead of scanning it (2 x on traces with stretches of 1e6 samples and more), 0 every seam walks alone,
 * 2 as 1 but the helpers stay until every workgroup of the launch is through with its own seams (never leave on idle polls:
 * for tests that must see them work -- counters[12], [13] of ps_get_timings; only for a call that has the chip to itself);
 * "bridge_budget" 1..256 (default 256): anchors a bridge may add before it gives up (tests lower it to reach the second
 * chance on small inputs);
 * "shared_device" n: ONE call for a host that keeps n contexts busy on one device (a pool of host threads, one context
 * each).  HIP maps the streams of a process onto its hardware queues, and streams that share a queue run their kernels one
 * after the other: of n contexts on Q queues, n_eff = min(n, Q) calls execute at a time, and a call is configured for
 * that many -- it sets k0_waves, k0_admit and lat_help to exactly what ps_pool_plan(n, Q) returns (the table is there and in
 * INTEGRATION.md); "k0_waves" / "k0_admit" / "lat_help" set afterwards still win.  Everything that asks whether the call is
 * one of a pool ("short_chain") goes by n itself, whatever Q is.  n <= 1 restores the defaults of a lone context (k0_waves 0,
 * lat_help 1, k0_admit 0);
 * "hw_queues" Q (1 .. 32; 0, the default: the process's own): the hardware queues the next "shared_device" plans for.  The
 * process's own number is GPU_MAX_HW_QUEUES as the HIP runtime reads it -- read once, unset or not a number: HIP's default
 * of 4; the library never sets the variable.  For tests and tools;
 * "single_pass" 1 (default): ps_detect_segment_trace streams a file trace once (see there), 0: it makes the two calls;
 * "gather_fused" 1 (default): the gather places its items from per-256-job count sums (no scan kernel in front of it), 0: rounds
 * 2-5's item scan + gather; "download_by_kernel" 1 (default): the status block returns by a kernel writing pinned memory;
 * "k0_unaligned" 0: K0's fast route only from 16-byte-aligned addresses (1: whatever the probe at ps_create said);
 * "debug" 1: the library reports on stderr which occupancy it found, the resident slots every launch sized by them gets, and
 * which seams gave up (prints only);
 * "slots_pct" 1..100 (default 100) share of the resident wave slots the kernels of up to 256 threads that are sized by them
 * (the scan kernels, the aligner, the pairwise aligner, the repeat splitter, the HMM E-step) are launched on, from the next launch on;
 * "pairwise_budget" bytes of score / pointer scratch per launch of ps_pairwise_batch (default 2 GiB);
 * "trf_budget" bytes of mask / pointer scratch per launch of ps_trf_split_batch (default 2 GiB);
 * "tree_jobs_per_wave" (default 4) subtree kernel: jobs / this many of its slots work, between half and all of them;
 * "tree_screen" 1 (default): on the 32-bit digest a lean kernel walks the subtree jobs first, proves the windows that hold no
 * split empty and leaves the subtree kernel the jobs it cannot decide (counters[14], [15] of ps_get_timings), 0: the subtree
 * kernel takes every job, launch for launch as before; same results either way;
 * "short_chain" 1 (default): a call on that route -- the 32-bit digest in the default mode with "tree_screen" 1 -- leaves out
 * the launches it can do without.  (a) A context that shares its device ("shared_device" n > 1) issues no look-ahead launch:
 * its seam bridges walk 16 windows without a hit ("bridge_patience", 1 .. 4096: tests) in their own wave instead of 3.  If
 * seams still run out of patience -- any number of them -- the look-ahead kernel runs behind the stitch and finishes them where
 * they stopped, and the stitch and what follows it run again: one more round trip for that call, no host stitch.  The next 16
 * calls of the context then launch the look-ahead kernel in the chain, patience 3, exactly as with the option off (data with
 * stretches of more than 8 window widths without a split: 237 of 1 536 seams at dwells of 8 .. 16 widths), before the option is
 * tried again.  A lone context keeps patience 3 and the look-ahead kernel with its helpers.  (b) The download kernel of a call without statistics leaves the status block zero
 * behind its copy, and the next call launches no upload kernel when it repeats the event layout and nothing else has used
 * the context in between.  0: the launches of the library before the option, launch for launch; 2 / 3: (a) / (b) alone, for
 * measurements.  Same results either way; counters[16] .. [18] of ps_get_timings say what a call did without;
 * "noise_k_ppm" (default 100 000 = 0.1): near-tie accounting of the 64-bit digest, margin factor in millionths;
 * "near_tie_log" n (default 65 536, 0 .. 2^30): records of the near-tie log that ps_get_near_ties reads (16 bytes each, device
 * memory allocated with the first segment call that logs), 0 = no log.
 * Unknown names return PS_ERR_ARG.
 * THE LIBRARY READS NO ENVIRONMENT VARIABLE OF ITS OWN (round 6): what a call returns depends on its arguments and on these
 * two setters only.  (GPU_MAX_HW_QUEUES, the runtime's variable, is read for "shared_device": it changes how a call is
 * scheduled, never what it returns.)  The experiments' switches that return stale or partial results ("dbg_phase", "dbg_k0_nogrp",
 * "scan_lds_pad", "rep_*") and the PORESEG_* variables exist in libporeseg_diag.so only (make -C pypore_amd/csrc diag;
 * ps_version() of that build says DIAGNOSTIC BUILD). */
int ps_set_option(ps_ctx *ctx, const char *name, int64_t value);
/* The current value of any option ps_set_option knows, as it was stored: the default, what was last set (a switch as 0 / 1,
 * "timing" clamped), for "k0_waves", "k0_admit" and "lat_help" what "shared_device" planned since; "k0_unaligned" answers what the
 * probe granted.  PS_ERR_ARG for an unknown name. */
int ps_get_option(const ps_ctx *ctx, const char *name, int64_t *value);

/* What option "shared_device" n sets on a process with hw_queues hardware queues: a pure function of min(n, hw_queues) -- no
 * context, no GPU.  n_eff = min(n_contexts, hw_queues) calls execute at a time (hw_queues <= 0: HIP's default of 4; more than
 * 32 counts as 32).
 *     n_eff      k0_waves  k0_admit  lat_help
 *     0, 1       0         0         1          a lone call: one-shot K0 on every slot it can get, no gate, helpers on
 *     2          0         0         0          measured: sixteen contexts on 2 queues
 *     3 .. 5     4         0         0          measured: sixteen contexts on 4 queues (HIP's default; 8 % under the row below)
 *     6 .. 11    1         0         0          measured: sixteen contexts on 8 queues
 *     12 .. 15   1         3         0          not measured: as the nearest measured point, the row below
 *     >= 16      1         3         0          measured with sixteen calls in flight (round 5, and again on 16 queues)
 * (tools/pool_plan_sweep.py, profiles/pool_queues_ab.json; DESIGN.md section 6 has the numbers and the rule that chose the rows.)
 * Down the table a call never gets a larger share of the chip: the K0 waves per SIMD (0 = every slot) and the K0s admitted
 * at a time (0 = all) do not grow, the helpers do not come back.  PS_ERR_ARG for a null pointer or a negative count. */
typedef struct ps_pool_plan_t {
    int32_t n_eff;                       /* calls that execute at a time: min(n_contexts, hw_queues) */
    int32_t k0_waves;                    /* option "k0_waves" */
    int32_t k0_admit;                    /* option "k0_admit" */
    int32_t lat_help;                    /* option "lat_help" */
} ps_pool_plan_t;
int ps_pool_plan(int32_t n_contexts, int32_t hw_queues, ps_pool_plan_t *out);
/* The hardware queues of this process as "shared_device" sees them: GPU_MAX_HW_QUEUES read once (unset or not a number: 4;
 * clamped to 1 .. 32).  No GPU needed. */
int ps_hw_queues(void);
/* The K0 gate of `device` ("k0_admit"), for tests: out[0] tickets taken so far, [1] calls that have gone through the gate with
 * their ticket and have not yet queued the event behind their K0 (or given the ticket up), right now, [2] the most there
 * have been of them at a time, [3] times a host thread waited for such a call before it queued its own wait, [4] times it
 * gave that up (200 ms) and went on without a wait.  [2] never exceeds the largest "k0_admit" in use while [4] is zero:
 * that is what keeps M K0s in flight and no more.  reset != 0 sets [2] back to [1] and [3], [4] to zero behind the read.
 * Host bookkeeping only: no GPU call.  device 0 .. 15. */
int ps_gate_stats(int device, int64_t *out, int32_t n_out, int reset);

/* Blocks until all work submitted on the context's stream has finished. */
int ps_synchronize(ps_ctx *ctx);

/* Replaces FastStatSplit.__init__ (cparsers.pyx:55-101): validates the widths with the
 * reference's three assertions and computes the public attribute `min_gain`. Host only. */
int ps_min_gain(const ps_split_params *p, double *min_gain_out);

/* Replaces FastStatSplit.parse (cparsers.pyx:103-118 -> _recursive_split :180-203 ->
 * _best_split_stepwise :157-178 -> var_c :31-38) for a batch of independent events
 * (one reference parse() call per event; Event.parse, DataTypes.py:286).
 *   d_samples  all events' samples, one contiguous device array
 *   h_ev_off   n_ev+1 host offsets into d_samples (event e = [h_ev_off[e], h_ev_off[e+1]))
 *   d_bounds   device out, capacity `cap` int32: breakpoints of event 0, then event 1, ...
 *              (event-local sample indices, ascending, excluding 0 and the event length --
 *              the list _recursive_split returns)
 *   h_bounds_off  host out, n_ev+1 offsets into d_bounds
 *   d_stats    nullable device out, capacity `cap + n_ev` entries: statistics of the
 *              segments of event 0, then event 1, ... (segment s of event e lives at
 *              h_bounds_off[e] + e + s)
 * Returns PS_ERR_CAPACITY if cap < total (h_bounds_off[n_ev] then holds the required size). */
int ps_segment_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                     const int64_t *h_ev_off, int32_t n_ev,
                     const ps_split_params *params,
                     int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off,
                     ps_segstat *d_stats);

/* ps_segment_batch plus one more output: d_is_spine (nullable device out, capacity `cap` bytes) is 1
 * for breakpoints found by the top-level chain of right recursions rec(a, len) ("spine anchors"),
 * 0 for breakpoints of left subtrees.  Two runs over overlapping pieces of one trace are identical
 * after any common spine anchor; pypore_amd/dist.py uses that to stitch a trace sharded across
 * GPUs (BASELINE config 5).  No reference counterpart. */
int ps_segment_batch_ex(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                        const int64_t *h_ev_off, int32_t n_ev,
                        const ps_split_params *params,
                        int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off,
                        ps_segstat *d_stats, uint8_t *d_is_spine);

/* Same as ps_segment_batch_ex for events that do NOT tile the sample array: event e is
 * [h_ev_start[e], h_ev_start[e] + h_ev_len[e]) of d_samples (the events lambda_event_parser cuts out
 * of a file trace, parsers.py:142-155 -> Event.parse, DataTypes.py:978-984, without copying them). */
int ps_segment_events(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                      const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                      const ps_split_params *params,
                      int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off,
                      ps_segstat *d_stats, uint8_t *d_is_spine);

/* The EXACT route for float64 input that lies on no ADC grid (round 6).  The reference takes any double[:] (cparsers.pyx:53)
 * and its decisions on such data depend on the rounding of its own prefix sums, c = np.cumsum(current) and c2 =
 * np.cumsum(np.multiply(current, current)) (cparsers.pyx:110-111): strictly sequential fp64 additions.  This entry forms
 * exactly those -- one chain per event, the events in parallel -- and scans every window of the recursion
 * (cparsers.pyx:157-203) with the reference's own expressions on them (var_c, :31-38; gain = var_summed - (low + high);
 * strict '>', first maximum): the same boundaries as the reference on the same input BY CONSTRUCTION, up to the logarithm's
 * last bit (counters[11] counts nothing here; a tie within 1e-12 of a gain is as undecided as everywhere else).
 *   d_current   float64 pA, device; event e = [h_ev_start[e], h_ev_start[e] + h_ev_len[e])
 *   d_bounds / cap / h_bounds_off   as ps_segment_batch; no statistics (the caller has the float64 values)
 * Cost: ~10-20 ns per sample and event for the chains (events run side by side), then one 512-thread workgroup per window
 * with two fp64 logarithms per candidate: a 1e6-sample event takes tens of milliseconds where the re-quantised route
 * (ps_requantise + ps_segment_batch) takes one.  Meant for the events that route flags (near ties) and for callers who
 * want the reference's own arithmetic; pypore_amd: SpeedyStatSplit(off_grid="exact" / "exact_on_near_tie"). */
int ps_segment_exact_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len,
                         int32_t n_ev, const ps_split_params *params, int32_t *d_bounds, int64_t cap,
                         int64_t *h_bounds_off);

/* StatSplit (parsers.py:220-503), the reference's older pure-Python segmenter, on the device: gains on the variance
 * (use_log 0) or its logarithm, each side of a split modelled as a level ("stepwise") or as a straight line plus noise
 * ("slanted"); windows of window_width samples advancing by window_width / 2, scanned when they hold at least 2 * min_width
 * samples (a window of exactly 2 * min_width has one candidate; cparsers.pyx:164 refuses it), threshold = min_gain_per_sample
 * * window_width (formed by the caller, as Python forms it), forced splits every max_width samples. */
#define PS_STATSPLIT_STEPWISE 0
#define PS_STATSPLIT_SLANTED  1
typedef struct ps_statsplit_params {
    int32_t min_width;                   /* >= 1                                     */
    int32_t max_width;                   /* >= min_width   (PS_ERR_ASSERT_WIDTH)     */
    int32_t window_width;                /* >= 2 min_width (PS_ERR_ASSERT_WINDOW)    */
    double  threshold;                   /* a gain must exceed it (strict)           */
    int32_t use_log;                     /* 0 / 1                                    */
    int32_t splitter;                    /* PS_STATSPLIT_*                           */
} ps_statsplit_params;

/* Segments events of a float64 current as StatSplit.parse does.  The prefix sums c = cumsum(x), c2 = cumsum(x * x) and, for
 * the slanted splitter, ct = cumsum(x * t) (t = 0, 1, ... from the event's first sample) are numpy's sequential chains, one
 * wave per event; one workgroup per event then walks _segment_cumulative with the reference's expressions, operation for
 * operation in fp64 without contraction: the reference's boundaries by construction, up to the logarithm's last bit when
 * use_log is set.
 *   d_current   float64 pA, device; event e = [h_ev_start[e], h_ev_start[e] + h_ev_len[e]), at most 2^30 samples each
 *   h_lo, h_hi  (each may be NULL: 0 / the event's length) the range [h_lo[e], h_hi[e]) of event e that is segmented, in
 *               samples from its start, 0 <= lo, hi <= length; the prefix sums always run from the event's first sample
 *   d_bounds / cap / h_bounds_off   as ps_segment_exact_f64: positions from the event's start, ascending per event;
 *               PS_ERR_CAPACITY with the required size in h_bounds_off[n_ev] when cap is too small
 * PS_ERR_INTERNAL: the interval stack or a boundary slot was too small (both are sized from the model, seg_statsplit.hpp).
 * Cost: the chains run at ~10-20 ns per sample and event, events side by side; one event is one workgroup, so a lone long
 * trace uses one compute unit. */
int ps_statsplit_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                     const int64_t *h_lo, const int64_t *h_hi, const ps_statsplit_params *params, int32_t *d_bounds,
                     int64_t cap, int64_t *h_bounds_off);

/* Diagnostics: the prefix sums ps_statsplit_f64 forms of ONE event, d_current[0 .. n): d_c, d_c2 and (when not NULL) d_ct,
 * n doubles each, device -- bit for bit np.cumsum(x), np.cumsum(x * x), np.cumsum(x * arange(n)). */
int ps_statsplit_prefix_f64(ps_ctx *ctx, const double *d_current, int64_t n, double *d_c, double *d_c2, double *d_ct);

/* Upper bound on the number of breakpoints ps_segment_batch can emit for these events
 * (sum over events of len/min_width): a safe `cap`. */
int64_t ps_bounds_capacity(const int64_t *h_ev_off, int32_t n_ev, int32_t min_width);

/* Replaces FastStatSplit.best_single_split (cparsers.pyx:120-155): one scan of the whole
 * array, start=0, end=n-1, candidates range(2, end-2), threshold 0.  Returns (gain, index)
 * or (0.0, -1). */
int ps_best_single_split(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                         int64_t n, double *gain_out, int32_t *index_out);

/* Replaces FastStatSplit.score_samples(current, no_split=True) (cparsers.pyx:205-249):
 * per-candidate gains of ONE window spanning the whole array; d_scores[n] (device) gets the
 * gain at every candidate index and 0 elsewhere; *split_out the chosen split or -1. */
int ps_score_window(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                    int64_t n, int32_t min_width, double min_gain,
                    double *d_scores, int32_t *split_out);

/* Diagnostic (tests only; no reference counterpart): audits the pruning bounds of the block-sum window scan ON THE
 * DEVICE, with the scan code of the product.  The trace [0, n) is taken as one event (K0 digest), every window
 * [h_windows[2i], h_windows[2i+1]) is scanned with all rows swept, and each bound the scan forms is compared with the
 * screened gains of the candidates it covers, evaluated one by one from the raw samples:
 *   out[0] blocks with a corner bound        out[1] of which violated      out[6] smallest margin (bound - largest gain)
 *   out[2] blocks with a two-boundary bound  out[3] of which violated      out[7] smallest margin
 *   out[4] groups (256 samples) with a bound out[5] of which violated      out[8] smallest margin
 *   out[9] windows with a coarse pass
 * A violation is a covered gain above the bound by more than 2 delta(n), the slack every pruning level carries
 * (DESIGN.md 4.3, 4.4).  Needs min_width >= 8 and counts inside the 32-bit digest (PS_ERR_ARG otherwise). */
int ps_audit_bounds(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                    const ps_split_params *params, const int32_t *h_windows, int32_t n_win, double *out12);

/* Replaces lambda_event_parser(threshold).parse with the default rules (parsers.py:124-155, rules
 * :133-135): events are the maximal runs of samples on one side of `threshold` (mask = x < threshold,
 * cut at every mask edge) that satisfy  length > min_duration,  min > min_current,  max < threshold.
 * Reference defaults: threshold 90, min_duration 100000, min_current -0.5.  Writes the kept events'
 * (start, length) in samples, ascending, to the host arrays; *n_events_out is the number found
 * (PS_ERR_CAPACITY if it exceeds cap).  One streaming pass over the trace (edge positions + per-chunk
 * min/max), then one workgroup per long piece. */
int ps_detect_events(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                     double threshold, int64_t min_duration, double min_current,
                     int64_t *h_starts, int64_t *h_lengths, int64_t cap, int64_t *n_events_out);

/* File.parse + Event.parse for every event of a whole file trace in ONE call and ONE pass over its samples (round 6):
 * ps_detect_events followed by ps_segment_events on the events it found, with the same results -- events (h_starts,
 * h_lengths, *n_events_out as ps_detect_events), boundaries (d_bounds / cap / h_bounds_off[n_events + 1] as ps_segment_events;
 * h_bounds_off must have room for ev_cap + 1 entries), optional statistics.  The block-sum kernel K0 runs once over the whole
 * trace (blocks aligned to the trace) and judges every 8-sample block against the threshold on its way (2 bits per block: all
 * below, all at or above, mixed; min / max per 1 024 samples); the detector reads those bits -- 1/64 of the samples' bytes --
 * and the samples of the mixed blocks only; the events -- which start at any sample -- are segmented from the same digest in
 * coordinates shifted by (start mod 8).  Replaces the loop `for event in file.parse(lambda_event_parser(threshold)): event.parse(SpeedyStatSplit(...))`
 * (parsers.py:124-155, DataTypes.py:589-602, 978-984).  Takes the two calls by itself when the block-sum scan does not apply
 * (min_width < 8, window_width > 64 512, options "scan_bs" 0 / "mode" 1 / "stitch_host" 1 / "single_pass" 0) or when a count of
 * the trace lies 2^14 or more from its first one (ps_get_timings counters[7] = 3 then). */
int ps_detect_segment_trace(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                            double threshold, int64_t min_duration, double min_current,
                            const ps_split_params *params,
                            int64_t *h_starts, int64_t *h_lengths, int64_t ev_cap, int64_t *n_events_out,
                            int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats);

/* Replaces Event.filter (DataTypes.py:258-274): scipy.signal.bessel(order, cutoff / (sampling_freq / 2), btype='low',
 * analog=0) applied with scipy.signal.filtfilt (forward and backward, odd extension by padlen = 3 (order + 1), initial
 * state lfilter_zi * first value).  order 1 (the reference's default): the scan / fused-halo kernels; orders 2..8: one
 * thread per segment with a halo (seg_filter.hpp).  Input as for the segmenter (fp32 on the grid or int16 counts,
 * n samples) or -- this entry only -- PS_DTYPE_F64, the float64 current itself; output d_out[n] in pA as fp64 (the
 * reference replaces Event.current by the float64 result).
 * PS_ERR_ARG for order outside 1..8, n <= padlen (scipy raises ValueError), a cutoff outside (0, Nyquist), and for a
 * filter of order >= 2 whose state needs more than 8192 samples to forget (cutoffs below ~0.2 % of Nyquist). */
int ps_filter_bessel(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, int32_t order,
                     double cutoff, double sampling_freq, double *d_out);

/* The representation step between ps_filter_bessel and ps_segment_batch for a filtered event (no reference counterpart:
 * the reference segments the float64 result of Event.filter directly, DataTypes.py:286; this library works on exact
 * integer sums).  d_in[n]: a filtered current in pA (fp64, device).  Writes d_out[n] (fp32, device): the current minus
 * *centre_out, rounded to multiples of *step_out -- centre = the mean rounded to the grid, step = the finest power of two
 * that keeps every count below 2^22 (what DataTypes.Event.parse does on the host for a single event).  Segment d_out with
 * quantum = *step_out; the gains are shift invariant, so the boundaries are those of the rounded current.  Synchronises
 * the context's stream twice: for the statistics (they come back to the host) and before returning (d_out is complete
 * and d_in no longer read when the call returns). */
int ps_requantise(ps_ctx *ctx, const double *d_in, int64_t n, float *d_out, double *centre_out, double *step_out);

/* A float64 current that is already on the device finds its way back to the int16 ADC counts it came from (the reference
 * takes any double[:], PyPore/parsers.py:524-528, cparsers.pyx:53,103; an .abf reader returns counts * scale + offset with a
 * scale that is almost never a power of two).  The three calls below are the full-array passes of that recovery; the caller
 * proposes the grid (pypore_amd.grid.affine_grid_device: the spacing from a small subset on the host, up to four refinements)
 * and takes every decision from the numbers that come back.  d_in[n]: fp64, device, 8-byte aligned, n >= 1.  Per sample the
 * kernels compute k = (x - origin) / quantum and kr = rint(k) with the IEEE operations numpy performs (no contraction, no
 * reciprocal, round half to even); every reduced quantity is a minimum, a maximum or an integer count, so the report does
 * not depend on the launch shape.  Each call runs on the context's stream and synchronises it before returning. */
typedef struct ps_grid_report {
    double  max_frac;         /* max |k - kr| over the samples for which it is defined (0 if there is none)         */
    double  min_frac_above;   /* the smallest |k - kr| that is > tol; INFINITY when there is none                    */
    double  min_count;        /* min kr                                                                              */
    double  max_count;        /* max kr                                                                              */
    int64_t n_nonfinite;      /* samples that are NaN or infinite                                                    */
    int64_t n_undefined;      /* samples whose |k - kr| is NaN (numpy's maximum would be NaN: the check has failed)  */
} ps_grid_report;
int ps_grid_check_f64(ps_ctx *ctx, const double *d_in, int64_t n, double origin, double quantum, double tol,
                      ps_grid_report *out);
/* d_out[i] = int16(kr - centre) (device, 2-byte aligned).  Only after a check that passed and whose re-centred range
 * [min_count - centre, max_count - centre] lies inside int16: the conversion of anything else is not defined. */
int ps_grid_counts_f64(ps_ctx *ctx, const double *d_in, int64_t n, double origin, double quantum, int64_t centre,
                       int16_t *d_out);
/* d_out[i] = float(d_in[i]) (device, 4-byte aligned; round to nearest even, numpy's astype) and *n_inexact_out = the number
 * of samples with double(float(x)) != x -- a NaN counts.  0: the float32 copy is the current, exactly. */
int ps_narrow_f64(ps_ctx *ctx, const double *d_in, int64_t n, float *d_out, int64_t *n_inexact_out);

/* Event.filter for MANY events of one device buffer in one call: event e is samples[ev_start[e] .. + ev_len[e]) of d_samples
 * (fmt as for ps_filter_bessel, PS_DTYPE_F64 included); events may overlap, touch and come in any order.  Its filtered current
 * goes to d_out + sum of the lengths before it (device, float64, room for the sum of all lengths), bit for bit what
 * ps_filter_bessel writes for that event alone.  Order 1 on the fused route (poles up to ~0.96) is ONE launch, one workgroup per
 * (event, tile); orders 2..8 take one launch per group of events whose scratch rows fit the context option
 * "filt_batch_scratch" (bytes, default 256 MiB; an event that alone exceeds it is a group of its own); slower order-1 filters
 * (the three-pass scan) have no batched kernel and are queued per event.  One status word and one host synchronisation for the
 * batch.  n_ev == 0 returns PS_OK.  Argument errors are ps_filter_bessel's; an event with a negative start or no samples, the
 * first event of at most padlen samples (both named in ps_last_error) and a batch of more than 2^24 - 1 tiles are refused too --
 * all before anything is queued. */
int ps_filter_bessel_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const int64_t *ev_start,
                           const int64_t *ev_len, int32_t n_ev, int32_t order, double cutoff, double sampling_freq, double *d_out);

/* Event.filter + the representation step for MANY events of one trace in one call (the inner loop of Experiment.parse,
 * DataTypes.py:975-984; File.parse_events here): event e is samples[ev_start[e] .. + ev_len[e]) of d_samples; its filtered
 * current (ps_filter_bessel) goes to d_filtered + sum of the lengths before it, its re-quantised copy (ps_requantise) to the
 * same position of d_rounded, its centre and grid step to h_centre[e] / h_step[e].  Same results as the two entries called
 * per event; one status check and two host synchronisations for the whole batch instead of three per event, and -- on the
 * filter routes ps_filter_bessel_batch has a kernel for -- three launches for the batch: filter, statistics, rounding. */
int ps_filter_requantise_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const int64_t *ev_start,
                               const int64_t *ev_len, int32_t n_ev, int32_t order, double cutoff, double sampling_freq,
                               double *d_filtered, float *d_rounded, double *h_centre, double *h_step);

/* Segment.mean / std / min / max (core.py:209-223, std = population) of caller-given ranges of one device buffer: range r is
 * samples [h_start[r], h_end[r]) of d_samples (n samples; int16 counts or float32 on the grid -- PS_DTYPE_F64 is PS_ERR_ARG),
 * its row goes to d_stats[r] (device).  The ranges may overlap, repeat, touch the buffer's two ends and come in any order: the
 * merged segments of HMM-guided segmentation (DataTypes.py:292-330) are such ranges.  Two launches whatever n_ranges is: every
 * range is cut into units of at most "range_tile" samples (context option, 64 .. 2^20, default 16 384; float32 units are at most
 * 2^14 samples), one workgroup per unit leaves exact integer sums of y = count - k0 and y^2 (k0: the count of the range's first
 * sample), then one lane per range adds them in unit order: mean = (k0 + S1 / n) q, std = sqrt(max(0, S2 / n - (S1 / n)^2)) q,
 * min and max from the integers, no multiply-add fused.  int16: S1 and S2 are exact in int64, S2 is rounded to double once;
 * float32: exact while S2 stays below 2^53.  The same ranges give the same bits however range_tile cuts them.
 * n_ranges == 0 returns PS_OK and launches nothing.  PS_ERR_ARG, with the first offending index in ps_last_error and nothing
 * launched: start < 0, end > n, end <= start, a range of more than 2^31 - 1 samples; also more than 2^24 - 1 units in one call.
 * One status word and one host synchronisation per call; the scratch (tables, partial rows) belongs to the context. */
int ps_range_stats(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, const int64_t *h_start,
                   const int64_t *h_end, int64_t n_ranges, ps_segstat *d_stats);

/* Replaces cSegmentAligner(model_means, model_stds, model_durs, skip_penalty, backslip_penalty).align(seq_means,
 * seq_stds, seq_durs) (calignment.pyx:20-100; called from SegmentAligner.align, alignment.py:33-46) for a BATCH of
 * sequences against one model: sequence q is entries [h_seq_off[q], h_seq_off[q+1]) of the three device arrays
 * (per-segment mean, std, duration -- e.g. the statistics ps_segment_batch produced).  Model arrays are host
 * pointers (m doubles each, 1 <= m <= 1024).  Outputs (device): d_scores[q] = score[s-1][m-1] -- the reference
 * returns it divided by numpy.sum(seq_durs), which the caller does in numpy to keep numpy's summation order --,
 * d_paths = the model index of every sequence segment (uint32 like the reference's unsigned j; same layout as the
 * inputs), d_status[q] = what the compiled reference does on that sequence:
 *   PS_ALIGN_OK; PS_ALIGN_VALUE_ERROR (empty sequence); PS_ALIGN_INDEX_ERROR (one-segment model with s > 1, or the
 *   traceback reaching model index 0 before the first sequence segment: `score[i-1, j-1]`, calignment.pyx:76);
 *   PS_ALIGN_ZERO_DIVISION (seq_std * model_std == 0, :49); PS_ALIGN_UNDEFINED (no final score above -1:
 *   double_argmax, :11-18, returns an uninitialised int there).  Scores and paths are bit-exact with the reference:
 *   the kernel keeps its operation order (sequential running maxima, fp64, no FMA contraction). */
#define PS_ALIGN_OK             0
#define PS_ALIGN_VALUE_ERROR    1
#define PS_ALIGN_INDEX_ERROR    2
#define PS_ALIGN_ZERO_DIVISION  3
#define PS_ALIGN_UNDEFINED      4
int ps_align_batch(ps_ctx *ctx, const double *h_model_means, const double *h_model_stds, const double *h_model_durs,
                   int32_t m, double skip_penalty, double backslip_penalty, const double *d_seq_means,
                   const double *d_seq_stds, const double *d_seq_durs, const int64_t *h_seq_off, int32_t n_seq,
                   double *d_scores, uint32_t *d_paths, int32_t *d_status);

/* Replaces PairwiseAligner(x, y) (alignment.py:97-313): Needleman-Wunsch, Smith-Waterman and the repeated local traceback
 * over two sequences of segment means.  Sequences are two sets, A (the x side, rows) and B (the y side, columns): set A is
 * d_a[h_a_off[k] .. h_a_off[k+1]) for k < n_a (fp64, device), B likewise; a NaN element is the gap marker '-' and scores 0
 * against everything (_score, :112-115), every other cell scores 3 - |x - y|^2 with the square taken by product.  A y of at
 * most 8190 elements (PS_ERR_ARG beyond); x is bounded by the scratch only.  All arithmetic is fp64 without contraction, and
 * the candidates of a cell are compared in the reference's order (first one wins), so results do not depend on the launch.
 *
 * ps_pairwise_scores: every pair of A x B on the score-only route (no matrix leaves the chip).  d_scores[k * n_b + l] =
 *   score[m][n] for PS_PW_GLOBAL, the maximum of the matrix for PS_PW_LOCAL; d_pos (optional, local only): two ints per
 *   pair, the row-major-first cell (i, j) holding that maximum, (0, 0) when no cell is above 0.
 *
 * ps_pairwise_batch: pair q = (A[h_pair_a[q]], B[h_pair_b[q]]), with traceback.  d_status[q]: PS_PW_OK, or
 *   PS_PW_INDEX_ERROR where the reference raises IndexError -- the local traceback marks the mirrored cell [j, i] of every
 *   cell it walks, which lies outside an m x n matrix when j > m or i > n (:229), and it reads xalign[-1] of an alignment
 *   that is empty or was trimmed to nothing (:246).  d_scores[q]: score[m][n] (global) or the maximum of the matrix.
 *   Alignments are index columns in WALK order (the alignment's last column first): d_cols_i / d_cols_j hold the 0-based
 *   element of x / y or -1 for a gap, pair q's columns in slot [h_col_off[q], h_col_off[q+1]); d_col_need[q] = the columns
 *   its alignments take.  Per alignment a of pair q, in slot h_aln_off[q] + a: d_aln_score, d_aln_start (first column
 *   within the pair's slot) and d_aln_len; d_aln_count[q] = alignments completed -- 1 for global, 0 or 1 for local, for
 *   PS_PW_LOCAL_REPEATED every alignment of at least min_length columns (counted before the trim) in the order the
 *   reference yields them, also those completed before a PS_PW_INDEX_ERROR.  When a slot of either kind is too small,
 *   PS_ERR_CAPACITY is returned: d_col_need and d_aln_count hold what every pair takes, the caller grows the slots and
 *   calls again.  The score matrix (fp64) and a pointer byte per cell live in a scratch per resident workgroup; the batch is
 *   split into launches whose scratch stays within option "pairwise_budget" bytes (default 2 GiB; a pair that needs more
 *   runs alone, up to 32 GiB).  Both calls synchronise the context's stream before returning. */
#define PS_PW_GLOBAL          0
#define PS_PW_LOCAL           1
#define PS_PW_LOCAL_REPEATED  2
#define PS_PW_OK              0
#define PS_PW_INDEX_ERROR     1
int ps_pairwise_scores(ps_ctx *ctx, const double *d_a, const int64_t *h_a_off, int32_t n_a, const double *d_b,
                       const int64_t *h_b_off, int32_t n_b, int32_t mode, double penalty, double *d_scores, int32_t *d_pos);
int ps_pairwise_batch(ps_ctx *ctx, const double *d_a, const int64_t *h_a_off, int32_t n_a, const double *d_b,
                      const int64_t *h_b_off, int32_t n_b, const int32_t *h_pair_a, const int32_t *h_pair_b, int32_t n_pairs,
                      int32_t mode, double penalty, int32_t min_length, double *d_scores, int32_t *d_status,
                      const int64_t *h_col_off, int32_t *d_cols_i, int32_t *d_cols_j, int32_t *d_col_need,
                      const int64_t *h_aln_off, double *d_aln_score, int32_t *d_aln_start, int32_t *d_aln_len,
                      int32_t *d_aln_count);

/* Replaces NaiveSplitter, the inner generator of NaiveTRF(seq, penalty, min_score) (alignment.py:806-870): the off-diagonal
 * local self-alignments of a sequence of segments with itself, which are the re-reads of an event in which the enzyme slipped
 * back.  Sequence q is the segments [h_off[q], h_off[q+1]) of d_mean / d_std (fp64, device; finite means, finite stds > 0:
 * the caller checks them), at most 2048 of them (PS_ERR_ARG beyond); an empty sequence is legal and yields nothing.  Cell
 * (i, j) of the (n + 1)^2 matrix is the maximum of 0, diagonal + 2 - |mean_i - mean_j|^2 / (std_i std_j), left + penalty and
 * up + penalty, first candidate winning a tie, a candidate whose SOURCE cell is masked left out; the mask starts as the
 * identity.  A repeat: the row-major-first maximum of the matrix, if above min_score, is walked back along the pointers to
 * the first cell whose pointer is 0; every walked cell and that end cell are masked, (score, length, i, j) -- the maximum,
 * the cells walked, the end cell -- is appended to the sequence's slot [h_slot_off[q], h_slot_off[q+1]) of d_score / d_len /
 * d_i / d_j, and the matrix is filled again.  A sequence ends when no cell is above min_score (d_status[q] =
 * PS_TRF_DONE) or after max_repeats yields (0: no cap; PS_TRF_MAX_REPEATS).  d_count[q] = its yields, also where the slot
 * was too small: the yields beyond the slot are counted, not stored, and the call returns PS_ERR_CAPACITY -- the caller
 * grows the slots and calls again.  PS_ERR_ARG for penalty >= 0 (the diagonal and the lower triangle, which the device does
 * not compute, would become observable) and for min_score < 0 (the reference never ends there).  All arithmetic is fp64
 * without contraction, division included, so the yields equal the reference's bit for bit.  A mask bit and a pointer of 2
 * bits per cell live in a scratch per resident workgroup; the batch is split into launches whose scratch stays within option
 * "trf_budget" bytes (default 2 GiB), sized by "slots_pct".  The call synchronises the context's stream before returning. */
#define PS_TRF_DONE         0
#define PS_TRF_MAX_REPEATS  1
int ps_trf_split_batch(ps_ctx *ctx, const double *d_mean, const double *d_std, const int64_t *h_off, int32_t n_seq,
                       double penalty, double min_score, int64_t max_repeats, double *d_score, int32_t *d_len, int32_t *d_i,
                       int32_t *d_j, const int64_t *h_slot_off, int32_t *d_count, int32_t *d_status);

/* A baked hidden Markov model (pypore_amd.hmm.Model.bake), host arrays.  States [0, n_emit) emit, states [n_emit, n_states)
 * are silent and grouped by topological level: level L is [level_ptr[L], level_ptr[L+1]), level_ptr[0] = n_emit,
 * level_ptr[n_levels] = n_states, and every silent predecessor of a silent state lies in a lower level.  kind[k]: 0 silent,
 * 1 normal, 2 uniform; param[3k..3k+2]: normal (mean, 1 / (2 std^2), -log(std sqrt(2 pi))), uniform (low, high,
 * -log(high - low)).  In-edges of k: [in_ptr[k], in_ptr[k+1]) of in_src / in_lp (source ascending, log probability); out-edges:
 * the same over out_dst / out_lp.  finite: paths end at `end` after the last observation; otherwise at any state.
 *
 * kind[k] = 3, a Gaussian kernel density: log density  -log(h sqrt(2 pi)) + log sum_i w_i exp(-(x - p_i)^2 / (2 h^2))  over
 * the state's points p_i with weights w_i (summing to 1) and bandwidth h.  The points of emitting state k are
 * [kde_ptr[k], kde_ptr[k+1]) of kde_pt (finite values) and kde_lw (log w_i, <= 0; -inf: the point is skipped): kde_ptr has
 * n_emit + 1 ascending entries from 0, a kind-3 state has at least one point and any other state none, and there are at
 * most 2^24 points in all (PS_ERR_ARG otherwise).  param[3k..3k+2] = (weighted mean of the points -- the shift c_k of
 * ps_hmm_expect's statistics --, 1 / (2 h^2), -log(h sqrt(2 pi))).  The sum is a log-sum-exp over the points in ascending
 * index: the largest term plus log1p of the others' exp.  The three kde_* fields were appended to the struct; they are read
 * only when some kind[k] is 3, so a caller built against the shorter struct, which never sets kind 3, stays correct.
 *
 * kind[k] = 4, a vector state: an observation is n_dim doubles (1 <= n_dim <= 16) and the state's log density is the
 * weighted sum  w_0 l_0(x_0) + w_1 l_1(x_1) + ...  of n_dim independent components, added in ascending d from the first
 * product.  Component d of emitting state k is entry i = k n_dim + d of comp_kind, comp_w (finite, > 0) and
 * comp_param[3i..3i+2]:
 *   comp_kind 1 normal       (mean, 1 / (2 std^2), -log(std sqrt(2 pi))):           c - (x - a)^2 b
 *   comp_kind 2 uniform      (low, high, -log(high - low)):                         c on [a, b], else -inf
 *   comp_kind 5 log-normal   (mu, 1 / (2 sigma^2), -log(sigma sqrt(2 pi))):         (c - (log x - a)^2 b) - log x for x > 0,
 *                                                                                    else -inf
 *   comp_kind 6 exponential  (0, rate, log rate):                                   c - x b for x >= 0, else -inf
 * Slot 0 of a triple is the shift c of the component's statistics in ps_hmm_expect.  In a vector model EVERY emitting state
 * is kind 4 (a plain normal state is one component of weight 1) and `param` is not read (it may be NULL); kind 4 beside kinds 1..3, n_dim
 * out of range, an unknown component kind, a bad weight or a null table is PS_ERR_ARG.  d_obs then holds n_dim doubles
 * per observation -- observation t of sequence q at (h_off[q] + t) n_dim; h_off still counts observations -- and
 * ps_hmm_expect's d_stats 1 + 2 n_dim doubles per emitting state.  n_dim and the three comp_* fields were appended to the
 * struct; they are read only when some kind[k] is 4, so a caller built against a shorter struct stays correct.
 *
 * kind[k] = 7, a mixture state: log density  log sum_i w_i p_i(x)  over the state's components, a weighted choice between
 * univariate distributions (weights summing to 1).  The components of emitting state k are [mix_ptr[k], mix_ptr[k+1]) of
 * mix_kind (1, 2, 5 or 6, as comp_kind), mix_param (the component's triple, as comp_param; slot 0 is the shift of its
 * statistics in ps_hmm_expect) and mix_lw (log w_i, <= 0; -inf: the component keeps its slot and is skipped): mix_ptr has
 * n_emit + 1 ascending entries from 0, a kind-7 state has at least one component and any other state none, and there are
 * at most 2^24 components in all.  param[3k..3k+2] = (0, 0, 0).  The sum is a log-sum-exp in ascending index over the
 * terms  log w_i + l_i(x)  that are > -inf -- the largest term plus log1p of the others' exp --, -inf when there is none,
 * never NaN; one component of weight 1 gives that component's own bits.  Observations are single doubles: a mixture state
 * stands beside kinds 1, 2, 3 and 7 only, and kind 7 beside kind 4 is refused as kinds 1..3 are.  A null table among the
 * four, a mix_ptr that does not start at 0 or descends, a kind-7 state without a component or another state with one, too
 * many components, an unknown component kind, or a log weight that is NaN or > 0 is PS_ERR_ARG.  mix_cdf and mix_draw
 * are read by ps_hmm_sample alone (see there) and may be NULL in every other call.  The six mix_* fields were appended to
 * the struct; they are read only when some kind[k] is 7, so a caller built against a shorter struct stays correct. */
typedef struct ps_hmm_model {
    int32_t n_states, n_emit, n_levels, start, end, finite;
    const int32_t *kind, *level_ptr, *in_ptr, *in_src, *out_ptr, *out_dst;
    const double *param, *in_lp, *out_lp;
    const int32_t *kde_ptr;
    const double *kde_pt, *kde_lw;
    int32_t n_dim;
    const int32_t *comp_kind;
    const double *comp_param, *comp_w;
    const int32_t *mix_ptr, *mix_kind;
    const double *mix_param, *mix_lw, *mix_cdf, *mix_draw;
} ps_hmm_model;

/* Decodes a BATCH of observation sequences against one model: sequence q is d_obs[h_off[q] .. h_off[q+1]) (fp64, device).
 * mode PS_HMM_VITERBI: d_logp[q] = the best path's log probability; the path (state indices, from start at step 0 to the
 *   last state, silent states included) goes to d_path[h_path_off[q] ..], its length to d_path_len[q] (0: impossible
 *   sequence, d_logp[q] = -inf).  When a path is longer than its slot h_path_off[q+1] - h_path_off[q], PS_ERR_CAPACITY is
 *   returned: the paths that fit are written and d_path_len holds every length, so the caller grows the slots and calls
 *   again.  Ties go to the lowest source state.
 * mode PS_HMM_FORWARD / PS_HMM_BACKWARD: d_logp[q] = the sequence's log probability (forward: f[n][end] for a finite
 *   model, else log-sum-exp of f[n]; backward: b[0][start]).
 * d_mat (optional, any mode): the (n+1) x n_states log matrix of the pass (Viterbi scores, forward or backward values),
 *   sequence q at row h_off[q] + q.  Limits: 1 <= n_states <= 4096 and an in-degree of at most 65535 (PS_ERR_ARG beyond).
 *   Viterbi splits the batch into launches whose backpointers ((n+1) x n_states bytes, two when an in-degree exceeds 255)
 *   fit in option "hmm_bp_budget" bytes (default 512 MiB).  The model's upload is kept by the context and reused while the
 *   arrays are unchanged.  Synchronises the context's stream before returning. */
#define PS_HMM_VITERBI   0
#define PS_HMM_FORWARD   1
#define PS_HMM_BACKWARD  2
int ps_hmm_batch(ps_ctx *ctx, const ps_hmm_model *model, int32_t mode, const double *d_obs, const int64_t *h_off,
                 int32_t n_seq, double *d_logp, double *d_mat, int32_t *d_path, const int64_t *h_path_off,
                 int32_t *d_path_len);

/* E-step of Baum-Welch over a BATCH (sequence q = d_obs[h_off[q] .. h_off[q+1]), fp64, device), summed over the sequences:
 * d_logp[q] = the sequence's log probability (as PS_HMM_FORWARD); d_counts[e] = the expected count of edge e, e in
 * out-edge CSR order (n_edges = out_ptr[n_states]; pypore_amd.hmm.Model.edges order); d_stats[3k .. 3k+2] = (W, A, B) of
 * emitting state k: the sums of the posterior g, g (x - c_k) and g (x - c_k)^2 over the observations, c_k = param[3k].
 * For a vector model (kind 4) d_stats holds 1 + 2 n_dim doubles per emitting state instead: W, then (A_d, B_d) for d = 0 ..
 * n_dim - 1, with A_d = sum g (y_d - c_d), B_d = sum g (y_d - c_d)^2, y_d = log x_d for a log-normal component and x_d
 * otherwise, c_d = the component's comp_param slot 0; at n_dim = 1 that is the (W, A, B) layout.
 * For a model with mixture states (kind 7) and n_mix = mix_ptr[n_emit] components d_stats holds 3 (n_emit + n_mix) doubles:
 * the states' (W, A, B) as ever -- a kind-7 state's shift is param[3k] = 0, so its row holds the raw moments --, then one
 * (W_i, A_i, B_i) per mixture component in table order.  Where state k's posterior g at observation x is positive, each
 * component i of k whose term  v_i = mix_lw[i] + l_i(x)  is > -inf has the responsibility  r = exp(v_i - e_k(x))  and adds
 * w = g r  to W_i,  w d  to A_i and  (w d) d  to B_i,  d = y - mix_param[3i],  y = log x for a log-normal component and x
 * otherwise.  The accumulators
 * (n_acc = n_edges + (1 + 2 n_dim) n_emit + 3 n_mix + 1, at most 2^26) live in LDS when 16 n_states + 8 n_acc fit in 64 KiB.
 * A sequence with logp = -inf contributes nothing and is counted in *h_skipped.  Forward matrices are kept in HBM for
 * launches of at most option "hmm_fb_budget" bytes (default 4 GiB; at least one sequence per launch); the accumulators
 * are per-workgroup rows summed in a fixed order, so the same call with the same options gives the same bits.  Limits as
 * ps_hmm_batch.  Synchronises the context's stream before returning. */
int ps_hmm_expect(ps_ctx *ctx, const ps_hmm_model *model, const double *d_obs, const int64_t *h_off, int32_t n_seq,
                  double *d_logp, double *d_counts, double *d_stats, int32_t *h_skipped);

/* Posterior decoding over a BATCH (sequence q = d_obs[h_off[q] .. h_off[q+1]), fp64, device; n = its length), nothing summed
 * over the sequences.  d_logp[q] = the sequence's log probability (as PS_HMM_FORWARD; required).  Every other output is
 * optional, a null pointer skips it:
 *   d_post       n_emit doubles per observation, row h_off[q] + t for observation t of sequence q (n rows of n_emit, not
 *                n + 1 rows of n_states): the log posterior  (f[t+1][k] + b[t+1][k]) - d_logp[q]  of emitting state k, -inf
 *                where either matrix entry is -inf.
 *   d_map_state  one int32 per observation, at h_off[q] + t: the emitting state with the largest entry of that row, the
 *                lowest state index on a tie (the rule Viterbi uses for sources).
 *   d_map_logp   [q] = the sum over t of those largest entries, added in ascending t: the same call gives the same bits, and
 *                they are the bits of that sum over d_post.
 *   d_counts_seq n_edges doubles per sequence at q * n_edges: that sequence's expected count of every out-edge, in the
 *                order and by the arithmetic of ps_hmm_expect's d_counts (which is their sum over q, in another order).
 *                The kernel zeroes the row.
 * A sequence with d_logp[q] = -inf: its d_post rows are -inf, its d_map_state entries -1, d_map_logp[q] = -inf, its counts
 * row 0.  An empty sequence has no rows, d_map_logp[q] = 0.0, and its counts row holds the silent edges at t = 0.  Forward
 * matrices are kept in HBM for launches of at most option "hmm_fb_budget" bytes, as for ps_hmm_expect; every output
 * belongs to one sequence, so the results do not depend on how the batch is cut.  Limits, status codes and the reuse of
 * the model's upload as ps_hmm_expect.  Synchronises the context's stream before returning. */
int ps_hmm_posterior(ps_ctx *ctx, const ps_hmm_model *model, const double *d_obs, const int64_t *h_off, int32_t n_seq,
                     double *d_logp, double *d_post, int32_t *d_map_state, double *d_map_logp, double *d_counts_seq);

/* What sampling reads beside the model (pypore_amd.hmm.Model._sample_tables), host arrays built in fp64 from the
 * distributions themselves, so that no decision of a walk depends on a device logarithm or exponential:
 *   out_cdf    n_cdf = out_ptr[n_states] doubles, aligned with out_dst: per state the running sum of its out-edges'
 *              probabilities, added one by one (>= 0 and ascending); the entry of the state's last out-edge of positive
 *              probability and every entry after it is exactly 1.0, so an edge of probability 0 is never taken;
 *   emit_param n_param = 2 n_emit doubles (2 n_emit n_dim for a vector model, component k n_dim + d): normal (mean, std),
 *              uniform (low, high - low), log-normal (mu, sigma), exponential (0, rate), kernel density (0, bandwidth);
 *   kde_cdf    n_kde = kde_ptr[n_emit] doubles, aligned with kde_pt: per kernel-density state the running sum of its
 *              points' weights, exactly 1.0 from the state's last point of positive weight on (NULL and 0 without kind-3
 *              states).
 * Every row of the three cdf tables is checked against the model (PS_ERR_ARG, the message names the table and the state): its
 * entries are finite and >= 0, none below its predecessor -- but a running sum that rounding carried past 1.0 may be followed
 * by the entries stored as 1.0 --, the last is exactly 1.0, and an entry above its predecessor (the first: above 0) is one
 * whose log probability in the model (out_lp, kde_lw, mix_lw) is > -inf: a row that gives an interval of u to an entry the
 * model calls impossible is refused.  An entry equal to its predecessor is never picked.
 * The weights comp_w of a vector model are not read: a weight scales a log density and defines nothing to draw from.
 * A model with mixture states (kind 7) brings two more tables in ps_hmm_model itself (this struct keeps its size; without
 * them ps_hmm_sample returns PS_ERR_ARG); emit_param still holds 2 doubles per emitting state, (0, 0) for a mixture state:
 *   mix_cdf    mix_ptr[n_emit] doubles, aligned with mix_lw: per mixture state the running sum of its components' weights,
 *              added one by one; the entry of the state's last component of positive weight and every entry after it is
 *              exactly 1.0, so a component of weight 0 is never picked;
 *   mix_draw   2 doubles per mixture component, by emit_param's rule for the component's kind. */
typedef struct ps_hmm_sample_tables {
    const double *out_cdf, *emit_param, *kde_cdf;
    int64_t n_cdf, n_param, n_kde;
} ps_hmm_sample_tables;

/* Samples n_seq sequences from the model: walks from `start` along the out-edges, an observation drawn on entering an
 * emitting state.  length = 0: a walk runs until it enters `end` (a model that is not finite: PS_ERR_ARG); length > 0: it
 * stops at `end` or right after its length-th emission, whichever comes first.  A walk that has made max_length (>= 1)
 * emissions without such an end stops there.
 *
 * The random stream: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with key
 * (seed & 0xffffffff, seed >> 32).  Sequence Q = first + q (first >= 0) owns the blocks j = 0, 1, 2, ... at counter
 * (j & 0xffffffff, j >> 32, Q & 0xffffffff, Q >> 32); a block r0..r3 gives  u0 = ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53  and u1
 * likewise from r2, r3.  Blocks are taken in walk order.  A transition out of state k takes one: the first out-edge e of
 * k with u0 < out_cdf[e].  An emission takes one per component in ascending d, with  z = sqrt(-2 log(1 - u0)) cos(2 pi u1):
 * normal  mean + std z;  uniform  low + u0 (high - low);  log-normal  exp(mu + sigma z);  exponential  -log(1 - u0) / rate;
 * a kernel-density state takes two: the first point i with u0 < kde_cdf[i], then  p_i + h z  from the next block; a mixture
 * state takes two as well: the first component i of the state with u0 < mix_cdf[i], then that component's draw by
 * (mix_kind[i], mix_draw[2i], mix_draw[2i+1]) from the next block.  No
 * multiply-add is fused.  So a call with the same arguments gives the same bits, a batch cut in two with `first` moved on
 * gives the bits of the whole, and a walk's path and length depend on (seed, Q, out_cdf) alone.
 *
 * Sequence q writes its observations, n_dim doubles each, to d_obs at slot [h_off[q], h_off[q+1]) (counted in
 * observations) and, when d_path and h_path_off are given, its path -- the states visited from `start` on, silent ones
 * included -- to d_path[h_path_off[q] .. h_path_off[q+1]).  d_len[q] and d_path_len[q] (optional without a path buffer)
 * always receive the full lengths; d_flags[q] = 0 (the walk entered `end` or made its `length` emissions), 1 (stopped at
 * max_length) or 2 (it stood in a state without out-edges).  A walk whose slot is full goes on counting without writing,
 * and the call returns PS_ERR_CAPACITY with every length reported and the sequences that fit written: the walks are
 * deterministic, so the caller sizes the slots exactly and calls again.  Limits as ps_hmm_batch; besides,
 * (max_length + 1) (n_levels + 1) + 2, the longest path there can be, must fit in int32 (PS_ERR_ARG).  The tables are
 * uploaded per call; the model's upload is the one ps_hmm_batch keeps.  Synchronises the context's stream before
 * returning. */
int ps_hmm_sample(ps_ctx *ctx, const ps_hmm_model *model, const ps_hmm_sample_tables *tables, uint64_t seed, int64_t first,
                  int32_t n_seq, int32_t length, int32_t max_length, double *d_obs, const int64_t *h_off, int32_t *d_len,
                  int32_t *d_flags, int32_t *d_path, const int64_t *h_path_off, int32_t *d_path_len);

/* Timing of the most recent ps_segment_batch, measured with HIP events on the context's stream.
 * ms[7] = the call's device work from the first upload to the last result copy (option "timing" >= 1, the
 * default); ms[3] = whole call on the host's wall clock.  With option "timing" = 2 an event is also recorded
 * between the phases: ms[0] spine kernel, ms[1] tree kernel, ms[2] gather+stats kernels, ms[4] stitch (assemble
 * kernels, or the host stitch), ms[5] bridge kernels, ms[6] block-prefix kernel (K0; 0 for the LDS-window scan)
 * -- every such event keeps the next kernel from starting back to back (about 6 us of idle GPU each), so the
 * breakdown is a diagnostic and off by default.  counters[0] window scans, [1] candidate
 * positions covered, [2] tiles, [3] tree jobs, [4] seams mended: 1 .. 999 999 seams continued on the device (option
 * "bridge_ext"), 1 000 000 + n the call was redone by the host stitch, with n repairs, [5] windows decided in fp64 (among
 * contenders or by a whole-window scan), [6] of which whole-window scans, [7] 1 = the call was redone on the 64-bit
 * digest, 2 = on the LDS-window kernels (counts too wide for the block sums), [8] [9] [10] window scans of the spine /
 * bridge / subtree kernels, [11] near ties: windows decided among fp64 contenders whose margin -- winner against the best
 * other candidate, or against min_gain -- is below 1e-9 * max(1, |gain|).  The device logarithm is not glibc's bit for bit
 * (gains differ by ~1e-11), so the reference could have decided such a window the other way; exact ties are decided like
 * the reference (first maximum wins, cparsers.pyx:175-177) and counted too; -1 = not counted: the call ran on the
 * LDS-window kernels (min_width < 8, option "scan_bs" 0 / "stitch_host" 1, counters[7] = 2, ps_segment_exact_f64); [12] chunk results (16 windows each) that the
 * look-ahead kernel's helpers published (option "lat_help"), [13] published chunks that a seam's owner took instead of
 * scanning them, [14] subtree jobs the screen kernel (option "tree_screen") handed on to the subtree kernel, [15] windows the
 * screen kernel decided (they are part of [0] and [10], so [10] - [15] are the windows the subtree kernel scanned); both
 * cover every round of the call, like [0] and [10], and both are -1 when the call did not launch the screen kernel; [16] [17]
 * look-ahead / upload launches the call did without (option "short_chain": 0 or 1 each), [18] seams its bridges left deferred
 * that the look-ahead kernel finished behind the stitch (they are part of [4]).  Twenty counters in all ([19] is reserved).
 * The indices by name, in the order above: ms[PS_MS_SPINE] .. ms[PS_MS_SEQ], counters[PS_CNT_WINDOWS] .. counters[PS_CNT_SEAMS_RESUMED]. */
enum { PS_MS_SPINE = 0, PS_MS_TREE, PS_MS_GATHER, PS_MS_TOTAL, PS_MS_STITCH, PS_MS_BRIDGE, PS_MS_BLOCKSUM, PS_MS_SEQ, PS_MS_COUNT = 8 };
enum { PS_CNT_WINDOWS = 0, PS_CNT_CANDIDATES, PS_CNT_TILES, PS_CNT_TREE_JOBS, PS_CNT_REPAIRS, PS_CNT_EXACT_RESCANS, PS_CNT_FULL_EXACT_SCANS,
       PS_CNT_WIDE_REDO, PS_CNT_WINDOWS_SPINE, PS_CNT_WINDOWS_BRIDGE, PS_CNT_WINDOWS_TREE, PS_CNT_NEAR_TIES, PS_CNT_HELPER_CHUNKS_PUBLISHED,
       PS_CNT_HELPER_CHUNKS_TAKEN, PS_CNT_TREE_DEFERRED, PS_CNT_WINDOWS_SCREEN, PS_CNT_LOOKAHEAD_SKIPPED, PS_CNT_UPLOAD_SKIPPED,
       PS_CNT_SEAMS_RESUMED, PS_CNT_COUNT = 20 };
int ps_get_timings(const ps_ctx *ctx, double *ms, int32_t n_ms, int64_t *counters, int32_t n_counters);
/* The twenty work counters of ps_get_timings in place (valid for the life of the context; host memory, updated by every
 * call before it returns): a caller that checks one of them after each call -- counters[11], the near ties -- reads it
 * there instead of making a second call. */
const int64_t *ps_counters(const ps_ctx *ctx);

/* Where the near ties of counters[11] lie: the windows of the context's most recent ps_segment_batch(_ex), ps_segment_events,
 * ps_detect_segment_trace (its detected events) or ps_segment_exact_f64 call that were decided by a margin inside the
 * reference's own rounding noise, one record per distinct (event, window, split), sorted by (event, window_start).
 * Coordinates are samples of the event: the window [window_start, window_end), split = the boundary the device placed in it
 * (an index of the event), or -1 when it placed none.  For such a window the reference may differ, usually by one sample.
 * The records are a SUPERSET of the decisions behind the returned boundaries: speculative scans (tile spines, look-ahead
 * helpers, seam bridges) are logged as well, just as counters[11] counts them -- a window of the final recursion starts at
 * 0 or a returned boundary plus a multiple of window_width / 2 and ends at min(that + window_width, 0 / a boundary / the
 * event's end), and its split, if any, is a returned boundary (pypore_amd.engine.consistent_sites filters on that).
 * *n_out >= 0: the number of records (PS_ERR_CAPACITY when it exceeds cap: nothing is written, call again with room);
 * *n_out = PS_NT_NOT_COUNTED: no margins were kept -- the call ran on the LDS-window kernels (counters[11] = -1: min_width < 8,
 * option "scan_bs" 0 / "stitch_host" 1, counters[7] = 2, ps_segment_exact_f64), option "near_tie_log" is 0, the call failed,
 * or the library is a PS_STAMP build; *n_out = PS_NT_INCOMPLETE: more near ties than the log holds (option "near_tie_log",
 * default 65 536 records = 1 MB of device memory per context; the count goes on, the records stop).  Either way the caller
 * treats every event of the call as flagged.  Synchronises the context's stream when there are records to fetch. */
#define PS_NT_NOT_COUNTED    -1
#define PS_NT_INCOMPLETE     -2
typedef struct ps_near_tie {
    int32_t event, window_start, window_end, split;   /* event-relative; split -1: none */
} ps_near_tie;
int ps_get_near_ties(const ps_ctx *ctx, ps_near_tie *out, int32_t cap, int64_t *n_out);

/* Synthetic step-signal generator (bit-identical to pypore_amd/synth.py):
 * sample i = level_counts[segment containing i] + noise(seed, i), written as fp32 pA
 * (count * 2^-5) or int16 counts.  h_seg_end[nseg] are the exclusive segment ends
 * (ascending, last >= n).  Bench/test infrastructure. */
int ps_synth_trace(ps_ctx *ctx, void *d_out, int32_t dtype, int64_t n, uint64_t seed,
                   const int64_t *h_seg_end, const int32_t *h_level_counts, int64_t nseg);

/* The reference's state parsers (parsers.py:572-679) on the device: what they RETURN, quirks included.
 * Both take float64 currents in the batch layout of ps_statsplit_f64 (event e = [h_ev_start[e], h_ev_start[e] + h_ev_len[e]),
 * at most 2^30 samples each) and write spans: (start, end) int32 pairs, positions from the event's start, event after event.
 *   d_spans     2 * cap int32 values, device
 *   h_span_off  n_ev + 1 entries: event e's spans are h_span_off[e] .. h_span_off[e + 1]; when cap is too small the call
 *               returns PS_ERR_CAPACITY with the required size in h_span_off[n_ev] and writes no span
 * PS_ERR_ARG (message in ps_last_error): a negative start or length, an event longer than 2^30 samples.
 *
 * ps_snakebase_f64 -- snakebase_parser.parse: with m = n - 1 and low the ascending positions j in [0, m) where
 * |current[j + 1] - current[j]| < 1e-3 (a NaN difference is not), the spans are (low[0], low[1]), (low[2], low[3]), ... and,
 * when low has an odd number of entries, (low[-1], m).  The parser's threshold takes no part in what the reference returns,
 * so it is no argument.  n of 0 or 1: no span.  No span is empty. */
int ps_snakebase_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                     int32_t *d_spans, int64_t cap, int64_t *h_span_off);

/* ps_filter_derivative_f64 -- FilterDerivativeSegmenter.parse: y = filtfilt(bessel(1, cutoff_freq / (sampling_freq / 2)),
 * current) (the kernels of ps_filter_bessel, one event after the other on the context's stream), deriv[j] = |y[j + 1] - y[j]|,
 * blocks[j] = deriv[j] > low_threshold, tics = the j + 1 with blocks[j + 1] != blocks[j], pairs (tics[0], tics[1]), (tics[2],
 * tics[3]), ... (an unpaired last tic is dropped; when blocks[0] is set the pairs are the gaps between the blocks, as in the
 * reference).  A pair (s, t) is kept when np.argmax(deriv[s:t]) > high_threshold -- the INDEX of the first maximum, as the
 * reference has it: with h = floor(high_threshold), max(deriv[s + h + 1 : t]) > max(deriv[s : s + h + 1]), strictly; an empty
 * right part is not kept, a negative high_threshold keeps every pair.  With the kept pairs (s_1, t_1) .. (s_k, t_k) the spans
 * are [0, s_1), [t_1, s_2), ..., [t_k, n); none kept: [0, n).  An empty event (prefiltered only) has no span.
 * prefiltered 1: d_current is y itself and no filter runs (cutoff_freq, sampling_freq unused) -- the decisions are then the
 * reference's bit for bit; with the filter they are the reference's wherever a decision's margin exceeds the filter's
 * distance from scipy (1e-11 of max|y|, docs/CALLERS.md).  Non-finite input is undefined, as it is in scipy.
 * PS_ERR_ARG also for: an event of n <= 6 samples when prefiltered is 0 (scipy's padlen), a cutoff outside (0, Nyquist), a
 * NaN threshold, prefiltered other than 0 / 1. */
typedef struct ps_filter_derivative_params {
    double low_threshold, high_threshold, cutoff_freq, sampling_freq;
    int32_t prefiltered;
} ps_filter_derivative_params;
int ps_filter_derivative_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                             const ps_filter_derivative_params *params, int32_t *d_spans, int64_t cap, int64_t *h_span_off);

#ifdef __cplusplus
}
#endif
#endif /* PORESEG_H */
