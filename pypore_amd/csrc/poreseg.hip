// poreseg.hip -- C ABI (include/poreseg.h) and host orchestration of libporeseg.so.
//
// Pipeline of ps_segment_batch, one stream, one host sync at the end:
//   phase 0  blocksum_kernel   K0: chunk-prefixed sums per 8-sample block (the only pass over the samples)
//   phase 1  spine_kernel      one workgroup per tile: speculative spine of rec(T, END)
//   phase 1b bridge_kernel     continues each tile's chain until it meets the downstream tile's
//   stitch   assemble_* kernels  true spine per event from the tile spines (host-side only as the fallback)
//   phase 3  tree_kernel       one job per true spine step: rec(a_k, a_{k+1}) in order
//   gather   item_scan + gather kernels -> contiguous, sorted boundary list per event
//   K2       segstat_kernel (optional)
// Which kernel runs with which grid is decided once each: by_dtype / by_nt (run-time sample type and workgroup width -> the
// kernels' template arguments), reserve_digest + launch_k0 (phase 0, for every route that runs K0), scan_shape (launch shape of
// the scan kernels), launch_scans_bs / launch_spine_nt (phases 1, 1b), launch_subtrees (phase 3), reserve_items (item buffers),
// begin_segment_call (prologue of the segment entry points).  What a segment call plans on the host -- its scan route, the tile
// tables of either stitch route, the host stitch, the seams of the second chance -- is plain C++ in seg_plan.hpp, checked on the
// CPU (tests/native/seg_plan_check.cpp); device_stitch_batch and host_stitch_batch act on it: buffers, uploads, launches.
// The context (ps_ctx) owns its GPU resources: DevBuf, HostBuf, Event and Stream free themselves, so ps_destroy is `delete ctx`
// and a half-built context of ps_create releases what it had.  The segmentation chain's members are flat; every other feature
// keeps its buffers and caches in one sub-struct of ps_ctx (filt, align, pw, ss, nt, hmm).  A new feature adds its
// sub-struct there and needs no entry anywhere else.  The context's options -- their defaults, names, ranges, PORESEG_* variables
// (diagnostic library) and which of them act on the context when set -- are one struct and one table in ctx_options.hpp, checked on
// the CPU (tests/native/ctx_options_check.cpp): ps_set_option, ps_get_option and diag_env go through it, and the code here reads
// ctx->opt.  ps_live_bytes counts what the owning buffers of the process hold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <complex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "poreseg.h"
#include "poreseg_pieces.h"
#include "seg_device.hpp"
#include "seg_align.hpp"
#include "seg_pairwise.hpp"
#include "seg_trf.hpp"
#include "seg_hmm.hpp"
#include "seg_ingest.hpp"
#include "seg_statsplit.hpp"
#include "seg_state.hpp"
#include "seg_ranges.hpp"
#include "seg_pieces.hpp"
#include "pool_plan.hpp"
#include "seg_plan.hpp"
#include "filt_plan.hpp"
#include "batch_plan.hpp"
#include "ctx_options.hpp"

using namespace ps;

namespace {

// Device + pinned host bytes the owning DevBufs and HostBufs of the process hold (ps_live_bytes): touched only where memory is
// really allocated or freed, never by a reserve() that finds room.
std::atomic<int64_t> g_live_bytes{0};

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

struct DevBuf : NoCopy {  // device memory that frees itself: an owner (reserve) or a view into another buffer (alias)
    void *p = nullptr;
    size_t cap = 0;
    bool owned = true;        // false: p points into another buffer (alias), nothing to free
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (!owned) { p = nullptr; cap = 0; owned = true; }
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; g_live_bytes -= cap; p = nullptr; cap = 0; }
        size_t want = std::max(bytes, cap + cap / 2);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) { cap = want; g_live_bytes += cap; }
        return e;
    }
    // as reserve(), but a fresh allocation is cleared (buffers whose stale contents are compared with an epoch)
    hipError_t reserve_zeroed(size_t bytes, hipStream_t st)
    {
        const void *before = p;
        const size_t cap0 = cap;
        hipError_t e = reserve(bytes);
        if (e == hipSuccess && (p != before || cap != cap0) && p) e = hipMemsetAsync(p, 0, cap, st);
        return e;
    }
    // Points this buffer into `blob` (one upload for several small arrays); a later reserve() allocates afresh.
    void alias(void *ptr) { release(); p = ptr; owned = false; }
    void release() { if (p && owned) { (void)hipFree(p); g_live_bytes -= cap; } p = nullptr; cap = 0; owned = true; }
    template <class T> T *as() { return static_cast<T *>(p); }
};

struct HostBuf : NoCopy { // pinned staging memory that frees itself
    void *p = nullptr;
    size_t cap = 0;
    ~HostBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        size_t want = std::max(bytes, cap + cap / 2);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) { cap = want; g_live_bytes += cap; }
        return e;
    }
    void release() { if (p) { (void)hipHostFree(p); g_live_bytes -= cap; } p = nullptr; cap = 0; }
    template <class T> T *as() { return static_cast<T *>(p); }
};

struct Event : NoCopy {   // an event of the context, destroyed with it
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

struct Stream : NoCopy {  // the context's stream: destroyed with it when the context made it (own), never when the caller handed it in
    hipStream_t s = nullptr;
    bool own = false;
    ~Stream() { if (own && s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

}  // namespace

static_assert(CtxOptions().mode == MODE_FAST && CtxOptions().bridge_patience == BR_PATIENCE_POOL, "ctx_options.hpp: defaults named in seg_device.hpp");
constexpr int LA_KEEP = 16;        // calls that keep the look-ahead launch after one that needed it (ps_ctx::la_keep)
struct ps_ctx {
    int device = 0;
    int n_cu = 0;             // compute units (queried once)
    // The stream and the events stand in front of every buffer: members go in reverse order, so the buffers are freed after
    // the destructor's synchronise and before the stream and the events are destroyed.
    Stream stream;
    Event ev[10];             // [0..7] phase marks (timing level 2), [8] start and [9] end of the call's device work (level 1)
    Event ev_front[2];        // hand-over events (no timing): [0] context stream -> front stream, [1] front stream -> context stream
    ~ps_ctx() { (void)hipSetDevice(device); if (stream.s) (void)hipStreamSynchronize(stream.s); }
    std::string err;
    CtxOptions opt;           // every option of ps_set_option as last set (ctx_options.hpp: the values and the table of their rules)
    int k0_unaligned = 1;     // what option k0_unaligned comes to: K0's fast route loads 16 bytes from sample-aligned addresses -- asked for (opt) and
                              // granted by the probe, once per device at ps_create and again when the option is set (k0_unaligned_probe)
    int64_t tile_len = 0, halo = 0;
    int lds_max_samples = 0;
    uint8_t *d_is_spine = nullptr;   // optional output of the current call
    WideRedo wide;            // the last call K0 refused (counts too wide) and where the calls after it start (seg_plan.hpp)
    bool chain_held = false;  // this call has a ticket of the device's K0 chain (K0Chain) and has not recorded its event yet
    unsigned long long chain_ticket = 0;
    bool defer_sync = false;  // (internal) ps_filter_requantise_batch: the filter entry only queues its kernels -- no status clear, copy, sync
    bool stream_idle = true;  // the context's stream had nothing queued when the current call began (no hand-over to the front stream needed)
    // host-side caches: workgroups per CU per kernel, dynamic-LDS attribute last set, the tile tables of the last call
    struct OccKey { const void *fn; int nt; size_t lds; int per_cu; };
    std::vector<OccKey> occ_cache;
    std::vector<std::pair<const void *, int>> attr_cache;
    struct TileCache {        // the device route's tile plan (seg_plan.hpp), what it was planned for, and whether its tables are on the device
        bool valid = false;
        DeviceTileKey key;
        DeviceTilePlan plan;
    } tile_cache;
    DevBuf bsum, ev_info, chunk_mabs, ev_boff, blk_mm, grp, up_dev;
    // The segmentation chain's own buffers are flat members.  The state of every self-contained feature stands together in a
    // sub-struct (filt, align, pw, trf, ss, sp, nt, hmm): its buffers and its host-side caches.  A new feature adds its group here
    // -- the buffers free themselves with the context --, and an option of it is a member of CtxOptions and a row of its table.
    struct {                // Bessel filter (ps_filter_bessel, ps_filter_bessel_batch, ps_filter_requantise_batch)
        DevBuf fwd, agg, zin;
        DevBuf tab, rq_par;   // a batch's event and unit tables (filt_plan.hpp; the re-quantisation's behind them), (centre, 1 / step, step) per event
    } filt;
    struct { DevBuf tab, part; } rng;        // statistics of caller-given ranges (ps_range_stats): the range and unit tables (range_plan.hpp), a RangePart per unit
    struct { DevBuf scratch; } pc;           // every piece of a trace (ps_detect_pieces): start bits, per-chunk tables and parts (piece_plan.hpp)
    struct { DevBuf in, scratch; } align;    // profile aligner (ps_align_batch)
    struct { DevBuf in, scratch; } pw;       // pairwise aligner (ps_pairwise_scores / ps_pairwise_batch): offsets and pair tables, per-workgroup matrices
    struct { DevBuf in, scratch; } trf;      // NaiveTRF's splitter (ps_trf_split_batch): offsets and the capacity flag, per-workgroup mask and pointer bits
    DevBuf ev_info_tr;        // single-pass file route (ps_detect_segment_trace): (centre, phase, first block) of the events cut out of a trace-aligned digest
    DevBuf blk_cls, cls_mm;   // ... K0's verdict per block against the detector's threshold (2 bits), min / max per 128 blocks
    DevBuf pre_c;             // exact route (ps_segment_exact_f64): c and c2 of the call's samples, 16 B per sample
    // StatSplit (ps_statsplit_f64): per-event tables, prefix sums (c, c2, ct), boundary slots, interval stacks, counts +
    // status word, output offsets
    struct { DevBuf tab, pre, tmp, stack, cnt, off; } ss;
    // State parsers (ps_snakebase_f64, ps_filter_derivative_f64): the compaction's tables (tab, tab2), predicate mask, tile counts
    // and their scan, hits before each event of the first / second compaction (off1, off2), hit list (hits: low / tics), pair
    // offsets, keep flags, kept pairs, the filtered current, event lengths, span offsets
    struct { DevBuf tab, tab2, mask, cnt, excl, off1, off2, hits, pair_off, keep, kept, y, len, span_off; } sp;
    // Near-tie log of the segment calls (DevCfg::nt_log, ps_get_near_ties): opt.near_tie_log records (0: off), allocated
    // with the first call that logs.  nt.seen: records the last segment call counted (-1: not counted), nt.call_cap the capacity
    // it ran with; nt.ev_start / nt.ev_len: its events, kept only when it logged any (the records are mapped to them on request).
    struct {
        DevBuf log;
        int64_t hdr_cap = -1;                  // the capacity the header on the device names; -1: none written
        int64_t seen = -1, call_cap = 0;
        std::vector<int64_t> ev_start, ev_len;
    } nt;
    struct {
        // HMM decoding (ps_hmm_batch): the model's last upload (host copy compared on every call), offsets, backpointers, results
        DevBuf model, off, bp, last, flags;
        std::vector<char> blob;
        // Baum-Welch E-step (ps_hmm_expect): forward matrices of one launch, per-workgroup accumulator rows, the skipped count
        DevBuf fmat, acc, skip;
        DevBuf pmax;                         // ps_hmm_posterior: the per-observation maxima that d_map_logp sums
        DevBuf samp;                         // ps_hmm_sample: the sampling tables, then the observation and path offsets
    } hmm;
    DevBuf ev_len, det_counts, det_tics, det_cand;
    DevBuf bridges, bmeta, tile_i32, sp_off, spine_items, asm_hdr, ev_first_tile;
    DevBuf bridge_ext, ext_slot, ext_list;          // second chance for seams that gave up (seg_device.hpp: EXT_MAX)
    DevBuf lat_state, lat_seam, lat_res;            // helpers of the look-ahead kernel (seg_device.hpp: LAT_D)
    unsigned lat_tag_next = 1;                      // tags handed to calls so far (24 bits; the results are cleared before they run out)
    unsigned lat_tag_base = 0;                      // this call's
    // la_keep: a pooled call whose bridges left seams deferred had the look-ahead kernel run behind its stitch, a round trip late;
    // the next LA_KEEP calls of the context launch it in the chain again, patience 3, as without the option (the data at hand has
    // long stretches without splits), then the option is tried anew.  la_now: the current call is one of those.
    int la_keep = 0;
    bool la_now = false;
    bool small_clean = false;                       // the last thing that touched the status block was a call's download kernel, which left it zero
    bool small_clean_in = false;                    // ... as the current call found it (make_cfg)
    HostBuf h_hdr;
    DevBuf spine_jobs, spine_scratch, spine_dense, spine_meta, tree_jobs, tree_scratch, tree_spill, tree_defer, screen_acc,
        tree_counts, items, item_pos, first_item, ev_off, bounds_off, small;
    HostBuf h_meta, h_dense, h_small, h_up;
    double ms[PS_MS_COUNT] = {};              // what ps_get_timings returns (include/poreseg.h: PS_MS_*, PS_CNT_*)
    int64_t counters[PS_CNT_COUNT] = {};
    ps_ctx() { counters[PS_CNT_TREE_DEFERRED] = counters[PS_CNT_WINDOWS_SCREEN] = -1; }     // (the screen kernel was not launched)
    bool screen_ran = false;  // the current call launched tree_screen_kernel
};

namespace {

int fail(ps_ctx *ctx, int code, const char *fmt, ...)
{
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, PS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The front stream of a device (option k0_shared): one stream per device and process on which the upload + K0 launches of
// all contexts are queued back to back (the mutex keeps one call's pair of launches and its event together).
struct FrontStream { std::mutex mu; hipStream_t s = nullptr; };
FrontStream g_front[16];
FrontStream *front_for(ps_ctx *ctx)
{
    if (ctx->device < 0 || ctx->device >= 16) return nullptr;
    FrontStream *f = &g_front[ctx->device];
    std::lock_guard<std::mutex> lk(f->mu);
    if (!f->s) {
#ifdef PS_DIAG
        int lo = 0, hi = 0;
        const char *pr = std::getenv(ENV_FRONT_PRIORITY);         // 1: highest priority the device offers (experiments)
        if (pr && std::atoi(pr) != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) {
            if (hipStreamCreateWithPriority(&f->s, hipStreamNonBlocking, hi) != hipSuccess) { f->s = nullptr; (void)hipGetLastError(); }
        }
#endif
        if (!f->s && hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking) != hipSuccess) { f->s = nullptr; (void)hipGetLastError(); return nullptr; }
    }
    return f;
}

// K0 admission (option k0_admit): at most M calls of a device have their K0 in flight at a time.  K0 is bound by HBM: T of them
// side by side only share the same bytes per second, and all of them -- with every call's scan kernels behind them -- finish late
// together (sixteen contexts: 0.188 -> 0.175 ms per step with M = 3, round 5).  Round 6: ON THE DEVICE.  The calls of a device
// take tickets; call t queues, in front of its K0, a wait for the event recorded behind the K0 of call t - M (hipStreamWaitEvent:
// a barrier packet in its own queue).  Round 5's gate had host threads poll hipEventQuery every 25 us under one mutex and could
// spin forever on a faulted device; here no host thread ever waits for the device.  Same step time as the polling
// gate (0.1709 against 0.1690 ms, 5 interleaved pairs: profiles/r06_experiments).
// A ticket is closed by the record behind its K0 (chain_publish) or when its call gives it up (chain_drop: a call that failed
// between the two).  Call t used to go on without a wait when ticket t - M was taken but not closed -- its thread had not queued
// its K0 yet --, so that more than M K0s could be in flight; with M small against the calls in flight that race decided how many
// ran.  Now the host thread of t waits until that ticket is closed: the other thread is inside a kernel launch, microseconds,
// and waits for nothing in there (the wait is bounded all the same).  Tickets are handed out in order, so every ticket below
// `next` has been taken: the ticket counter is the slots' "taken" generation, gen / dropped are their "closed" ones.  A ticket is
// OPEN from the moment its call leaves chain_enter until it is closed.  Call t leaves only behind the record of t - M, so the
// open tickets of a residue class mod M are one at most, M in all: open_max (ps_gate_stats) says so.
struct K0Chain {
    static constexpr int RING = 64;
    std::mutex mu;
    std::condition_variable cv;                         // a ticket was closed
    hipEvent_t ev[RING] = {};
    unsigned long long gen[RING];                       // ticket whose K0 the event was last recorded behind (+1; 0: never)
    unsigned long long dropped[RING];                   // ticket last given up on the slot without a record (+1; 0: never)
    unsigned long long left[RING];                      // ticket whose call last left chain_enter on the slot (+1; 0: never)
    unsigned long long next = 0;
    bool made = false;
    long long open = 0, open_max = 0, host_waits = 0, gave_up = 0;     // ps_gate_stats
    bool closed(unsigned long long w) const { return gen[w % RING] == w + 1 || dropped[w % RING] == w + 1; }
    void close(unsigned long long t, bool recorded)
    {
        (recorded ? gen : dropped)[t % RING] = t + 1;
        if (left[t % RING] == t + 1) --open;
        cv.notify_all();
    }
};
K0Chain g_chain[16];
int chain_enter(ps_ctx *ctx, int device, int max_in_flight, hipStream_t st, unsigned long long *ticket)
{
    K0Chain &c = g_chain[device & 15];
    std::unique_lock<std::mutex> lk(c.mu);
    if (!c.made) {
        for (int i = 0; i < K0Chain::RING; ++i) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&c.ev[i], hipEventDisableTiming));
            c.gen[i] = c.dropped[i] = c.left[i] = 0;
        }
        c.made = true;
    }
    const unsigned long long t = c.next++;
    *ticket = t;
    const int m = std::max(1, std::min(max_in_flight, K0Chain::RING / 2));
    if (t >= static_cast<unsigned long long>(m)) {
        const unsigned long long w = t - static_cast<unsigned long long>(m);
        if (!c.closed(w)) {
            ++c.host_waits;
            // (bounded: a thread that died between its ticket and its record must not stop the device's other calls for good)
            if (!c.cv.wait_for(lk, std::chrono::milliseconds(200), [&] { return c.closed(w); })) ++c.gave_up;
        }
        if (c.gen[w % K0Chain::RING] == w + 1) {
            const hipError_t e = hipStreamWaitEvent(st, c.ev[w % K0Chain::RING], 0);
            if (e != hipSuccess) {
                c.close(t, false);
                return fail(ctx, PS_ERR_HIP, "hipStreamWaitEvent (K0 gate) failed: %s", hipGetErrorString(e));
            }
        }
    }
    c.left[t % K0Chain::RING] = t + 1;
    c.open_max = std::max(c.open_max, ++c.open);
    return PS_OK;
}
int chain_publish(ps_ctx *ctx, int device, hipStream_t st, unsigned long long ticket)     // K0 has been queued on st
{
    K0Chain &c = g_chain[device & 15];
    std::lock_guard<std::mutex> lk(c.mu);
    const hipError_t e = hipEventRecord(c.ev[ticket % K0Chain::RING], st);
    c.close(ticket, e == hipSuccess);
    if (e != hipSuccess) return fail(ctx, PS_ERR_HIP, "hipEventRecord (K0 gate) failed: %s", hipGetErrorString(e));
    return PS_OK;
}
// the call gives its ticket up (it failed between chain_enter and its record): whoever waits for it goes on without a wait
void chain_drop(ps_ctx *ctx)
{
    if (!ctx->chain_held) return;
    ctx->chain_held = false;
    K0Chain &c = g_chain[ctx->device & 15];
    std::lock_guard<std::mutex> lk(c.mu);
    c.close(ctx->chain_ticket, false);
}
// status word + work counters live in ctx->small: [0] status (u32, padded to 8), [1..3] work, [4] dense count
// (hdr: the stitch header lives behind the counters so that one copy brings both back)
// (SMALL_TAIL bytes behind it hold the per-event offsets of small batches, so that one copy brings everything back)
constexpr size_t SMALL_TAIL = 64 * 1024;
struct SmallLayout { unsigned long long status, work0, work1, work2, dense, stamp[12], life[9], qctl, qhead, tree_tail; AsmHeader hdr;
                     unsigned long long lat_ctl[6]; int lat_prog[LAT_D];        // (helpers of the look-ahead kernel, seg_device.hpp: LAT_D)
                     unsigned long long nt_cur;                                 // near-tie records of the call (DevCfg::nt_cur)
                     unsigned long long tree_defer[3]; };                       // tree_screen_kernel: [0] jobs on its deferred list (of the current round),
                                                                                // [1] windows it decided, [2] jobs it deferred (both over all rounds of the call)

int make_cfg(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int mw, int maxw, int W,
             double min_gain, DevCfg *c)
{
    // (every entry that queues work on the status block comes through here: whatever it is, the block is no longer known clean)
    ctx->small_clean_in = ctx->small_clean;
    ctx->small_clean = false;
    if (!fmt) return fail(ctx, PS_ERR_ARG, "sample format is NULL");
    if (fmt->dtype != PS_DTYPE_F32 && fmt->dtype != PS_DTYPE_I16)
        return fail(ctx, PS_ERR_ARG, "unknown dtype %d", fmt->dtype);
    if (!(fmt->quantum > 0) || !std::isfinite(fmt->quantum))
        return fail(ctx, PS_ERR_ARG, "quantum must be positive and finite");
    c->samples = d_samples;
    c->dtype = fmt->dtype;
    // (fp32 samples are absolute values: offset_counts is not added to them -- it names the level the caller subtracted
    //  upstream, include/poreseg.h)
    c->off_counts = fmt->dtype == PS_DTYPE_F32 ? 0 : fmt->offset_counts;
    c->dc_counts = fmt->dtype == PS_DTYPE_F32 ? static_cast<double>(fmt->offset_counts) : 0.0;
    c->noise_k = opt_noise_k(ctx->opt.noise_k_ppm);
    c->inv_q = static_cast<float>(1.0 / fmt->quantum);
    c->q = fmt->quantum;
    c->q2 = fmt->quantum * fmt->quantum;
    c->mw = mw; c->maxw = maxw; c->W = W; c->half = W / 2;
    c->min_gain = min_gain;
    c->mode = ctx->opt.mode;
    c->prune = ctx->opt.prune;
    c->lds_cap = std::max(1, std::min(W, ctx->lds_max_samples));
    c->bsum = nullptr; c->ev_info = nullptr; c->chunk_tot = nullptr; c->blk_mm = nullptr; c->grp = nullptr; c->bs_wide = 0;
    c->blk_cls = nullptr; c->cls_mm = nullptr; c->cls_kthr = 0;
    c->k0_unaligned = ctx->k0_unaligned;
    c->pre_c = nullptr; c->pre_c2 = nullptr;
    c->dbg = ctx->small.as<SmallLayout>()->stamp;
    c->nt_log = nullptr;
    c->rep_eval = ctx->opt.rep_eval; c->rep_stage = ctx->opt.rep_stage; c->rep_sum = ctx->opt.rep_sum;
    return PS_OK;
}

// dynamic LDS of the scan kernels: window samples (+ alignment slack) and the per-block sums of
// the pruned screen (one int2 per PBLK samples, at most one extra slot per thread)
inline size_t lds_bytes_for(int lds_cap, int nt)
{
    return (((static_cast<size_t>(lds_cap) + 32) * sizeof(lds_t) + 15) & ~static_cast<size_t>(15)) +
           (static_cast<size_t>(lds_cap) / PBLK + static_cast<size_t>(nt) + 8) * sizeof(int2);
}

// LDS budget: 160 KB per CU minus the static Shared block and a little slack
constexpr int LDS_BYTES_MAX = 160 * 1024 - static_cast<int>(sizeof(Shared)) - 512 - 64;

// Compute units of the context's device (queried once)
int cu_count(ps_ctx *ctx)
{
    if (ctx->n_cu <= 0) {
        hipDeviceProp_t prop;
        ctx->n_cu = hipGetDeviceProperties(&prop, ctx->device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    return ctx->n_cu;
}

// The sample type of a call, known at run time, as the compile-time DT of its kernels: f(std::integral_constant<int, DT>).
// FLAGS are the bits the call site decides at compile time (DT_WIDE): a site that serves both digests names each of them in a
// call of its own, so only the kernels that site launches are instantiated.
template <int FLAGS = 0, typename F> auto by_dtype(int dtype, F &&f)
{
    if (dtype == PS_DTYPE_F32) return f(std::integral_constant<int, PS_DTYPE_F32 | FLAGS>());
    return f(std::integral_constant<int, PS_DTYPE_I16 | FLAGS>());
}

// A workgroup width of the LDS-window kernels (options spine_nt / tree_nt) as the compile-time NT: the widths the call site
// lists are the ones its kernel is built for, the last of them serves every other value.
template <int NT0, int... NTS, typename F> int by_nt(int nt, F &&f)
{
    if constexpr (sizeof...(NTS) == 0) return f(std::integral_constant<int, NT0>());
    else return nt == NT0 ? f(std::integral_constant<int, NT0>()) : by_nt<NTS...>(nt, f);
}

// Resident workgroups of a kernel on this device (occupancy x CUs): the scan kernels are launched with one
// workgroup per slot and stride over their jobs.  The cache holds the device's workgroups per CU; slots_pct applies on
// every lookup, so a change of the option takes effect at the next launch.
template <typename K> unsigned resident_slots(ps_ctx *ctx, K kernel, int nt, size_t lds)
{
    const void *fn = reinterpret_cast<const void *>(kernel);
    int per_cu = -1;
    for (const auto &k : ctx->occ_cache)
        if (k.fn == fn && k.nt == nt && k.lds == lds) { per_cu = k.per_cu; break; }
    if (per_cu < 0) {
        cu_count(ctx);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, nt, lds) != hipSuccess || per_cu <= 0)
            per_cu = 1;
        if (ctx->opt.debug) fprintf(stderr, "[poreseg] occupancy: %d workgroups of %d threads per CU (dynamic LDS %zu), %d CUs\n", per_cu, nt, lds, ctx->n_cu);
        ctx->occ_cache.push_back({fn, nt, lds, per_cu});
    }
    unsigned slots = static_cast<unsigned>(per_cu) * static_cast<unsigned>(ctx->n_cu);
    const int pct = nt <= 256 ? ctx->opt.slots_pct : 100;
    slots = std::max(1u, static_cast<unsigned>(static_cast<unsigned long long>(slots) * static_cast<unsigned>(pct) / 100u));
    if (ctx->opt.debug) fprintf(stderr, "[poreseg] resident slots: %u (%d threads, dynamic LDS %zu, slots_pct %d)\n", slots, nt, lds, pct);
    return slots;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) only when the value changes (it is a driver call on every launch otherwise)
hipError_t set_dyn_lds(ps_ctx *ctx, const void *fn, int lds)
{
    for (auto &a : ctx->attr_cache)
        if (a.first == fn) {
            if (a.second == lds) return hipSuccess;
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e == hipSuccess) a.second = lds;
            return e;
        }
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) ctx->attr_cache.push_back({fn, lds});
    return e;
}

// Launch shape of a scan kernel: its dynamic LDS (with the attribute that allows it), the workgroups the device keeps resident
// and the grid -- one workgroup per slot, striding over its jobs, and no more workgroups than `want`.
struct ScanShape { size_t lds = 0; unsigned slots = 0, grid = 0; };
template <typename K> int scan_shape(ps_ctx *ctx, K kernel, int nt, size_t lds, unsigned want, ScanShape *s)
{
    HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), static_cast<int>(lds)));
    s->lds = lds;
    s->slots = resident_slots(ctx, kernel, nt, lds);
    s->grid = std::max(1u, std::min(want, s->slots));
    return PS_OK;
}
// ... of spine_kernel, bridge_kernel and tree_kernel: NT threads; the LDS-window widths hold the window's image, a single wave
// (block-sum scan) holds nothing (scan_lds_pad: diagnostics)
template <int NT, typename K> int scan_shape(ps_ctx *ctx, K kernel, const DevCfg &cfg, unsigned want, ScanShape *s)
{
    return scan_shape(ctx, kernel, NT, NT == 64 ? static_cast<size_t>(ctx->opt.scan_lds_pad) : lds_bytes_for(cfg.lds_cap, NT), want, s);
}

template <int NT, int DT> int launch_spine(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, bool list_mode = false)
{
    ScanShape s;
    if (int rc = scan_shape<NT>(ctx, spine_kernel<NT, DT>, cfg, nj, &s)) return rc;
    hipLaunchKernelGGL((spine_kernel<NT, DT>), dim3(s.grid), dim3(NT), s.lds, ctx->stream, cfg,
                       ctx->spine_jobs.as<SpineJob>(), ctx->spine_scratch.as<int2>(),
                       list_mode ? nullptr : ctx->spine_dense.as<int2>(), ctx->spine_meta.as<int4>(), &sm->dense, reinterpret_cast<unsigned *>(&sm->status), &sm->work0,
                       static_cast<int>(nj));
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

template <int NT, int DT> int launch_tree(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, size_t n_jobs,
                                          const AsmHeader *d_hdr, int par_max_jobs = 0, bool screened = false)
{
    ScanShape s;
    if (int rc = scan_shape<NT>(ctx, tree_kernel<NT, DT>, cfg, nj, &s)) return rc;
    hipLaunchKernelGGL((tree_kernel<NT, DT>), dim3(s.grid), dim3(NT), s.lds, ctx->stream, cfg,
                       ctx->tree_jobs.as<TreeJob>(), ctx->tree_scratch.as<int32_t>(), ctx->tree_spill.as<int2>(),
                       ctx->tree_counts.as<int32_t>(), reinterpret_cast<unsigned *>(&sm->status), &sm->work0,
                       static_cast<long long>(n_jobs), d_hdr,
                       // (not on the 64-bit digest: those are filtered events, whose jobs hold many windows each -- 32 of them:
                       //  subtree kernel 1.30 ms on all slots, 1.71 ms with the rule)
                       NT == 64 && !(DT & DT_WIDE) ? ctx->opt.tree_jobs_per_wave : 0, par_max_jobs,
                       screened ? ctx->tree_defer.as<int2>() : nullptr, screened ? sm->tree_defer : nullptr,
                       screened ? ctx->screen_acc.as<unsigned long long>() : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

// Narrow digest: the screen in front of the subtree kernel (seg_device.hpp: tree_screen_kernel) -- single-wave workgroups without
// LDS, one per resident slot, striding over the jobs; the subtree kernel behind it walks the deferred list.
template <int DT> int launch_tree_screened(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, size_t n_jobs,
                                           const AsmHeader *d_hdr)
{
    ScanShape s;
    if (int rc = scan_shape(ctx, tree_screen_kernel<DT>, 64, 0, nj, &s)) return rc;
    hipLaunchKernelGGL((tree_screen_kernel<DT>), dim3(s.grid), dim3(64), 0, ctx->stream, cfg, ctx->tree_jobs.as<TreeJob>(),
                       ctx->tree_defer.as<int2>(), sm->tree_defer, ctx->screen_acc.as<unsigned long long>(),
                       static_cast<long long>(n_jobs), d_hdr);
    HIP_TRY(ctx, hipGetLastError());
    ctx->screen_ran = true;
    const int rc = launch_tree<64, DT>(ctx, cfg, nj, sm, n_jobs, d_hdr, 0, true);
    // (screen_acc is zero between calls because the subtree kernel clears what it collects: if that kernel was not launched,
    //  what the screen's waves left there must not reach the next call's counters)
    if (rc != PS_OK) (void)hipMemsetAsync(ctx->screen_acc.p, 0, ctx->screen_acc.cap, ctx->stream);
    return rc;
}

// LDS-window scan: the spine kernel at the option's width (spine_nt)
int launch_spine_nt(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, bool list_mode)
{
    return by_nt<256, 512, 1024>(ctx->opt.spine_nt, [&](auto nt) {
        return by_dtype(cfg.dtype, [&](auto dt) { return launch_spine<decltype(nt)::value, dt()>(ctx, cfg, nj, sm, list_mode); });
    });
}

// block-sum scan, TREE_W waves per workgroup sharing the workgroup's job list (tree_mw_kernel)
template <int DT> int launch_tree_mw(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, size_t n_jobs,
                                     const AsmHeader *d_hdr)
{
    ScanShape s;
    if (int rc = scan_shape(ctx, tree_mw_kernel<DT>, 64 * TREE_W, sizeof(SharedT<64>) * TREE_W, (nj + TREE_W - 1) / TREE_W, &s)) return rc;
    hipLaunchKernelGGL((tree_mw_kernel<DT>), dim3(s.grid), dim3(64 * TREE_W), s.lds, ctx->stream, cfg,
                       ctx->tree_jobs.as<TreeJob>(), ctx->tree_scratch.as<int32_t>(), ctx->tree_spill.as<int2>(),
                       ctx->tree_counts.as<int32_t>(), reinterpret_cast<unsigned *>(&sm->status), &sm->work0,
                       static_cast<long long>(n_jobs), d_hdr, &sm->tree_tail, ctx->opt.tree_tail_pct);
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

// deep jobs (filtered events on the 64-bit digest): the PAR_W waves of a workgroup share one job (tree_par_kernel)
template <int DT> int launch_tree_par(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, size_t n_jobs,
                                      const AsmHeader *d_hdr)
{
    ScanShape s;
    if (int rc = scan_shape(ctx, tree_par_kernel<DT>, 64 * PAR_W, sizeof(SharedT<64>) * PAR_W + sizeof(ParQ), nj, &s)) return rc;
    // calls with at most one job per workgroup slot are this kernel's; the others go to tree_kernel (decided on the device,
    // where the job count is known: both are launched, one of them returns at once)
    const int par_max = static_cast<int>(s.slots);
    hipLaunchKernelGGL((tree_par_kernel<DT>), dim3(s.grid), dim3(64 * PAR_W), s.lds, ctx->stream, cfg,
                       ctx->tree_jobs.as<TreeJob>(), ctx->tree_scratch.as<int32_t>(), ctx->tree_spill.as<int2>(),
                       ctx->tree_counts.as<int32_t>(), reinterpret_cast<unsigned *>(&sm->status), &sm->work0,
                       static_cast<long long>(n_jobs), d_hdr, par_max);
    HIP_TRY(ctx, hipGetLastError());
    return launch_tree<64, DT>(ctx, cfg, nj, sm, n_jobs, d_hdr, par_max);
}

// Phase 3: which kernel takes the call's subtree jobs.  On the 64-bit digest (filtered events: deep recursions) tree_par, then
// tree_mw, then one wave per job; on the 32-bit digest tree_mw, then one wave per job; without a digest the LDS-window kernel
// at the option's width (tree_nt).
int launch_subtrees(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm, size_t n_jobs, const AsmHeader *d_hdr)
{
    if (cfg.bsum != nullptr && cfg.bs_wide) {
        if (ctx->opt.tree_par) return by_dtype<DT_WIDE>(cfg.dtype, [&](auto dt) { return launch_tree_par<dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
        if (ctx->opt.tree_mw) return by_dtype<DT_WIDE>(cfg.dtype, [&](auto dt) { return launch_tree_mw<dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
        return by_dtype<DT_WIDE>(cfg.dtype, [&](auto dt) { return launch_tree<64, dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
    }
    if (cfg.bsum != nullptr) {
        if (ctx->opt.tree_mw) return by_dtype(cfg.dtype, [&](auto dt) { return launch_tree_mw<dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
#ifndef PS_STAMP
        // the screen proves windows empty from the group records, in the product's mode only: without them (option groups 0,
        // prune 0) it could decide nothing, and verify mode checks every window of the full scan
        // (reserve_items sizes the screen's buffers with the job buffers; a caller whose jobs did not come through it gets the
        //  subtree kernel alone, which computes the same)
        const bool reserved = ctx->tree_defer.cap >= n_jobs * sizeof(int2) &&
                              ctx->screen_acc.cap >= static_cast<size_t>(SCREEN_ACC) * SCREEN_ACC_STRIDE * sizeof(unsigned long long);
        if (ctx->opt.tree_screen && reserved && cfg.mode == MODE_FAST && cfg.grp != nullptr && cfg.prune) {
            return by_dtype(cfg.dtype, [&](auto dt) { return launch_tree_screened<dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
        }
#endif
        return by_dtype(cfg.dtype, [&](auto dt) { return launch_tree<64, dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
    }
    return by_nt<512, 256>(ctx->opt.tree_nt, [&](auto nt) {
        return by_dtype(cfg.dtype, [&](auto dt) { return launch_tree<decltype(nt)::value, dt()>(ctx, cfg, nj, sm, n_jobs, d_hdr); });
    });
}

int check_status(ps_ctx *ctx, unsigned st)
{
    if (st & ST_OFF_GRID)
        return fail(ctx, PS_ERR_OFF_GRID, "fp32 sample is not an integer multiple of quantum (or |count| >= 2^23)");
    if (st & ST_VERIFY_MISMATCH) {
        const SmallLayout *h = ctx->h_small.as<SmallLayout>();
        return fail(ctx, PS_ERR_INTERNAL, "verify mode: fp32 screen disagreed with the exact scan (window [%lld,%lld): screen %lld, exact %lld)",
                    static_cast<long long>(h->stamp[4]), static_cast<long long>(h->stamp[5]), static_cast<long long>(h->stamp[6]), static_cast<long long>(h->stamp[7]));
    }
    if (st & ST_STACK_OVERFLOW) return fail(ctx, PS_ERR_INTERNAL, "device DFS stack overflow");
    if (st & ST_OUT_OVERFLOW) return fail(ctx, PS_ERR_INTERNAL, "device scratch overflow");
    return PS_OK;
}


// Runs spine_kernel over `jobs`, returns the per-tile anchor lists.
int run_spines(ps_ctx *ctx, const DevCfg &cfg, const std::vector<SpineJob> &jobs, int64_t scratch_entries,
               std::vector<TileList> &out)
{
    const size_t nj = jobs.size();
    out.assign(nj, TileList());
    if (nj == 0) return PS_OK;
    HIP_TRY(ctx, ctx->spine_jobs.reserve(nj * sizeof(SpineJob)));
    HIP_TRY(ctx, ctx->spine_scratch.reserve(static_cast<size_t>(scratch_entries) * sizeof(int2)));
    HIP_TRY(ctx, ctx->spine_dense.reserve(static_cast<size_t>(scratch_entries) * sizeof(int2)));
    HIP_TRY(ctx, ctx->spine_meta.reserve(nj * sizeof(int4)));
    HIP_TRY(ctx, ctx->h_up.reserve(nj * sizeof(SpineJob)));
    std::memcpy(ctx->h_up.p, jobs.data(), nj * sizeof(SpineJob));
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->spine_jobs.p, ctx->h_up.p, nj * sizeof(SpineJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(&sm->dense, 0, sizeof(unsigned long long), ctx->stream));
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    if (int lrc = launch_spine_nt(ctx, cfg, static_cast<unsigned>(nj), sm, false)) return lrc;
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(ctx, ctx->h_meta.reserve(nj * sizeof(int4)));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->spine_meta.p, nj * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const SmallLayout hs = *ctx->h_small.as<SmallLayout>();
    int rc = check_status(ctx, static_cast<unsigned>(hs.status));
    if (rc) return rc;
    const size_t total = static_cast<size_t>(hs.dense);
    if (total) {
        HIP_TRY(ctx, ctx->h_dense.reserve(total * sizeof(int2)));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_dense.p, ctx->spine_dense.p, total * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    float ms = 0;
    if (ctx->opt.timing >= 2 && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->ms[PS_MS_SPINE] += ms;
    const int4 *meta = ctx->h_meta.as<int4>();
    const int2 *dense = ctx->h_dense.as<int2>();
    for (size_t j = 0; j < nj; ++j) {
        TileList &t = out[j];
        t.start = jobs[j].start;
        t.ended = meta[j].y != 0;
        t.a.resize(static_cast<size_t>(meta[j].x));
        for (int i = 0; i < meta[j].x; ++i) {
            t.a[i].pos = dense[meta[j].z + i].x;
            t.a[i].kind = dense[meta[j].z + i].y;
        }
    }
    return PS_OK;
}

}  // namespace

namespace {
constexpr int RC_FALLBACK = 1;      // internal: the device stitch gave up, use the host-stitch pipeline
constexpr int RC_WIDE = 2;          // internal: counts too wide for the block sums, use the LDS-window scan
// What a batch call works on and where its results go, the same on every route it may be redone on
struct SegBatch {
    const int64_t *ev_start, *ev_len;
    int32_t n_ev;
    int mw, W;
    int32_t *d_bounds;
    int64_t cap;
    int64_t *h_bounds_off;
    ps_segstat *d_stats;
    std::chrono::steady_clock::time_point t_begin;
};
// The work counters of a call that came through, from the status block it brought back (ps_get_timings; with PS_STAMP: the
// phase stamps on stderr)
void read_call_counters(ps_ctx *ctx, const DevCfg &cfg, const SmallLayout &hs)
{
    ctx->counters[PS_CNT_WINDOWS] = static_cast<int64_t>(hs.work0);
    ctx->counters[PS_CNT_CANDIDATES] = static_cast<int64_t>(hs.work1);
    ctx->counters[PS_CNT_EXACT_RESCANS] = static_cast<int64_t>(hs.work2 & 0xffffffffULL) + static_cast<int64_t>(hs.work2 >> 32);   // exact decisions
    ctx->counters[PS_CNT_FULL_EXACT_SCANS] = static_cast<int64_t>(hs.work2 >> 32);                                                   // of which full fp64 window scans (block-sum scan)
#ifndef PS_STAMP
    for (int k = 0; k < 3; ++k) ctx->counters[PS_CNT_WINDOWS_SPINE + k] = static_cast<int64_t>(hs.life[3 * k + 1]);              // window scans of the spine / bridge / subtree kernels
    // near-tie decisions (seg_bs.hpp: bs_decide); -1: not counted -- the call ran on the LDS-window kernels, which decide every window
    // by one fp64 scan and keep no margins (a caller that redoes near ties on the exact route redoes such a call)
    ctx->counters[PS_CNT_NEAR_TIES] = cfg.bsum ? static_cast<int64_t>(hs.stamp[0]) : -1;
    // ... and their records (ps_get_near_ties): the cursor came back with the status block
    ctx->nt.seen = cfg.bsum && cfg.nt_log ? static_cast<int64_t>(hs.nt_cur) : -1;
#else
    ctx->nt.seen = -1;                                 // (the stamps take the near-tie count's words: not counted)
#endif
    ctx->counters[PS_CNT_TREE_DEFERRED] = ctx->screen_ran ? static_cast<int64_t>(hs.tree_defer[2]) : -1;                         // subtree jobs the screen deferred
    ctx->counters[PS_CNT_WINDOWS_SCREEN] = ctx->screen_ran ? static_cast<int64_t>(hs.tree_defer[1]) : -1;                         // windows the screen decided
    ctx->counters[PS_CNT_HELPER_CHUNKS_PUBLISHED] = static_cast<int64_t>(hs.lat_ctl[4]);                                                   // look-ahead helpers: chunk results published
    ctx->counters[PS_CNT_HELPER_CHUNKS_TAKEN] = static_cast<int64_t>(hs.lat_ctl[5]);                                                   // ... and taken by an owner instead of scanning
#ifdef PS_STAMP
    {
        static const char *nm[12] = {"level", "sweep", "drain", "decide", "contend", "setup", "exact", "outside", "-", "-", "-", "-"};
        unsigned long long tot = 0;
        for (int i = 0; i < 8; ++i) tot += hs.stamp[i];
        fprintf(stderr, "[poreseg stamps] lane-0 cycles summed over waves (spine+bridge+tree):");
        for (int i = 0; i < 8; ++i) fprintf(stderr, " %s=%.1f%%", nm[i], 100.0 * hs.stamp[i] / (tot ? tot : 1));
        fprintf(stderr, " total=%llu cycles, windows=%llu -> %.0f cycles/window\n", tot, hs.work0, (double)tot / (hs.work0 ? hs.work0 : 1));
        fprintf(stderr, "[poreseg stamps] rows swept %llu, non-empty drains %llu, blocks drained %llu, hit-like windows %llu\n",
                hs.stamp[8], hs.stamp[9], hs.stamp[10], hs.stamp[11]);
        fprintf(stderr, "[poreseg stamps] blocks queued although not prunable (first block of a window, variance floor): %llu\n", hs.stamp[6]);
        for (int k = 0; k < 3; ++k)
            fprintf(stderr, "[poreseg stamps] %s: longest workgroup %llu cycles, windows %llu, sum of lifetimes %llu cycles\n",
                    k == 0 ? "spine" : k == 1 ? "bridge" : "tree", hs.life[3 * k], hs.life[3 * k + 1], hs.life[3 * k + 2]);
    }
#endif
}

// Option debug: says on stderr which seams of a failed device stitch gave up (their records are fetched for this alone)
void report_failed_seams(ps_ctx *ctx)
{
    const size_t nt = static_cast<size_t>(ctx->counters[PS_CNT_TILES]);
    std::vector<int4> bm(nt), mt(nt);
    std::vector<SpineJob> jb(nt);
    if (!nt || hipMemcpy(bm.data(), ctx->bmeta.p, nt * sizeof(int4), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(mt.data(), ctx->spine_meta.p, nt * sizeof(int4), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(jb.data(), ctx->spine_jobs.p, nt * sizeof(SpineJob), hipMemcpyDeviceToHost) != hipSuccess)
        return;
    int shown = 0;
    size_t n_open = 0, n_gave_up = 0, n_defer = 0;
    for (size_t g = 0; g < nt; ++g) {
        if (bm[g].w == BR_DEFER || bm[g].w == BR_DEFER_REACHED) ++n_defer;
        else if (bm[g].w == BR_FAIL && mt[g].x == 0 && bm[g].x == 0) ++n_open;
        else if (bm[g].w == BR_FAIL) ++n_gave_up;
    }
    fprintf(stderr, "[poreseg] stitch failed: %zu tiles; bridges that gave up after anchors of their own %zu, open tiles not bridged %zu, deferred and not finished %zu\n",
            nt, n_gave_up, n_open, n_defer);
    for (size_t g = 0; g < nt && shown < 6; ++g)
        if ((bm[g].w == BR_FAIL && !(mt[g].x == 0 && bm[g].x == 0)) || bm[g].w == BR_DEFER || bm[g].w == BR_DEFER_REACHED) {
            fprintf(stderr, "[poreseg] stitch failed: tile %zu (event %d, tile %zu of %d, [%d, %d) of %d) bridge status %d after %d anchors (next window %d); its own list: %d anchors, ended %d, open at %d\n",
                    g, jb[g].ev, g - static_cast<size_t>(jb[g].first_tile), jb[g].ntiles, jb[g].start, jb[g].stop, jb[g].end,
                    bm[g].w, bm[g].x, bm[g].y, mt[g].x, mt[g].y, mt[g].z);
            ++shown;
        }
}

// The gather: every true anchor behind the boundaries of its left subtree, per-event offsets -- one kernel that places its items
// from per-256-job count sums (device stitch, gather_fused), else the item scan and the gather of rounds 2-5
int queue_gather(ps_ctx *ctx, const SegBatch &B, int64_t n_items, const AsmHeader *d_hdr, bool fused)
{
    const int32_t n_ev = B.n_ev;
    int32_t *const d_bounds = B.d_bounds;
    const int64_t cap = B.cap;
    if (fused) {
        const int64_t blocks = (n_items >> GS_LOG) + 1;
        const unsigned gg = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(blocks, 1024)));
        hipLaunchKernelGGL(gather_scan_kernel, dim3(gg), dim3(1 << GS_LOG), 0, ctx->stream, ctx->items.as<Item>(),
                           ctx->tree_jobs.as<TreeJob>(), ctx->tree_counts.as<int32_t>(), ctx->tree_scratch.as<int32_t>(),
                           static_cast<long long>(n_items), d_bounds, cap, ctx->d_is_spine, d_hdr, ctx->first_item.as<int64_t>(),
                           n_ev, ctx->bounds_off.as<int64_t>());
        HIP_TRY(ctx, hipGetLastError());
    } else {
    hipLaunchKernelGGL(item_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, ctx->items.as<Item>(),
                       ctx->tree_counts.as<int32_t>(), n_items, ctx->item_pos.as<int64_t>(), d_hdr,
                       ctx->first_item.as<int64_t>(), n_ev, ctx->bounds_off.as<int64_t>());
    HIP_TRY(ctx, hipGetLastError());
    }
    if (n_items && !fused) {
        const unsigned gg = static_cast<unsigned>(d_hdr ? std::min<int64_t>(n_items, 16384) : n_items);
        hipLaunchKernelGGL(gather_kernel, dim3(gg), dim3(64), 0, ctx->stream,
                           ctx->items.as<Item>(), ctx->tree_jobs.as<TreeJob>(), ctx->tree_counts.as<int32_t>(),
                           ctx->tree_scratch.as<int32_t>(), ctx->item_pos.as<int64_t>(), n_items, d_bounds, cap, ctx->d_is_spine,
                           d_hdr);
        HIP_TRY(ctx, hipGetLastError());
    }
    return PS_OK;
}

// Status block and per-event offsets go back to the host: in one piece where the offsets ride behind the block (one_copy) -- by
// download_kernel into pinned memory, which may leave the block zero behind it (may_clear, option short_chain; *dl_clear: the
// words it clears), or by a plain copy -- else by two copies
int queue_download(ps_ctx *ctx, size_t evb, bool one_copy, bool may_clear, int *dl_clear)
{
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    if (one_copy) {
        HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout) + evb));
        void *h_dev = nullptr;                         // the pinned block as the device sees it (else: plain copy)
        if (ctx->opt.download_by_kernel && hipHostGetDevicePointer(&h_dev, ctx->h_small.p, 0) != hipSuccess) { h_dev = nullptr; (void)hipGetLastError(); }
        if (h_dev) {
            static_assert(sizeof(SmallLayout) % 8 == 0, "the status block is copied in 8-byte words");
            const long long nw = static_cast<long long>((sizeof(SmallLayout) + evb) / 8);
            // (a call without statistics on the screened route, see short_route: the calls the option was measured on)
            if (may_clear && ctx->screen_ran && (opt_short_chain_bits(ctx->opt.short_chain) & SC_NO_UPLOAD)) *dl_clear = static_cast<int>(sizeof(SmallLayout) / 8);
            hipLaunchKernelGGL(download_kernel, dim3(static_cast<unsigned>(std::min<long long>((nw + 255) / 256, 64))), dim3(256), 0, ctx->stream,
                               ctx->small.as<unsigned long long>(), static_cast<unsigned long long *>(h_dev), nw, *dl_clear, &sm->hdr.fail);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout) + evb, hipMemcpyDeviceToHost, ctx->stream));
        }
    } else {
        HIP_TRY(ctx, ctx->h_meta.reserve(evb));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->bounds_off.p, evb, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    }
    return PS_OK;
}

// Phase 3 onwards.  Expects tree_jobs / items / first_item / ev_off populated on the device.
// d_hdr == nullptr: n_tj / n_items are the exact counts (host stitch).  Otherwise they are upper bounds used
// to size the launches and the kernels read the counts from *d_hdr on the device; the header and the status
// word are then checked after the single synchronisation at the end (*hdr_out receives the header).
int finish_batch(ps_ctx *ctx, const DevCfg &cfg, const SegBatch &B, size_t n_tj, int64_t n_items, const AsmHeader *d_hdr = nullptr,
                 AsmHeader *hdr_out = nullptr, bool wide_check = false)
{
    const int32_t n_ev = B.n_ev;
    int32_t *const d_bounds = B.d_bounds;
    const int64_t cap = B.cap;
    int64_t *const h_bounds_off = B.h_bounds_off;
    ps_segstat *const d_stats = B.d_stats;
    int rc;
    const size_t evb = (static_cast<size_t>(n_ev) + 1) * sizeof(int64_t);
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    if (n_tj) {
        const unsigned g = static_cast<unsigned>(std::min<size_t>(n_tj, 0x7fffffff));
        if (int lrc = launch_subtrees(ctx, cfg, g, sm, n_tj, d_hdr)) return lrc;
    }
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    const bool fused = d_hdr != nullptr && ctx->opt.gather_fused;      // (device stitch: job index == item index)
    const bool one_copy = ctx->bounds_off.p == ctx->small.as<char>() + sizeof(SmallLayout);
    int dl_clear = 0;                                  // (option short_chain: the download kernel leaves the status block zero behind its copy)
    if (int grc = queue_gather(ctx, B, n_items, d_hdr, fused)) return grc;
    const bool stats_from_digest = d_stats != nullptr && cfg.bsum != nullptr && cfg.blk_mm != nullptr;
    if (stats_from_digest) {
        // K2 from the K0 digest: launched before the sync, the segment count is read on the device
        const int64_t scap = cap + n_ev;
        const unsigned sg = static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(scap, 1), 8192));
        by_dtype(cfg.dtype, [&](auto dt) {
            hipLaunchKernelGGL(segstat_bs_kernel<dt()>, dim3(sg), dim3(64), 0, ctx->stream, cfg, ctx->ev_off.as<int64_t>(),
                               ctx->ev_len.as<int64_t>(), n_ev, d_bounds, ctx->bounds_off.as<int64_t>(), d_stats, scap,
                               reinterpret_cast<unsigned *>(&sm->status), d_hdr);
        });
        HIP_TRY(ctx, hipGetLastError());
        if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
    }
    if (int drc = queue_download(ctx, evb, one_copy, fused && d_stats == nullptr, &dl_clear)) return drc;
    if (ctx->opt.timing >= 1) HIP_TRY(ctx, hipEventRecord(ctx->ev[9], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    {
        float seq = 0;                                 // the call's device work, upload to result copies, by HIP events
        if (ctx->opt.timing >= 1 && hipEventElapsedTime(&seq, ctx->ev[8], ctx->ev[9]) == hipSuccess) ctx->ms[PS_MS_SEQ] = seq;
    }
    std::memcpy(h_bounds_off, one_copy ? ctx->h_small.as<char>() + sizeof(SmallLayout) : ctx->h_meta.as<char>(), evb);
    const SmallLayout hs = *ctx->h_small.as<SmallLayout>();
    if (wide_check && (static_cast<unsigned>(hs.status) & ST_WIDE_RANGE)) return RC_WIDE;    // counts too wide for the block sums
    rc = check_status(ctx, static_cast<unsigned>(hs.status));
    if (rc) return rc;
    if (d_hdr) {
        const AsmHeader hd = hs.hdr;
        if (hdr_out) *hdr_out = hd;
        if (hd.fail) {
            if (ctx->opt.debug) report_failed_seams(ctx);
            return RC_FALLBACK;
        }
    }
    read_call_counters(ctx, cfg, hs);
    const int64_t total = h_bounds_off[n_ev];
    if (total > cap)
        return fail(ctx, PS_ERR_CAPACITY, "bounds capacity %lld < required %lld", static_cast<long long>(cap),
                    static_cast<long long>(total));
    if (d_stats && !stats_from_digest) {
        const int64_t nseg = total + n_ev;
        if (nseg > 0) {
            by_dtype(cfg.dtype, [&](auto dt) {
                hipLaunchKernelGGL(segstat_kernel<dt()>, dim3(static_cast<unsigned>(nseg)), dim3(STAT_NT), 0,
                                   ctx->stream, cfg, ctx->ev_off.as<int64_t>(), ctx->ev_len.as<int64_t>(), n_ev, d_bounds,
                                   ctx->bounds_off.as<int64_t>(), d_stats, reinterpret_cast<unsigned *>(&sm->status));
            });
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    if (!stats_from_digest) {
        if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    float ms = 0;
    if (ctx->opt.timing >= 2 && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->ms[PS_MS_TREE] = ms;
    if (ctx->opt.timing >= 2 && hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4]) == hipSuccess) ctx->ms[PS_MS_GATHER] = ms;
    ctx->ms[PS_MS_TOTAL] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - B.t_begin).count();
    ctx->small_clean = dl_clear > 0;                   // (the copy of a call that came through left the status block zero)
    return PS_OK;
}


// The helpers' shared state for this call (none when switched off, or not the block-sum pipeline)
LatHelp lat_help_of(ps_ctx *ctx, const DevCfg &cfg, SmallLayout *sm)
{
    if (!ctx->opt.lat_help || cfg.bsum == nullptr || !ctx->lat_res.p) return LAT_NONE;
    LatHelp h;
    h.ctl = sm->lat_ctl;
    h.state = ctx->lat_state.as<unsigned long long>();
    h.seam = ctx->lat_seam.as<int>();
    h.prog = sm->lat_prog;
    h.res = ctx->lat_res.as<unsigned long long>();
    h.tag_base = ctx->lat_tag_base;
    h.stay = ctx->opt.lat_help == 2 ? 1 : 0;
    return h;
}

template <int DT> int launch_bridge_la(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm)
{
    const unsigned grid = std::min(nj, resident_slots(ctx, bridge_la_kernel<DT>, 64 * BR_LA, 0));
    hipLaunchKernelGGL((bridge_la_kernel<DT>), dim3(grid), dim3(64 * BR_LA), 0, ctx->stream, cfg,
                       ctx->spine_jobs.as<SpineJob>(), ctx->spine_scratch.as<int2>(), ctx->spine_meta.as<int4>(),
                       ctx->bridges.as<int2>(), ctx->bmeta.as<int4>(), reinterpret_cast<unsigned *>(&sm->status),
                       &sm->work0, static_cast<int>(nj), nullptr, nullptr, nullptr, 0, ctx->opt.bridge_budget, static_cast<int>(EXT_MAX),
                       lat_help_of(ctx, cfg, sm));
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

// Option short_chain applies on the route of the screened subtrees only -- the 32-bit digest in the product's mode with
// tree_screen 1 (launch_subtrees) -- and leaves every other route its launches, one for one.
bool short_route(const ps_ctx *ctx, const DevCfg &cfg)
{
    return cfg.bsum != nullptr && !cfg.bs_wide && !ctx->opt.tree_mw && ctx->opt.tree_screen && cfg.mode == MODE_FAST && cfg.grp != nullptr && cfg.prune;
}
// (a pooled call on that route issues no look-ahead launch: its bridges keep walking in their own wave)
bool no_look_ahead(const ps_ctx *ctx, const DevCfg &cfg)
{
    return (opt_short_chain_bits(ctx->opt.short_chain) & SC_NO_LA) != 0 && ctx->opt.shared_device > 1 && ctx->opt.bridge_ext && !ctx->la_now && short_route(ctx, cfg);
}

template <int NT, int DT> int launch_bridge(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm)
{
    ScanShape s;
    if (int rc = scan_shape<NT>(ctx, bridge_kernel<NT, DT>, cfg, nj, &s)) return rc;
    hipLaunchKernelGGL((bridge_kernel<NT, DT>), dim3(s.grid), dim3(NT), s.lds, ctx->stream, cfg,
                       ctx->spine_jobs.as<SpineJob>(), ctx->spine_scratch.as<int2>(), ctx->spine_meta.as<int4>(),
                       ctx->bridges.as<int2>(), ctx->bmeta.as<int4>(), reinterpret_cast<unsigned *>(&sm->status),
                       &sm->work0, static_cast<int>(nj), ctx->opt.bridge_single, ctx->opt.bridge_budget,
                       NT == 64 ? lat_help_of(ctx, cfg, sm) : LAT_NONE,
                       no_look_ahead(ctx, cfg) ? ctx->opt.bridge_patience : static_cast<int>(BR_PATIENCE));
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

// Every segment call (and every redo of one on another route) starts its timings and work counters from zero
void reset_call_stats(ps_ctx *ctx)
{
    for (double &m : ctx->ms) m = 0;
    for (int64_t &c : ctx->counters) c = 0;
    ctx->counters[PS_CNT_TREE_DEFERRED] = ctx->counters[PS_CNT_WINDOWS_SCREEN] = -1;
    ctx->screen_ran = false;
}

// The buffers sized by the items of a call -- true spine anchors, one subtree job each at most -- for up to items_cap of them
// (the first sizing of the device stitch, and again when a second-chance round makes room for the anchors it may add)
int reserve_items(ps_ctx *ctx, int64_t items_cap, int64_t total_len, int mw)
{
    const size_t n = static_cast<size_t>(std::max<int64_t>(1, items_cap));
    const size_t tscratch_bound = static_cast<size_t>(total_len / mw + items_cap + 1);     // tree output regions: (base+pred)/mw + item
    HIP_TRY(ctx, ctx->spine_items.reserve(n * sizeof(int4)));
    HIP_TRY(ctx, ctx->tree_jobs.reserve(n * sizeof(TreeJob)));
    HIP_TRY(ctx, ctx->tree_counts.reserve((n + (static_cast<size_t>(items_cap) >> GS_LOG) + 2) * sizeof(int32_t)));   // (+ the sums per 256 jobs: gather_scan_kernel)
    HIP_TRY(ctx, ctx->items.reserve(n * sizeof(Item)));
    HIP_TRY(ctx, ctx->item_pos.reserve((static_cast<size_t>(items_cap) + 1) * sizeof(int64_t)));
    HIP_TRY(ctx, ctx->tree_scratch.reserve(tscratch_bound * sizeof(int32_t)));
    HIP_TRY(ctx, ctx->tree_spill.reserve(tscratch_bound * sizeof(int2)));
    if (ctx->opt.tree_screen) {
        HIP_TRY(ctx, ctx->tree_defer.reserve(n * sizeof(int2)));                       // the screen's deferred list: at most every job
        // ... and where its waves leave their window counts.  Invariant: all zero between calls -- zeroed here when allocated,
        // and the subtree kernel launched behind the screen clears every line it collects (launch_tree_screened clears them
        // itself if that launch fails)
        HIP_TRY(ctx, ctx->screen_acc.reserve_zeroed(static_cast<size_t>(SCREEN_ACC) * SCREEN_ACC_STRIDE * sizeof(unsigned long long), ctx->stream));
    }
    return PS_OK;
}

// K0's digest of nb_pad blocks (k0_padded_blocks: a wave of K0 takes 256 blocks, the arrays are padded to whole waves, +1: the
// end boundary) of n_ev events: block sums, the events' centres, totals + max|k| per chunk.  The caller says what it wants beside
// them: the 64-bit digest, the group records of the coarse pass, per-block min / max for the statistics kernel, the detector's
// verdict per block (ps_detect_segment_trace).
struct DigestWant { bool wide = false, grp = false, blk_mm = false, cls = false; };
int reserve_digest(ps_ctx *ctx, int64_t nb_pad, int32_t n_ev, const DigestWant &want)
{
    const size_t nb = static_cast<size_t>(nb_pad);
    // (at least 16 KB: a wave block of K0's general route fetches -- and ignores -- the head of this buffer, seg_bs.hpp)
    HIP_TRY(ctx, ctx->bsum.reserve(std::max<size_t>(16384, nb * (want.wide ? sizeof(int4) : sizeof(uint2)))));
    HIP_TRY(ctx, ctx->ev_info.reserve(static_cast<size_t>(std::max(1, n_ev)) * sizeof(int4)));
    HIP_TRY(ctx, ctx->chunk_mabs.reserve(static_cast<size_t>(nb_pad / BS_CHUNK + 1) * (want.wide ? 2 : 1) * sizeof(int4)));
    // group records of the coarse pass (16 B per 32 blocks; +1: the end boundary's)
    if (want.grp) HIP_TRY(ctx, ctx->grp.reserve(static_cast<size_t>(nb_pad / BS_GRP + 1) * sizeof(uint4)));
    // per-block min/max for the statistics kernel (4 B per block; int16 pairs)
    if (want.blk_mm) HIP_TRY(ctx, ctx->blk_mm.reserve(nb * sizeof(int)));
    // K0's verdict per block against the detector's threshold (2 bits), min / max per 128 blocks
    if (want.cls) {
        HIP_TRY(ctx, ctx->blk_cls.reserve(static_cast<size_t>(nb_pad / 4 + 64)));
        HIP_TRY(ctx, ctx->cls_mm.reserve(static_cast<size_t>(nb_pad / BS_CHUNK + 2) * sizeof(int2)));
    }
    return PS_OK;
}

// One call's K0: the event tables on the device, and what differs between the routes that launch it.
struct K0Call {
    const int64_t *ev_start, *ev_len, *ev_boff;
    int32_t n_ev;
    int64_t n_samples, nb_pad;
    bool persistent = true;   // false: one wave per wave block whatever k0_waves says (ps_audit_bounds)
    bool admit = false;       // the call takes a ticket of the device's K0 chain (k0_admit) in front of K0; k0_done() records it
    bool batch = false;       // diagnostic library: the batch route, where k0_sets applies ...
    bool repeat = false;      // ... and a call that repeats the previous one's layout, where dbg_phase / dbg_k0_nogrp apply
};
// (NS_F32 / NS_I16: register sets of a wave for either sample type, seg_bs.hpp: blocksum_kernel<DT, NS>)
template <int FLAGS, int NS_F32, int NS_I16>
void enqueue_k0(ps_ctx *ctx, const DevCfg &cfg, hipStream_t st, const K0Call &k, unsigned grid, uint4 *grp)
{
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    by_dtype<FLAGS>(cfg.dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        constexpr int NS = sdt(DT) == PS_DTYPE_F32 ? NS_F32 : NS_I16;
        hipLaunchKernelGGL((blocksum_kernel<DT, NS>), dim3(grid), dim3(64 * K0_WAVES), 0, st, cfg, k.ev_start, k.ev_len, k.ev_boff, k.n_ev,
                           k.n_samples, ctx->bsum.p, ctx->ev_info.as<int4>(), ctx->chunk_mabs.as<int4>(),
                           reinterpret_cast<unsigned *>(&sm->status), grp);
    });
}
// K0 on stream st: chunk-prefixed block sums (one streaming pass), per-event centre m, totals + max|k| per 256 blocks, on the
// digest reserve_digest() sized (FLAGS: DT_WIDE for the 64-bit one).  cfg as K0 sees it: grp / blk_mm / blk_cls set, bsum not yet.
template <int FLAGS> int launch_k0(ps_ctx *ctx, const DevCfg &cfg, hipStream_t st, const K0Call &k)
{
    const bool f32 = cfg.dtype == PS_DTYPE_F32;
    int ns = 2;                                        // register sets of a persistent wave (option k0_sets)
    bool skip_k0 = false;
    uint4 *k0_grp = const_cast<uint4 *>(static_cast<const uint4 *>(cfg.grp));
#ifdef PS_DIAG
    if (k.batch && !(FLAGS & DT_WIDE) && ctx->opt.k0_sets > 2 && ctx->opt.k0_waves > 0) ns = ctx->opt.k0_sets;
    skip_k0 = ctx->opt.dbg_phase == 1 && k.repeat;         // diagnostics: the previous call's digest
    if (ctx->opt.dbg_k0_nogrp && k.repeat) k0_grp = nullptr;
#endif
    // K0 is persistent (round 5): k0_waves workgroups per CU (K0_WAVES waves each, i.e. that many waves per SIMD), every
    // wave striding over the wave blocks of the call with its next block's samples in flight.  One or two waves per SIMD
    // saturate HBM; the rest of the SIMD stays free for the scan waves of the other calls in flight.  k0_waves = 0: one wave
    // per wave block as in rounds 3 and 4 (the launch then fills every slot the registers allow).
    const unsigned n_cu = k.persistent ? static_cast<unsigned>(cu_count(ctx)) : 0u;
    const unsigned k0_full = static_cast<unsigned>((k.nb_pad / K0_WB + K0_WAVES - 1) / K0_WAVES);
    // (a wave block of int16 samples is half the bytes: twice the waves keep the same bytes in flight)
    const unsigned k0_per_cu = static_cast<unsigned>(ctx->opt.k0_waves) * ((f32 || ns > 2) ? 1u : 2u);   // (ns > 2: diagnostic library only)
    const unsigned k0_grid = k.persistent && ctx->opt.k0_waves > 0 ? std::min(k0_full, k0_per_cu * n_cu * (4u / K0_WAVES)) : k0_full;
    if (k.admit && ctx->opt.k0_admit > 0) {
        const int grc = chain_enter(ctx, ctx->device, ctx->opt.k0_admit, st, &ctx->chain_ticket);
        if (grc) return grc;
        ctx->chain_held = true;
    }
    bool queued = skip_k0;
#ifdef PS_DIAG
    // (measured and rejected, round 6 -- docs/ROUND_6.md: fatter K0 waves hold fewer registers per byte in flight, but a lone K0
    //  wave per SIMD cannot issue fast enough beside four scan waves; the instances exist in the diagnostic library only)
    if constexpr (!(FLAGS & DT_WIDE)) {
        if (!queued && ns == 3) { enqueue_k0<FLAGS, 3, 6>(ctx, cfg, st, k, k0_grid, k0_grp); queued = true; }
        if (!queued && ns == 4) { enqueue_k0<FLAGS, 4, 8>(ctx, cfg, st, k, k0_grid, k0_grp); queued = true; }
    }
#endif
    if (!queued) enqueue_k0<FLAGS, 2, 2>(ctx, cfg, st, k, k0_grid, k0_grp);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        chain_drop(ctx);                               // (nobody waits for a K0 that was never queued)
        return fail(ctx, PS_ERR_HIP, "K0 launch failed: %s", hipGetErrorString(le));
    }
    return PS_OK;
}
// K0 is behind this point of st: the call M tickets later waits for it on the device
int k0_done(ps_ctx *ctx, hipStream_t st)
{
    if (!ctx->chain_held) return PS_OK;
    ctx->chain_held = false;
    return chain_publish(ctx, ctx->device, st, ctx->chain_ticket);
}

// Phases 1 and 1b of the block-sum pipeline: single-wave spines, then single-wave bridges; the seams that run into a stretch
// without splits are finished by the look-ahead kernel
template <int FLAGS> int launch_scans_bs(ps_ctx *ctx, const DevCfg &cfg, unsigned nj, SmallLayout *sm)
{
    if (int rc = by_dtype<FLAGS>(cfg.dtype, [&](auto dt) { return launch_spine<64, dt()>(ctx, cfg, nj, sm, true); })) return rc;
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
    if (int rc = by_dtype<FLAGS>(cfg.dtype, [&](auto dt) { return launch_bridge<64, dt()>(ctx, cfg, nj, sm); })) return rc;
    if (no_look_ahead(ctx, cfg)) { ctx->counters[PS_CNT_LOOKAHEAD_SKIPPED] += 1; return PS_OK; }
    return by_dtype<FLAGS>(cfg.dtype, [&](auto dt) { return launch_bridge_la<dt()>(ctx, cfg, nj, sm); });
}

// Device-stitch pipeline: tile spines without halo, seam bridges, assemble kernel (true spine,
// tree jobs, items) -- no host round trip before the final synchronisation.
// Returns RC_FALLBACK when a seam could not be bridged on the device (rare); the caller then runs
// the host-stitch pipeline, which repairs seams one by one.
// digest_ready (round 6, ps_detect_segment_trace): the digest of the WHOLE trace is already in the context's buffers (K0 ran over
// it as one event, trace-aligned blocks): no K0 here; the events get (centre of the trace, phase, first block) from
// ev_info_trace_kernel and the scans run in shifted coordinates (seg_bs.hpp: scan_window_ph).
// device_stitch_batch_ runs the steps below in their order; DeviceCall is what they hand on to each other.
struct DeviceCall {
    DevCfg cfg;               // the call's configuration; queue_upload_k0 enters the digest
    bool use_bs = false;      // block-sum scan on the 32-bit digest, or ...
    bool wide = false;        // ... on the 64-bit (wide) digest; neither: the LDS-window kernels
    bool digest_ready = false;
    bool reuse = false;       // the call repeats the previous one's layout: its plan, and its tables on the device, serve again
    size_t nj = 0;            // tiles
    int64_t max_items = 0;    // true anchors the first stitch round has room for
};

// Step 1.  The tile tables depend only on the event layout and the parameters: a call that repeats the previous one's
// (the bench loop; a file segmented with several parameter sets) reuses the tables that are still on the device.  Any other
// call plans (seg_plan.hpp) and stages its upload.
int plan_or_reuse(ps_ctx *ctx, const SegBatch &B, DeviceCall &C)
{
    ps_ctx::TileCache &tc = ctx->tile_cache;
    const int64_t L = ctx->tile_len;
    C.reuse = tc.valid && tc.key.matches(B.ev_start, B.ev_len, B.n_ev, B.mw, B.W, L, C.use_bs);
    if (!C.reuse) {
        tc.valid = false;
        tc.plan = plan_device_tiles(B.ev_start, B.ev_len, B.n_ev, B.mw, B.W, L, C.use_bs);
        if (tc.plan.too_many) return RC_FALLBACK;
        const size_t up_bytes = tc.plan.up_bytes(B.n_ev);
        HIP_TRY(ctx, ctx->h_up.reserve(up_bytes + 64));
        HIP_TRY(ctx, ctx->up_dev.reserve(up_bytes + 64));
        tc.plan.stage(ctx->h_up.as<char>(), B.ev_start, B.ev_len, B.n_ev);
        tc.key.set(B.ev_start, B.ev_len, B.n_ev, B.mw, B.W, L, C.use_bs);
    }
    C.nj = tc.plan.jobs.size();
    C.max_items = tc.plan.list_entries + static_cast<int64_t>(C.nj) * BR_MAX;
    ctx->counters[PS_CNT_TILES] = static_cast<int64_t>(C.nj);
    return PS_OK;
}

// Step 2.  The buffers of the scans and of the stitch, sized by the plan (a call that repeats the layout finds them all)
int reserve_call_buffers(ps_ctx *ctx, const SegBatch &B, const DeviceCall &C)
{
    const DeviceTilePlan &plan = ctx->tile_cache.plan;
    const size_t nj = C.nj, evb = DeviceTilePlan::table_bytes(B.n_ev);
    HIP_TRY(ctx, ctx->spine_scratch.reserve(std::max<int64_t>(1, plan.list_entries) * sizeof(int2)));
    HIP_TRY(ctx, ctx->spine_meta.reserve(std::max<size_t>(4, nj) * sizeof(int4)));
    HIP_TRY(ctx, ctx->bridges.reserve(std::max<size_t>(1, nj) * BR_MAX * sizeof(int2)));
    if (C.use_bs && ctx->opt.lat_help) {
        // (published chunk results carry the tag of their listing; a fresh buffer is zero, tags start at 1, and before the 24
        //  bits run out the buffer is cleared)
        const size_t res_bytes = static_cast<size_t>(LAT_D) * LAT_C * sizeof(unsigned long long);
        HIP_TRY(ctx, ctx->lat_state.reserve(LAT_D * sizeof(unsigned long long)));
        HIP_TRY(ctx, ctx->lat_seam.reserve(LAT_D * sizeof(int)));
        HIP_TRY(ctx, ctx->lat_res.reserve_zeroed(res_bytes, ctx->stream));
        if (ctx->lat_tag_next + 2u * LAT_TAGS >= (1u << 24)) {
            HIP_TRY(ctx, hipMemsetAsync(ctx->lat_res.p, 0, res_bytes, ctx->stream));
            ctx->stream_idle = false;
            ctx->lat_tag_next = 1;
        }
        ctx->lat_tag_base = ctx->lat_tag_next;
        ctx->lat_tag_next += LAT_TAGS;
    }
    HIP_TRY(ctx, ctx->bmeta.reserve(std::max<size_t>(1, nj) * sizeof(int4)));
    HIP_TRY(ctx, ctx->tile_i32.reserve(std::max<size_t>(1, nj) * 4 * sizeof(int)));
    HIP_TRY(ctx, ctx->sp_off.reserve((nj + 1) * sizeof(long long)));
    if (int irc = reserve_items(ctx, C.max_items, plan.total_len, B.mw)) return irc;
    HIP_TRY(ctx, ctx->first_item.reserve(evb));
    if (evb <= SMALL_TAIL) ctx->bounds_off.alias(ctx->small.as<char>() + sizeof(SmallLayout));   // comes back with the status block
    else HIP_TRY(ctx, ctx->bounds_off.reserve(evb));
    ctx->asm_hdr.alias(&ctx->small.as<SmallLayout>()->hdr);
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    return PS_OK;
}

// The call's tables go up and the status block is cleared, on stream fs: by upload_kernel from the pinned blob, by plain copies
// where the device cannot see it, or not at all (option short_chain)
int queue_upload(ps_ctx *ctx, const SegBatch &B, const DeviceCall &C, hipStream_t fs, bool front)
{
    const char *up = ctx->h_up.as<char>();
    const size_t up_bytes = ctx->tile_cache.plan.up_bytes(B.n_ev);
    void *up_devptr = nullptr;                     // the pinned blob as the device sees it (else: plain copy)
    if (ctx->opt.upload_by_kernel && hipHostGetDevicePointer(&up_devptr, const_cast<char *>(up), 0) != hipSuccess) { up_devptr = nullptr; (void)hipGetLastError(); }
    // (option short_chain: the tables are still on the device and the previous call's download kernel left the status block zero)
    // (... on the route the option applies to, short_route, as far as it is known before K0: every other route launches what it launched)
    const bool short_rt = C.use_bs && !C.wide && !C.digest_ready && ctx->opt.groups && !ctx->opt.tree_mw && ctx->opt.tree_screen && C.cfg.mode == MODE_FAST && C.cfg.prune;
    const bool skip_upload = C.reuse && ctx->small_clean_in && !front && short_rt && ctx->opt.upload_by_kernel && (opt_short_chain_bits(ctx->opt.short_chain) & SC_NO_UPLOAD);
    ctx->small_clean_in = false;                   // (a redo of this call on another digest starts from a block it cleared itself)
    if (skip_upload) ctx->counters[PS_CNT_UPLOAD_SKIPPED] += 1;
    else if (up_devptr) {
        // (tables still on the device from the previous call: the kernel only clears the status block)
        const long long n16 = C.reuse ? 0 : static_cast<long long>((up_bytes + 15) / 16);
        const unsigned ug = static_cast<unsigned>(std::max<long long>(1, std::min<long long>((n16 + 255) / 256, 1024)));
        hipLaunchKernelGGL(upload_kernel, dim3(ug), dim3(256), 0, fs, static_cast<const int4 *>(up_devptr),
                           ctx->up_dev.as<int4>(), n16, ctx->small.as<unsigned long long>(),
                           static_cast<int>(sizeof(SmallLayout) / sizeof(unsigned long long)));
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), fs));
        if (!C.reuse) HIP_TRY(ctx, hipMemcpyAsync(ctx->up_dev.p, up, up_bytes, hipMemcpyHostToDevice, fs));
    }
    ctx->tile_cache.valid = true;
    // the five arrays of the blob: [jobs | ev_first_tile | ev_start | ev_len | boff]
    char *dup = ctx->up_dev.as<char>();
    const size_t jb = ctx->tile_cache.plan.jobs_bytes(), evb = DeviceTilePlan::table_bytes(B.n_ev);
    ctx->spine_jobs.alias(dup);
    ctx->ev_first_tile.alias(dup + jb);
    ctx->ev_off.alias(dup + jb + evb);
    ctx->ev_len.alias(dup + jb + 2 * evb);
    ctx->ev_boff.alias(dup + jb + 3 * evb);
    return PS_OK;
}

// K0 over the call's events on stream fs -- or, where the digest of the whole trace is there already (digest_ready), the
// events' places in it -- and the digest entered into the call's configuration
int queue_digest(ps_ctx *ctx, const SegBatch &B, DeviceCall &C, hipStream_t fs, bool front)
{
    DevCfg &cfg = C.cfg;
    const int32_t n_ev = B.n_ev;
    if (C.use_bs && C.nj && C.digest_ready) {
        HIP_TRY(ctx, ctx->ev_info_tr.reserve(static_cast<size_t>(std::max(1, n_ev)) * sizeof(int4)));
        hipLaunchKernelGGL(ev_info_trace_kernel, dim3(static_cast<unsigned>(std::min(64, (n_ev + 255) / 256))), dim3(256), 0, fs,
                           ctx->ev_off.as<int64_t>(), n_ev, ctx->ev_info.as<int4>(), ctx->ev_info_tr.as<int4>());
        HIP_TRY(ctx, hipGetLastError());
        cfg.bsum = ctx->bsum.p;
        cfg.ev_info = ctx->ev_info_tr.as<int4>();
        cfg.chunk_tot = ctx->chunk_mabs.as<int4>();
        cfg.grp = ctx->opt.groups ? ctx->grp.p : nullptr;
        cfg.blk_mm = B.d_stats ? ctx->blk_mm.as<int>() : nullptr;
    } else if (C.use_bs && C.nj) {
        const DeviceTilePlan &plan = ctx->tile_cache.plan;
        const int64_t nb_pad = k0_padded_blocks(plan.boff[n_ev]);
        DigestWant want;
        want.wide = C.wide;
        want.grp = !C.wide && ctx->opt.groups;
        want.blk_mm = B.d_stats && !C.wide;
        if (int drc = reserve_digest(ctx, nb_pad, n_ev, want)) return drc;
        if (want.grp) cfg.grp = ctx->grp.p;
        if (want.blk_mm) cfg.blk_mm = ctx->blk_mm.as<int>();
        K0Call k0 = {ctx->ev_off.as<int64_t>(), ctx->ev_len.as<int64_t>(), ctx->ev_boff.as<int64_t>(), n_ev, plan.sample_end, nb_pad};
        k0.admit = !front;                             // (the front stream serialises the K0s of its contexts by itself)
        k0.batch = true;
        k0.repeat = C.reuse;
        if (int krc = C.wide ? launch_k0<DT_WIDE>(ctx, cfg, fs, k0) : launch_k0<0>(ctx, cfg, fs, k0)) return krc;
        cfg.bsum = ctx->bsum.p;
        cfg.ev_info = ctx->ev_info.as<int4>();
        cfg.chunk_tot = ctx->chunk_mabs.as<int4>();
    }
    return PS_OK;
}

// Step 3.  Upload + K0 are queued on the context's own stream, or on the device's front stream (k0_shared) -- then under the
// front stream's mutex until K0's event is recorded, and the context's stream continues behind that event.
// *k0_only (diagnostic library, dbg_phase 2): the call ends here.
int queue_upload_k0(ps_ctx *ctx, const SegBatch &B, DeviceCall &C, bool *k0_only)
{
    FrontStream *front = (ctx->opt.k0_shared && C.use_bs && C.nj) ? front_for(ctx) : nullptr;
    hipStream_t fs = front ? front->s : ctx->stream;
    std::unique_lock<std::mutex> front_lock;
    if (front) {
        front_lock = std::unique_lock<std::mutex>(front->mu);
        if (!ctx->stream_idle) {                       // (work the caller left on the context's stream -- a filter, a re-quantisation -- comes first)
            HIP_TRY(ctx, hipEventRecord(ctx->ev_front[0], ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(fs, ctx->ev_front[0], 0));
        }
    }
    if (int urc = queue_upload(ctx, B, C, fs, front != nullptr)) return urc;
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[7], fs));
    if (int drc = queue_digest(ctx, B, C, fs, front != nullptr)) return drc;
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[0], fs));
    if (int crc = k0_done(ctx, fs)) return crc;         // (K0 is behind this event)
    *k0_only = false;
#ifdef PS_DIAG
    if (ctx->opt.dbg_phase == 2) {                           // diagnostics: K0 only
        if (front) front_lock.unlock();
        HIP_TRY(ctx, hipStreamSynchronize(fs));
        for (int e = 0; e <= B.n_ev; ++e) B.h_bounds_off[e] = 0;
        *k0_only = true;
        return PS_OK;
    }
#endif
    if (front) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_front[1], fs));
        front_lock.unlock();
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_front[1], 0));
    }
    return PS_OK;
}

// Step 4.  Phases 1 and 1b over the tiles, on the context's stream
int queue_scans(ps_ctx *ctx, const DeviceCall &C)
{
    const DevCfg &cfg = C.cfg;
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    if (C.nj) {
        const unsigned g = static_cast<unsigned>(C.nj);
        int lrc;
        if (C.wide) lrc = launch_scans_bs<DT_WIDE>(ctx, cfg, g, sm);      // (the 64-bit digest: same kernels, compiled for it)
        else if (C.use_bs) lrc = launch_scans_bs<0>(ctx, cfg, g, sm);
        else {
            // LDS-window scan at the option's width (spine_nt); the widest spine is bridged by the 512-thread kernel
            lrc = launch_spine_nt(ctx, cfg, g, sm, true);
            if (lrc) return lrc;
            if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
            lrc = by_nt<256, 512>(ctx->opt.spine_nt, [&](auto nt) {
                return by_dtype(cfg.dtype, [&](auto dt) { return launch_bridge<decltype(nt)::value, dt()>(ctx, cfg, g, sm); });
            });
        }
        if (lrc) return lrc;
    }
    if (ctx->opt.timing >= 2) HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    return PS_OK;
}

// One stitch: the true spine per event from the tile lists and the bridges, then items and subtree jobs for up to items_cap
// anchors.  No host round trip here: the downstream kernels read the item count from the header on the device (launches sized
// by the host-side upper bound), header and status are checked after the final sync.
struct StitchShape { size_t tile_lds = 0; int use_lds = 0; };     // per-tile arrays of the stitch live in LDS when they fit
int queue_stitch(ps_ctx *ctx, const SegBatch &B, const DeviceCall &C, const StitchShape &shape, int64_t items_cap, int ext_stride)
{
    const size_t nj = C.nj, njp = std::max<size_t>(1, nj);
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    int *ti = ctx->tile_i32.as<int>();
    hipLaunchKernelGGL(assemble_tiles_kernel, dim3(1), dim3(1024), shape.use_lds ? shape.tile_lds : 0, ctx->stream,
                       static_cast<int>(nj), ctx->spine_meta.as<int4>(), ctx->bmeta.as<int4>(),
                       ctx->ev_first_tile.as<int64_t>(), B.n_ev, ti, ti + njp, ti + 2 * njp, ti + 3 * njp,
                       ctx->sp_off.as<long long>(), ctx->first_item.as<int64_t>(), ctx->asm_hdr.as<AsmHeader>(),
                       static_cast<long long>(items_cap), shape.use_lds, reinterpret_cast<const unsigned *>(&sm->status));
    HIP_TRY(ctx, hipGetLastError());
    if (items_cap > 0) {
        const unsigned ag = static_cast<unsigned>(std::min<int64_t>((items_cap + 255) / 256, 2048));
        hipLaunchKernelGGL(assemble_items_kernel, dim3(ag), dim3(256), 0,
                           ctx->stream, ctx->spine_jobs.as<SpineJob>(), static_cast<int>(nj), ctx->spine_meta.as<int4>(),
                           ctx->spine_scratch.as<int2>(), ctx->bridges.as<int2>(), ti + 3 * njp,
                           ctx->sp_off.as<long long>(), static_cast<long long>(items_cap), B.mw, B.W, ctx->tree_jobs.as<TreeJob>(),
                           ctx->items.as<Item>(), ctx->tree_counts.as<int32_t>(), ctx->asm_hdr.as<AsmHeader>(),
                           C.cfg.bsum != nullptr ? C.cfg.ev_info : nullptr,
                           ctx->bridge_ext.as<int2>(), ctx->ext_slot.as<int>(), ext_stride);
        HIP_TRY(ctx, hipGetLastError());
    }
    return PS_OK;
}

// A call that issued no look-ahead launch (option short_chain) and whose bridges left seams deferred: the look-ahead
// kernel it did without runs now, once, over every deferred seam, however many, from the window each stopped at --
// exactly what it would have done behind the bridge kernel, one round trip later.  Seams that gave up are the business
// of the rounds after it.
int resume_deferred_seams(ps_ctx *ctx, const DeviceCall &C, int64_t n_def)
{
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    if (ctx->opt.debug) fprintf(stderr, "[poreseg] look-ahead kernel behind the stitch: %lld deferred seams\n", static_cast<long long>(n_def));
    HIP_TRY(ctx, hipMemsetAsync(&sm->hdr, 0, sizeof(AsmHeader), ctx->stream));
    if (ctx->opt.tree_screen) HIP_TRY(ctx, hipMemsetAsync(&sm->tree_defer[0], 0, sizeof sm->tree_defer[0], ctx->stream));
    if (int lrc = by_dtype(C.cfg.dtype, [&](auto dt) { return launch_bridge_la<dt()>(ctx, C.cfg, static_cast<unsigned>(C.nj), sm); })) return lrc;
    ctx->la_keep = LA_KEEP;
    ctx->counters[PS_CNT_REPAIRS] += n_def;
    ctx->counters[PS_CNT_SEAMS_RESUMED] += n_def;
    return PS_OK;
}

// The seams of `list` are continued by the look-ahead kernel, their further anchors in the side buffer from slot slots_used on
int extend_seams(ps_ctx *ctx, const DeviceCall &C, const std::vector<int> &list, int slots_used, int ext_stride)
{
    const size_t nj = C.nj, n_ext = list.size();
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    HIP_TRY(ctx, ctx->bridge_ext.reserve(static_cast<size_t>(EXT_SLOTS) * EXT_MAX * sizeof(int2)));
    HIP_TRY(ctx, ctx->ext_slot.reserve(nj * sizeof(int)));
    HIP_TRY(ctx, ctx->ext_list.reserve(static_cast<size_t>(EXT_SLOTS) * (EXT_MAX / EXT_MAX_MANY) * sizeof(int)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ext_list.p, list.data(), n_ext * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                       // (the list is the caller's local)
    HIP_TRY(ctx, hipMemsetAsync(&sm->hdr, 0, sizeof(AsmHeader), ctx->stream));
    // (the next round's screen starts a new list; what the rounds so far decided and deferred stays, as in work[])
    if (ctx->opt.tree_screen) HIP_TRY(ctx, hipMemsetAsync(&sm->tree_defer[0], 0, sizeof sm->tree_defer[0], ctx->stream));
    const unsigned g = static_cast<unsigned>(n_ext);
    auto extend = [&](auto dt) {
        hipLaunchKernelGGL((bridge_la_kernel<dt(), true>), dim3(g), dim3(64 * BR_LA), 0, ctx->stream, C.cfg,
                           ctx->spine_jobs.as<SpineJob>(), ctx->spine_scratch.as<int2>(), ctx->spine_meta.as<int4>(),
                           ctx->bridges.as<int2>(), ctx->bmeta.as<int4>(), reinterpret_cast<unsigned *>(&sm->status),
                           &sm->work0, static_cast<int>(n_ext), ctx->ext_list.as<int>(), ctx->bridge_ext.as<int2>(),
                           ctx->ext_slot.as<int>(), slots_used, BR_MAX, ext_stride);
    };
    if (C.wide) by_dtype<DT_WIDE>(C.cfg.dtype, extend);
    else by_dtype(C.cfg.dtype, extend);
    HIP_TRY(ctx, hipGetLastError());
    ctx->counters[PS_CNT_REPAIRS] += static_cast<int64_t>(n_ext);
    return PS_OK;
}

// Step 5.  Stitch, subtrees and gather, to the call's one synchronisation (finish_batch); a stitch that failed gets its
// second chance on the device (the block-sum pipeline only: it has the look-ahead kernel) and the round is run again.
int stitch_rounds(ps_ctx *ctx, const SegBatch &B, const DeviceCall &C)
{
    const size_t nj = C.nj;
    StitchShape shape;
    shape.tile_lds = (nj + 1) * sizeof(long long) + 4 * nj * sizeof(int);      // (nj+1) int64 + 4*nj int32
    shape.use_lds = shape.tile_lds <= 150 * 1024;
    if (shape.use_lds)
        HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(assemble_tiles_kernel), static_cast<int>(shape.tile_lds)));
    AsmHeader hd = {};
    int rc = PS_OK;
    int64_t items_cap = C.max_items;                    // (grows with the seams a second-chance round extends)
    int slots_used = 0, ext_stride = EXT_MAX;
    const bool no_la = nj && no_look_ahead(ctx, C.cfg);
    bool la_done = false, stride_set = false;          // (the look-ahead kernel ran behind the stitch; the stride of the side buffer is fixed)
    for (int round = 0;; ++round) {
        if (int qrc = queue_stitch(ctx, B, C, shape, items_cap, ext_stride)) return qrc;
        if (ctx->opt.timing >= 2 && round == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
        rc = finish_batch(ctx, C.cfg, B, static_cast<size_t>(items_cap), items_cap, ctx->asm_hdr.as<AsmHeader>(), &hd, C.use_bs);
        if (rc != RC_FALLBACK || !C.use_bs || !nj || round == EXT_ROUNDS + (la_done ? 1 : 0) || !ctx->opt.bridge_ext) break;
        HIP_TRY(ctx, ctx->h_meta.reserve(2 * nj * sizeof(int4)));
        int4 *h_bm = ctx->h_meta.as<int4>(), *h_mt = h_bm + nj;
        HIP_TRY(ctx, hipMemcpyAsync(h_bm, ctx->bmeta.p, nj * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_mt, ctx->spine_meta.p, nj * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const SecondChance sc = pick_second_chance(h_bm, h_mt, nj, ctx->opt.bridge_budget, slots_used, stride_set, ext_stride, no_la && !la_done);
        if (sc.n_deferred) {
            if (int lrc = resume_deferred_seams(ctx, C, sc.n_deferred)) return lrc;
            la_done = true;
            continue;
        }
        ext_stride = sc.ext_stride;
        stride_set = true;
        if (sc.list.empty() || sc.hopeless) break;
        if (ctx->opt.debug) fprintf(stderr, "[poreseg] second chance, round %d: %zu seams continued on the device\n", round + 1, sc.list.size());
        if (int erc = extend_seams(ctx, C, sc.list, slots_used, ext_stride)) return erc;
        slots_used += static_cast<int>(sc.list.size());
        // room for the anchors the continued seams may add
        items_cap += static_cast<int64_t>(sc.list.size()) * ext_stride;
        if (int irc = reserve_items(ctx, items_cap, ctx->tile_cache.plan.total_len, B.mw)) return irc;
    }
    ctx->counters[PS_CNT_TREE_JOBS] = hd.n_items;
    if (slots_used > 0 || la_done) ctx->small_clean = false;   // (a second round: the next call uploads as ever)
    float ms = 0;
    if (ctx->opt.timing >= 2 && nj && hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[0]) == hipSuccess) ctx->ms[PS_MS_BLOCKSUM] = ms;       // blocksum_kernel (K0)
    if (ctx->opt.timing >= 2 && nj && hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[6]) == hipSuccess) ctx->ms[PS_MS_SPINE] = ms;       // spine_kernel
    if (ctx->opt.timing >= 2 && nj && hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[1]) == hipSuccess) ctx->ms[PS_MS_BRIDGE] = ms;       // bridge_kernel
    if (ctx->opt.timing >= 2 && hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[5]) == hipSuccess) ctx->ms[PS_MS_STITCH] = ms;     // device stitch incl. header sync
    return rc;
}

int device_stitch_batch_(ps_ctx *ctx, const DevCfg &cfg_in, int bs_mode, const SegBatch &B, bool digest_ready)
{
    DeviceCall C;
    C.cfg = cfg_in;
    ctx->la_now = ctx->la_keep > 0;
    if (ctx->la_now) --ctx->la_keep;
    C.use_bs = bs_mode != 0;                           // 1: block-sum scan on the 32-bit digest, 2: on the 64-bit (wide) digest
    C.wide = bs_mode == 2;
    C.cfg.bs_wide = C.wide ? 1 : 0;
    C.digest_ready = digest_ready;
    if (int rc = plan_or_reuse(ctx, B, C)) return rc;
    if (int rc = reserve_call_buffers(ctx, B, C)) return rc;
    bool k0_only = false;
    if (int rc = queue_upload_k0(ctx, B, C, &k0_only)) return rc;
    if (k0_only) return PS_OK;
    if (int rc = queue_scans(ctx, C)) return rc;
    return stitch_rounds(ctx, B, C);
}
// (whatever way the call ends: a ticket of the K0 chain that was not recorded is forgotten)
int device_stitch_batch(ps_ctx *ctx, const DevCfg &cfg_in, int bs_mode, const SegBatch &B, bool digest_ready = false)
{
    const int rc = device_stitch_batch_(ctx, cfg_in, bs_mode, B, digest_ready);
    chain_drop(ctx);                                    // (a call that failed between its ticket and its record gives the ticket up)
    return rc;
}

// The host stitch's subtree jobs, items and per-event tables go to the device, the buffers of phase 3 and the gather sized by them
int upload_host_stitch(ps_ctx *ctx, const SegBatch &B, const HostStitch &st)
{
    const int32_t n_ev = B.n_ev;
    const size_t n_tj = st.tjobs.size(), n_items = st.items.size(), tscratch = static_cast<size_t>(st.tscratch);
    const size_t evb = (static_cast<size_t>(n_ev) + 1) * sizeof(int64_t);
    const size_t up_bytes = n_tj * sizeof(TreeJob) + n_items * sizeof(Item) + evb * 3;
    HIP_TRY(ctx, ctx->h_up.reserve(up_bytes + 64));
    HIP_TRY(ctx, ctx->tree_jobs.reserve(std::max<size_t>(1, n_tj) * sizeof(TreeJob)));
    // (item_scan_kernel reads counts[item index] speculatively: cover the items as well)
    HIP_TRY(ctx, ctx->tree_counts.reserve(std::max<size_t>(std::max<size_t>(1, n_tj), n_items) * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->tree_counts.p, 0, std::max<size_t>(std::max<size_t>(1, n_tj), n_items) * sizeof(int32_t), ctx->stream));   // (tree_job stores only non-zero counts)
    HIP_TRY(ctx, ctx->tree_scratch.reserve(std::max<size_t>(1, tscratch) * sizeof(int32_t)));
    HIP_TRY(ctx, ctx->tree_spill.reserve(std::max<size_t>(1, tscratch) * sizeof(int2)));
    HIP_TRY(ctx, ctx->items.reserve(std::max<size_t>(1, n_items) * sizeof(Item)));
    HIP_TRY(ctx, ctx->item_pos.reserve((n_items + 1) * sizeof(int64_t)));
    HIP_TRY(ctx, ctx->first_item.reserve(evb));
    HIP_TRY(ctx, ctx->ev_off.reserve(evb));
    HIP_TRY(ctx, ctx->ev_len.reserve(evb));
    HIP_TRY(ctx, ctx->bounds_off.reserve(evb));
    char *up = ctx->h_up.as<char>();
    size_t o = 0;
    if (n_tj) {
        std::memcpy(up + o, st.tjobs.data(), n_tj * sizeof(TreeJob));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->tree_jobs.p, up + o, n_tj * sizeof(TreeJob), hipMemcpyHostToDevice, ctx->stream));
        o += n_tj * sizeof(TreeJob);
    }
    if (n_items) {
        std::memcpy(up + o, st.items.data(), n_items * sizeof(Item));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->items.p, up + o, n_items * sizeof(Item), hipMemcpyHostToDevice, ctx->stream));
        o += n_items * sizeof(Item);
    }
    o = (o + 7) & ~static_cast<size_t>(7);
    std::memcpy(up + o, st.first_item.data(), evb);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->first_item.p, up + o, evb, hipMemcpyHostToDevice, ctx->stream));
    o += evb;
    std::memcpy(up + o, B.ev_start, evb - sizeof(int64_t));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ev_off.p, up + o, evb, hipMemcpyHostToDevice, ctx->stream));
    o += evb;
    std::memcpy(up + o, B.ev_len, evb - sizeof(int64_t));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ev_len.p, up + o, evb, hipMemcpyHostToDevice, ctx->stream));
    return PS_OK;
}

// Host-stitch pipeline (the fallback of the device stitch, and option stitch_host): halo tiles, one spine workgroup each; their
// anchor lists come back and the true spine of every event is walked on the host (seg_plan.hpp: stitch_lists), a seam whose
// list stops short repaired by a spine launch of its own; then phase 3 and the gather as on the device route.
int host_stitch_batch(ps_ctx *ctx, const DevCfg &cfg, const SegBatch &B)
{
    const HostTilePlan plan = plan_host_tiles(B.ev_start, B.ev_len, B.n_ev, B.mw, B.W, ctx->tile_len, ctx->halo);
    ctx->counters[PS_CNT_TILES] = static_cast<int64_t>(plan.jobs.size());
    std::vector<TileList> lists;
    int rc = run_spines(ctx, cfg, plan.jobs, plan.scratch, lists);
    if (rc) return rc;

    const auto t_stitch0 = std::chrono::steady_clock::now();
    auto repair = [&](int32_t e, int32_t z, int64_t stop, TileList *ext) {
        const std::vector<SpineJob> rj(1, make_spine_job(B.ev_start[e], e, B.ev_len[e], z, stop, B.mw, 0));
        std::vector<TileList> got;
        rc = run_spines(ctx, cfg, rj, rj[0].out_cap, got);
        if (rc) return false;
        ctx->counters[PS_CNT_REPAIRS] += 1;
        *ext = std::move(got[0]);
        return true;
    };
    HostStitch st;
    switch (stitch_lists(plan, lists, B.ev_start, B.ev_len, B.n_ev, B.mw, B.W, repair, &st)) {
    case STITCH_OK: break;
    case STITCH_REPAIR_FAILED: return rc;
    case STITCH_NO_PROGRESS: return fail(ctx, PS_ERR_INTERNAL, "seam repair made no progress");
    }
    ctx->counters[PS_CNT_TREE_JOBS] = static_cast<int64_t>(st.tjobs.size());
    ctx->ms[PS_MS_STITCH] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_stitch0).count();

    rc = upload_host_stitch(ctx, B, st);
    if (rc) return rc;
    return finish_batch(ctx, cfg, B, st.tjobs.size(), static_cast<int64_t>(st.items.size()));
}
}  // namespace

namespace {
// Do 16-byte global loads from 2- and 4-byte-aligned addresses return the right bytes on this device?  (They do on gfx950 --
// tools/probes/unaligned_probe.hip, at 92 % of the aligned rate -- but the headline kernel must not rest on a stand-alone
// probe run once on one box)  Once per device and process; -1 not probed yet, 0 no, 1 yes.
std::mutex g_probe_mu;
int g_unaligned_ok[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
int k0_unaligned_probe(int device, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_probe_mu);
    int &ok = g_unaligned_ok[device & 15];
    if (ok >= 0) return ok;
    ok = 0;
    unsigned char h[128];
    for (int i = 0; i < 128; ++i) h[i] = static_cast<unsigned char>(37 * i + 11);
    DevBuf d_buf, bad_buf;
    if (d_buf.reserve(256) != hipSuccess || bad_buf.reserve(sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return ok; }
    unsigned char *d = d_buf.as<unsigned char>();
    unsigned *bad = bad_buf.as<unsigned>();
    unsigned hb = 1;
    if (hipMemcpyAsync(d, h, 128, hipMemcpyHostToDevice, st) == hipSuccess && hipMemsetAsync(bad, 0, sizeof(unsigned), st) == hipSuccess) {
        hipLaunchKernelGGL(k0_unaligned_probe_kernel<2>, dim3(1), dim3(64), 0, st, d, 16, bad);     // int16: offsets 0, 2, .. 30 bytes
        hipLaunchKernelGGL(k0_unaligned_probe_kernel<4>, dim3(1), dim3(64), 0, st, d, 16, bad);     // fp32: offsets 0, 4, .. 60 bytes
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(&hb, bad, sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess)
            ok = hb == 0 ? 1 : 0;
    }
    d_buf.release(); bad_buf.release(); (void)hipGetLastError();
    return ok;
}
}  // namespace

#ifdef PS_DIAG
// libporeseg_diag.so only (make -C pypore_amd/csrc diag): a new context takes its settings from PORESEG_* variables, as every
// build did until round 5 -- every option that has a variable (ctx_options.hpp), by the setter's own rules: a value it refuses is
// reported and the default stays.  The product library has no getenv: what a call returns depends on its arguments and on
// ps_set_option / ps_set_tiling, never on the caller's environment.
namespace {
void diag_env(ps_ctx *ctx)
{
    for (const char *name : opt_apply_env(&ctx->opt, std::getenv)) fprintf(stderr, "[poreseg] the environment's value of option %s is refused\n", name);
    if (!ctx->opt.k0_unaligned) ctx->k0_unaligned = 0;
    // what is no whole number for an option: the tiling, the stitch route by name, and PORESEG_DEBUG set to nothing
    if (const char *e = std::getenv(ENV_TILE)) ctx->tile_len = std::atoll(e);
    if (const char *e = std::getenv(ENV_HALO)) ctx->halo = std::atoll(e);
    if (const char *e = std::getenv(ENV_STITCH)) ctx->opt.stitch_host = std::string(e) == "host";
    if (const char *e = std::getenv(ENV_DEBUG)) ctx->opt.debug = ctx->opt.debug || e[0] == 0;
}
}  // namespace
#endif

namespace {
// The hardware queues of the process: the HIP runtime reads GPU_MAX_HW_QUEUES when it starts and maps every stream onto that
// many queues; the library reads it once as well (and never sets it) -- the one variable of the environment it looks at.
int process_hw_queues()
{
    static const int q = hw_queues_parse(std::getenv("GPU_MAX_HW_QUEUES"));
    return q;
}
}  // namespace

extern "C" {

const char *ps_version(void)
{
#ifdef PS_DIAG
    return "poreseg 0.2 (gfx950) DIAGNOSTIC BUILD";
#else
    return "poreseg 0.2 (gfx950)";
#endif
}

int ps_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ps_create(int device, void *stream, ps_ctx **out)
{
    if (!out) return PS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PS_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PS_ERR_NO_DEVICE;
    ps_ctx *ctx = new ps_ctx();
    ctx->device = device;
    if (stream) {
        ctx->stream.s = static_cast<hipStream_t>(stream);
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream.s, hipStreamNonBlocking) != hipSuccess) { delete ctx; return PS_ERR_HIP; }
        ctx->stream.own = true;
    }
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e.e) != hipSuccess) { delete ctx; return PS_ERR_HIP; }
    for (auto &e : ctx->ev_front)
        if (hipEventCreateWithFlags(&e.e, hipEventDisableTiming) != hipSuccess) { delete ctx; return PS_ERR_HIP; }
    if (ctx->small.reserve(sizeof(SmallLayout) + SMALL_TAIL) != hipSuccess) { delete ctx; return PS_ERR_HIP; }
    ctx->lds_max_samples = (LDS_BYTES_MAX - 1024 * 8 - 256) / (static_cast<int>(sizeof(lds_t)) + 1);   // samples + block sums
    ctx->k0_unaligned = k0_unaligned_probe(device, ctx->stream);
#ifdef PS_DIAG
    diag_env(ctx);                                      // libporeseg_diag.so: the PORESEG_* variables of the experiments (tools/)
#endif
    *out = ctx;
    return PS_OK;
}

void ps_destroy(ps_ctx *ctx)
{
    if (!ctx) return;
    chain_drop(ctx);
    delete ctx;
}

int64_t ps_live_bytes(void) { return g_live_bytes.load(); }

const char *ps_last_error(const ps_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ps_set_tiling(ps_ctx *ctx, int64_t tile_len, int64_t halo)
{
    if (!ctx || tile_len < 0 || halo < 0) return PS_ERR_ARG;
    ctx->tile_len = tile_len;
    ctx->halo = halo;
    return PS_OK;
}

#ifdef PS_DIAG
// (diagnostic library, round 6 experiment) the context's own stream re-created on a subset of the compute units: `count` CUs
// starting at bit `first` of the device's CU mask, every `stride`-th bit, or all the others (hipExtStreamCreateWithCUMask); count 0:
// an ordinary stream again.  What it showed (tools/r6/cu_mask_probe.py, docs/ROUND_6.md): contiguous masks work (64 CUs = two
// XCDs: K0 at 1.9 TB/s), a pool of sixteen masked streams + masked front streams for K0 does not (every masked stream is a
// hardware queue of its own: 0.67 ms per step) -- K0 on CUs of its own is not reachable through stream masks.
static int diag_mask_stream(ps_ctx *ctx, hipStream_t *st, int first, int count, int stride, bool invert)
{
    cu_count(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(*st));
    HIP_TRY(ctx, hipStreamDestroy(*st));
    *st = nullptr;
    if (count <= 0) { HIP_TRY(ctx, hipStreamCreateWithFlags(st, hipStreamNonBlocking)); return PS_OK; }
    const int words = (ctx->n_cu + 31) / 32;
    std::vector<uint32_t> mask(static_cast<size_t>(words), invert ? 0xffffffffu : 0u);
    for (int k = 0; k < count; ++k) {
        const int b = first + k * std::max(1, stride);
        if (b < 0 || b >= ctx->n_cu) continue;
        if (invert) mask[b >> 5] &= ~(1u << (b & 31)); else mask[b >> 5] |= 1u << (b & 31);
    }
    if (ctx->n_cu & 31) mask[words - 1] &= (1u << (ctx->n_cu & 31)) - 1u;
    HIP_TRY(ctx, hipExtStreamCreateWithCUMask(st, static_cast<uint32_t>(words), mask.data()));
    return PS_OK;
}
#endif

int ps_set_option(ps_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name) return PS_ERR_ARG;
    const CtxOptions before = ctx->opt;
    const OptRow *row = nullptr;
    if (opt_set(&ctx->opt, name, value, &row) != OPT_OK) return fail(ctx, PS_ERR_ARG, "unknown option or value: %s", name);
    switch (row->effect) {                              // the options that act on the context
    case FX_SHARED_DEVICE: {                            // one call that sets what ps_pool_plan says for that many contexts
        ps_pool_plan_t plan;
        if (pool_plan(ctx->opt.shared_device, ctx->opt.hw_queues > 0 ? ctx->opt.hw_queues : process_hw_queues(), &plan) != PS_OK) {
            ctx->opt = before;
            return fail(ctx, PS_ERR_ARG, "shared_device: no plan for %lld contexts", static_cast<long long>(value));
        }
        ctx->la_keep = 0;
        ctx->opt.k0_waves = plan.k0_waves;
        ctx->opt.lat_help = plan.lat_help;
        ctx->opt.k0_admit = plan.k0_admit;
        break;
    }
    case FX_SHORT_CHAIN: if (ctx->opt.short_chain != before.short_chain) ctx->small_clean = false; break;
    case FX_BRIDGE_PATIENCE: ctx->la_keep = 0; break;
    case FX_WIDE_BS: ctx->wide.forget(); break;
    case FX_K0_UNALIGNED: ctx->k0_unaligned = ctx->opt.k0_unaligned ? k0_unaligned_probe(ctx->device, ctx->stream) : 0; break;
    case FX_CU_MASK:                                    // (diagnostic library) the context's OWN stream on those CUs only
#ifdef PS_DIAG
        if (ctx->stream.own)
            return diag_mask_stream(ctx, &ctx->stream.s, static_cast<int>(value & 0xfff), static_cast<int>((value >> 12) & 0xfff),
                                    static_cast<int>((value >> 24) & 0xff), ((value >> 32) & 1) != 0);
#endif
        ctx->opt = before;
        return fail(ctx, PS_ERR_ARG, "unknown option or value: %s", name);
    case FX_NONE: break;
    }
    return PS_OK;
}

int ps_get_option(const ps_ctx *ctx, const char *name, int64_t *value)
{
    if (!ctx || !name || !value) return PS_ERR_ARG;
    const OptRow *row = nullptr;
    if (opt_get(ctx->opt, name, value, &row) != OPT_OK) return PS_ERR_ARG;
    if (row->effect == FX_K0_UNALIGNED) *value = ctx->k0_unaligned;     // what the probe granted
    return PS_OK;
}

int ps_pool_plan(int32_t n_contexts, int32_t hw_queues, ps_pool_plan_t *out) { return pool_plan(n_contexts, hw_queues, out); }

int ps_hw_queues(void) { return process_hw_queues(); }

int ps_gate_stats(int device, int64_t *out, int32_t n_out, int reset)
{
    if (device < 0 || device >= 16 || (!out && n_out > 0) || n_out < 0) return PS_ERR_ARG;
    K0Chain &c = g_chain[device];
    std::lock_guard<std::mutex> lk(c.mu);
    const int64_t v[5] = {static_cast<int64_t>(c.next), c.open, c.open_max, c.host_waits, c.gave_up};
    for (int i = 0; i < n_out; ++i) out[i] = i < 5 ? v[i] : 0;
    if (reset) { c.open_max = c.open; c.host_waits = 0; c.gave_up = 0; }
    return PS_OK;
}

int ps_synchronize(ps_ctx *ctx)
{
    if (!ctx) return PS_ERR_ARG;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

// cparsers.pyx:55-101
int ps_min_gain(const ps_split_params *p, double *out)
{
    if (!p || !out) return PS_ERR_ARG;
    double fpr = p->false_positive_rate, sps = p->prior_segments_per_second;
    const double sf = p->sampling_freq;
    if (!(fpr != 0.0)) fpr = sf;                                         // :64-65
    if (!(sps != 0.0)) sps = sf / 2.;                                    // :66-67
    if (!(p->max_width >= p->min_width)) return PS_ERR_ASSERT_WIDTH;     // :69
    if (!(p->window_width >= 2 * p->min_width)) return PS_ERR_ASSERT_WINDOW;  // :71
    if (p->cutoff_freq != 0.0 && !(p->cutoff_freq <= 0.5 * sf)) return PS_ERR_ASSERT_CUTOFF;  // :74
    double mg;
    if (p->min_gain_per_sample != 0.0) {
        mg = p->min_gain_per_sample * p->window_width;                   // :84
    } else {
        const double k = p->cutoff_freq != 0.0 ? p->cutoff_freq / (0.5 * sf) : 1.0;   // :89
        mg = (-std::log(sps / (sf - sps)) - std::log(fpr / sf)) / k;     // :95-97
    }
    *out = mg * 2;                                                       // :101
    return PS_OK;
}

int64_t ps_bounds_capacity(const int64_t *h_ev_off, int32_t n_ev, int32_t min_width)
{
    if (!h_ev_off || n_ev < 0 || min_width < 1) return -1;
    int64_t cap = 0;
    for (int e = 0; e < n_ev; ++e) cap += (h_ev_off[e + 1] - h_ev_off[e]) / min_width + 1;
    return cap;
}

int ps_segment_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                     const int64_t *h_ev_off, int32_t n_ev, const ps_split_params *params,
                     int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats)
{
    return ps_segment_batch_ex(ctx, d_samples, fmt, h_ev_off, n_ev, params, d_bounds, cap, h_bounds_off, d_stats, nullptr);
}

int ps_segment_batch_ex(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                        const int64_t *h_ev_off, int32_t n_ev, const ps_split_params *params,
                        int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats,
                        uint8_t *d_is_spine)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_ev_off || n_ev < 0) return fail(ctx, PS_ERR_ARG, "null/negative argument");
    std::vector<int64_t> st(static_cast<size_t>(n_ev) + 1, 0), ln(static_cast<size_t>(n_ev) + 1, 0);
    for (int e = 0; e < n_ev; ++e) { st[e] = h_ev_off[e]; ln[e] = h_ev_off[e + 1] - h_ev_off[e]; }
    return ps_segment_events(ctx, d_samples, fmt, st.data(), ln.data(), n_ev, params, d_bounds, cap, h_bounds_off,
                             d_stats, d_is_spine);
}

static int segment_events_impl(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                               const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, const ps_split_params *params,
                               int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats,
                               uint8_t *d_is_spine, bool d_f64);

int ps_segment_events(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                      const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, const ps_split_params *params,
                      int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats,
                      uint8_t *d_is_spine)
{
    return segment_events_impl(ctx, d_samples, fmt, ev_start, ev_len, n_ev, params, d_bounds, cap, h_bounds_off, d_stats, d_is_spine, false);
}

// The exact route for float64 input on no ADC grid (include/poreseg.h): the reference's own prefix sums -- numpy's sequential
// cumsums, one chain per event (cumsum_ref_kernel) -- and every window scanned with the reference's expressions on them
// (scan_exact_prefix), under the same recursion kernels and device stitch as every other call (LDS-window pipeline: one
// workgroup per window).  Nothing is re-quantised, no sample is read after the cumsums.
int ps_segment_exact_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                         const ps_split_params *params, int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off)
{
    if (!ctx) return PS_ERR_ARG;
    const ps_sample_format fmt = {PS_DTYPE_F32, 0, 1.0};        // (unused by the scans of this route: they read c and c2 only)
    return segment_events_impl(ctx, d_current, &fmt, h_ev_start, h_ev_len, n_ev, params, d_bounds, cap, h_bounds_off, nullptr, nullptr, true);
}

// ---- StatSplit (seg_statsplit.hpp) -----------------------------------------------------------------------------------
// The call's per-event tables go up in one copy (SsEvents: start, len, pre, lo, hi, slot), the prefix sums lie event after
// event (pre[e]); returns the launch-ready view of them.
static int statsplit_upload(ps_ctx *ctx, const std::vector<int64_t> &tab, int32_t n_ev, SsEvents *ev)
{
    HIP_TRY(ctx, ctx->ss.tab.reserve(tab.size() * sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ss.tab.p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    const int64_t *t = ctx->ss.tab.as<int64_t>();
    const size_t n = static_cast<size_t>(n_ev);
    ev->start = t; ev->len = t + n; ev->pre = t + 2 * n; ev->lo = t + 3 * n; ev->hi = t + 4 * n; ev->slot = t + 5 * n;
    ev->n_ev = n_ev;
    return PS_OK;
}

// The counts per event are known: h_off (n + 1 entries) from them, the capacity check (`what` names the capacity in the error),
// the offsets on the device in buf (none for a total of 0).
extern "C++" template <class Count>
static int offsets_to_device(ps_ctx *ctx, DevBuf &buf, const Count *counts, size_t n, int64_t cap, const char *what, int64_t *h_off)
{
    int64_t total = 0;
    if (offsets_from_counts(counts, n, cap, h_off, &total))
        return fail(ctx, PS_ERR_CAPACITY, "%s capacity %lld < required %lld", what, static_cast<long long>(cap), static_cast<long long>(total));
    if (total == 0) return PS_OK;
    HIP_TRY(ctx, buf.reserve((n + 1) * sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, h_off, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    return PS_OK;
}

int ps_statsplit_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                     const int64_t *h_lo, const int64_t *h_hi, const ps_statsplit_params *params, int32_t *d_bounds,
                     int64_t cap, int64_t *h_bounds_off)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_ev_start || !h_ev_len || !params || !h_bounds_off || n_ev < 0 || cap < 0 || (cap > 0 && !d_bounds))
        return fail(ctx, PS_ERR_ARG, "null/negative argument");
    const int64_t mw = params->min_width, maxw = params->max_width, W = params->window_width;
    if (mw < 1) return fail(ctx, PS_ERR_ARG, "min_width must be >= 1");
    if (!(maxw >= mw)) return fail(ctx, PS_ERR_ASSERT_WIDTH, "reference assertion failed (parsers.py:243)");
    if (!(W >= 2 * mw)) return fail(ctx, PS_ERR_ASSERT_WINDOW, "reference assertion failed (parsers.py:244)");
    if ((params->use_log != 0 && params->use_log != 1) ||
        (params->splitter != PS_STATSPLIT_STEPWISE && params->splitter != PS_STATSPLIT_SLANTED))
        return fail(ctx, PS_ERR_ARG, "use_log must be 0 or 1 and splitter PS_STATSPLIT_STEPWISE or PS_STATSPLIT_SLANTED");
    const bool slanted = params->splitter == PS_STATSPLIT_SLANTED;
    const size_t n = static_cast<size_t>(n_ev);
    StatsplitTables T;                                                // (batch_plan.hpp; 2^30: the slanted splitter's N fits in int64)
    int32_t bad = -1;
    if (const BatchPlanError err = plan_statsplit_tables(h_ev_start, h_ev_len, n_ev, h_lo, h_hi, mw, &T, &bad)) {
        const long long len = h_ev_len[bad];
        if (err == BATCH_PLAN_RANGE)
            return fail(ctx, PS_ERR_ARG, "event %d: range [%lld, %lld) outside its %lld samples", bad, static_cast<long long>(h_lo ? h_lo[bad] : 0),
                        h_hi ? static_cast<long long>(h_hi[bad]) : len, len);
        return fail(ctx, PS_ERR_ARG, "event %d length %lld out of range (2^30 samples at most)", bad, len);
    }
    const int64_t total_len = T.total_len, slots = T.slots, stack_cap = T.stack_cap;
    for (int e = 0; e <= n_ev; ++e) h_bounds_off[e] = 0;
    if (n_ev == 0) return PS_OK;
    if (total_len > 0 && !d_current) return fail(ctx, PS_ERR_ARG, "d_current is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned n_wg = static_cast<unsigned>(std::min<int64_t>(n_ev, 4ll * cu_count(ctx)));   // (more events: grid stride)
    SsEvents ev;
    int rc = statsplit_upload(ctx, T.tab, n_ev, &ev);
    if (rc) return rc;
    const size_t pre_n = static_cast<size_t>(std::max<int64_t>(1, total_len));
    HIP_TRY(ctx, ctx->ss.pre.reserve((slanted ? 3 : 2) * pre_n * sizeof(double)));
    HIP_TRY(ctx, ctx->ss.tmp.reserve(static_cast<size_t>(slots) * sizeof(int32_t)));
    HIP_TRY(ctx, ctx->ss.stack.reserve(static_cast<size_t>(n_wg) * static_cast<size_t>(stack_cap) * sizeof(SsFrame)));
    HIP_TRY(ctx, ctx->ss.cnt.reserve((n + 2) * sizeof(int32_t)));     // counts, then the status word
    SsCfg cfg;
    cfg.C = ctx->ss.pre.as<double>(); cfg.C2 = cfg.C + pre_n; cfg.Ct = slanted ? cfg.C2 + pre_n : nullptr;
    cfg.mw = static_cast<int>(mw); cfg.maxw = static_cast<int>(maxw); cfg.W = static_cast<int>(W);
    cfg.thresh = params->threshold;
    cfg.stack = ctx->ss.stack.as<SsFrame>(); cfg.stack_cap = stack_cap;
    cfg.tmp = ctx->ss.tmp.as<int32_t>();
    cfg.count = ctx->ss.cnt.as<int32_t>();
    cfg.status = reinterpret_cast<unsigned *>(cfg.count + n);
    HIP_TRY(ctx, hipMemsetAsync(cfg.status, 0, sizeof(unsigned), ctx->stream));
    hipLaunchKernelGGL(statsplit_prefix_kernel, dim3(static_cast<unsigned>(std::min<int64_t>(n_ev, 65535))), dim3(64), 0, ctx->stream,
                       d_current, ev, const_cast<double *>(cfg.C), const_cast<double *>(cfg.C2), const_cast<double *>(cfg.Ct));
    HIP_TRY(ctx, hipGetLastError());
    const int mode = (params->use_log ? 1 : 0) | (slanted ? 2 : 0);
    switch (mode) {
    case 0: hipLaunchKernelGGL(statsplit_kernel<0>, dim3(n_wg), dim3(SS_NT), 0, ctx->stream, ev, cfg); break;
    case 1: hipLaunchKernelGGL(statsplit_kernel<1>, dim3(n_wg), dim3(SS_NT), 0, ctx->stream, ev, cfg); break;
    case 2: hipLaunchKernelGGL(statsplit_kernel<2>, dim3(n_wg), dim3(SS_NT), 0, ctx->stream, ev, cfg); break;
    default: hipLaunchKernelGGL(statsplit_kernel<3>, dim3(n_wg), dim3(SS_NT), 0, ctx->stream, ev, cfg); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> cnt(n + 1);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), cfg.count, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned st = static_cast<unsigned>(cnt[n]);
    if (st & SS_ST_STACK) return fail(ctx, PS_ERR_INTERNAL, "StatSplit: device interval stack overflow");
    if (st & SS_ST_OUT) return fail(ctx, PS_ERR_INTERNAL, "StatSplit: device boundary slot overflow");
    if ((rc = offsets_to_device(ctx, ctx->ss.off, cnt.data(), n, cap, "bounds", h_bounds_off))) return rc;
    if (h_bounds_off[n_ev] == 0) return PS_OK;
    hipLaunchKernelGGL(statsplit_gather_kernel, dim3(static_cast<unsigned>(std::min<int64_t>(n_ev, 4096))), dim3(256), 0, ctx->stream,
                       cfg.tmp, ev.slot, ctx->ss.off.as<int64_t>(), n_ev, d_bounds);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_statsplit_prefix_f64(ps_ctx *ctx, const double *d_current, int64_t n, double *d_c, double *d_c2, double *d_ct)
{
    if (!ctx) return PS_ERR_ARG;
    if (n < 0 || n > (1ll << 30) || (n > 0 && (!d_current || !d_c || !d_c2))) return fail(ctx, PS_ERR_ARG, "null pointer or bad length");
    if (n == 0) return PS_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<int64_t> tab = {0, n, 0, 0, n, 0, 0};           // one event: start, len, pre, lo, hi, slot[2]
    SsEvents ev;
    const int rc = statsplit_upload(ctx, tab, 1, &ev);
    if (rc) return rc;
    hipLaunchKernelGGL(statsplit_prefix_kernel, dim3(1), dim3(64), 0, ctx->stream, d_current, ev, d_c, d_c2, d_ct);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

// What the two segment entry points (ps_segment_events and its kin, ps_detect_segment_trace) do first, each behind the
// pointer checks of its own arguments: the reference's assertions and its min_gain, the widths, the events' ranges (the trace
// route has no events yet: n_ev 0), the call's configuration, the device.
struct SegCall {
    std::chrono::steady_clock::time_point t_begin;
    int mw = 0, maxw = 0, W = 0;
    DevCfg cfg;
};
static int begin_segment_call(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const ps_split_params *params,
                              const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, SegCall *c)
{
    c->t_begin = std::chrono::steady_clock::now();
    chain_drop(ctx);                                   // (a ticket of the K0 chain that an earlier call did not record is given up)
    double min_gain = 0;
    int rc = ps_min_gain(params, &min_gain);
    if (rc) return fail(ctx, rc, "reference assertion failed (cparsers.pyx:69-76)");
    const int mw = params->min_width, maxw = params->max_width, W = params->window_width;
    if (mw < 1 || W < 2) return fail(ctx, PS_ERR_ARG, "min_width must be >= 1 and window_width >= 2");
    int64_t total_len = 0;
    for (int e = 0; e < n_ev; ++e) {
        const int64_t len = ev_len[e];
        if (len < 0 || ev_start[e] < 0 || len > 0x7fffffff - 2LL * W - 8)
            return fail(ctx, PS_ERR_ARG, "event %d length %lld out of range", e, static_cast<long long>(len));
        total_len += len;
    }
    if (total_len > 0 && !d_samples) return fail(ctx, PS_ERR_ARG, "d_samples is NULL");
    c->mw = mw; c->maxw = maxw; c->W = W;
    rc = make_cfg(ctx, d_samples, fmt, mw, maxw, W, min_gain, &c->cfg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return PS_OK;
}

// Near-tie log (ps_get_near_ties): every segment call starts with "not counted" and no events of its own ...
static void nt_reset(ps_ctx *ctx)
{
    ctx->nt.seen = -1;
    ctx->nt.call_cap = ctx->opt.near_tie_log;
    ctx->nt.ev_start.clear();
    ctx->nt.ev_len.clear();
}

// ... points the call's configuration at the log (block-sum scan only: the LDS-window kernels keep no margins) ...
static int nt_arm(ps_ctx *ctx, DevCfg &cfg)
{
    if (ctx->nt.call_cap <= 0) return PS_OK;
    const void *before = ctx->nt.log.p;
    HIP_TRY(ctx, ctx->nt.log.reserve(offsetof(NtLog, rec) + static_cast<size_t>(ctx->nt.call_cap) * sizeof(NtRec)));
    if (ctx->nt.log.p != before || ctx->nt.hdr_cap != ctx->nt.call_cap) {       // (a new buffer or a new capacity: once, not per call)
        NtLog h = {};
        h.cur = &ctx->small.as<SmallLayout>()->nt_cur;
        h.cap = ctx->nt.call_cap;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->nt.log.p, &h, offsetof(NtLog, rec), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->nt.hdr_cap = ctx->nt.call_cap;
    }
    cfg.nt_log = ctx->nt.log.as<NtLog>();
    return PS_OK;
}

// ... and keeps its events when it logged anything (finish_batch set nt.seen from the cursor): the records are mapped on request
static void nt_keep(ps_ctx *ctx, const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev)
{
    if (ctx->nt.seen <= 0 || ctx->nt.seen > ctx->nt.call_cap) return;
    ctx->nt.ev_start.assign(ev_start, ev_start + n_ev);
    ctx->nt.ev_len.assign(ev_len, ev_len + n_ev);
}

static int segment_events_body(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                               const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, const ps_split_params *params,
                               int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats,
                               uint8_t *d_is_spine, bool d_f64)
{
    if (!ctx) return PS_ERR_ARG;
    ctx->d_is_spine = d_is_spine;
    if (!ev_start || !ev_len || !params || !h_bounds_off || n_ev < 0 || cap < 0 || (cap > 0 && !d_bounds))
        return fail(ctx, PS_ERR_ARG, "null/negative argument");
    SegCall call;
    int rc = begin_segment_call(ctx, d_samples, fmt, params, ev_start, ev_len, n_ev, &call);
    if (rc) return rc;
    const auto t_begin = call.t_begin;
    const int mw = call.mw, W = call.W;
    DevCfg &cfg = call.cfg;
    if (!d_f64) { rc = nt_arm(ctx, cfg); if (rc) return rc; }
    reset_call_stats(ctx);
    ctx->stream_idle = true;
    if (ctx->opt.k0_shared && hipStreamQuery(ctx->stream) != hipSuccess) { ctx->stream_idle = false; (void)hipGetLastError(); }
    if (ctx->opt.timing >= 1) HIP_TRY(ctx, hipEventRecord(ctx->ev[8], ctx->stream));
    if (ctx->opt.stitch_host) HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));   // (the device-stitch path clears it with its upload)
    if (d_f64) {
        // exact route: c = cumsum(x), c2 = cumsum(x * x) per event, laid out like the samples (event e at ev_start[e])
        int64_t sample_end = 0;
        for (int e = 0; e < n_ev; ++e) sample_end = std::max(sample_end, ev_start[e] + ev_len[e]);
        const size_t evb = static_cast<size_t>(std::max(1, n_ev)) * sizeof(int64_t);
        HIP_TRY(ctx, ctx->pre_c.reserve(std::max<size_t>(16, 2 * static_cast<size_t>(sample_end) * sizeof(double))));
        HIP_TRY(ctx, ctx->det_cand.reserve(2 * evb));
        HIP_TRY(ctx, ctx->h_hdr.reserve(2 * evb));
        int64_t *h_ev = ctx->h_hdr.as<int64_t>();
        for (int e = 0; e < n_ev; ++e) { h_ev[e] = ev_start[e]; h_ev[n_ev + e] = ev_len[e]; }
        if (n_ev > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->det_cand.p, h_ev, 2 * static_cast<size_t>(n_ev) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
            double *C = ctx->pre_c.as<double>(), *C2 = C + sample_end;
            hipLaunchKernelGGL(cumsum_ref_kernel, dim3(static_cast<unsigned>(std::min<int64_t>(n_ev, 65535))), dim3(64), 0, ctx->stream,
                               static_cast<const double *>(d_samples), ctx->det_cand.as<int64_t>(), ctx->det_cand.as<int64_t>() + n_ev, n_ev, C, C2);
            HIP_TRY(ctx, hipGetLastError());
            cfg.pre_c = C; cfg.pre_c2 = C2;
        }
    }

    const SegBatch B = {ev_start, ev_len, n_ev, mw, W, d_bounds, cap, h_bounds_off, d_stats, t_begin};
    if (!ctx->opt.stitch_host) {
        // The route (seg_plan.hpp): the block-sum scan where the call fits it, else the LDS-window kernels.  Counts too wide for
        // the 32-bit digest (K0 says so: RC_WIDE): the call is redone on the 64-bit digest, and if that refuses too on the
        // LDS-window kernels; the calls after it on the same grid start where it ended (PS_CNT_WIDE_REDO: 1 = 64-bit digest, 2 =
        // LDS-window scan).
        WideRedo &wide = ctx->wide;
        const bool use_bs = scan_route_bs(ctx->opt.scan_bs != 0, mw, W, ctx->opt.mode == MODE_EXACT, d_f64);
        rc = device_stitch_batch(ctx, cfg, wide.begin(use_bs, fmt->quantum), B);
        while (rc == RC_WIDE) {
            const int bs_mode = wide.refused(ctx->opt.wide_bs != 0, fmt->quantum);
            reset_call_stats(ctx);
            HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
            ctx->stream_idle = false;                  // (the front stream, if used, waits for this memset)
            rc = device_stitch_batch(ctx, cfg, bs_mode, B);
        }
        if (wide.redo) ctx->counters[PS_CNT_WIDE_REDO] = wide.redo;
        if (rc != RC_FALLBACK) return rc;
        // a seam could not be bridged on the device: redo with the host stitch (halo tiles + repairs)
        reset_call_stats(ctx);
        ctx->counters[PS_CNT_REPAIRS] = 1000000;
        HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    }
    return host_stitch_batch(ctx, cfg, B);
}

static int segment_events_impl(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt,
                               const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, const ps_split_params *params,
                               int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats,
                               uint8_t *d_is_spine, bool d_f64)
{
    if (!ctx) return PS_ERR_ARG;
    nt_reset(ctx);
    const int rc = segment_events_body(ctx, d_samples, fmt, ev_start, ev_len, n_ev, params, d_bounds, cap, h_bounds_off, d_stats,
                                       d_is_spine, d_f64);
    if (rc == PS_OK && n_ev == 0) ctx->nt.seen = 0;           // (no event, no window: none -- as ps_detect_segment_trace says)
    else if (rc == PS_OK) nt_keep(ctx, ev_start, ev_len, n_ev);
    else ctx->nt.seen = -1;
    return rc;
}

static int single_scan(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, int mode,
                       int mw, double min_gain, double *d_scores, double *gain_out, int32_t *idx_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_samples || n < 0 || n > 0x7fffffff) return fail(ctx, PS_ERR_ARG, "bad samples/n");
    DevCfg cfg;
    int rc = make_cfg(ctx, d_samples, fmt, mw, 0, 0, min_gain, &cfg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    HIP_TRY(ctx, ctx->spine_meta.reserve(64));
    if (d_scores && n) HIP_TRY(ctx, hipMemsetAsync(d_scores, 0, static_cast<size_t>(n) * sizeof(double), ctx->stream));
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    double *d_gain = ctx->spine_meta.as<double>();
    int *d_idx = reinterpret_cast<int *>(d_gain + 1);
    cfg.lds_cap = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(n, ctx->lds_max_samples)));
    {
        const size_t lds = lds_bytes_for(cfg.lds_cap, 1024);
        rc = by_dtype(cfg.dtype, [&](auto dt) {
            HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(single_scan_kernel<1024, dt()>), static_cast<int>(lds)));
            hipLaunchKernelGGL((single_scan_kernel<1024, dt()>), dim3(1), dim3(1024), lds, ctx->stream, cfg,
                               static_cast<int>(n), mode, d_scores, d_gain, d_idx,
                               reinterpret_cast<unsigned *>(&sm->status), &sm->work0);
            return PS_OK;
        });
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    HIP_TRY(ctx, ctx->h_meta.reserve(64));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, d_gain, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
    if (rc) return rc;
    if (gain_out) *gain_out = *ctx->h_meta.as<double>();
    if (idx_out) *idx_out = *reinterpret_cast<int *>(ctx->h_meta.as<double>() + 1);
    return PS_OK;
}

// cparsers.pyx:120-155
int ps_best_single_split(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                         double *gain_out, int32_t *index_out)
{
    if (!gain_out || !index_out) return fail(ctx, PS_ERR_ARG, "null output");
    return single_scan(ctx, d_samples, fmt, n, 1, 1, 0.0, nullptr, gain_out, index_out);
}

// cparsers.pyx:205-249 with no_split=True
int ps_score_window(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                    int32_t min_width, double min_gain, double *d_scores, int32_t *split_out)
{
    if (min_width < 1) return fail(ctx, PS_ERR_ARG, "min_width must be >= 1");
    double g;
    return single_scan(ctx, d_samples, fmt, n, 0, min_width, min_gain, d_scores, &g, split_out);
}


// Diagnostic (tests/test_bound_audit.py): the pruning bounds of the block-sum window scan against the gains they cover,
// on the device, with the product's own scan code (scan_window_bs<.., AUDIT>).  K0 on the one event [0, n), then one wave
// per window.  out[12]: see bs_audit_note (seg_bs.hpp); the three margins are returned as doubles.
int ps_audit_bounds(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, const ps_split_params *params,
                    const int32_t *h_windows, int32_t n_win, double *out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_samples || !params || !h_windows || !out || n < 16 || n > 0x7fffffff || n_win < 1) return fail(ctx, PS_ERR_ARG, "bad argument");
    double mg = 0;
    int rc = ps_min_gain(params, &mg);
    if (rc) return fail(ctx, rc, "invalid split parameters");
    DevCfg cfg;
    rc = make_cfg(ctx, d_samples, fmt, params->min_width, params->max_width, params->window_width, mg, &cfg);
    if (rc) return rc;
    if (params->min_width < 8) return fail(ctx, PS_ERR_ARG, "the block-sum scan needs min_width >= 8");
    for (int i = 0; i < n_win; ++i)
        if (h_windows[2 * i] < 0 || h_windows[2 * i + 1] > n || h_windows[2 * i + 1] - h_windows[2 * i] <= 2 * params->min_width)
            return fail(ctx, PS_ERR_ARG, "window %d: [%d, %d) is not a window the recursion would scan", i, h_windows[2 * i], h_windows[2 * i + 1]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cfg.mode = MODE_FAST;
    const int64_t nb_total = (n + 7) / 8, nb_pad = k0_padded_blocks(nb_total);
    const int64_t tab[4] = {0, n, 0, nb_total};                            // ev_start | ev_len | ev_boff[0..1]
    const size_t win_bytes = static_cast<size_t>(n_win) * 2 * sizeof(int32_t);
    DigestWant want;
    want.grp = true;
    rc = reserve_digest(ctx, nb_pad, 1, want);
    if (rc) return rc;
    HIP_TRY(ctx, ctx->up_dev.reserve(sizeof(tab) + 128 + win_bytes));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    char *d = ctx->up_dev.as<char>();
    unsigned long long acc[12] = {0, 0, 0, 0, 0, 0, 0x7fffffffull, 0x7fffffffull, 0x7fffffffull, 0, 0, 0};
    HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d + 32, acc, sizeof(acc), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d + 128, h_windows, win_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                        // (the host arrays are the caller's / the stack's)
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    const int64_t *dt = reinterpret_cast<const int64_t *>(d);
    cfg.grp = ctx->grp.p;
    // (always one wave per wave block, the narrow digest with its group records, no admission: the audit is no call of a pool)
    K0Call k0 = {dt, dt + 1, dt + 2, 1, n, nb_pad};
    k0.persistent = false;
    rc = launch_k0<0>(ctx, cfg, ctx->stream, k0);
    if (rc) return rc;
    cfg.bsum = ctx->bsum.p;
    cfg.ev_info = ctx->ev_info.as<int4>();
    cfg.chunk_tot = ctx->chunk_mabs.as<int4>();
    cfg.dbg = reinterpret_cast<unsigned long long *>(d + 32);
    const unsigned g = static_cast<unsigned>(std::min<int32_t>(n_win, 4096));
    by_dtype(cfg.dtype, [&](auto dt_) {
        hipLaunchKernelGGL((audit_kernel<dt_()>), dim3(g), dim3(64), 0, ctx->stream, cfg, reinterpret_cast<const int2 *>(d + 128), n_win,
                           reinterpret_cast<unsigned *>(&sm->status));
    });
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(acc, d + 32, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tile_cache.valid = false;                                          // (the tables of the last batch call are gone)
    const unsigned st = static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status);
    if (st & ST_WIDE_RANGE) return fail(ctx, PS_ERR_ARG, "counts too wide for the 32-bit digest: nothing to audit");
    rc = check_status(ctx, st);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i) out[i] = static_cast<double>(acc[i]);
    for (int i = 6; i < 9; ++i) {
        int k = static_cast<int>(static_cast<unsigned>(acc[i] & 0xffffffffull));
        if (k == 0x7fffffff) { out[i] = INFINITY; continue; }
        k ^= (k >> 31) & 0x7fffffff;
        float f;
        std::memcpy(&f, &k, sizeof(f));
        out[i] = static_cast<double>(f);
    }
    return PS_OK;
}

// Replaces lambda_event_parser.parse with the default rules (parsers.py:124-155).
namespace {
// The detector after its streaming pass: edges (sample positions where the mask flips) -> pieces longer than min_duration
// (parsers.py:133) -> their extremes (piece_minmax_kernel: whole 4 096-sample chunks from the table the streaming pass left in
// det_counts, the ragged ends from the samples) -> the rules min > min_current, max < threshold (:134-135).
int events_from_edges(ps_ctx *ctx, const DevCfg &cfg, int64_t n, std::vector<int> &tics, double threshold, int64_t min_duration,
                      double min_current, int64_t *h_starts, int64_t *h_lengths, int64_t cap, int64_t *n_events_out)
{
    std::sort(tics.begin(), tics.end());
    std::vector<int2> cand;
    int a = 0;
    for (size_t p = 0; p <= tics.size(); ++p) {
        const int b = p == tics.size() ? static_cast<int>(n) : tics[p];
        if (static_cast<int64_t>(b) - a > min_duration) cand.push_back(make_int2(a, b));
        a = b;
    }
    const size_t nc = cand.size();
    if (nc == 0) return PS_OK;
    HIP_TRY(ctx, ctx->det_cand.reserve(nc * sizeof(int2) * 2));
    HIP_TRY(ctx, ctx->h_up.reserve(nc * sizeof(int2)));
    std::memcpy(ctx->h_up.p, cand.data(), nc * sizeof(int2));
    int2 *d_cand = ctx->det_cand.as<int2>(), *d_mm = d_cand + nc;
    HIP_TRY(ctx, hipMemcpyAsync(d_cand, ctx->h_up.p, nc * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    by_dtype(cfg.dtype, [&](auto dt) {
        hipLaunchKernelGGL((piece_minmax_kernel<dt()>), dim3(static_cast<unsigned>(nc)), dim3(256), 0, ctx->stream, cfg, d_cand, static_cast<int>(nc), ctx->det_counts.as<int2>(), d_mm);
    });
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, ctx->h_dense.reserve(nc * sizeof(int2)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_dense.p, d_mm, nc * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int2 *hm = ctx->h_dense.as<int2>();
    int64_t kept = 0;
    for (size_t i = 0; i < nc; ++i) {
        const double mn = static_cast<double>(hm[i].x) * cfg.q, mx = static_cast<double>(hm[i].y) * cfg.q;
        if (mn > min_current && mx < threshold) {                                        // parsers.py:134-135
            if (kept < cap) { h_starts[kept] = cand[i].x; h_lengths[kept] = cand[i].y - cand[i].x; }
            ++kept;
        }
    }
    *n_events_out = kept;
    if (kept > cap) return fail(ctx, PS_ERR_CAPACITY, "event capacity %lld < %lld", static_cast<long long>(cap), static_cast<long long>(kept));
    return PS_OK;
}

// One streaming pass that leaves the edge list in `tics` and min / max per DET_CHUNK samples in det_counts.  by_blocks = false:
// edge_scan_kernel over the samples; true (ps_detect_segment_trace): edge_cls_kernel over the per-block verdicts K0 left.
int detect_edges(ps_ctx *ctx, const DevCfg &cfg, int64_t n, double threshold, bool by_blocks, std::vector<int> &tics,
                 unsigned *status_out)
{
    const int nb = static_cast<int>((n + DET_CHUNK - 1) / DET_CHUNK);
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    unsigned *d_ntics = reinterpret_cast<unsigned *>(&sm->dense);
    HIP_TRY(ctx, ctx->det_counts.reserve(static_cast<size_t>(nb) * sizeof(int2)));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    size_t tics_cap = std::max<size_t>(ctx->det_tics.cap / sizeof(int), 1u << 16);
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIP_TRY(ctx, ctx->det_tics.reserve(tics_cap * sizeof(int)));
        // (by_blocks: K0 ran just before on this stream and its status bits -- off grid, counts too wide -- are still wanted; the
        //  edge count is still zero from the call's setup kernel on the first attempt)
        if (!by_blocks) HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
        else if (attempt > 0) HIP_TRY(ctx, hipMemsetAsync(&sm->dense, 0, sizeof(unsigned long long), ctx->stream));
        const unsigned cls_grid = static_cast<unsigned>((((n + 7) / 8 + 63) / 64 + CLS_NT - 1) / CLS_NT);
        by_dtype(cfg.dtype, [&](auto dt) {
            if (by_blocks) hipLaunchKernelGGL((edge_cls_kernel<dt()>), dim3(cls_grid), dim3(CLS_NT), 0, ctx->stream, cfg, n, threshold,
                                              ctx->blk_cls.as<unsigned char>(), ctx->cls_mm.as<int2>(), ctx->ev_info.as<int4>(),
                                              ctx->det_tics.as<int>(), d_ntics, static_cast<unsigned>(tics_cap),
                                              ctx->det_counts.as<int2>(), reinterpret_cast<unsigned *>(&sm->status));
            else hipLaunchKernelGGL((edge_scan_kernel<dt()>), dim3(nb), dim3(DET_NT), 0, ctx->stream, cfg, n, threshold,
                                    ctx->det_tics.as<int>(), d_ntics, static_cast<unsigned>(tics_cap), ctx->det_counts.as<int2>(),
                                    reinterpret_cast<unsigned *>(&sm->status));
        });
        HIP_TRY(ctx, hipGetLastError());
        // speculative copy of the first edges together with the count: one sync in the common case
        const size_t spec = std::min<size_t>(tics_cap, 4096);
        HIP_TRY(ctx, ctx->h_dense.reserve(std::max(spec, static_cast<size_t>(1)) * sizeof(int)));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_dense.p, ctx->det_tics.p, spec * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const SmallLayout hs = *ctx->h_small.as<SmallLayout>();
        if (status_out) *status_out = static_cast<unsigned>(hs.status);
        if (by_blocks && (static_cast<unsigned>(hs.status) & ST_WIDE_RANGE)) return PS_OK;      // (the caller takes the other route)
        const int rc = check_status(ctx, static_cast<unsigned>(hs.status));
        if (rc) return rc;
        const size_t ne = static_cast<unsigned>(hs.dense);
        if (ne > tics_cap) { tics_cap = ne + 1024; continue; }          // list overflowed: rerun with room for all edges
        tics.resize(ne);
        if (ne <= spec) std::memcpy(tics.data(), ctx->h_dense.p, ne * sizeof(int));
        else HIP_TRY(ctx, hipMemcpy(tics.data(), ctx->det_tics.p, ne * sizeof(int), hipMemcpyDeviceToHost));
        break;
    }
    return PS_OK;
}
}  // namespace

int ps_detect_events(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                     double threshold, int64_t min_duration, double min_current,
                     int64_t *h_starts, int64_t *h_lengths, int64_t cap, int64_t *n_events_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!n_events_out || n < 0 || n > 0x7fffffff || cap < 0 || (cap > 0 && (!h_starts || !h_lengths)))
        return fail(ctx, PS_ERR_ARG, "bad argument");
    *n_events_out = 0;
    if (n == 0) return PS_OK;
    if (!d_samples) return fail(ctx, PS_ERR_ARG, "d_samples is NULL");
    DevCfg cfg;
    int rc = make_cfg(ctx, d_samples, fmt, 1, 1, 2, 0.0, &cfg);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int> tics;
    rc = detect_edges(ctx, cfg, n, threshold, false, tics, nullptr);
    if (rc) return rc;
    return events_from_edges(ctx, cfg, n, tics, threshold, min_duration, min_current, h_starts, h_lengths, cap, n_events_out);
}

// Every piece the threshold cuts the trace into (seg_pieces.hpp; planned by piece_plan.hpp): four launches, one status word, ONE
// host synchronisation -- the kernels write only the rows the caller's tables have room for, the count comes back with the status.
int ps_detect_pieces(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, double threshold,
                     int64_t *d_edges, ps_segstat *d_stats, int64_t cap, int64_t *n_pieces_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!n_pieces_out) return fail(ctx, PS_ERR_ARG, "bad argument");
    *n_pieces_out = 0;
    PiecePlan plan;
    if (plan_pieces(n, cap, fmt && fmt->dtype == PS_DTYPE_F32, &plan) != PIECE_PLAN_OK || !d_edges || (cap > 0 && !d_stats))
        return fail(ctx, PS_ERR_ARG, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) {                                       // no piece: edges[0] = n
        HIP_TRY(ctx, hipMemsetAsync(d_edges, 0, sizeof(int64_t), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return PS_OK;
    }
    if (!d_samples) return fail(ctx, PS_ERR_ARG, "d_samples is NULL");
    DevCfg cfg;
    if (int rc = make_cfg(ctx, d_samples, fmt, 1, 1, 2, 0.0, &cfg)) return rc;
    HIP_TRY(ctx, ctx->pc.scratch.reserve(plan.bytes()));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    char *at = ctx->pc.scratch.as<char>();
    uint16_t *d_bits = reinterpret_cast<uint16_t *>(at); at += plan.b_bits;
    int *d_cnt = reinterpret_cast<int *>(at); at += plan.b_cnt;
    int *d_last = reinterpret_cast<int *>(at); at += plan.b_last;
    int *d_base = reinterpret_cast<int *>(at); at += plan.b_base;
    int *d_open = reinterpret_cast<int *>(at); at += plan.b_open;
    PiecePart *d_head = reinterpret_cast<PiecePart *>(at); at += plan.b_head;
    PiecePart *d_tail = reinterpret_cast<PiecePart *>(at);
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    unsigned *st = reinterpret_cast<unsigned *>(&sm->status);
    HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    const dim3 grid(static_cast<unsigned>(plan.chunks));
    by_dtype(cfg.dtype, [&](auto dt) {
        hipLaunchKernelGGL((piece_mark_kernel<dt()>), grid, dim3(PIECE_NT), 0, ctx->stream, cfg, n, threshold, d_bits, d_cnt, d_last, st);
        hipLaunchKernelGGL(piece_scan_kernel, dim3(1), dim3(PIECE_SCAN_NT), 0, ctx->stream, static_cast<const int *>(d_cnt),
                           static_cast<const int *>(d_last), plan.chunks, plan.scan_per_thread, d_base, d_open, n, cap, d_edges, &sm->dense);
        hipLaunchKernelGGL((piece_stats_kernel<dt()>), grid, dim3(PIECE_NT), 0, ctx->stream, cfg, n, plan.span_max,
                           static_cast<const uint16_t *>(d_bits), static_cast<const int *>(d_cnt), static_cast<const int *>(d_last),
                           static_cast<const int *>(d_base), static_cast<const int *>(d_open), d_head, d_tail, d_edges, d_stats, cap, st);
        hipLaunchKernelGGL((piece_seam_kernel<dt()>), grid, dim3(PIECE_NT), 0, ctx->stream, cfg, static_cast<const int *>(d_cnt),
                           static_cast<const int *>(d_last), static_cast<const int *>(d_base), static_cast<const PiecePart *>(d_head),
                           static_cast<const PiecePart *>(d_tail), d_stats, cap);
        return 0;
    });
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    // (the context's stream does not block on torch's: the caller may read the tables, or free d_samples, as soon as this returns)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const SmallLayout hs = *ctx->h_small.as<SmallLayout>();
    if (int rc = check_status(ctx, static_cast<unsigned>(hs.status))) return rc;
    if (static_cast<unsigned>(hs.status) & ST_WIDE_RANGE)
        return fail(ctx, PS_ERR_ARG, "counts too wide: a float32 sample lies more than %d counts from its piece's first (the sums of squares could overflow)", plan.span_max);
    const int64_t pieces = static_cast<int64_t>(hs.dense);
    *n_pieces_out = pieces;
    if (!piece_capacity_ok(pieces, cap)) return fail(ctx, PS_ERR_CAPACITY, "piece capacity %lld < %lld", static_cast<long long>(cap), static_cast<long long>(pieces));
    return PS_OK;
}

// File.parse + Event.parse for a whole file trace with ONE pass over its samples (round 6).  The two calls
// ps_detect_events + ps_segment_events stream the samples twice: once for the detector's edges and extremes, once -- the 92 %
// of them that lie in events -- for K0's block sums.  Here K0 runs over the WHOLE trace as one event (its blocks aligned to the
// trace) and judges every block against the detector's threshold on its way (DevCfg::blk_cls: 2 bits per block, min / max per 128
// blocks), the detector reads those bits -- 1/64 of the samples' bytes -- instead of the samples (edge_cls_kernel), and the
// events it cuts out -- they start at any sample -- are segmented from the same digest: an event that starts ph = start mod 8
// samples into a block is scanned in coordinates shifted by ph (EvRef::ph, scan_window_ph).  Same events, same boundaries, same
// statistics (to the last bits of the final fp64 expressions) as the two calls (tests/test_single_pass.py, tools/r6/fuzz_single_pass.py).  Falls back to the two calls by itself
// when the block-sum scan does not apply (min_width < 8, W > 64 512, options) or the trace's counts leave the 32-bit digest
// about its first sample (|k - k_0| >= 2^14: the sums are centred on the trace's first sample here, not on each event's).
int ps_detect_segment_trace(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n,
                            double threshold, int64_t min_duration, double min_current, const ps_split_params *params,
                            int64_t *h_starts, int64_t *h_lengths, int64_t ev_cap, int64_t *n_events_out,
                            int32_t *d_bounds, int64_t cap, int64_t *h_bounds_off, ps_segstat *d_stats)
{
    if (!ctx) return PS_ERR_ARG;
    nt_reset(ctx);                                     // (a call that fails from here on reports "not counted")
    if (!n_events_out || !params || !h_bounds_off || n < 0 || n > 0x7fffffff - 16 || ev_cap < 0 || cap < 0 ||
        (ev_cap > 0 && (!h_starts || !h_lengths)) || (cap > 0 && !d_bounds))
        return fail(ctx, PS_ERR_ARG, "bad argument");
    *n_events_out = 0;
    h_bounds_off[0] = 0;
    if (n == 0) { ctx->nt.seen = 0; return PS_OK; }
    if (!d_samples) return fail(ctx, PS_ERR_ARG, "d_samples is NULL");
    SegCall call;
    int rc = begin_segment_call(ctx, d_samples, fmt, params, nullptr, nullptr, 0, &call);
    if (rc) return rc;
    const auto t_begin = call.t_begin;
    const int mw = call.mw, W = call.W;
    DevCfg &cfg = call.cfg;
    auto two_calls = [&]() -> int {
        int r2 = ps_detect_events(ctx, d_samples, fmt, n, threshold, min_duration, min_current, h_starts, h_lengths, ev_cap, n_events_out);
        if (r2) return r2;
        return ps_segment_events(ctx, d_samples, fmt, h_starts, h_lengths, static_cast<int32_t>(*n_events_out), params, d_bounds, cap,
                                 h_bounds_off, d_stats, nullptr);
    };
    const bool use_bs = scan_route_bs(ctx->opt.scan_bs != 0, mw, W, ctx->opt.mode == MODE_EXACT, false) && !ctx->opt.stitch_host && ctx->opt.single_pass &&
                        !ctx->wide.remembers(fmt->quantum);
    if (!use_bs) return two_calls();
    rc = nt_arm(ctx, cfg);
    if (rc) return rc;
    reset_call_stats(ctx);
    ctx->d_is_spine = nullptr;
    if (ctx->opt.timing >= 1) HIP_TRY(ctx, hipEventRecord(ctx->ev[8], ctx->stream));
    // ---- K0 over the whole trace: one event [0, n), blocks aligned to the trace, per-block extremes on -------------------------
    const int64_t nb_total = (n + 7) / 8, nb_pad = k0_padded_blocks(nb_total);
    DigestWant want;
    want.grp = ctx->opt.groups != 0;
    want.blk_mm = d_stats != nullptr;
    want.cls = true;
    rc = reserve_digest(ctx, nb_pad, 1, want);
    if (rc) return rc;
    HIP_TRY(ctx, ctx->det_cand.reserve(4 * sizeof(int64_t)));
    // below(k) <=> double(k) * q < threshold (below_thr): monotone in k, so there is ONE integer kthr with below(k) <=> k < kthr
    int kthr;
    {
        const double q = cfg.q;
        double kk = std::ceil(threshold / q);
        kk = std::max(-2147483000.0, std::min(2147483000.0, kk));
        long long k = static_cast<long long>(kk);
        while (k > -2147483000LL && !(static_cast<double>(k - 1) * q < threshold)) --k;
        while (k < 2147483000LL && static_cast<double>(k) * q < threshold) ++k;
        kthr = static_cast<int>(k);
    }
    // (one launch: the status block cleared, the table of the call's one event -- the whole trace -- written)
    hipLaunchKernelGGL(trace_setup_kernel, dim3(1), dim3(256), 0, ctx->stream, reinterpret_cast<unsigned long long *>(ctx->small.p),
                       static_cast<int>(sizeof(SmallLayout) / sizeof(unsigned long long)), ctx->det_cand.as<long long>(),
                       static_cast<long long>(n), static_cast<long long>(nb_total));
    HIP_TRY(ctx, hipGetLastError());
    cfg.grp = ctx->opt.groups ? ctx->grp.p : nullptr;
    cfg.blk_mm = d_stats ? ctx->blk_mm.as<int>() : nullptr;
    cfg.blk_cls = ctx->blk_cls.as<unsigned char>();
    cfg.cls_mm = ctx->cls_mm.as<int2>();
    cfg.cls_kthr = kthr;
    {
        // (the narrow digest, on the context's own stream, with the per-block verdicts cfg names)
        const int64_t *d_ev = ctx->det_cand.as<int64_t>();
        K0Call k0 = {d_ev, d_ev + 1, d_ev + 2, 1, n, nb_pad};
        k0.admit = true;
        rc = launch_k0<0>(ctx, cfg, ctx->stream, k0);
        if (rc) return rc;
        rc = k0_done(ctx, ctx->stream);
        if (rc) return rc;
    }
    // ---- the detector on K0's verdicts per block ----------------------------------------------------------------------------
    std::vector<int> tics;
    unsigned st = 0;
    rc = detect_edges(ctx, cfg, n, threshold, true, tics, &st);
    if (rc) return rc;
    if (st & ST_WIDE_RANGE) { ctx->counters[PS_CNT_WIDE_REDO] = 3; const int r2 = two_calls(); ctx->counters[PS_CNT_WIDE_REDO] = 3; return r2; }    // counts too wide about the trace's first sample
    rc = events_from_edges(ctx, cfg, n, tics, threshold, min_duration, min_current, h_starts, h_lengths, ev_cap, n_events_out);
    if (rc) return rc;
    const int32_t n_ev = static_cast<int32_t>(*n_events_out);
    if (n_ev == 0) { ctx->nt.seen = 0; return PS_OK; }    // (no event, no window: none)
    for (int e = 0; e < n_ev; ++e)
        if (h_lengths[e] > 0x7fffffff - 2LL * W - 16) return fail(ctx, PS_ERR_ARG, "event %d length %lld out of range", e, static_cast<long long>(h_lengths[e]));
    // ---- every event from the trace's digest ----------------------------------------------------------------------------------
    cfg.bsum = ctx->bsum.p;
    cfg.blk_cls = nullptr;
    const SegBatch B = {h_starts, h_lengths, n_ev, mw, W, d_bounds, cap, h_bounds_off, d_stats, t_begin};
    rc = device_stitch_batch(ctx, cfg, 1, B, true);
    if (rc == RC_FALLBACK || rc == RC_WIDE) {          // (a seam the device could not mend: the two calls, with the host stitch behind them)
        return ps_segment_events(ctx, d_samples, fmt, h_starts, h_lengths, n_ev, params, d_bounds, cap, h_bounds_off, d_stats, nullptr);
    }
    if (rc == PS_OK) nt_keep(ctx, h_starts, h_lengths, n_ev);
    else ctx->nt.seen = -1;
    return rc;
}

int ps_get_near_ties(const ps_ctx *ctx, ps_near_tie *out, int32_t cap, int64_t *n_out)
{
    if (!ctx || !n_out || cap < 0 || (cap > 0 && !out)) return PS_ERR_ARG;
    if (ctx->nt.seen < 0) { *n_out = PS_NT_NOT_COUNTED; return PS_OK; }
    if (ctx->nt.seen > ctx->nt.call_cap) { *n_out = PS_NT_INCOMPLETE; return PS_OK; }
    if (ctx->nt.seen == 0) { *n_out = 0; return PS_OK; }
    std::vector<NtRec> rec(static_cast<size_t>(ctx->nt.seen));
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipMemcpyAsync(rec.data(), static_cast<const char *>(ctx->nt.log.p) + offsetof(NtLog, rec), rec.size() * sizeof(NtRec), hipMemcpyDeviceToHost,
                       ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipGetLastError(); return PS_ERR_HIP; }
    // each record to every event that holds its window (events may overlap in ps_segment_events): events by start, the
    // largest end so far, walked back from the last event that starts at or before the window
    const int64_t *st = ctx->nt.ev_start.data(), *ln = ctx->nt.ev_len.data();
    const size_t ne = ctx->nt.ev_start.size();
    std::vector<int32_t> ord(ne);
    for (size_t e = 0; e < ne; ++e) ord[e] = static_cast<int32_t>(e);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return st[a] < st[b]; });
    std::vector<int64_t> reach(ne);
    for (size_t i = 0; i < ne; ++i) reach[i] = std::max(i ? reach[i - 1] : INT64_MIN, st[ord[i]] + ln[ord[i]]);
    std::vector<ps_near_tie> sites;
    for (const NtRec &r : rec) {
        const int64_t g = r.start, ge = r.start + r.len;
        size_t i = static_cast<size_t>(std::upper_bound(ord.begin(), ord.end(), g, [&](int64_t v, int32_t e) { return v < st[e]; }) - ord.begin());
        while (i > 0 && reach[i - 1] >= ge) {
            const int32_t e = ord[--i];
            if (st[e] <= g && ge <= st[e] + ln[e]) {
                // (the device keeps the split relative to the window's start; the ABI reports it as an index of the event)
                const int32_t ws = static_cast<int32_t>(g - st[e]);
                sites.push_back({e, ws, static_cast<int32_t>(ge - st[e]), r.split < 0 ? -1 : ws + r.split});
            }
        }
    }
    auto key = [](const ps_near_tie &a) { return std::make_tuple(a.event, a.window_start, a.window_end, a.split); };
    std::sort(sites.begin(), sites.end(), [&](const ps_near_tie &a, const ps_near_tie &b) { return key(a) < key(b); });
    sites.erase(std::unique(sites.begin(), sites.end(), [&](const ps_near_tie &a, const ps_near_tie &b) { return key(a) == key(b); }),
                sites.end());
    *n_out = static_cast<int64_t>(sites.size());
    if (sites.size() > static_cast<size_t>(cap)) return PS_ERR_CAPACITY;
    std::copy(sites.begin(), sites.end(), out);
    return PS_OK;
}

int ps_get_timings(const ps_ctx *ctx, double *ms, int32_t n_ms, int64_t *counters, int32_t n_counters)
{
    if (!ctx) return PS_ERR_ARG;
    for (int i = 0; i < n_ms && ms; ++i) ms[i] = i < PS_MS_COUNT ? ctx->ms[i] : 0.0;
    for (int i = 0; i < n_counters && counters; ++i) counters[i] = i < PS_CNT_COUNT ? ctx->counters[i] : 0;
    return PS_OK;
}

// The context's twenty work counters where ps_get_timings copies them from: a host that looks at one of them after every
// call (the near-tie count, PS_CNT_NEAR_TIES) reads it in place instead of making a second call.
const int64_t *ps_counters(const ps_ctx *ctx) { return ctx ? ctx->counters : nullptr; }

int ps_synth_trace(ps_ctx *ctx, void *d_out, int32_t dtype, int64_t n, uint64_t seed,
                   const int64_t *h_seg_end, const int32_t *h_level_counts, int64_t nseg)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_out || n < 0 || nseg < 1 || !h_seg_end || !h_level_counts) return fail(ctx, PS_ERR_ARG, "bad argument");
    if (h_seg_end[nseg - 1] < n) return fail(ctx, PS_ERR_ARG, "segment table does not cover n");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t b1 = static_cast<size_t>(nseg) * sizeof(int64_t), b2 = static_cast<size_t>(nseg) * sizeof(int32_t);
    HIP_TRY(ctx, ctx->tree_scratch.reserve(b1 + b2));
    char *d = ctx->tree_scratch.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(d, h_seg_end, b1, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d + b1, h_level_counts, b2, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pageable host sources must outlive the copy
    hipLaunchKernelGGL(synth_kernel, dim3(4096), dim3(256), 0, ctx->stream, d_out, dtype, n,
                       static_cast<unsigned long long>(seed), reinterpret_cast<const int64_t *>(d),
                       reinterpret_cast<const int32_t *>(d + b1), nseg);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

}  // extern "C"

namespace {

// Host arrays staged back to back through h_up and copied to the start of `dev` in one transfer (the layout is the caller's:
// 8-byte tables before 4-byte ones).  The first `head` bytes are not copied from anywhere: fill(h_up) writes them in place.
struct HostTable { const void *p; size_t bytes; };
template <typename Fill>
int upload_tables(ps_ctx *ctx, DevBuf &dev, size_t head, Fill &&fill, const HostTable *first, const HostTable *last)
{
    size_t bytes = head;
    for (const HostTable *t = first; t != last; ++t) bytes += t->bytes;
    HIP_TRY(ctx, ctx->h_up.reserve(bytes));
    HIP_TRY(ctx, dev.reserve(bytes));
    fill(ctx->h_up.p);
    char *h = static_cast<char *>(ctx->h_up.p) + head;
    for (const HostTable *t = first; t != last; ++t) {
        if (t->bytes) std::memcpy(h, t->p, t->bytes);
        h += t->bytes;
    }
    HIP_TRY(ctx, hipMemcpyAsync(dev.p, ctx->h_up.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PS_OK;
}
template <typename Fill>
int upload_tables(ps_ctx *ctx, DevBuf &dev, size_t head, Fill &&fill, std::initializer_list<HostTable> tables)
{
    return upload_tables(ctx, dev, head, fill, tables.begin(), tables.end());
}
int upload_tables(ps_ctx *ctx, DevBuf &dev, std::initializer_list<HostTable> tables)
{
    return upload_tables(ctx, dev, 0, [](void *) {}, tables.begin(), tables.end());
}

// The sample format of a filter call as the kernels' DevCfg: float32 on a grid / int16 counts as everywhere, or -- the filter
// entries only -- PS_DTYPE_F64, the current itself.
int filter_cfg(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, DevCfg *cfg)
{
    if (fmt && fmt->dtype == PS_DTYPE_F64) {
        const ps_sample_format f32 = {PS_DTYPE_F32, 0, 1.0};
        if (int rc = make_cfg(ctx, d_samples, &f32, 1, 1, 2, 0.0, cfg)) return rc;
        cfg->dtype = PS_DTYPE_F64; cfg->q = 1.0; cfg->q2 = 1.0; cfg->inv_q = 1.0f;
        return PS_OK;
    }
    return make_cfg(ctx, d_samples, fmt, 1, 1, 2, 0.0, cfg);
}

// scipy.signal.bessel(1, wn, 'low', analog=False): one real pole, bilinear transform with pre-warping (fs = 2)
FiltCoef filter_coef1(double wn)
{
    FiltCoef f;
    const double wo = 4.0 * std::tan(3.14159265358979323846 * wn / 2.0);
    f.b0 = wo / (4.0 + wo); f.b1 = f.b0; f.a1 = (wo - 4.0) / (wo + 4.0);
    f.alpha = -f.a1; f.beta = f.b1 - f.a1 * f.b0;
    f.zi = (f.b1 - f.a1 * f.b0) / (1.0 + f.a1);        // lfilter_zi: steady state of the delay for a unit step input
    return f;
}

// scipy.signal.bessel(N, wn, 'low', analog=False, output='ba') for N = 2..8: poles of the phase-normalised analog
// prototype (what scipy.signal.besselap(N, 'phase') returns; conjugates implied), lp2lp with the pre-warped frequency,
// bilinear transform with fs = 2, polynomial expansion.  Then lfilter_zi (steady state of the delays for a unit step:
// (I - A) zi = B), the halo H from the powers of the state matrix and the segment length S.
struct FiltDesignN { FiltN f; int H, S; };
int filter_design_n(ps_ctx *ctx, int order, double wn, FiltDesignN *design)
{
    typedef std::complex<double> cd;
    static const double poles[FILT_MAXORD + 1][4][2] = {       // [order][pair][re, im]; im == 0: a single real pole
        {{0, 0}}, {{-0.9999999999999998, 0.0}},
        {{-0.8660254037844384, 0.4999999999999999}},
        {{-0.9416000265332067, 0.0}, {-0.7456403858480766, 0.7113666249728351}},
        {{-0.9047587967882447, 0.27091873300387465}, {-0.6572111716718827, 0.830161435004873}},
        {{-0.9264420773877602, 0.0}, {-0.8515536193688396, 0.44271746394433265}, {-0.5905759446119191, 0.9072067564574549}},
        {{-0.9093906830472273, 0.1856964396793047}, {-0.7996541858328288, 0.5621717346937318}, {-0.5385526816693109, 0.9616876881954278}},
        {{-0.919487155649029, 0.0}, {-0.8800029341523375, 0.32166527623077396}, {-0.7527355434093214, 0.6504696305522552},
         {-0.4966917256672317, 1.0025085084544205}},
        {{-0.909683154665291, 0.1412437976671423}, {-0.8473250802359334, 0.42590175382729345}, {-0.7111381808485397, 0.7186517314108402},
         {-0.4621740412532123, 1.0343886811269012}}};
    const double wo = 4.0 * std::tan(3.14159265358979323846 * wn / 2.0);
    std::vector<cd> p;
    for (int k = 0; k < (order + 1) / 2; ++k) {
        const double re = poles[order][k][0], im = poles[order][k][1];
        if (im == 0.0) p.push_back(cd(re * wo, 0.0));
        else { p.push_back(cd(re, im) * wo); p.push_back(cd(re, -im) * wo); }
    }
    cd den(1.0, 0.0);
    for (const cd &q : p) den *= (cd(4.0, 0.0) - q);
    const double gain = std::pow(wo, order) * (cd(1.0, 0.0) / den).real();
    std::vector<cd> ac(order + 1, cd(0.0, 0.0));
    ac[0] = cd(1.0, 0.0);
    for (int k = 0; k < order; ++k) {
        const cd pz = (cd(4.0, 0.0) + p[k]) / (cd(4.0, 0.0) - p[k]);
        for (int j = k + 1; j >= 1; --j) ac[j] = ac[j] - pz * ac[j - 1];
    }
    std::vector<double> bc(order + 1, 0.0);
    bc[0] = 1.0;
    for (int k = 0; k < order; ++k)
        for (int j = k + 1; j >= 1; --j) bc[j] += bc[j - 1];
    FiltN f = {};
    f.order = order; f.pad = 3 * (order + 1);
    for (int j = 0; j <= order; ++j) { f.a[j] = ac[j].real(); f.b[j] = gain * bc[j]; }
    // state matrix A (z' = A z + B x) and zi = (I - A)^-1 B by Gaussian elimination with pivoting
    double A[FILT_MAXORD][FILT_MAXORD] = {}, M[FILT_MAXORD][FILT_MAXORD + 1] = {};
    for (int r = 0; r < order; ++r) {
        A[r][0] = -f.a[r + 1];
        if (r + 1 < order) A[r][r + 1] += 1.0;
        for (int c2 = 0; c2 < order; ++c2) M[r][c2] = (r == c2 ? 1.0 : 0.0) - A[r][c2];
        M[r][order] = f.b[r + 1] - f.a[r + 1] * f.b[0];
    }
    for (int c2 = 0; c2 < order; ++c2) {
        int piv = c2;
        for (int r = c2 + 1; r < order; ++r) if (std::fabs(M[r][c2]) > std::fabs(M[piv][c2])) piv = r;
        if (M[piv][c2] == 0.0) return fail(ctx, PS_ERR_ARG, "filter has no steady state");
        for (int k = 0; k <= order; ++k) std::swap(M[c2][k], M[piv][k]);
        for (int r = 0; r < order; ++r) {
            if (r == c2) continue;
            const double g = M[r][c2] / M[c2][c2];
            for (int k = c2; k <= order; ++k) M[r][k] -= g * M[c2][k];
        }
    }
    for (int r = 0; r < order; ++r) f.zi[r] = M[r][order] / M[r][r];
    // halo: smallest multiple of 64 with ||A^H||_inf <= 2^-70 (A^64 by squaring, then one factor per step)
    auto mul = [&](const double X[FILT_MAXORD][FILT_MAXORD], const double Y[FILT_MAXORD][FILT_MAXORD], double Z[FILT_MAXORD][FILT_MAXORD]) {
        double T[FILT_MAXORD][FILT_MAXORD] = {};
        for (int i = 0; i < order; ++i) for (int j = 0; j < order; ++j) for (int k = 0; k < order; ++k) T[i][j] += X[i][k] * Y[k][j];
        std::memcpy(Z, T, sizeof(T));
    };
    double A64[FILT_MAXORD][FILT_MAXORD], P[FILT_MAXORD][FILT_MAXORD];
    std::memcpy(A64, A, sizeof(A));
    for (int k = 0; k < 6; ++k) mul(A64, A64, A64);
    std::memcpy(P, A64, sizeof(P));
    int H = 0;
    for (int h = 64; h <= 8192; h += 64) {
        double nrm = 0.0;
        for (int i = 0; i < order; ++i) { double r = 0.0; for (int j = 0; j < order; ++j) r += std::fabs(P[i][j]); nrm = std::max(nrm, r); }
        if (nrm <= 8.47e-22) { H = h; break; }          // 2^-70
        mul(P, A64, P);
    }
    if (!H) return fail(ctx, PS_ERR_ARG, "a Bessel filter of order %d this slow (cutoff / Nyquist = %g) does not run on the device", order, wn);
    design->f = f; design->H = H; design->S = std::max(1024, 4 * H);
    return PS_OK;
}

// One event, orders 2..8: the design above and one launch of filt_halo_kernel.
int filter_order_n(ps_ctx *ctx, const DevCfg &cfg, int64_t n, int order, double wn, double *d_out)
{
    FiltDesignN design;
    if (int rc = filter_design_n(ctx, order, wn, &design)) return rc;
    const FiltN &f = design.f;
    const int H = design.H, S = design.S;
    const int64_t m = n + 2LL * f.pad, nseg = (m + S - 1) / S;
    HIP_TRY(ctx, ctx->filt.fwd.reserve(static_cast<size_t>(nseg) * static_cast<size_t>(S + H) * sizeof(double)));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    if (!ctx->defer_sync) HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    unsigned *st = reinterpret_cast<unsigned *>(&ctx->small.as<SmallLayout>()->status);
    const dim3 grid(static_cast<unsigned>((nseg + 63) / 64));
    if (cfg.dtype == PS_DTYPE_F32)      hipLaunchKernelGGL((filt_halo_kernel<PS_DTYPE_F32>), grid, dim3(64), 0, ctx->stream, cfg, f, n, S, H, ctx->filt.fwd.as<double>(), d_out, st);
    else if (cfg.dtype == PS_DTYPE_F64) hipLaunchKernelGGL((filt_halo_kernel<PS_DTYPE_F64>), grid, dim3(64), 0, ctx->stream, cfg, f, n, S, H, ctx->filt.fwd.as<double>(), d_out, st);
    else                                hipLaunchKernelGGL((filt_halo_kernel<PS_DTYPE_I16>), grid, dim3(64), 0, ctx->stream, cfg, f, n, S, H, ctx->filt.fwd.as<double>(), d_out, st);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->defer_sync) return PS_OK;                   // (a batch: one status check for all of its events)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
}
}  // namespace

extern "C" {

int ps_filter_bessel(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, int32_t order,
                     double cutoff, double sampling_freq, double *d_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_samples || !d_out) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (order < 1 || order > FILT_MAXORD)
        return fail(ctx, PS_ERR_ARG, "Bessel orders 1..%d run on the device (the reference's default is 1)", FILT_MAXORD);
    const int padlen = 3 * (order + 1);                  // scipy: 3 * max(len(a), len(b))
    if (n <= padlen) return fail(ctx, PS_ERR_ARG, "the length of the input must be greater than padlen, which is %d", padlen);
    const double wn = cutoff / (sampling_freq / 2.0);
    if (!(wn > 0.0) || !(wn < 1.0)) return fail(ctx, PS_ERR_ARG, "cutoff must lie strictly between 0 and the Nyquist frequency");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevCfg cfg;
    if (int rc = filter_cfg(ctx, d_samples, fmt, &cfg)) return rc;
    if (order > 1) return filter_order_n(ctx, cfg, n, order, wn, d_out);
    const FiltCoef f = filter_coef1(wn);
    FiltGeom g;
    g.n = n; g.total = n + 2 * FILT_PAD;
    // Fast filters (the state forgets within a halo of <= 1024 samples): both directions in one kernel over tiles
    // with halos.  alpha^H <= 2^-60.  The route is filt_plan.hpp's: the batch entry takes the same one.
    {
        const int H = filt_route1(f.alpha, ctx->opt.filter_fused);
        if (H) {
            g.lead = 0; g.padded = g.total;
            const int T = filt_tile(H);
            const dim3 fgrid(static_cast<unsigned>(filt_units(n, FILT_PAD, T)));
            HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
            if (!ctx->defer_sync) HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
            unsigned *fst = reinterpret_cast<unsigned *>(&ctx->small.as<SmallLayout>()->status);
            if (cfg.dtype == PS_DTYPE_F32)      hipLaunchKernelGGL((filt_fused_kernel<PS_DTYPE_F32>), fgrid, dim3(FILT_NT), 0, ctx->stream, cfg, f, g, H, d_out, fst);
            else if (cfg.dtype == PS_DTYPE_F64) hipLaunchKernelGGL((filt_fused_kernel<PS_DTYPE_F64>), fgrid, dim3(FILT_NT), 0, ctx->stream, cfg, f, g, H, d_out, fst);
            else                                hipLaunchKernelGGL((filt_fused_kernel<PS_DTYPE_I16>), fgrid, dim3(FILT_NT), 0, ctx->stream, cfg, f, g, H, d_out, fst);
            HIP_TRY(ctx, hipGetLastError());
            if (ctx->defer_sync) return PS_OK;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
        }
    }
    const int64_t n_chunks = (g.total + FILT_CHUNK - 1) / FILT_CHUNK;
    g.padded = n_chunks * FILT_CHUNK;                  // the intermediate is stored behind a lead-in (seg_filter.hpp)
    g.lead = g.padded - g.total;
    HIP_TRY(ctx, ctx->filt.fwd.reserve(static_cast<size_t>(g.padded) * sizeof(double)));
    HIP_TRY(ctx, ctx->filt.agg.reserve(static_cast<size_t>(n_chunks) * 2 * sizeof(double2)));
    HIP_TRY(ctx, ctx->filt.zin.reserve(static_cast<size_t>(n_chunks) * sizeof(double)));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    if (!ctx->defer_sync) HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    SmallLayout *sm = ctx->small.as<SmallLayout>();
    unsigned *st = reinterpret_cast<unsigned *>(&sm->status);
    double *fwd = ctx->filt.fwd.as<double>();
    double2 *agg = ctx->filt.agg.as<double2>(), *agg_b = agg + n_chunks;
    double *zin = ctx->filt.zin.as<double>();
    const dim3 grid(static_cast<unsigned>(n_chunks));
#define PS_FILT(DT)                                                                                                          \
    hipLaunchKernelGGL((filt_local_kernel<DT>), grid, dim3(FILT_NT), 0, ctx->stream, cfg, f, g, agg, st);                     \
    hipLaunchKernelGGL((filt_carry_kernel<0, DT>), dim3(1), dim3(1024), 0, ctx->stream, cfg, f, fwd, g, agg, n_chunks, zin);   \
    hipLaunchKernelGGL((filt_apply_kernel<0, DT>), grid, dim3(FILT_NT), 0, ctx->stream, cfg, f, fwd, g, zin, fwd, agg_b, st); \
    hipLaunchKernelGGL((filt_carry_kernel<1, DT>), dim3(1), dim3(1024), 0, ctx->stream, cfg, f, fwd, g, agg_b, n_chunks, zin); \
    hipLaunchKernelGGL((filt_apply_kernel<1, DT>), grid, dim3(FILT_NT), 0, ctx->stream, cfg, f, fwd, g, zin, d_out, agg_b, st);
    if (cfg.dtype == PS_DTYPE_F32) { PS_FILT(PS_DTYPE_F32) } else if (cfg.dtype == PS_DTYPE_F64) { PS_FILT(PS_DTYPE_F64) } else { PS_FILT(PS_DTYPE_I16) }
#undef PS_FILT
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->defer_sync) return PS_OK;                   // (a batch: one status check for all of its events)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
}

int ps_requantise(ps_ctx *ctx, const double *d_in, int64_t n, float *d_out, double *centre_out, double *step_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_in || !d_out || !centre_out || !step_out || n < 1) return fail(ctx, PS_ERR_ARG, "null pointer or empty input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(1024, (n + 8 * RQ_NT - 1) / (8 * RQ_NT)));
    HIP_TRY(ctx, ctx->filt.agg.reserve(static_cast<size_t>(grid) * 3 * sizeof(double)));
    HIP_TRY(ctx, ctx->h_meta.reserve(static_cast<size_t>(grid) * 3 * sizeof(double)));
    hipLaunchKernelGGL(requant_stats_kernel, dim3(grid), dim3(RQ_NT), 0, ctx->stream, d_in, static_cast<long long>(n), ctx->filt.agg.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->filt.agg.p, static_cast<size_t>(grid) * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const double *part = ctx->h_meta.as<double>();
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    for (unsigned g = 0; g < grid; ++g) { sum += part[3 * g]; mn = std::min(mn, part[3 * g + 1]); mx = std::max(mx, part[3 * g + 2]); }
    if (!std::isfinite(sum) || !std::isfinite(mn) || !std::isfinite(mx)) return fail(ctx, PS_ERR_ARG, "the current holds NaN or infinity");
    double centre = sum / static_cast<double>(n);
    const double span = std::max(mx - centre, centre - mn);              // = max |x - centre| (subtraction is monotone)
    const double step = span > 0.0 ? std::ldexp(1.0, static_cast<int>(std::ceil(std::log2(span * 1.01))) - 22) : 1.0;
    centre = std::nearbyint(centre / step) * step;
    const unsigned rg = static_cast<unsigned>(std::min<int64_t>(65535, (n + 4 * RQ_NT - 1) / (4 * RQ_NT)));
    hipLaunchKernelGGL(requant_round_kernel, dim3(rg), dim3(RQ_NT), 0, ctx->stream, d_in, static_cast<long long>(n), centre, 1.0 / step, step, d_out);
    HIP_TRY(ctx, hipGetLastError());
    // (the context's stream does not block on torch's: the caller may read d_out, or free d_in, as soon as this returns)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *centre_out = centre; *step_out = step;
    return PS_OK;
}

// ---- float64 currents on the device back to their ADC grid (seg_ingest.hpp; grid.affine_grid_device, engine.to_device_with_counts) ----
static int ingest_args(ps_ctx *ctx, const double *d_in, int64_t n)
{
    if (!d_in || n < 1) return fail(ctx, PS_ERR_ARG, "null pointer or empty input");
    if (reinterpret_cast<uintptr_t>(d_in) & 7u) return fail(ctx, PS_ERR_ARG, "float64 samples must be 8-byte aligned");
    return PS_OK;
}

int ps_grid_check_f64(ps_ctx *ctx, const double *d_in, int64_t n, double origin, double quantum, double tol, ps_grid_report *out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!out) return fail(ctx, PS_ERR_ARG, "null pointer or empty input");
    if (int rc = ingest_args(ctx, d_in, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned grid = ingest_grid(n);
    HIP_TRY(ctx, ctx->filt.agg.reserve(static_cast<size_t>(grid) * sizeof(GridPartial)));
    HIP_TRY(ctx, ctx->h_meta.reserve(static_cast<size_t>(grid) * sizeof(GridPartial)));
    hipLaunchKernelGGL(grid_check_kernel, dim3(grid), dim3(ING_NT), 0, ctx->stream, ingest_span(d_in, n), static_cast<long long>(n), d_in,
                       origin, quantum, tol, ctx->filt.agg.as<GridPartial>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->filt.agg.p, static_cast<size_t>(grid) * sizeof(GridPartial), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const GridPartial *part = ctx->h_meta.as<GridPartial>();
    ps_grid_report r = {0.0, INFINITY, INFINITY, -INFINITY, 0, 0};
    for (unsigned g = 0; g < grid; ++g) {                                // (minima, maxima and counts: any order gives the same)
        r.max_frac = std::fmax(r.max_frac, part[g].max_frac); r.min_frac_above = std::fmin(r.min_frac_above, part[g].min_frac_above);
        r.min_count = std::fmin(r.min_count, part[g].min_count); r.max_count = std::fmax(r.max_count, part[g].max_count);
        r.n_nonfinite += static_cast<int64_t>(part[g].n_nonfinite); r.n_undefined += static_cast<int64_t>(part[g].n_undefined);
    }
    *out = r;
    return PS_OK;
}

int ps_grid_counts_f64(ps_ctx *ctx, const double *d_in, int64_t n, double origin, double quantum, int64_t centre, int16_t *d_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_out) return fail(ctx, PS_ERR_ARG, "null pointer or empty input");
    if (int rc = ingest_args(ctx, d_in, n)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 1u) return fail(ctx, PS_ERR_ARG, "int16 counts must be 2-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(grid_counts_kernel, dim3(ingest_grid(n)), dim3(ING_NT), 0, ctx->stream, ingest_span(d_in, n), static_cast<long long>(n), d_in,
                       origin, quantum, static_cast<long long>(centre), reinterpret_cast<short *>(d_out));
    HIP_TRY(ctx, hipGetLastError());
    // (the context's stream does not block on torch's: the caller may read d_out, or free d_in, as soon as this returns)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_narrow_f64(ps_ctx *ctx, const double *d_in, int64_t n, float *d_out, int64_t *n_inexact_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (!d_out || !n_inexact_out) return fail(ctx, PS_ERR_ARG, "null pointer or empty input");
    if (int rc = ingest_args(ctx, d_in, n)) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(ctx, PS_ERR_ARG, "float32 samples must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned grid = ingest_grid(n);
    HIP_TRY(ctx, ctx->filt.agg.reserve(static_cast<size_t>(grid) * sizeof(unsigned long long)));
    HIP_TRY(ctx, ctx->h_meta.reserve(static_cast<size_t>(grid) * sizeof(unsigned long long)));
    hipLaunchKernelGGL(narrow_f64_kernel, dim3(grid), dim3(ING_NT), 0, ctx->stream, ingest_span(d_in, n), static_cast<long long>(n), d_in, d_out,
                       ctx->filt.agg.as<unsigned long long>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->filt.agg.p, static_cast<size_t>(grid) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long *part = ctx->h_meta.as<unsigned long long>();
    unsigned long long bad = 0;
    for (unsigned g = 0; g < grid; ++g) bad += part[g];
    *n_inexact_out = static_cast<int64_t>(bad);
    return PS_OK;
}

}  // extern "C"

namespace {

// A batch of events of one device buffer, filtered: validated, planned (filt_plan.hpp) and queued on the context's stream, the
// status block cleared in front of it.  Nothing is queued when the call is refused.  The caller copies the status block back
// with its next synchronisation and checks it (one status word for the batch).  Event e's result goes to d_out + (sum of the
// lengths before e).
//   order 1, fused route: one launch of filt_fused_batch_kernel, one workgroup per (event, tile)
//   orders 2..8:          one launch of filt_halo_batch_kernel per scratch group of the plan (option filt_batch_scratch)
//   order 1, scan route:  no batched kernel -- the events are queued one after the other through ps_filter_bessel, longest first
//                         (its scratch grows at most once, before anything that uses it is in flight)
// rq (optional): the tables of the re-quantisation that follows go up in the same transfer; *d_rq_ev, *d_rq_unit: where they are.
int filter_batch_queue(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const int64_t *ev_start, const int64_t *ev_len,
                       int32_t n_ev, int32_t order, double cutoff, double sampling_freq, double *d_out, const RequantPlan *rq = nullptr,
                       const RequantEvent **d_rq_ev = nullptr, const FiltUnit **d_rq_unit = nullptr)
{
    if (!d_samples || !d_out || !ev_start || !ev_len) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (order < 1 || order > FILT_MAXORD)
        return fail(ctx, PS_ERR_ARG, "Bessel orders 1..%d run on the device (the reference's default is 1)", FILT_MAXORD);
    const double wn = cutoff / (sampling_freq / 2.0);
    if (!(wn > 0.0) || !(wn < 1.0)) return fail(ctx, PS_ERR_ARG, "cutoff must lie strictly between 0 and the Nyquist frequency");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevCfg cfg;
    if (int rc = filter_cfg(ctx, d_samples, fmt, &cfg)) return rc;
    const int pad = filt_padlen(order);
    FiltCoef f1 = {};
    FiltDesignN dn = {};
    int H = 0;
    int64_t unit = FILT_CHUNK, row_bytes = 0;            // (the scan route is planned for its refusals only)
    if (order == 1) {
        f1 = filter_coef1(wn);
        H = filt_route1(f1.alpha, ctx->opt.filter_fused);
        if (H) unit = filt_tile(H);
    } else {
        if (int rc = filter_design_n(ctx, order, wn, &dn)) return rc;
        H = dn.H; unit = dn.S;
        row_bytes = static_cast<int64_t>(dn.S + dn.H) * static_cast<int64_t>(sizeof(double));
    }
    const bool per_event = order == 1 && !H;
    FiltPlan plan;
    switch (plan_filter_batch(ev_start, ev_len, n_ev, pad, unit, row_bytes, ctx->opt.filt_batch_scratch, &plan)) {
    case FILT_PLAN_OK: break;
    case FILT_PLAN_RANGE: return fail(ctx, PS_ERR_ARG, "event %d: empty or negative range", plan.bad_event);
    case FILT_PLAN_SHORT:
        return fail(ctx, PS_ERR_ARG, "event %d: the length of the input must be greater than padlen, which is %d", plan.bad_event, pad);
    default: return fail(ctx, PS_ERR_ARG, "too many samples for one call");
    }
    // (a launch holds fewer than 2^32 threads)
    if (plan.unit.size() > 0xffffffu || (rq && rq->unit.size() > 0xffffffu)) return fail(ctx, PS_ERR_ARG, "too many samples for one call");
    size_t rows_max = 0;
    for (const FiltGroup &g : plan.group) rows_max = std::max(rows_max, static_cast<size_t>(g.units));
    if (row_bytes) HIP_TRY(ctx, ctx->filt.fwd.reserve(rows_max * static_cast<size_t>(row_bytes)));
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    ctx->small_clean = false;
    const size_t ne = static_cast<size_t>(n_ev);
    const size_t b_ev = per_event ? 0 : ne * sizeof(FiltEvent), b_unit = per_event ? 0 : plan.unit.size() * sizeof(FiltUnit);
    const size_t b_rq_ev = rq ? ne * sizeof(RequantEvent) : 0, b_rq_unit = rq ? rq->unit.size() * sizeof(FiltUnit) : 0;
    if (b_ev + b_rq_ev)
        if (int rc = upload_tables(ctx, ctx->filt.tab, {{plan.ev.data(), b_ev}, {rq ? rq->ev.data() : nullptr, b_rq_ev}, {plan.unit.data(), b_unit},
                                                        {rq ? rq->unit.data() : nullptr, b_rq_unit}})) return rc;
    const char *tab = ctx->filt.tab.as<char>();
    const FiltEvent *d_ev = reinterpret_cast<const FiltEvent *>(tab);
    const FiltUnit *d_unit = reinterpret_cast<const FiltUnit *>(tab + b_ev + b_rq_ev);
    if (d_rq_ev) *d_rq_ev = reinterpret_cast<const RequantEvent *>(tab + b_ev);
    if (d_rq_unit) *d_rq_unit = reinterpret_cast<const FiltUnit *>(tab + b_ev + b_rq_ev + b_unit);
    HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    unsigned *st = reinterpret_cast<unsigned *>(&ctx->small.as<SmallLayout>()->status);
    if (per_event) {
        std::vector<int> by_len(ne);
        for (int e = 0; e < n_ev; ++e) by_len[e] = e;
        std::sort(by_len.begin(), by_len.end(), [&](int a, int b) { return ev_len[a] > ev_len[b]; });
        const size_t es = cfg.dtype == PS_DTYPE_I16 ? 2 : cfg.dtype == PS_DTYPE_F64 ? 8 : 4;
        ctx->defer_sync = true;
        int rc = PS_OK;
        for (size_t k = 0; k < ne && rc == PS_OK; ++k) {
            const int e = by_len[k];
            rc = ps_filter_bessel(ctx, static_cast<const char *>(d_samples) + static_cast<size_t>(ev_start[e]) * es, fmt, ev_len[e], order, cutoff,
                                  sampling_freq, d_out + plan.ev[e].out_off);
        }
        ctx->defer_sync = false;
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        return PS_OK;
    }
    if (order == 1) {
        const dim3 grid(static_cast<unsigned>(plan.unit.size()));
#define PS_FILT(DT) hipLaunchKernelGGL((filt_fused_batch_kernel<DT>), grid, dim3(FILT_NT), 0, ctx->stream, cfg, f1, H, d_ev, d_unit, d_out, st);
        if (cfg.dtype == PS_DTYPE_F32) { PS_FILT(PS_DTYPE_F32) } else if (cfg.dtype == PS_DTYPE_F64) { PS_FILT(PS_DTYPE_F64) } else { PS_FILT(PS_DTYPE_I16) }
#undef PS_FILT
    } else {
        double *scratch = ctx->filt.fwd.as<double>();
        for (const FiltGroup &g : plan.group) {            // (one scratch for all groups: they run in stream order)
            const dim3 grid(static_cast<unsigned>((g.units + 63) / 64));
#define PS_FILT(DT) hipLaunchKernelGGL((filt_halo_batch_kernel<DT>), grid, dim3(64), 0, ctx->stream, cfg, dn.f, dn.S, dn.H, d_ev, d_unit, g.unit0, \
                                       g.units, scratch, d_out, st);
            if (cfg.dtype == PS_DTYPE_F32) { PS_FILT(PS_DTYPE_F32) } else if (cfg.dtype == PS_DTYPE_F64) { PS_FILT(PS_DTYPE_F64) } else { PS_FILT(PS_DTYPE_I16) }
#undef PS_FILT
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

}  // namespace

extern "C" {

int ps_filter_bessel_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const int64_t *ev_start, const int64_t *ev_len,
                           int32_t n_ev, int32_t order, double cutoff, double sampling_freq, double *d_out)
{
    if (!ctx) return PS_ERR_ARG;
    if (n_ev < 0) return fail(ctx, PS_ERR_ARG, "null pointer or negative count");
    if (n_ev == 0) return PS_OK;
    if (int rc = filter_batch_queue(ctx, d_samples, fmt, ev_start, ev_len, n_ev, order, cutoff, sampling_freq, d_out)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    // (the context's stream does not block on torch's: the caller may read d_out, or free d_samples, as soon as this returns)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
}

int ps_range_stats(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, int64_t n, const int64_t *h_start, const int64_t *h_end,
                   int64_t n_ranges, ps_segstat *d_stats)
{
    if (!ctx) return PS_ERR_ARG;
    if (n_ranges < 0 || n < 0) return fail(ctx, PS_ERR_ARG, "null pointer or negative count");
    if (n_ranges == 0) return PS_OK;
    if (!d_samples || !fmt || !h_start || !h_end || !d_stats) return fail(ctx, PS_ERR_ARG, "null pointer or negative count");
    if (fmt->dtype == PS_DTYPE_F64)
        return fail(ctx, PS_ERR_ARG, "range statistics take int16 counts or float32 samples on a grid, not float64");
    if (fmt->dtype != PS_DTYPE_F32 && fmt->dtype != PS_DTYPE_I16) return fail(ctx, PS_ERR_ARG, "unknown dtype %d", fmt->dtype);
    // validated and planned (range_plan.hpp) before anything is reserved or queued
    RangePlan plan;
    int64_t bad = -1;
    switch (plan_ranges(h_start, h_end, n_ranges, n, range_unit(fmt->dtype == PS_DTYPE_F32, ctx->opt.range_tile), &plan, &bad)) {
    case RANGE_PLAN_OK: break;
    case RANGE_PLAN_START: return fail(ctx, PS_ERR_ARG, "range %lld: negative start", static_cast<long long>(bad));
    case RANGE_PLAN_END: return fail(ctx, PS_ERR_ARG, "range %lld: ends behind the %lld samples", static_cast<long long>(bad), static_cast<long long>(n));
    case RANGE_PLAN_EMPTY: return fail(ctx, PS_ERR_ARG, "range %lld: empty (end <= start)", static_cast<long long>(bad));
    case RANGE_PLAN_LONG: return fail(ctx, PS_ERR_ARG, "range %lld: longer than 2^31 - 1 samples", static_cast<long long>(bad));
    default: return fail(ctx, PS_ERR_ARG, "too many ranges or units for one call (option range_tile: %lld)", ctx->opt.range_tile);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevCfg cfg;
    if (int rc = make_cfg(ctx, d_samples, fmt, 1, 1, 2, 0.0, &cfg)) return rc;
    const size_t b_row = plan.row.size() * sizeof(RangeRow), n_unit = plan.unit.size();
    HIP_TRY(ctx, ctx->h_small.reserve(sizeof(SmallLayout)));
    HIP_TRY(ctx, ctx->rng.part.reserve(n_unit * sizeof(RangePart)));
    if (int rc = upload_tables(ctx, ctx->rng.tab, {{plan.row.data(), b_row}, {plan.unit.data(), n_unit * sizeof(RangeUnit)}})) return rc;
    const RangeRow *d_row = ctx->rng.tab.as<RangeRow>();
    const RangeUnit *d_unit = reinterpret_cast<const RangeUnit *>(ctx->rng.tab.as<char>() + b_row);
    RangePart *d_part = ctx->rng.part.as<RangePart>();
    HIP_TRY(ctx, hipMemsetAsync(ctx->small.p, 0, sizeof(SmallLayout), ctx->stream));
    unsigned *st = reinterpret_cast<unsigned *>(&ctx->small.as<SmallLayout>()->status);
    const int32_t nr = static_cast<int32_t>(n_ranges);
    by_dtype(cfg.dtype, [&](auto dt) {
        hipLaunchKernelGGL((range_part_kernel<dt()>), dim3(static_cast<unsigned>(n_unit)), dim3(RANGE_NT), 0, ctx->stream, cfg, d_row, d_unit, d_part, st);
        hipLaunchKernelGGL((range_final_kernel<dt()>), dim3(static_cast<unsigned>((n_ranges + RANGE_NT - 1) / RANGE_NT)), dim3(RANGE_NT), 0, ctx->stream,
                           cfg, d_row, nr, static_cast<const RangePart *>(d_part), d_stats);
        return 0;
    });
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    // (the context's stream does not block on torch's: the caller may read d_stats, or free d_samples, as soon as this returns)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
}

int ps_filter_requantise_batch(ps_ctx *ctx, const void *d_samples, const ps_sample_format *fmt, const int64_t *ev_start,
                               const int64_t *ev_len, int32_t n_ev, int32_t order, double cutoff, double sampling_freq,
                               double *d_filtered, float *d_rounded, double *h_centre, double *h_step)
{
    if (!ctx) return PS_ERR_ARG;
    if (n_ev < 0 || (n_ev > 0 && (!d_samples || !fmt || !ev_start || !ev_len || !d_filtered || !d_rounded || !h_centre || !h_step)))
        return fail(ctx, PS_ERR_ARG, "null pointer or negative count");
    if (n_ev == 0) return PS_OK;
    for (int e = 0; e < n_ev; ++e)
        if (ev_len[e] < 1 || ev_start[e] < 0) return fail(ctx, PS_ERR_ARG, "event %d: empty or negative range", e);
    // 1. every event's filter (filter_batch_queue: one launch on the fused route), one status word for all of them; the tables
    //    of steps 2 and 3 go up with the filter's
    RequantPlan rq;
    plan_requant_batch(ev_len, n_ev, &rq);
    const RequantEvent *d_rq_ev = nullptr;
    const FiltUnit *d_rq_unit = nullptr;
    if (int rc = filter_batch_queue(ctx, d_samples, fmt, ev_start, ev_len, n_ev, order, cutoff, sampling_freq, d_filtered, &rq, &d_rq_ev, &d_rq_unit))
        return rc;
    int rc = PS_OK;
    // 2. sum / min / max of every filtered current: one launch, all events' partial results in one copy
    const size_t pbytes = rq.unit.size() * 3 * sizeof(double);
    HIP_TRY(ctx, ctx->filt.agg.reserve(pbytes));         // (the filters above are done with it only in stream order: reserve() may
    HIP_TRY(ctx, ctx->h_meta.reserve(pbytes));           //  free and allocate, which waits for the device -- correct, and rare)
    const dim3 rq_grid(static_cast<unsigned>(rq.unit.size()));
    hipLaunchKernelGGL(requant_stats_batch_kernel, rq_grid, dim3(RQ_NT), 0, ctx->stream, d_filtered, d_rq_ev, d_rq_unit, ctx->filt.agg.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta.p, ctx->filt.agg.p, pbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status));
    if (rc) return rc;
    // 3. centre and grid step per event (ps_requantise's rule) as a table, then the rounding pass: one launch
    const double *part = ctx->h_meta.as<double>();
    std::vector<double> par(3 * static_cast<size_t>(n_ev));
    for (int e = 0; e < n_ev; ++e) {
        double sum = 0.0, mn = INFINITY, mx = -INFINITY;
        const size_t g0 = static_cast<size_t>(rq.ev[e].poff), g1 = g0 + static_cast<size_t>(rq.ev[e].grid);
        for (size_t g = g0; g < g1; ++g) { sum += part[3 * g]; mn = std::min(mn, part[3 * g + 1]); mx = std::max(mx, part[3 * g + 2]); }
        if (!std::isfinite(sum) || !std::isfinite(mn) || !std::isfinite(mx)) return fail(ctx, PS_ERR_ARG, "the current of event %d holds NaN or infinity", e);
        double centre = sum / static_cast<double>(ev_len[e]);
        const double span = std::max(mx - centre, centre - mn);
        const double step = span > 0.0 ? std::ldexp(1.0, static_cast<int>(std::ceil(std::log2(span * 1.01))) - 22) : 1.0;
        centre = std::nearbyint(centre / step) * step;
        h_centre[e] = centre; h_step[e] = step;
        par[3 * static_cast<size_t>(e)] = centre; par[3 * static_cast<size_t>(e) + 1] = 1.0 / step; par[3 * static_cast<size_t>(e) + 2] = step;
    }
    // (h_up is free again: the tables of step 1 were copied before the synchronisation above)
    if (int rc2 = upload_tables(ctx, ctx->filt.rq_par, {{par.data(), par.size() * sizeof(double)}})) return rc2;
    hipLaunchKernelGGL(requant_round_batch_kernel, rq_grid, dim3(RQ_NT), 0, ctx->stream, d_filtered, d_rq_ev, d_rq_unit, ctx->filt.rq_par.as<double>(),
                       d_rounded);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

}  // extern "C"

namespace {

// check_offsets (batch_plan.hpp) of a set of sequences, `what` names it in the error; *longest = the longest sequence
int sequence_offsets(ps_ctx *ctx, const int64_t *off, int32_t n, const char *what, int64_t *longest)
{
    int32_t bad = -1;
    switch (check_offsets(off, n, longest, &bad)) {
    case BATCH_PLAN_OK: return PS_OK;
    case BATCH_PLAN_LONG: return fail(ctx, PS_ERR_ARG, "%s %d too long", what, bad);
    default: return fail(ctx, PS_ERR_ARG, "%s offsets must be non-negative and ascending", what);
    }
}
// check_slot_offsets (batch_plan.hpp) of the slots of n items, `what` names them in the error
int slot_offsets(ps_ctx *ctx, const int64_t *off, int32_t n, const char *what)
{
    int32_t bad = -1;
    return check_slot_offsets(off, n, &bad) ? fail(ctx, PS_ERR_ARG, "%s offsets must be non-negative and ascending", what) : PS_OK;
}

}  // namespace

extern "C" {

int ps_align_batch(ps_ctx *ctx, const double *h_model_means, const double *h_model_stds, const double *h_model_durs,
                   int32_t m, double skip_penalty, double backslip_penalty, const double *d_seq_means,
                   const double *d_seq_stds, const double *d_seq_durs, const int64_t *h_seq_off, int32_t n_seq,
                   double *d_scores, uint32_t *d_paths, int32_t *d_status)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_model_means || !h_model_stds || !h_model_durs || !h_seq_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (m < 1 || m > ALIGN_M_MAX) return fail(ctx, PS_ERR_ARG, "model of %d segments: the device aligner takes 1..%d", m, ALIGN_M_MAX);
    if (n_seq < 0) return fail(ctx, PS_ERR_ARG, "negative sequence count");
    if (n_seq == 0) return PS_OK;
    if (!d_scores || !d_paths || !d_status) return fail(ctx, PS_ERR_ARG, "null output pointer");
    int64_t s_max = 0;
    if (int rc = sequence_offsets(ctx, h_seq_off, n_seq, "sequence", &s_max)) return rc;
    if (h_seq_off[n_seq] > 0 && (!d_seq_means || !d_seq_stds || !d_seq_durs)) return fail(ctx, PS_ERR_ARG, "null sequence pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one upload: model rows (mean, std, dur*skip, dur*backslip, first-row penalty, dur), then the offsets
    auto model_rows = [&](void *staging) {
        double *h = static_cast<double *>(staging);
        double run = 0.0;                                   // np.cumsum(model_dur): sequential (calignment.pyx:30)
        for (int j = 0; j < m; ++j) {
            run = j ? run + h_model_durs[j] : h_model_durs[j];
            h[j] = h_model_means[j];
            h[m + j] = h_model_stds[j];
            h[2 * m + j] = h_model_durs[j] * skip_penalty;              // :57
            h[3 * m + j] = h_model_durs[j] * backslip_penalty;          // :61-62
            h[4 * m + j] = skip_penalty * (run - h_model_durs[j]);      // :52
            h[5 * m + j] = h_model_durs[j];
        }
    };
    if (int rc = upload_tables(ctx, ctx->align.in, static_cast<size_t>(6) * m * sizeof(double), model_rows,
                               {{h_seq_off, (static_cast<size_t>(n_seq) + 1) * sizeof(int64_t)}})) return rc;
    AlignModel M;
    const double *dm = ctx->align.in.as<double>();
    M.mean = dm; M.std = dm + m; M.dsp = dm + 2 * m; M.dbp = dm + 3 * m; M.pen0 = dm + 4 * m; M.dur = dm + 5 * m;
    M.m = m; M.skip_pen = skip_penalty; M.back_pen = backslip_penalty;
    const long long *d_off = reinterpret_cast<const long long *>(dm + 6 * m);
    // the traceback block, the LDS and the scratch -- score, skip_score and backslip_score of one sequence per resident
    // workgroup -- are align_plan's (batch_plan.hpp)
    AlignPlan A;
    if (align_plan(m, n_seq, s_max, &A)) return fail(ctx, PS_ERR_ARG, "a %lld x %d alignment needs more than 32 GiB of scratch", (long long)s_max, m);
    const int B = A.B;
    const size_t lds = A.lds;
    const unsigned long long per_wg = A.per_wg;            // doubles
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)));
    const unsigned grid = std::min({static_cast<unsigned>(n_seq), resident_slots(ctx, align_kernel, ALIGN_NT, lds), A.grid_cap});
    HIP_TRY(ctx, ctx->align.scratch.reserve(static_cast<size_t>(grid) * per_wg * sizeof(double)));
    hipLaunchKernelGGL(align_kernel, dim3(grid), dim3(ALIGN_NT), lds, ctx->stream, M, d_seq_means, d_seq_stds, d_seq_durs,
                       d_off, n_seq, ctx->align.scratch.as<double>(), static_cast<long long>(per_wg), B, d_scores, d_paths, d_status);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_pairwise_scores(ps_ctx *ctx, const double *d_a, const int64_t *h_a_off, int32_t n_a, const double *d_b,
                       const int64_t *h_b_off, int32_t n_b, int32_t mode, double penalty, double *d_scores, int32_t *d_pos)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_a_off || !h_b_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (mode != PS_PW_GLOBAL && mode != PS_PW_LOCAL) return fail(ctx, PS_ERR_ARG, "ps_pairwise_scores: mode %d is neither global nor local", mode);
    if (n_a < 0 || n_b < 0) return fail(ctx, PS_ERR_ARG, "negative sequence count");
    if (!std::isfinite(penalty)) return fail(ctx, PS_ERR_ARG, "the penalty must be finite");
    if (n_a == 0 || n_b == 0) return PS_OK;
    if (!d_scores) return fail(ctx, PS_ERR_ARG, "null output pointer");
    int64_t m_max = 0, n_max = 0;
    if (int rc = sequence_offsets(ctx, h_a_off, n_a, "A sequence", &m_max)) return rc;
    if (int rc = sequence_offsets(ctx, h_b_off, n_b, "B sequence", &n_max)) return rc;
    if (n_max > PW_N_MAX) return fail(ctx, PS_ERR_ARG, "a B sequence of %lld elements: the device pairwise aligner takes up to %d", (long long)n_max, PW_N_MAX);
    if ((h_a_off[n_a] > 0 && !d_a) || (h_b_off[n_b] > 0 && !d_b)) return fail(ctx, PS_ERR_ARG, "null sequence pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = upload_tables(ctx, ctx->pw.in, {{h_a_off, (static_cast<size_t>(n_a) + 1) * sizeof(int64_t)},
                                                  {h_b_off, (static_cast<size_t>(n_b) + 1) * sizeof(int64_t)}})) return rc;
    const long long *da_off = ctx->pw.in.as<long long>(), *db_off = da_off + n_a + 1;
    const int n_cap = static_cast<int>(std::max<int64_t>(n_max, 1));
    const size_t lds = pw_lds_bytes(n_cap);
    const long long jobs = static_cast<long long>(n_a) * n_b;
    auto launch = [&](auto kernel) -> int {
        HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), static_cast<int>(lds)));
        const unsigned grid = static_cast<unsigned>(std::min<long long>(jobs, resident_slots(ctx, kernel, PW_NT, lds)));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(PW_NT), lds, ctx->stream, d_a, da_off, n_a, d_b, db_off, n_b, penalty, n_cap,
                           d_scores, d_pos);
        return PS_OK;
    };
    if (int rc = mode == PS_PW_LOCAL ? launch(pw_score_kernel<true>) : launch(pw_score_kernel<false>)) return rc;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_pairwise_batch(ps_ctx *ctx, const double *d_a, const int64_t *h_a_off, int32_t n_a, const double *d_b,
                      const int64_t *h_b_off, int32_t n_b, const int32_t *h_pair_a, const int32_t *h_pair_b, int32_t n_pairs,
                      int32_t mode, double penalty, int32_t min_length, double *d_scores, int32_t *d_status,
                      const int64_t *h_col_off, int32_t *d_cols_i, int32_t *d_cols_j, int32_t *d_col_need,
                      const int64_t *h_aln_off, double *d_aln_score, int32_t *d_aln_start, int32_t *d_aln_len,
                      int32_t *d_aln_count)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_a_off || !h_b_off || !h_col_off || !h_aln_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (mode != PS_PW_GLOBAL && mode != PS_PW_LOCAL && mode != PS_PW_LOCAL_REPEATED) return fail(ctx, PS_ERR_ARG, "unknown mode %d", mode);
    if (n_a < 0 || n_b < 0 || n_pairs < 0) return fail(ctx, PS_ERR_ARG, "negative count");
    if (!std::isfinite(penalty)) return fail(ctx, PS_ERR_ARG, "the penalty must be finite");
    if (n_pairs == 0) return PS_OK;
    if (!h_pair_a || !h_pair_b) return fail(ctx, PS_ERR_ARG, "null pair table");
    if (!d_scores || !d_status || !d_cols_i || !d_cols_j || !d_col_need || !d_aln_score || !d_aln_start || !d_aln_len || !d_aln_count)
        return fail(ctx, PS_ERR_ARG, "null output pointer");
    int64_t m_max = 0, n_max = 0;
    if (int rc = sequence_offsets(ctx, h_a_off, n_a, "A sequence", &m_max)) return rc;
    if (int rc = sequence_offsets(ctx, h_b_off, n_b, "B sequence", &n_max)) return rc;
    if ((h_a_off[n_a] > 0 && !d_a) || (h_b_off[n_b] > 0 && !d_b)) return fail(ctx, PS_ERR_ARG, "null sequence pointer");
    for (int32_t q = 0; q < n_pairs; ++q) {
        if (h_pair_a[q] < 0 || h_pair_a[q] >= n_a || h_pair_b[q] < 0 || h_pair_b[q] >= n_b) return fail(ctx, PS_ERR_ARG, "pair %d names a sequence that is not there", q);
        if (!slot_ok(h_col_off, q) || !slot_ok(h_aln_off, q)) return fail(ctx, PS_ERR_ARG, "slot offsets must be non-negative and ascending");
        const int64_t m = h_a_off[h_pair_a[q] + 1] - h_a_off[h_pair_a[q]], n = h_b_off[h_pair_b[q] + 1] - h_b_off[h_pair_b[q]];
        if (n > PW_N_MAX) return fail(ctx, PS_ERR_ARG, "pair %d: y of %lld elements, the device pairwise aligner takes up to %d", q, (long long)n, PW_N_MAX);
        if (m * n > INT32_MAX) return fail(ctx, PS_ERR_ARG, "pair %d: %lld x %lld cells, 2^31 - 1 at most", q, (long long)m, (long long)n);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one upload: the four 8-byte tables, the two pair tables, the capacity flag
    const size_t na = static_cast<size_t>(n_a) + 1, nb = static_cast<size_t>(n_b) + 1, np = static_cast<size_t>(n_pairs);
    const int32_t no_flags[2] = {0, 0};
    if (int rc = upload_tables(ctx, ctx->pw.in, {{h_a_off, na * 8}, {h_b_off, nb * 8}, {h_col_off, (np + 1) * 8}, {h_aln_off, (np + 1) * 8},
                                                  {h_pair_a, np * 4}, {h_pair_b, np * 4}, {no_flags, sizeof(no_flags)}})) return rc;
    PwBatch P;
    P.a = d_a; P.b = d_b;
    P.a_off = ctx->pw.in.as<long long>(); P.b_off = P.a_off + na; P.col_off = P.b_off + nb; P.aln_off = P.col_off + np + 1;
    int *di = reinterpret_cast<int *>(const_cast<long long *>(P.aln_off + np + 1));
    P.pair_a = di; P.pair_b = di + np; P.flag = di + 2 * np;
    P.mode = mode; P.min_length = min_length; P.penalty = penalty;
    P.scores = d_scores; P.status = d_status; P.cols_i = d_cols_i; P.cols_j = d_cols_j; P.col_need = d_col_need;
    P.aln_score = d_aln_score; P.aln_start = d_aln_start; P.aln_len = d_aln_len; P.aln_count = d_aln_count;
    // Launches: consecutive pairs while the scratch of their launch -- one matrix of the launch's largest pair per workgroup,
    // a workgroup per pair up to the resident slots -- stays within the budget; a launch whose first pair alone leaves room
    // for few matrices runs on that many workgroups (next_scratch_launch, batch_plan.hpp)
    const unsigned long long budget = static_cast<unsigned long long>(std::max<long long>(1, ctx->opt.pairwise_budget));
    auto dims = [&](int32_t q) {
        const int64_t m = h_a_off[h_pair_a[q] + 1] - h_a_off[h_pair_a[q]], n = h_b_off[h_pair_b[q] + 1] - h_b_off[h_pair_b[q]];
        return PwDims{static_cast<unsigned long long>(m) * static_cast<unsigned long long>(n), static_cast<unsigned long long>(m), static_cast<int>(n)};
    };
    auto run = [&](auto kernel) -> int {
        auto slots = [&](size_t lds) { return resident_slots(ctx, kernel, PW_NT, lds); };
        ScratchLaunch<PwDims> L;
        for (int32_t q0 = 0; q0 < n_pairs; q0 = L.q1) {
            if (next_scratch_launch(q0, n_pairs, budget, dims, slots, &L)) return fail(ctx, PS_ERR_ARG, "pair %d needs more than 32 GiB of scratch", q0);
            HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), static_cast<int>(L.lds)));
            HIP_TRY(ctx, ctx->pw.scratch.reserve(static_cast<size_t>(L.grid) * L.per_wg));
            if (ctx->opt.debug) fprintf(stderr, "[poreseg] pairwise launch: pairs %d..%d, grid %u, %llu bytes of scratch per workgroup, dynamic LDS %zu\n", L.q0, L.q1, L.grid, L.per_wg, L.lds);
            hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(PW_NT), L.lds, ctx->stream, P, L.q0, L.q1 - L.q0, L.dims.n_cap, ctx->pw.scratch.as<unsigned char>(),
                               L.per_wg, L.dims.cells, L.dims.rows);
            HIP_TRY(ctx, hipGetLastError());
        }
        return PS_OK;
    };
    if (int rc = mode == PS_PW_GLOBAL ? run(pw_batch_kernel<false>) : run(pw_batch_kernel<true>)) return rc;
    int flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, P.flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) return fail(ctx, PS_ERR_CAPACITY, "an alignment slot is too small (d_col_need and d_aln_count hold what the pairs take)");
    return PS_OK;
}

int ps_trf_split_batch(ps_ctx *ctx, const double *d_mean, const double *d_std, const int64_t *h_off, int32_t n_seq,
                       double penalty, double min_score, int64_t max_repeats, double *d_score, int32_t *d_len, int32_t *d_i,
                       int32_t *d_j, const int64_t *h_slot_off, int32_t *d_count, int32_t *d_status)
{
    if (!ctx) return PS_ERR_ARG;
    if (!h_off || !h_slot_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (n_seq < 0 || max_repeats < 0) return fail(ctx, PS_ERR_ARG, "negative count");
    // the reference never ends for min_score < 0 (the border cell (0, 0) is yielded for ever); with penalty >= 0 the
    // diagonal and the lower triangle are no longer unobservable
    if (!(penalty < 0.0) || !std::isfinite(penalty)) return fail(ctx, PS_ERR_ARG, "ps_trf_split_batch: the penalty must be finite and < 0");
    if (!(min_score >= 0.0) || !std::isfinite(min_score)) return fail(ctx, PS_ERR_ARG, "ps_trf_split_batch: min_score must be finite and >= 0");
    if (n_seq == 0) return PS_OK;
    if (!d_score || !d_len || !d_i || !d_j || !d_count || !d_status) return fail(ctx, PS_ERR_ARG, "null output pointer");
    int64_t n_max = 0;
    if (int rc = sequence_offsets(ctx, h_off, n_seq, "sequence", &n_max)) return rc;
    if (n_max > TRF_N_MAX) return fail(ctx, PS_ERR_ARG, "a sequence of %lld segments: the device repeat splitter takes up to %d", (long long)n_max, TRF_N_MAX);
    if (h_off[n_seq] > 0 && (!d_mean || !d_std)) return fail(ctx, PS_ERR_ARG, "null sequence pointer");
    if (int rc = slot_offsets(ctx, h_slot_off, n_seq, "slot")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one upload: the two 8-byte tables, the capacity flag
    const size_t ns = static_cast<size_t>(n_seq) + 1;
    const int32_t no_flags[2] = {0, 0};
    if (int rc = upload_tables(ctx, ctx->trf.in, {{h_off, ns * 8}, {h_slot_off, ns * 8}, {no_flags, sizeof(no_flags)}})) return rc;
    TrfBatch P;
    P.mean = d_mean; P.std = d_std;
    P.off = ctx->trf.in.as<long long>(); P.slot_off = P.off + ns;
    P.flag = reinterpret_cast<int *>(const_cast<long long *>(P.slot_off + ns));
    P.penalty = penalty; P.min_score = min_score; P.max_repeats = max_repeats;
    P.score = d_score; P.len = d_len; P.i = d_i; P.j = d_j; P.count = d_count; P.status = d_status;
    // Launches: consecutive sequences while the scratch of their launch -- the mask and pointer bits of the launch's longest
    // sequence per workgroup, a workgroup per sequence up to the resident slots -- stays within the budget; a launch whose
    // first sequence alone leaves room for few workgroups runs on that many (next_scratch_launch, batch_plan.hpp)
    const unsigned long long budget = static_cast<unsigned long long>(std::max<long long>(1, ctx->opt.trf_budget));
    static_assert(trf_lds_bytes(TRF_N_MAX) <= 64u << 10, "beyond 64 KiB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize (set_dyn_lds)");
    auto dims = [&](int32_t q) { return TrfDims{static_cast<int>(h_off[q + 1] - h_off[q])}; };
    auto slots = [&](size_t lds) { return resident_slots(ctx, trf_kernel, TRF_NT, lds); };
    ScratchLaunch<TrfDims> L;
    for (int32_t q0 = 0; q0 < n_seq; q0 = L.q1) {
        next_scratch_launch(q0, n_seq, budget, dims, slots, &L);        // (never refused: 1.6 MB of scratch at TRF_N_MAX)
        HIP_TRY(ctx, ctx->trf.scratch.reserve(static_cast<size_t>(L.grid) * L.per_wg));
        if (ctx->opt.debug) fprintf(stderr, "[poreseg] trf launch: sequences %d..%d, grid %u, %llu bytes of scratch per workgroup, dynamic LDS %zu\n", L.q0, L.q1, L.grid, L.per_wg, L.lds);
        hipLaunchKernelGGL(trf_kernel, dim3(L.grid), dim3(TRF_NT), L.lds, ctx->stream, P, L.q0, L.q1 - L.q0, L.dims.n_cap, ctx->trf.scratch.as<unsigned char>(), L.per_wg);
        HIP_TRY(ctx, hipGetLastError());
    }
    int flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, P.flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) return fail(ctx, PS_ERR_CAPACITY, "a repeat slot is too small (d_count holds the yields every sequence has)");
    return PS_OK;
}

}  // extern "C"

namespace {

// A sequence-model call's model: the sizes and decisions hmm_plan.hpp derives from it (I), and the kernels' structs aimed at its
// device copy.  A vector model takes the HmmDevV instantiations, one with mixture states the HmmDevM ones, one with
// kernel-density states (and no mixture) the HmmDevK ones, any other the HmmDev ones.
struct HmmCall {
    HmmModelInfo I;
    HmmDevK DK;
    HmmDevV DV;
    HmmDevM DM;
    const long long *d_off = nullptr;
};
template <typename F> int with_model(const HmmCall &C, F &&f)
{
    return C.I.vec ? f(C.DV) : C.I.mix ? f(C.DM) : C.I.kde ? f(C.DK) : f(static_cast<const HmmDev &>(C.DK));
}

// The model's arrays checked and packed into one blob (hmm_model_check, hmm_blob_layout, hmm_blob_pack: hmm_plan.hpp); the
// device copy is reused while the blob is unchanged -- a changed parameter, weight, kind or split is a changed blob.
int hmm_upload(ps_ctx *ctx, const ps_hmm_model *m, HmmCall *C)
{
    std::string why;
    if (!hmm_model_check(m, &C->I, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
    const HmmBlobLayout L = hmm_blob_layout(C->I);
    std::vector<char> blob;
    hmm_blob_pack(m, L, &blob);
    if (blob != ctx->hmm.blob || !ctx->hmm.model.p) {
        HIP_TRY(ctx, ctx->hmm.model.reserve(blob.size()));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hmm.model.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));       // (blob is a local: the copy completes before it goes)
        ctx->hmm.blob.swap(blob);
    }
    hmm_blob_resolve(ctx->hmm.model.p, L, C->I, &C->DK, &C->DV, &C->DM);
    return PS_OK;
}

// The launch plan the sequence-model entry points share: next_chunk (batch_plan.hpp) cuts a batch into launches.

// The forward pass of sequences [q0, q1): logp, and the matrix (optional) with sequence q at row off[q] + q - row0 of fmat
template <typename MD>
int launch_forward(ps_ctx *ctx, const MD &D, const double *d_obs, const long long *d_off, int32_t q0, int32_t q1, double *d_logp,
                   double *fmat, long long row0)
{
    const size_t lds = hmm_lds_bytes(D.S);
    HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(hmm_fwd_kernel<HMM_FORWARD, uint8_t, MD>), static_cast<int>(lds)));
    hipLaunchKernelGGL((hmm_fwd_kernel<HMM_FORWARD, uint8_t, MD>), dim3(q1 - q0), dim3(HMM_NT), lds, ctx->stream, D, d_obs, d_off,
                       q0, d_logp, fmat, row0, static_cast<uint8_t *>(nullptr), 0ll, static_cast<int *>(nullptr));
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

// What ps_hmm_batch, ps_hmm_expect and ps_hmm_posterior begin with: the arguments checked (host_ok: the entry point's own
// host pointers are there), the model uploaded -- a bad one is refused whatever the batch --, own(C): the entry point's
// checks that need the model (and what it does for an empty batch), and last, for a batch that is not empty, the offsets,
// followed by the path slots' where there are some, on the device.  An empty batch leaves d_off null.
template <typename Own>
int hmm_begin(ps_ctx *ctx, const ps_hmm_model *model, bool host_ok, const double *d_obs, const int64_t *h_off,
              const int64_t *h_path_off, int32_t n_seq, const double *d_logp, HmmCall *C, Own &&own)
{
    if (!ctx) return PS_ERR_ARG;
    if (!model || !h_off || !host_ok) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (n_seq < 0) return fail(ctx, PS_ERR_ARG, "negative sequence count");
    int64_t longest = 0;
    if (int rc = sequence_offsets(ctx, h_off, n_seq, "sequence", &longest)) return rc;
    if (h_path_off) if (int rc = slot_offsets(ctx, h_path_off, n_seq, "path")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = hmm_upload(ctx, model, C)) return rc;
    if (int rc = own(*C)) return rc;
    if (n_seq == 0) return PS_OK;
    if (!d_logp || (h_off[n_seq] > 0 && !d_obs)) return fail(ctx, PS_ERR_ARG, "null device pointer");
    const size_t nb = (static_cast<size_t>(n_seq) + 1) * sizeof(int64_t);
    if (int rc = upload_tables(ctx, ctx->hmm.off, {{h_off, nb}, {h_path_off, h_path_off ? nb : 0}})) return rc;
    C->d_off = ctx->hmm.off.as<long long>();
    return PS_OK;
}

template <typename BP, typename MD>
int hmm_viterbi(ps_ctx *ctx, const MD &D, const double *d_obs, const int64_t *h_off, const long long *d_off, int32_t n_seq,
                double *d_logp, double *d_mat, int32_t *d_path, int32_t *d_path_len)
{
    const size_t S = static_cast<size_t>(D.S), lds = hmm_lds_bytes(D.S);
    const long long *d_path_off = d_off + n_seq + 1;
    const long long budget = std::max<long long>(1, ctx->opt.hmm_bp_budget);
    HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(hmm_fwd_kernel<HMM_VITERBI, BP, MD>), static_cast<int>(lds)));
    HIP_TRY(ctx, ctx->hmm.last.reserve(static_cast<size_t>(n_seq) * sizeof(int)));
    HIP_TRY(ctx, ctx->hmm.flags.reserve(sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->hmm.flags.p, 0, sizeof(int), ctx->stream));
    for (int32_t q0 = 0, q1; q0 < n_seq; q0 = q1) {
        long long bytes;
        q1 = next_chunk(h_off, q0, n_seq, S * sizeof(BP), budget, &bytes);
        if (std::string why; !hmm_launch_check(q0, bytes, true, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
        HIP_TRY(ctx, ctx->hmm.bp.reserve(static_cast<size_t>(bytes)));
        const long long bp_row0 = h_off[q0] + q0;
        const int nq = q1 - q0;
        BP *bp = ctx->hmm.bp.as<BP>();
        hipLaunchKernelGGL((hmm_fwd_kernel<HMM_VITERBI, BP, MD>), dim3(nq), dim3(HMM_NT), lds, ctx->stream, D, d_obs, d_off, q0, d_logp,
                           d_mat, 0ll, bp, bp_row0, ctx->hmm.last.as<int>());
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(hmm_trace_kernel<BP>, dim3((nq + HMM_NT - 1) / HMM_NT), dim3(HMM_NT), 0, ctx->stream, static_cast<HmmDev>(D), d_off, q0, nq,
                           static_cast<const BP *>(bp), bp_row0, static_cast<const int *>(ctx->hmm.last.as<int>()),
                           static_cast<const double *>(d_logp), d_path_off, d_path, d_path_len, ctx->hmm.flags.as<int>());
        HIP_TRY(ctx, hipGetLastError());
    }
    int flags = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flags, ctx->hmm.flags.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flags & 2) return fail(ctx, PS_ERR_INTERNAL, "a Viterbi traceback left the model");
    if (flags & 1) return fail(ctx, PS_ERR_CAPACITY, "a Viterbi path is longer than its slot (d_path_len holds the lengths)");
    return PS_OK;
}

template <bool ACC_LDS, typename MD>
int hmm_expect_run(ps_ctx *ctx, const MD &D, const double *d_obs, const int64_t *h_off, const long long *d_off,
                   int32_t n_seq, int n_acc, int E, double *d_logp, double *d_counts, double *d_stats, int32_t *h_skipped)
{
    const size_t lds = hmm_lds_bytes(D.S, ACC_LDS ? n_acc : 0);
    HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(hmm_expect_kernel<ACC_LDS, MD>), static_cast<int>(lds)));
    // a grid of resident workgroups (it depends on the device and the model only, never on timing), within the row budget
    const size_t row_bytes = static_cast<size_t>(n_acc) * sizeof(double);
    const unsigned G = budget_grid(static_cast<unsigned>(n_seq), resident_slots(ctx, (hmm_expect_kernel<ACC_LDS, MD>), HMM_NT, lds), HMM_EXPECT_ROWS, row_bytes);
    HIP_TRY(ctx, ctx->hmm.acc.reserve(G * row_bytes));
    HIP_TRY(ctx, ctx->hmm.skip.reserve(sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->hmm.acc.p, 0, G * row_bytes, ctx->stream));
    const long long budget = std::max<long long>(1, ctx->opt.hmm_fb_budget);
    for (int32_t q0 = 0, q1; q0 < n_seq; q0 = q1) {
        long long bytes;
        q1 = next_chunk(h_off, q0, n_seq, static_cast<size_t>(D.S) * sizeof(double), budget, &bytes);
        if (std::string why; !hmm_launch_check(q0, bytes, false, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
        HIP_TRY(ctx, ctx->hmm.fmat.reserve(static_cast<size_t>(bytes)));
        const long long row0 = h_off[q0] + q0;
        if (int rc = launch_forward(ctx, D, d_obs, d_off, q0, q1, d_logp, ctx->hmm.fmat.as<double>(), row0)) return rc;
        hipLaunchKernelGGL((hmm_expect_kernel<ACC_LDS, MD>), dim3(G), dim3(HMM_NT), lds, ctx->stream, D, d_obs, d_off, q0, q1,
                           static_cast<const double *>(d_logp), static_cast<const double *>(ctx->hmm.fmat.as<double>()), row0,
                           ctx->hmm.acc.as<double>(), n_acc);
        HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(hmm_expect_reduce_kernel, dim3((n_acc + 255) / 256), dim3(256), 0, ctx->stream,
                       static_cast<const double *>(ctx->hmm.acc.as<double>()), static_cast<int>(G), n_acc, E, d_counts, d_stats,
                       ctx->hmm.skip.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    double skipped = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&skipped, ctx->hmm.skip.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *h_skipped = static_cast<int32_t>(skipped);
    return PS_OK;
}

// ps_hmm_posterior: forward matrices per launch as in hmm_expect_run, one workgroup per sequence.  CNT: 0 no counts, 1 the
// sequence's counts row updated in global memory, 2 in LDS behind the two score rows.
template <int CNT, typename MD>
int hmm_posterior_run(ps_ctx *ctx, const MD &D, const double *d_obs, const int64_t *h_off, const long long *d_off,
                      int32_t n_seq, int E, double *d_logp, double *d_post, int32_t *d_map_state, double *d_map_logp,
                      double *d_counts_seq)
{
    const size_t lds = hmm_lds_bytes(D.S, CNT == 2 ? E : 0);
    HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(hmm_posterior_kernel<CNT, MD>), static_cast<int>(lds)));
    if (d_map_logp) HIP_TRY(ctx, ctx->hmm.pmax.reserve(std::max<size_t>(1, static_cast<size_t>(h_off[n_seq])) * sizeof(double)));
    const long long budget = std::max<long long>(1, ctx->opt.hmm_fb_budget);
    for (int32_t q0 = 0, q1; q0 < n_seq; q0 = q1) {
        long long bytes;
        q1 = next_chunk(h_off, q0, n_seq, static_cast<size_t>(D.S) * sizeof(double), budget, &bytes);
        if (std::string why; !hmm_launch_check(q0, bytes, false, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
        HIP_TRY(ctx, ctx->hmm.fmat.reserve(static_cast<size_t>(bytes)));
        const long long row0 = h_off[q0] + q0;
        if (ctx->opt.debug) fprintf(stderr, "[poreseg] posterior launch: sequences %d..%d, %lld bytes of forward matrix, dynamic LDS %zu\n", q0, q1, bytes, lds);
        if (int rc = launch_forward(ctx, D, d_obs, d_off, q0, q1, d_logp, ctx->hmm.fmat.as<double>(), row0)) return rc;
        hipLaunchKernelGGL((hmm_posterior_kernel<CNT, MD>), dim3(q1 - q0), dim3(HMM_NT), lds, ctx->stream, D, d_obs, d_off, q0,
                           static_cast<const double *>(d_logp), static_cast<const double *>(ctx->hmm.fmat.as<double>()), row0, d_post,
                           d_map_state, d_map_logp, ctx->hmm.pmax.as<double>(), CNT ? d_counts_seq : nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

}  // namespace

extern "C" {

int ps_hmm_batch(ps_ctx *ctx, const ps_hmm_model *model, int32_t mode, const double *d_obs, const int64_t *h_off,
                 int32_t n_seq, double *d_logp, double *d_mat, int32_t *d_path, const int64_t *h_path_off,
                 int32_t *d_path_len)
{
    // (the mode is judged between hmm_begin's first checks, so they stand here too, in their order)
    if (!ctx) return PS_ERR_ARG;
    if (!model || !h_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (mode != PS_HMM_VITERBI && mode != PS_HMM_FORWARD && mode != PS_HMM_BACKWARD) return fail(ctx, PS_ERR_ARG, "unknown mode %d", mode);
    if (n_seq < 0) return fail(ctx, PS_ERR_ARG, "negative sequence count");
    const bool vit = mode == PS_HMM_VITERBI;
    if (vit && (!h_path_off || (n_seq > 0 && (!d_path_len || !d_path))))
        return fail(ctx, PS_ERR_ARG, "Viterbi needs the path buffer, its offsets and the length array");
    HmmCall C;
    if (int rc = hmm_begin(ctx, model, true, d_obs, h_off, vit ? h_path_off : nullptr, n_seq, d_logp, &C,
                           [](const HmmCall &) { return PS_OK; })) return rc;
    if (!C.d_off) return PS_OK;
    if (vit)
        return with_model(C, [&](const auto &M) {
            return hmm_bp_wide(C.I) ? hmm_viterbi<uint16_t>(ctx, M, d_obs, h_off, C.d_off, n_seq, d_logp, d_mat, d_path, d_path_len)
                                    : hmm_viterbi<uint8_t>(ctx, M, d_obs, h_off, C.d_off, n_seq, d_logp, d_mat, d_path, d_path_len);
        });
    const int rc = with_model(C, [&](const auto &M) -> int {
        using MD = std::decay_t<decltype(M)>;
        if (mode == PS_HMM_FORWARD) return launch_forward(ctx, M, d_obs, C.d_off, 0, n_seq, d_logp, d_mat, 0ll);
        const size_t lds = hmm_lds_bytes(M.S);
        HIP_TRY(ctx, set_dyn_lds(ctx, reinterpret_cast<const void *>(hmm_bwd_kernel<MD>), static_cast<int>(lds)));
        hipLaunchKernelGGL(hmm_bwd_kernel<MD>, dim3(n_seq), dim3(HMM_NT), lds, ctx->stream, M, d_obs, C.d_off, 0, d_logp, d_mat);
        HIP_TRY(ctx, hipGetLastError());
        return PS_OK;
    });
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_hmm_expect(ps_ctx *ctx, const ps_hmm_model *model, const double *d_obs, const int64_t *h_off, int32_t n_seq,
                  double *d_logp, double *d_counts, double *d_stats, int32_t *h_skipped)
{
    HmmCall C;
    int n_acc = 0;
    auto own = [&](const HmmCall &c) -> int {
        const int E = c.I.E, NE = c.I.NE;
        if (std::string why; !hmm_acc_check(c.I, true, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
        n_acc = static_cast<int>(c.I.n_acc());
        if ((E > 0 && !d_counts) || (NE > 0 && !d_stats)) return fail(ctx, PS_ERR_ARG, "null device pointer");
        *h_skipped = 0;
        if (n_seq == 0) {
            if (E > 0) HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, static_cast<size_t>(E) * sizeof(double), ctx->stream));
            if (NE > 0) HIP_TRY(ctx, hipMemsetAsync(d_stats, 0, static_cast<size_t>(c.I.n_stats()) * sizeof(double), ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return PS_OK;
    };
    if (int rc = hmm_begin(ctx, model, h_skipped != nullptr, d_obs, h_off, nullptr, n_seq, d_logp, &C, own)) return rc;
    if (!C.d_off) return PS_OK;
    const int E = C.I.E;
    const bool in_lds = hmm_expect_in_lds(C.I, ctx->opt.hmm_expect_lds);
    return with_model(C, [&](const auto &M) {
        return in_lds ? hmm_expect_run<true>(ctx, M, d_obs, h_off, C.d_off, n_seq, n_acc, E, d_logp, d_counts, d_stats, h_skipped)
                      : hmm_expect_run<false>(ctx, M, d_obs, h_off, C.d_off, n_seq, n_acc, E, d_logp, d_counts, d_stats, h_skipped);
    });
}

int ps_hmm_posterior(ps_ctx *ctx, const ps_hmm_model *model, const double *d_obs, const int64_t *h_off, int32_t n_seq,
                     double *d_logp, double *d_post, int32_t *d_map_state, double *d_map_logp, double *d_counts_seq)
{
    HmmCall C;
    auto own = [&](const HmmCall &c) -> int {
        if (std::string why; !hmm_acc_check(c.I, false, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
        return PS_OK;
    };
    if (int rc = hmm_begin(ctx, model, true, d_obs, h_off, nullptr, n_seq, d_logp, &C, own)) return rc;
    if (!C.d_off) return PS_OK;
    const int E = C.I.E;
    const int cnt = hmm_posterior_cnt(C.I, d_counts_seq != nullptr, ctx->opt.hmm_expect_lds);
    return with_model(C, [&](const auto &M) {
        switch (cnt) {
        case 0: return hmm_posterior_run<0>(ctx, M, d_obs, h_off, C.d_off, n_seq, E, d_logp, d_post, d_map_state, d_map_logp, d_counts_seq);
        case 1: return hmm_posterior_run<1>(ctx, M, d_obs, h_off, C.d_off, n_seq, E, d_logp, d_post, d_map_state, d_map_logp, d_counts_seq);
        default: return hmm_posterior_run<2>(ctx, M, d_obs, h_off, C.d_off, n_seq, E, d_logp, d_post, d_map_state, d_map_logp, d_counts_seq);
        }
    });
}

int ps_hmm_sample(ps_ctx *ctx, const ps_hmm_model *model, const ps_hmm_sample_tables *tables, uint64_t seed, int64_t first,
                  int32_t n_seq, int32_t length, int32_t max_length, double *d_obs, const int64_t *h_off, int32_t *d_len,
                  int32_t *d_flags, int32_t *d_path, const int64_t *h_path_off, int32_t *d_path_len)
{
    if (!ctx) return PS_ERR_ARG;
    if (!model || !tables || !h_off) return fail(ctx, PS_ERR_ARG, "null pointer");
    if (n_seq < 0) return fail(ctx, PS_ERR_ARG, "negative sequence count");
    if (first < 0 || first > INT64_MAX - n_seq) return fail(ctx, PS_ERR_ARG, "first must be >= 0 and first + n_seq fit in int64");
    if (length < 0) return fail(ctx, PS_ERR_ARG, "negative length");
    if (max_length < 1) return fail(ctx, PS_ERR_ARG, "max_length must be >= 1");
    const bool want_path = d_path && h_path_off;
    if ((d_path != nullptr) != (h_path_off != nullptr)) return fail(ctx, PS_ERR_ARG, "a path buffer and its offsets go together");
    if (want_path && n_seq > 0 && !d_path_len) return fail(ctx, PS_ERR_ARG, "paths need the length array");
    int64_t longest = 0;
    if (int rc = sequence_offsets(ctx, h_off, n_seq, "observation slot", &longest)) return rc;
    if (want_path) if (int rc = slot_offsets(ctx, h_path_off, n_seq, "path")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HmmCall C;
    if (int rc = hmm_upload(ctx, model, &C)) return rc;
    if (std::string why; !hmm_sample_check(model, tables, C.I, length, max_length, &why)) return fail(ctx, PS_ERR_ARG, "%s", why.c_str());
    if (n_seq == 0) return PS_OK;
    if (!d_len || !d_flags || (h_off[n_seq] > 0 && !d_obs)) return fail(ctx, PS_ERR_ARG, "null device pointer");
    const HmmSampleLayout U = hmm_sample_layout(model, tables, C.I, h_off, want_path ? h_path_off : nullptr, n_seq);
    HostTable up[HMM_U_COUNT];
    for (int t = 0; t < HMM_U_COUNT; ++t) up[t] = {U.src[t], U.bytes[t]};
    if (int rc = upload_tables(ctx, ctx->hmm.samp, 0, [](void *) {}, up, up + HMM_U_COUNT)) return rc;
    HmmSampleDev T;
    const long long *d_off, *d_path_off;
    hmm_sample_resolve(ctx->hmm.samp.p, U, &T, &C.DM, &d_off, &d_path_off);
    const int rc = with_model(C, [&](const auto &M) -> int {
        using MD = std::decay_t<decltype(M)>;
        hipLaunchKernelGGL(hmm_sample_kernel<MD>, dim3((n_seq + HMM_NT - 1) / HMM_NT), dim3(HMM_NT), 0, ctx->stream, M, T,
                           static_cast<unsigned long long>(seed), static_cast<long long>(first), n_seq, length, max_length, d_obs,
                           d_off, d_len, d_flags, want_path ? d_path : nullptr, d_path_off, d_path_len);
        HIP_TRY(ctx, hipGetLastError());
        return PS_OK;
    });
    if (rc) return rc;
    // the lengths against the slots, on the host: the kernel keeps no shared flag
    std::vector<int32_t> lens(static_cast<size_t>(n_seq)), plens(want_path ? static_cast<size_t>(n_seq) : 0);
    HIP_TRY(ctx, hipMemcpyAsync(lens.data(), d_len, lens.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (want_path) HIP_TRY(ctx, hipMemcpyAsync(plens.data(), d_path_len, plens.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int64_t short_obs = 0, short_path = 0;
    hmm_short_slots(lens.data(), h_off, want_path ? plens.data() : nullptr, h_path_off, n_seq, &short_obs, &short_path);
    if (short_obs || short_path)
        return fail(ctx, PS_ERR_CAPACITY, "%lld observation slots and %lld path slots are too small (d_len and d_path_len hold the lengths)",
                    static_cast<long long>(short_obs), static_cast<long long>(short_path));
    return PS_OK;
}

}  // extern "C"

// ---- the state parsers: snakebase and filter-derivative (seg_state.hpp) -------------------------------------------------------
namespace {

// One compaction's tables on the device: start, npos, tile_off (n_ev + 1) in one copy; *n_tiles = its tiles.  `tab` must
// outlive the call's next synchronisation (pageable source).
int sp_upload(ps_ctx *ctx, DevBuf &buf, std::vector<int64_t> &tab, const int64_t *start, const int64_t *npos, int32_t n_ev,
              SpEvents *ev, int64_t *n_tiles)
{
    const size_t n = static_cast<size_t>(n_ev);
    if (plan_tile_table(start, npos, n_ev, &tab, n_tiles)) return fail(ctx, PS_ERR_ARG, "too many samples for one call");
    HIP_TRY(ctx, buf.reserve(tab.size() * sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    const int64_t *t = buf.as<int64_t>();
    ev->start = t; ev->npos = t + n; ev->tile_off = t + 2 * n; ev->n_ev = n_ev;
    return PS_OK;
}

// Pass 1, the scan and the hits before each event (d_off, n_ev + 1 entries) of one compaction, queued; h_off receives d_off
// with the caller's next synchronisation.
template <class Pred>
int sp_count(ps_ctx *ctx, Pred pred, const SpEvents &ev, int64_t n_tiles, DevBuf &off, std::vector<int64_t> &h_off)
{
    const size_t n1 = static_cast<size_t>(ev.n_ev) + 1;
    h_off.assign(n1, 0);
    HIP_TRY(ctx, off.reserve(n1 * sizeof(int64_t)));
    if (n_tiles == 0) {
        HIP_TRY(ctx, hipMemsetAsync(off.p, 0, n1 * sizeof(int64_t), ctx->stream));
        return PS_OK;
    }
    const size_t nt = static_cast<size_t>(n_tiles);
    HIP_TRY(ctx, ctx->sp.mask.reserve(nt * SP_WORDS * sizeof(unsigned long long)));
    HIP_TRY(ctx, ctx->sp.cnt.reserve(nt * sizeof(uint32_t)));
    HIP_TRY(ctx, ctx->sp.excl.reserve((nt + 1) * sizeof(int64_t)));
    hipLaunchKernelGGL(sp_count_kernel<Pred>, dim3(static_cast<unsigned>(n_tiles)), dim3(SP_NT), 0, ctx->stream, pred, ev,
                       ctx->sp.mask.as<unsigned long long>(), ctx->sp.cnt.as<uint32_t>());
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(SP_SCAN_NT), 0, ctx->stream, ctx->sp.cnt.as<uint32_t>(), n_tiles, ctx->sp.excl.as<int64_t>());
    hipLaunchKernelGGL(sp_event_off_kernel, dim3(static_cast<unsigned>((n1 + 255) / 256)), dim3(256), 0, ctx->stream, ev,
                       ctx->sp.excl.as<int64_t>(), off.as<int64_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_off.data(), off.p, n1 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    return PS_OK;
}

// Pass 2 of the compaction sp_count queued last: its `total` hits into out (positions + add)
int sp_scatter(ps_ctx *ctx, const SpEvents &ev, int64_t n_tiles, int64_t total, int32_t add, DevBuf &out)
{
    HIP_TRY(ctx, out.reserve(static_cast<size_t>(std::max<int64_t>(total, 1)) * sizeof(int32_t)));
    if (total == 0) return PS_OK;
    hipLaunchKernelGGL(sp_scatter_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(SP_NT), 0, ctx->stream, ev,
                       ctx->sp.mask.as<unsigned long long>(), ctx->sp.excl.as<int64_t>(), add, out.as<int32_t>());
    HIP_TRY(ctx, hipGetLastError());
    return PS_OK;
}

int sp_args(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev, int32_t *d_spans,
            int64_t cap, int64_t *h_span_off, int64_t min_len)
{
    if (!h_ev_start || !h_ev_len || !h_span_off || n_ev < 0 || cap < 0 || (cap > 0 && !d_spans))
        return fail(ctx, PS_ERR_ARG, "null/negative argument");
    int64_t total = 0;
    int32_t bad = -1;
    switch (check_events(h_ev_start, h_ev_len, n_ev, nullptr, nullptr, min_len, &total, &bad)) {
    case BATCH_PLAN_OK: break;
    case BATCH_PLAN_NEGATIVE: return fail(ctx, PS_ERR_ARG, "event %d: negative start or length", bad);
    case BATCH_PLAN_LONG:
        return fail(ctx, PS_ERR_ARG, "event %d length %lld out of range (2^30 samples at most)", bad, static_cast<long long>(h_ev_len[bad]));
    default: return fail(ctx, PS_ERR_ARG, "event %d: the length of the input must be greater than padlen, which is %d", bad, FILT_PAD);
    }
    for (int e = 0; e <= n_ev; ++e) h_span_off[e] = 0;
    if (total > 0 && !d_current) return fail(ctx, PS_ERR_ARG, "d_current is NULL");
    return PS_OK;
}

}  // namespace

extern "C" {

int ps_snakebase_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                     int32_t *d_spans, int64_t cap, int64_t *h_span_off)
{
    if (!ctx) return PS_ERR_ARG;
    if (int rc = sp_args(ctx, d_current, h_ev_start, h_ev_len, n_ev, d_spans, cap, h_span_off, 0)) return rc;
    if (n_ev == 0) return PS_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = static_cast<size_t>(n_ev);
    std::vector<int64_t> npos(n), tab, hit_off;
    for (size_t e = 0; e < n; ++e) npos[e] = std::max<int64_t>(0, h_ev_len[e] - 1);      // m = n - 1 differences
    SpEvents ev;
    int64_t n_tiles = 0;
    if (int rc = sp_upload(ctx, ctx->sp.tab, tab, h_ev_start, npos.data(), n_ev, &ev, &n_tiles)) return rc;
    if (int rc = sp_count(ctx, SnakePred{d_current}, ev, n_tiles, ctx->sp.off1, hit_off)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> n_spans(n);
    for (size_t e = 0; e < n; ++e) n_spans[e] = (hit_off[e + 1] - hit_off[e] + 1) / 2;
    if (int rc = offsets_to_device(ctx, ctx->sp.span_off, n_spans.data(), n, cap, "span", h_span_off)) return rc;
    const int64_t total = h_span_off[n_ev];
    if (total == 0) return PS_OK;
    if (int rc = sp_scatter(ctx, ev, n_tiles, hit_off[n], 0, ctx->sp.hits)) return rc;
    hipLaunchKernelGGL(sp_snake_spans_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, ctx->stream, ev,
                       ctx->sp.hits.as<int32_t>(), ctx->sp.off1.as<int64_t>(), ctx->sp.span_off.as<int64_t>(), total, d_spans);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

int ps_filter_derivative_f64(ps_ctx *ctx, const double *d_current, const int64_t *h_ev_start, const int64_t *h_ev_len, int32_t n_ev,
                             const ps_filter_derivative_params *params, int32_t *d_spans, int64_t cap, int64_t *h_span_off)
{
    if (!ctx) return PS_ERR_ARG;
    if (!params) return fail(ctx, PS_ERR_ARG, "null/negative argument");
    const bool filter = params->prefiltered == 0;
    if (params->prefiltered != 0 && params->prefiltered != 1) return fail(ctx, PS_ERR_ARG, "prefiltered must be 0 or 1");
    if (std::isnan(params->low_threshold) || std::isnan(params->high_threshold)) return fail(ctx, PS_ERR_ARG, "a threshold is NaN");
    if (filter) {
        const double wn = params->cutoff_freq / (params->sampling_freq / 2.0);
        if (!(wn > 0.0) || !(wn < 1.0)) return fail(ctx, PS_ERR_ARG, "cutoff must lie strictly between 0 and the Nyquist frequency");
    }
    if (int rc = sp_args(ctx, d_current, h_ev_start, h_ev_len, n_ev, d_spans, cap, h_span_off, filter ? FILT_PAD + 1 : 0)) return rc;
    if (n_ev == 0) return PS_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = static_cast<size_t>(n_ev);
    // np.argmax(...) > high_threshold: the index is at least h1 = floor(high_threshold) + 1; every index when it is negative
    const double ht = params->high_threshold;
    const int32_t h1 = ht < 0.0 ? 0 : (ht >= 2147483646.0 ? INT32_MAX : static_cast<int32_t>(std::floor(ht)) + 1);
    // 1. y: the caller's (prefiltered) or the order-1 Bessel filtfilt of every event, packed: the batched float64 filter on the
    //    context's stream
    const double *d_y = d_current;
    std::vector<int64_t> start(h_ev_start, h_ev_start + n);
    if (filter) {
        int64_t total_len = 0;
        for (size_t e = 0; e < n; ++e) { start[e] = total_len; total_len += h_ev_len[e]; }
        HIP_TRY(ctx, ctx->sp.y.reserve(static_cast<size_t>(total_len) * sizeof(double)));
        const ps_sample_format f64 = {PS_DTYPE_F64, 0, 1.0};
        // (filter_batch_queue: one launch for all events on the fused route; it packs the results as `start` does)
        if (int rc = filter_batch_queue(ctx, d_current, &f64, h_ev_start, h_ev_len, n_ev, 1, params->cutoff_freq, params->sampling_freq,
                                        ctx->sp.y.as<double>())) return rc;
        d_y = ctx->sp.y.as<double>();
    }
    // 2. the tics: j + 1 where blocks[j + 1] != blocks[j], j in [0, n - 2)
    std::vector<int64_t> npos(n), tab, tab2, tic_off, kept_off(n + 1, 0);
    for (size_t e = 0; e < n; ++e) npos[e] = std::max<int64_t>(0, h_ev_len[e] - 2);
    SpEvents ev;
    int64_t n_tiles = 0;
    if (int rc = sp_upload(ctx, ctx->sp.tab, tab, start.data(), npos.data(), n_ev, &ev, &n_tiles)) return rc;
    if (int rc = sp_count(ctx, FdPred{d_y, params->low_threshold}, ev, n_tiles, ctx->sp.off1, tic_off)) return rc;
    if (filter) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small.p, ctx->small.p, sizeof(SmallLayout), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (filter) if (int rc = check_status(ctx, static_cast<unsigned>(ctx->h_small.as<SmallLayout>()->status))) return rc;
    if (int rc = sp_scatter(ctx, ev, n_tiles, tic_off[n], 1, ctx->sp.hits)) return rc;
    // 3. the pairs (tics[2 i], tics[2 i + 1]), an unpaired last tic dropped: judged, the kept ones compacted
    std::vector<int64_t> pair_off(n + 1, 0), n_pairs(n);
    for (size_t e = 0; e < n; ++e) { n_pairs[e] = (tic_off[e + 1] - tic_off[e]) / 2; pair_off[e + 1] = pair_off[e] + n_pairs[e]; }
    const int64_t pairs = pair_off[n];
    HIP_TRY(ctx, ctx->sp.pair_off.reserve((n + 1) * sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sp.pair_off.p, pair_off.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    SpPairs pr;
    pr.start = ev.start; pr.tic_off = ctx->sp.off1.as<int64_t>(); pr.pair_off = ctx->sp.pair_off.as<int64_t>(); pr.n_ev = n_ev;
    SpEvents ev2 = {};
    int64_t n_tiles2 = 0;
    if (pairs > 0) {
        HIP_TRY(ctx, ctx->sp.keep.reserve(static_cast<size_t>(pairs)));
        const unsigned jgrid = static_cast<unsigned>(std::min<int64_t>((pairs + 3) / 4, 1 << 20));
        hipLaunchKernelGGL(sp_judge_kernel, dim3(jgrid), dim3(256), 0, ctx->stream, d_y, pr, ctx->sp.hits.as<int32_t>(), pairs, h1,
                           ctx->sp.keep.as<uint8_t>());
        HIP_TRY(ctx, hipGetLastError());
        if (int rc = sp_upload(ctx, ctx->sp.tab2, tab2, pair_off.data(), n_pairs.data(), n_ev, &ev2, &n_tiles2)) return rc;
        if (int rc = sp_count(ctx, KeepPred{ctx->sp.keep.as<uint8_t>()}, ev2, n_tiles2, ctx->sp.off2, kept_off)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        HIP_TRY(ctx, ctx->sp.off2.reserve((n + 1) * sizeof(int64_t)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->sp.off2.p, 0, (n + 1) * sizeof(int64_t), ctx->stream));
    }
    // 4. the spans [0, s_1), [t_1, s_2), ..., [t_k, n): one more than the kept pairs (an empty event has none)
    std::vector<int64_t> n_spans(n);
    for (size_t e = 0; e < n; ++e) n_spans[e] = h_ev_len[e] > 0 ? kept_off[e + 1] - kept_off[e] + 1 : 0;
    if (int rc = offsets_to_device(ctx, ctx->sp.span_off, n_spans.data(), n, cap, "span", h_span_off)) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    const int64_t total = h_span_off[n_ev];
    if (total == 0) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); return PS_OK; }
    if (int rc = sp_scatter(ctx, ev2, n_tiles2, kept_off[n], 0, ctx->sp.kept)) return rc;
    HIP_TRY(ctx, ctx->sp.len.reserve(n * sizeof(int64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sp.len.p, h_ev_len, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sp_fd_spans_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, ctx->stream, pr,
                       ctx->sp.len.as<int64_t>(), ctx->sp.hits.as<int32_t>(), ctx->sp.kept.as<int32_t>(), ctx->sp.off2.as<int64_t>(),
                       ctx->sp.span_off.as<int64_t>(), total, d_spans);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PS_OK;
}

}  // extern "C"
