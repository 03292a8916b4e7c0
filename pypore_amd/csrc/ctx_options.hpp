// ctx_options.hpp -- the options of a context (ps_set_option / ps_get_option, include/poreseg.h): their values, and ONE table that
// says for each its name, its PORESEG_* variable, the values it accepts, how a value is normalised, whether only the diagnostic
// library has it, and whether setting it acts on the context.  ps_set_option, ps_get_option and the diagnostic library's reading
// of the environment all go through opt_set / opt_get / opt_apply_env below; a default stands in CtxOptions and nowhere else.
// A new option is one member of CtxOptions and one row of OPT_ROWS.  Plain host C++, no HIP: poreseg.hip includes it, and so does
// the stand-alone program tests/native/ctx_options_check.cpp, which runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <stdint.h>

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "poreseg.h"
#include "seg_types.hpp"
#include "pool_plan.hpp"
#include "range_plan.hpp"
#include "filt_plan.hpp"

namespace ps {

// What the options are, as the setter left them (include/poreseg.h describes each at length).
struct CtxOptions {
    // ---- the segmentation chain ----
    int mode = 0;                 // MODE_FAST (seg_device.hpp) 0: screen + exact, 1: exact fp64 scans only, 2: verify
    int spine_nt = 512, tree_nt = 256;   // workgroup sizes of the LDS-window kernels
    int prune = 1;                // 0: no block pruning in the LDS-window scan
    int scan_bs = 1;              // 1: block-sum scan with single-wave workgroups (seg_bs.hpp), 0: LDS-window scan
    int groups = 1;               // 1: K0 writes group records and the window scans start with the coarse pass over them (narrow digest), 0: every row is swept
    int wide_bs = 1;              // 1: counts too wide for the 32-bit digest are retried on the 64-bit digest, 0: straight to the LDS-window scan
    int stitch_host = 0;          // 1: host stitch with halo tiles (the fallback path) always
    int timing = 1;               // 0: no events, 1: start/end of the sequence, 2: an event between the phases as well (each costs
                                  // ~6 us of idle GPU: the next kernel does not start back to back)
    int debug = 0;                // the library says on stderr which seams gave up, which occupancy it found (prints only; results unchanged)
    int noise_k_ppm = 100000;     // near-tie accounting of the wide route, in millionths (DevCfg::noise_k: opt_noise_k)
    long long near_tie_log = 65536;   // records of the near-tie log (DevCfg::nt_log, ps_get_near_ties), 0: off
    // K0
    int k0_waves = 0;             // > 0: K0 runs as a persistent kernel, this many waves per SIMD (twice that for int16 samples) striding over the call with
                                  // their next wave block's samples in flight (round 5) -- what a context that shares the chip wants (0.193 -> 0.170 ms
                                  // per step with sixteen calls in flight); 0: one wave per wave block, as many as the registers allow -- faster
                                  // for a call that has the chip to itself (1e9 samples: K0 0.91 against 0.98 ms)
    int k0_admit = 0;             // > 0: at most this many calls of the device have their K0 in flight (K0Chain); 0: no limit
    int k0_shared = 0;            // 1: upload + K0 of this context run on the device's shared FRONT stream (round 5): the K0 launches of all contexts that
                                  // ask for it are serialised there, back to back, and the context's own stream takes over behind an event.  K0 is the
                                  // one kernel of a call that is bound by HBM; several of them at once only share the same bytes per second while the
                                  // scan kernels behind each of them wait -- in a row, call i's scans run under call i+1's K0 (measured slower: nothing sets it)
    int k0_unaligned = 1;         // as asked for: 1 K0's fast route loads 16 bytes from sample-aligned addresses where the probe of ps_create allows
                                  // it (ps_ctx::k0_unaligned has the answer), 0 the 16-byte condition of rounds 1-4 (tests)
    int upload_by_kernel = 1;     // 1: the call's host tables are fetched by a kernel (no SDMA hand-over), 0: hipMemcpyAsync
    int download_by_kernel = 1;   // 1 (round 6): status block + per-event offsets go back by a kernel writing pinned memory, 0: hipMemcpyAsync
    int single_pass = 1;          // 1 (round 6): ps_detect_segment_trace runs K0 once over the whole trace (detector + every event from one digest), 0: the two calls
    int gather_fused = 1;         // 1 (round 6): the gather places its items from per-256-job count sums (gather_scan_kernel), no item_scan_kernel; 0: rounds 2-5
    // subtree jobs
    int tree_mw = 0;              // 1: block-sum tree kernel with TREE_W waves per workgroup sharing their job list (round 3: single-wave workgroups
                                  // are faster at four waves per SIMD and need no spills)
    int tree_par = 1;             // 1: subtree jobs on the 64-bit digest (filtered events: deep recursions) are shared by the waves of a workgroup (tree_par_kernel), 0: one wave per job
    int tree_tail_pct = 0;        // tree_mw_kernel: share of the job list drawn dynamically (counter in HBM) at the end
    int tree_jobs_per_wave = 4;   // subtree kernel: jobs / this many slots work, between half and all of them (0: all)
    int tree_screen = 1;          // 1: on the narrow digest tree_screen_kernel runs in front of the subtree kernel and leaves it the jobs it cannot
                                  // prove empty (seg_device.hpp), 0: the subtree kernel takes every job, launch for launch as before
    // Share of the resident wave slots the single-wave scan kernels are launched on (experiments; the subtree kernel
    // decides on the device how many of its slots work: tree_jobs_per_wave, seg_device.hpp: tree_kernel).  Measured on
    // the bench trace with 100 / 75 / 62 / 50 / 44 / 37 %: four calls in flight 0.274 / 0.253 / 0.250 / 0.2445 / 0.257 /
    // 0.270 ms per step, one call 0.522 / 0.499 / 0.511 / 0.505 / 0.572 / 0.563 ms (below 50 % the spine kernel's 2 048
    // tiles are no longer all resident); on the 1e9-sample trace 50 % costs 23 % (spine 0.76 -> 1.12 ms, subtrees 0.68 ->
    // 0.90): with many jobs per slot four waves per SIMD deliver 1.4 x the throughput of two.
    int slots_pct = 100;
    // seams
    int bridge_single = 1 << 30;  // anchors a single-wave bridge adds before it hands the seam to the look-ahead kernel (measured: handing over early is slower)
    int bridge_budget = BR_MAX;   // anchors before a seam gives up -- tests lower it to reach the second chance on small inputs
    int bridge_ext = 1;           // 0: a seam that gave up goes straight to the host stitch, as before round 5
    int bridge_patience = 16;     // BR_PATIENCE_POOL (seg_device.hpp): windows without a hit that a bridge of a pooled call walks before it defers
                                  // its seam (short_chain) -- tests lower it to reach the hand-over on small inputs
    // lat_help: 0 every seam walks alone, 1 idle workgroups of the look-ahead kernel help (they leave when nothing has been listed
    // for ~0.1 ms), 2 as 1 but the helpers stay until every workgroup of the launch is through with its own seams -- for a test
    // that must SEE the helpers work; only for a call that has the chip to itself (a helper then waits for nobody)
    int lat_help = 1;
    // short_chain: 1 the launches a call can do without are left out, 0 the launches of the library before the option, launch for
    // launch; 2 / 3 one part at a time, for measurements (opt_short_chain_bits): no look-ahead launch in a pooled call -- its
    // bridges walk bridge_patience windows, a seam still deferred takes the second chance -- / the download kernel leaves the status
    // block zero, so that a call that repeats the layout launches no upload
    int short_chain = 1;
    // shared_device: the number of contexts that share this device (a pool of host threads, include/poreseg.h) as last set (<= 1: a
    // lone context).  Of n contexts min(n, hardware queues) calls execute at a time: setting it plans k0_waves, k0_admit and
    // lat_help for that many (pool_plan.hpp), but a call is a pooled call whenever n > 1
    int shared_device = 0;
    int hw_queues = 0;            // the hardware queues the next shared_device plans for (0: the process's own, GPU_MAX_HW_QUEUES) -- tests, tools
    // ---- the other features: bytes of scratch per launch, and their switches ----
    int filter_fused = 1;         // 1: fast filters run both directions in one kernel over tiles with halos, 0: always the exact three-pass scan
    long long filt_batch_scratch = FILT_BATCH_SCRATCH_DEFAULT;   // order-n scratch rows per launch of a filter batch
    long long range_tile = RANGE_TILE_DEFAULT;                   // ps_range_stats: samples per unit at most
    long long pairwise_budget = 2ll << 30;   // pairwise scratch
    long long trf_budget = 2ll << 30;        // splitter scratch
    long long hmm_bp_budget = 512ll << 20;   // Viterbi backpointers
    long long hmm_fb_budget = 4ll << 30;     // forward matrices
    bool hmm_expect_lds = true;   // 0: the E-step's accumulator rows stay in global memory
    // ---- the diagnostic library only (make -C pypore_amd/csrc diag): switches that return WRONG or stale results ----
    int dbg_phase = 0;            // 1 a call that repeats the previous one's layout skips K0 (the digest is still there: what the scan kernels cost
                                  // on their own), 2 K0 only
    int dbg_k0_nogrp = 0;         // 1 a call that repeats the previous one's layout runs K0 WITHOUT its group-record part (the records of the previous
                                  // call are still there and the scans read those: what K0's ~37 instructions per block cost the step)
    int k0_sets = 2;              // register sets of a persistent K0 wave (seg_bs.hpp: blocksum_kernel<DT, NS>)
    int scan_lds_pad = 0;         // unused dynamic LDS per single-wave scan workgroup -- caps the scan waves per SIMD
    int rep_eval = 1, rep_stage = 1, rep_sum = 1;
    long long cu_mask = 0;        // first | count << 12 | stride << 24 | invert << 32: the context's OWN stream on those CUs only (count 0: all)
};

#ifdef PS_DIAG
constexpr bool OPT_DIAG_BUILD = true;
#else
constexpr bool OPT_DIAG_BUILD = false;
#endif

enum OptNorm : int { OPT_AS_GIVEN, OPT_BOOL, OPT_CLAMP };     // what is stored: the value, value != 0, the value clamped to lo .. hi (never refused)
enum OptEnv : int { ENV_INT, ENV_MILLIONTHS };                // the variable's text: a whole number, or a decimal fraction of which the option takes the millionths
// what ps_set_option does on the context after a value went in
enum OptEffect : int { FX_NONE, FX_SHARED_DEVICE, FX_SHORT_CHAIN, FX_BRIDGE_PATIENCE, FX_WIDE_BS, FX_K0_UNALIGNED, FX_CU_MASK };
enum OptStatus : int { OPT_OK, OPT_UNKNOWN, OPT_REFUSED };

struct OptRow {
    const char *name;
    const char *env;              // the PORESEG_* variable the diagnostic library and engine.options_from_env read, or nullptr
    int64_t (*read)(const CtxOptions &);
    void (*write)(CtxOptions &, int64_t);
    int64_t lo, hi;               // accepted (OPT_CLAMP: stored) values
    bool (*also)(int64_t);        // a further condition on a value in lo .. hi (a set of values, a predicate), or nullptr
    OptNorm norm;
    bool diag;                    // the diagnostic library only: unknown to the product
    OptEffect effect;
    OptEnv env_text;
};

template <auto M> int64_t opt_read(const CtxOptions &o) { return static_cast<int64_t>(o.*M); }
template <auto M> void opt_write(CtxOptions &o, int64_t v) { o.*M = static_cast<std::remove_reference_t<decltype(o.*M)>>(v); }
#define PS_OPT(member) &opt_read<&CtxOptions::member>, &opt_write<&CtxOptions::member>

constexpr int64_t OPT_ANY_LO = INT64_MIN, OPT_ANY_HI = INT64_MAX;
inline bool opt_spine_nt_ok(int64_t v) { return v == 256 || v == 512 || v == 1024; }
inline bool opt_tree_nt_ok(int64_t v) { return v == 256 || v == 512; }

// One row per option.  RANGE: lo .. hi or refused; BOOL: any value, stored as value != 0.
#define PS_ROW_RANGE(name, env, member, lo, hi) {name, env, PS_OPT(member), lo, hi, nullptr, OPT_AS_GIVEN, false, FX_NONE, ENV_INT}
#define PS_ROW_BOOL(name, env, member) {name, env, PS_OPT(member), OPT_ANY_LO, OPT_ANY_HI, nullptr, OPT_BOOL, false, FX_NONE, ENV_INT}
#define PS_ROW_DIAG(name, env, member, lo, hi, norm, fx) {name, env, PS_OPT(member), lo, hi, nullptr, norm, true, fx, ENV_INT}
constexpr OptRow OPT_ROWS[] = {
    PS_ROW_RANGE("mode", "PORESEG_MODE", mode, 0, 2),
    {"spine_nt", "PORESEG_SPINE_NT", PS_OPT(spine_nt), 256, 1024, opt_spine_nt_ok, OPT_AS_GIVEN, false, FX_NONE, ENV_INT},
    {"tree_nt", "PORESEG_TREE_NT", PS_OPT(tree_nt), 256, 512, opt_tree_nt_ok, OPT_AS_GIVEN, false, FX_NONE, ENV_INT},
    PS_ROW_BOOL("prune", "PORESEG_PRUNE", prune),
    PS_ROW_BOOL("scan_bs", "PORESEG_SCAN_BS", scan_bs),
    PS_ROW_BOOL("groups", "PORESEG_GROUPS", groups),
    {"wide_bs", "PORESEG_WIDE_BS", PS_OPT(wide_bs), OPT_ANY_LO, OPT_ANY_HI, nullptr, OPT_BOOL, false, FX_WIDE_BS, ENV_INT},
    PS_ROW_BOOL("stitch_host", nullptr, stitch_host),               // (PORESEG_STITCH=host: text, read where the variables are read)
    {"timing", "PORESEG_TIMING", PS_OPT(timing), 0, 2, nullptr, OPT_CLAMP, false, FX_NONE, ENV_INT},
    PS_ROW_BOOL("debug", "PORESEG_DEBUG", debug),
    {"noise_k_ppm", "PORESEG_NOISE_K", PS_OPT(noise_k_ppm), 0, INT32_MAX, nullptr, OPT_AS_GIVEN, false, FX_NONE, ENV_MILLIONTHS},
    PS_ROW_RANGE("near_tie_log", nullptr, near_tie_log, 0, int64_t(1) << 30),
    PS_ROW_RANGE("k0_waves", "PORESEG_K0_WAVES", k0_waves, 0, 16),
    PS_ROW_RANGE("k0_admit", "PORESEG_K0_MAX", k0_admit, 0, INT32_MAX),
    PS_ROW_BOOL("k0_shared", "PORESEG_K0_SHARED", k0_shared),
    {"k0_unaligned", "PORESEG_K0_UNALIGNED", PS_OPT(k0_unaligned), OPT_ANY_LO, OPT_ANY_HI, nullptr, OPT_BOOL, false, FX_K0_UNALIGNED, ENV_INT},
    PS_ROW_BOOL("upload_by_kernel", "PORESEG_UPLOAD", upload_by_kernel),
    PS_ROW_BOOL("download_by_kernel", "PORESEG_DOWNLOAD", download_by_kernel),
    PS_ROW_BOOL("single_pass", "PORESEG_SINGLE_PASS", single_pass),
    PS_ROW_BOOL("gather_fused", "PORESEG_GATHER_FUSED", gather_fused),
    PS_ROW_BOOL("tree_mw", "PORESEG_TREE_MW", tree_mw),
    PS_ROW_BOOL("tree_par", "PORESEG_TREE_PAR", tree_par),
    PS_ROW_RANGE("tree_tail_pct", "PORESEG_TREE_TAIL", tree_tail_pct, 0, 100),
    PS_ROW_RANGE("tree_jobs_per_wave", "PORESEG_TREE_JPW", tree_jobs_per_wave, 0, 1024),
    PS_ROW_BOOL("tree_screen", "PORESEG_TREE_SCREEN", tree_screen),
    PS_ROW_RANGE("slots_pct", "PORESEG_SLOTS_PCT", slots_pct, 1, 100),
    PS_ROW_RANGE("bridge_single", "PORESEG_BRIDGE_SINGLE", bridge_single, 1, INT32_MAX),
    PS_ROW_RANGE("bridge_budget", "PORESEG_BRIDGE_BUDGET", bridge_budget, 1, BR_MAX),
    PS_ROW_RANGE("bridge_ext", "PORESEG_BRIDGE_EXT", bridge_ext, 0, 1),
    {"bridge_patience", "PORESEG_BRIDGE_PATIENCE", PS_OPT(bridge_patience), 1, 4096, nullptr, OPT_AS_GIVEN, false, FX_BRIDGE_PATIENCE, ENV_INT},
    PS_ROW_RANGE("lat_help", "PORESEG_LAT_HELP", lat_help, 0, 2),
    {"short_chain", "PORESEG_SHORT_CHAIN", PS_OPT(short_chain), 0, 3, nullptr, OPT_AS_GIVEN, false, FX_SHORT_CHAIN, ENV_INT},
    {"shared_device", nullptr, PS_OPT(shared_device), 0, 4096, nullptr, OPT_AS_GIVEN, false, FX_SHARED_DEVICE, ENV_INT},
    PS_ROW_RANGE("hw_queues", nullptr, hw_queues, 0, HW_QUEUES_MAX),
    PS_ROW_BOOL("filter_fused", "PORESEG_FILTER_FUSED", filter_fused),
    PS_ROW_RANGE("filt_batch_scratch", nullptr, filt_batch_scratch, 1, OPT_ANY_HI),
    {"range_tile", nullptr, PS_OPT(range_tile), RANGE_TILE_MIN, RANGE_TILE_MAX, range_tile_ok, OPT_AS_GIVEN, false, FX_NONE, ENV_INT},
    PS_ROW_RANGE("pairwise_budget", nullptr, pairwise_budget, 1, OPT_ANY_HI),
    PS_ROW_RANGE("trf_budget", nullptr, trf_budget, 1, OPT_ANY_HI),
    PS_ROW_RANGE("hmm_bp_budget", nullptr, hmm_bp_budget, 1, OPT_ANY_HI),
    PS_ROW_RANGE("hmm_fb_budget", nullptr, hmm_fb_budget, 1, OPT_ANY_HI),
    PS_ROW_BOOL("hmm_expect_lds", nullptr, hmm_expect_lds),
    PS_ROW_DIAG("dbg_phase", "PORESEG_DBG_PHASE", dbg_phase, 0, 2, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("dbg_k0_nogrp", "PORESEG_DBG_K0_NOGRP", dbg_k0_nogrp, OPT_ANY_LO, OPT_ANY_HI, OPT_BOOL, FX_NONE),
    PS_ROW_DIAG("k0_sets", "PORESEG_K0_SETS", k0_sets, 2, 4, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("scan_lds_pad", "PORESEG_SCAN_LDS_PAD", scan_lds_pad, 0, 65536, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("rep_eval", "PORESEG_REP_EVAL", rep_eval, 1, INT32_MAX, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("rep_stage", "PORESEG_REP_STAGE", rep_stage, 1, INT32_MAX, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("rep_sum", "PORESEG_REP_SUM", rep_sum, 1, INT32_MAX, OPT_AS_GIVEN, FX_NONE),
    PS_ROW_DIAG("cu_mask", nullptr, cu_mask, OPT_ANY_LO, OPT_ANY_HI, OPT_AS_GIVEN, FX_CU_MASK),
};
#undef PS_ROW_RANGE
#undef PS_ROW_BOOL
#undef PS_ROW_DIAG
#undef PS_OPT

// The variables of the diagnostic library that are no option's: the tiling (ps_set_tiling), stitch_host as text ("host"), and the
// front stream's priority.  PORESEG_DEBUG set to nothing at all counts as 1.
constexpr const char *ENV_TILE = "PORESEG_TILE", *ENV_HALO = "PORESEG_HALO", *ENV_STITCH = "PORESEG_STITCH", *ENV_DEBUG = "PORESEG_DEBUG",
                     *ENV_FRONT_PRIORITY = "PORESEG_FRONT_PRIORITY";

// The row of an option this build has, or nullptr.
inline const OptRow *opt_find(const char *name)
{
    if (!name) return nullptr;
    for (const OptRow &r : OPT_ROWS)
        if ((OPT_DIAG_BUILD || !r.diag) && !std::strcmp(r.name, name)) return &r;
    return nullptr;
}

// Sets one option.  *row (may be null) names the row that took or refused the value; a refused value leaves the option as it was.
inline OptStatus opt_set(CtxOptions *o, const char *name, int64_t value, const OptRow **row = nullptr)
{
    const OptRow *r = opt_find(name);
    if (row) *row = r;
    if (!r) return OPT_UNKNOWN;
    if (r->norm == OPT_BOOL) value = value != 0;
    else if (r->norm == OPT_CLAMP) value = value < r->lo ? r->lo : value > r->hi ? r->hi : value;
    else if (value < r->lo || value > r->hi || (r->also && !r->also(value))) return OPT_REFUSED;
    r->write(*o, value);
    return OPT_OK;
}

inline OptStatus opt_get(const CtxOptions &o, const char *name, int64_t *value, const OptRow **row = nullptr)
{
    const OptRow *r = opt_find(name);
    if (row) *row = r;
    if (!r) return OPT_UNKNOWN;
    *value = r->read(o);
    return OPT_OK;
}

// A variable's text as the value its option is set to: false when it is no number of the row's kind.
inline bool opt_env_value(const OptRow &r, const char *text, int64_t *value)
{
    char *end = nullptr;
    errno = 0;
    if (r.env_text == ENV_MILLIONTHS) {
        const double x = std::strtod(text, &end) * 1.0e6;
        if (!(x >= -9.0e18 && x <= 9.0e18)) return false;       // (NaN too)
        *value = std::llround(x);
    } else {
        *value = std::strtoll(text, &end, 10);
    }
    if (end == text || errno == ERANGE) return false;
    while (*end == ' ' || *end == '\t' || *end == '\n') ++end;
    return *end == 0;
}

// Sets every option of this build whose variable `env` (a getenv) knows and holds text, through opt_set; a variable that is
// absent or empty leaves its option alone.  Returns the options whose variable held what opt_set refused or no number at all.
template <class Getenv> std::vector<const char *> opt_apply_env(CtxOptions *o, Getenv env)
{
    std::vector<const char *> refused;
    for (const OptRow &r : OPT_ROWS) {
        if (!r.env || (r.diag && !OPT_DIAG_BUILD)) continue;
        const char *text = env(r.env);
        if (!text || !text[0]) continue;
        int64_t value = 0;
        if (!opt_env_value(r, text, &value) || opt_set(o, r.name, value) != OPT_OK) refused.push_back(r.name);
    }
    return refused;
}

// short_chain as set (0 .. 3) <-> the launches a call does without
enum : int { SC_NO_LA = 1, SC_NO_UPLOAD = 2, SC_ALL = 3 };
constexpr int OPT_SHORT_CHAIN_BITS[4] = {0, SC_ALL, SC_NO_LA, SC_NO_UPLOAD};
inline int opt_short_chain_bits(int short_chain) { return OPT_SHORT_CHAIN_BITS[short_chain & 3]; }
inline int opt_short_chain_of_bits(int bits)
{
    for (int v = 0; v < 4; ++v)
        if (OPT_SHORT_CHAIN_BITS[v] == bits) return v;
    return -1;
}
// noise_k_ppm -> the factor the kernels see (100 000 -> 0.1f)
inline float opt_noise_k(int noise_k_ppm) { return static_cast<float>(static_cast<double>(noise_k_ppm) * 1.0e-6); }

}  // namespace ps
