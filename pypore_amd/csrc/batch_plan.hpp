// batch_plan.hpp -- the host's planning of the batch entry points (ps_align_batch, ps_pairwise_batch, ps_trf_split_batch, the
// ps_hmm_* entries, ps_statsplit_f64, ps_snakebase_f64, ps_filter_derivative_f64): the sizes and caps planning and kernels
// share, what the entries refuse in their offset and event tables, how a batch is cut into launches under a scratch budget, the
// grid of a launch, the per-event tables.  Plain host C++ on <stdint.h> and the standard library, no HIP: poreseg.hip and the
// kernel headers include it and define none of it again, and so does the stand-alone program tests/native/batch_plan_check.cpp,
// which runs it under the address and undefined-behaviour sanitizers.  A refusal is an error code and the index it names; the
// messages are the entry points'.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

// the functions the kernels call too: host and device under HIP, plain functions in a host build
#if defined(__HIP__) || defined(__HIPCC__)
#define PS_HD __host__ __device__
#else
#define PS_HD
#endif

namespace ps {

enum BatchPlanError {
    BATCH_PLAN_OK = 0,
    BATCH_PLAN_ORDER,       // an offset is negative or below its predecessor
    BATCH_PLAN_LONG,        // a sequence longer than INT32_MAX / 2, an event longer than 2^30
    BATCH_PLAN_NEGATIVE,    // an event's start or length is negative
    BATCH_PLAN_RANGE,       // an event's [lo, hi) leaves its samples
    BATCH_PLAN_SHORT,       // an event shorter than min_len
    BATCH_PLAN_TOO_MANY,    // more than INT32_MAX tiles
    BATCH_PLAN_SCRATCH,     // one item alone needs more than SCRATCH_ITEM_MAX bytes
    BATCH_PLAN_CAPACITY     // the counts add up to more than the capacity
};

// ---- sizes and caps --------------------------------------------------------------------------------------------------------

// the pairwise aligner (seg_pairwise.hpp)
constexpr int PW_NT = 64;
constexpr int PW_N_MAX = 8190;                  // y elements (LDS: y and the border row, 16 bytes per element)
PS_HD inline size_t pw_lds_bytes(int n_cap) { return (2 * static_cast<size_t>(n_cap) + 2) * sizeof(double); }
// bytes of scratch per workgroup: scores, row maxima (8-byte entries first), first columns, pointer bytes
PS_HD inline unsigned long long pw_scratch_bytes(unsigned long long cells, unsigned long long rows)
{
    return (8ull * cells + 8ull * rows + 4ull * rows + cells + 15ull) & ~15ull;
}

// the repeat splitter (seg_trf.hpp)
constexpr int TRF_NT = 64;
constexpr int TRF_N_MAX = 2048;                 // segments per sequence (LDS: 24 bytes per segment; scratch: 1.6 MB at the cap)
PS_HD constexpr size_t trf_lds_bytes(int n_cap) { return (3 * static_cast<size_t>(n_cap) + 1) * sizeof(double); }
// 64-bit words per row of the mask in skewed coordinates (steps of a stripe: at most n + 63); the pointers take twice that
PS_HD inline unsigned long long trf_row_words(int n_cap) { return (static_cast<unsigned long long>(n_cap) + 127ull) / 64ull; }
// bytes of scratch per workgroup: mask rows 0 .. n_cap, pointer rows 1 .. n_cap
PS_HD inline unsigned long long trf_scratch_bytes(int n_cap)
{
    const unsigned long long w = trf_row_words(n_cap), n = static_cast<unsigned long long>(n_cap);
    return 8ull * w * (n + 1ull) + 16ull * w * n;
}

// the segment aligner (seg_align.hpp)
constexpr int ALIGN_NT = 64;
constexpr int ALIGN_M_MAX = 1024;               // model segments (LDS: 13+ rows of m doubles)
constexpr int ALIGN_B_MAX = 32;                 // rows per traceback block
// LDS (doubles): 5 model rows, 2 score rows, skip, back | traceback block: (B+1) score rows, B skip rows, B back rows
// | 3 x 64 sequence values | 2 dummy cells
PS_HD inline size_t align_lds_doubles(int m, int B) { return static_cast<size_t>(9 + 3 * B + 1) * m + 3 * 64 + 2; }

// the sequence models (seg_hmm.hpp).  ps_hmm_expect: LDS bytes at most for the accumulator row beside the two score rows (else
// the row stays in global memory), and the bytes of all workgroups' rows at most (the grid shrinks to fit)
constexpr int HMM_NT = 64;                      // one wave per workgroup
constexpr size_t HMM_EXPECT_LDS = 64u << 10;
constexpr size_t HMM_EXPECT_ROWS = 256u << 20;

// the state parsers' compaction (seg_state.hpp)
constexpr int SP_NT = 256;                         // threads of a compaction workgroup
constexpr int SP_ROUNDS = 8;                       // positions per thread
constexpr int SP_TILE = SP_NT * SP_ROUNDS;         // positions per tile (2 048)

// ---- offset and event tables -----------------------------------------------------------------------------------------------

// entry q of a slot-offset table (n + 1 entries): non-negative and not above its successor
inline bool slot_ok(const int64_t *off, int32_t q) { return off[q] >= 0 && off[q + 1] >= off[q]; }

inline BatchPlanError check_slot_offsets(const int64_t *off, int32_t n, int32_t *bad)
{
    for (int32_t q = 0; q < n; ++q)
        if (!slot_ok(off, q)) { *bad = q; return BATCH_PLAN_ORDER; }
    return BATCH_PLAN_OK;
}

// Offsets of a set of sequences: non-negative, ascending (the signs first: the difference of two non-negative offsets cannot
// overflow), no sequence longer than INT32_MAX / 2; *longest = the longest sequence
inline BatchPlanError check_offsets(const int64_t *off, int32_t n, int64_t *longest, int32_t *bad)
{
    *longest = 0;
    for (int32_t q = 0; q < n; ++q) {
        *bad = q;
        if (!slot_ok(off, q)) return BATCH_PLAN_ORDER;
        const int64_t len = off[q + 1] - off[q];
        if (len > INT32_MAX / 2) return BATCH_PLAN_LONG;
        *longest = std::max(*longest, len);
    }
    *bad = -1;
    return BATCH_PLAN_OK;
}

// The event table of StatSplit and the state parsers, events taken in order: start >= 0 and len >= 0 (BATCH_PLAN_NEGATIVE),
// len <= 2^30 (BATCH_PLAN_LONG), the optional ranges lo[e], hi[e] within [0, len] each -- hi below lo is an empty range --
// (BATCH_PLAN_RANGE), len >= min_len (BATCH_PLAN_SHORT); *bad names the event.  *total = the samples of all events: the caller
// may pass no data only when it is 0.
constexpr int64_t EVENT_LEN_MAX = 1ll << 30;
inline BatchPlanError check_events(const int64_t *start, const int64_t *len, int32_t n_ev, const int64_t *lo, const int64_t *hi,
                                   int64_t min_len, int64_t *total, int32_t *bad)
{
    *total = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        *bad = e;
        if (len[e] < 0 || start[e] < 0) return BATCH_PLAN_NEGATIVE;
        if (len[e] > EVENT_LEN_MAX) return BATCH_PLAN_LONG;
        if ((lo && (lo[e] < 0 || lo[e] > len[e])) || (hi && (hi[e] < 0 || hi[e] > len[e]))) return BATCH_PLAN_RANGE;
        if (len[e] < min_len) return BATCH_PLAN_SHORT;
        *total += len[e];
    }
    *bad = -1;
    return BATCH_PLAN_OK;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------

// The grid of a launch that wants `want` workgroups on a device that keeps `slots` resident, each with per_wg_bytes of a buffer
// of budget_bytes: as many as fit, one at least (a lone workgroup may exceed the budget).
inline unsigned budget_grid(unsigned want, unsigned slots, unsigned long long budget_bytes, unsigned long long per_wg_bytes)
{
    return static_cast<unsigned>(std::max<unsigned long long>(1, std::min<unsigned long long>(std::min(want, slots), budget_bytes / per_wg_bytes)));
}

// q1 of the launch that starts at sequence q0: as many sequences as keep (len + 1) * row_bytes within the budget, at least
// one; *bytes = what they take
inline int32_t next_chunk(const int64_t *h_off, int32_t q0, int32_t n_seq, size_t row_bytes, long long budget, long long *bytes)
{
    *bytes = (h_off[q0 + 1] - h_off[q0] + 1) * static_cast<long long>(row_bytes);
    int32_t q1 = q0 + 1;
    while (q1 < n_seq) {
        const long long more = (h_off[q1 + 1] - h_off[q1] + 1) * static_cast<long long>(row_bytes);
        if (*bytes + more > budget) break;
        *bytes += more; ++q1;
    }
    return q1;
}

// What a scratch launch is sized by.  A dims type starts as the smallest item, says whether an item would enlarge the launch's
// scratch (grown_by), takes an item in (component-wise maximum) and gives the scratch of one workgroup and the dynamic LDS.
struct PwDims {                                 // a pair: cells = m * n, rows = m, n_cap = n (a longer y alone only costs LDS)
    unsigned long long cells = 1, rows = 1;
    int n_cap = 1;
    bool grown_by(const PwDims &d) const { return d.cells > cells || d.rows > rows; }
    void join(const PwDims &d) { cells = std::max(cells, d.cells); rows = std::max(rows, d.rows); n_cap = std::max(n_cap, d.n_cap); }
    unsigned long long scratch_bytes() const { return pw_scratch_bytes(cells, rows); }
    size_t lds_bytes() const { return pw_lds_bytes(n_cap); }
};
struct TrfDims {                                // a sequence of n_cap segments
    int n_cap = 1;
    bool grown_by(const TrfDims &d) const { return d.n_cap > n_cap; }
    void join(const TrfDims &d) { n_cap = std::max(n_cap, d.n_cap); }
    unsigned long long scratch_bytes() const { return trf_scratch_bytes(n_cap); }
    size_t lds_bytes() const { return trf_lds_bytes(n_cap); }
};

// One launch of "a workgroup per item, scratch sized by the launch's largest item": items [q0, q1) on `grid` workgroups of
// per_wg bytes of scratch and lds bytes of dynamic LDS each.
template <class Dims> struct ScratchLaunch {
    int32_t q0 = 0, q1 = 0;
    Dims dims;
    unsigned long long per_wg = 0;
    size_t lds = 0;
    unsigned grid = 0;
};
constexpr unsigned long long SCRATCH_ITEM_MAX = 32ull << 30;

// The launch that starts at item q0 < n.  Consecutive items join it; one that enlarges its scratch joins only while
// min(items so far + 1, slots of the launch's first item) workgroups of the enlarged scratch stay within the budget (the slots
// of the first item bound the grid; more LDS only lowers them).  Then grid = budget_grid(items, slots(final LDS), budget,
// per_wg): a launch whose first item alone leaves room for few workgroups runs on that many.  item(q) gives the dims of item q;
// slots(lds) the resident workgroups at that dynamic LDS -- asked once after the first item, at its LDS, and once for the
// finished launch.  BATCH_PLAN_SCRATCH: the launch (its first item, then) needs more than SCRATCH_ITEM_MAX per workgroup.
template <class Dims, class Item, class Slots>
BatchPlanError next_scratch_launch(int32_t q0, int32_t n, unsigned long long budget, Item &&item, Slots &&slots, ScratchLaunch<Dims> *L)
{
    *L = ScratchLaunch<Dims>();
    L->q0 = L->q1 = q0;
    unsigned first_slots = 0;
    while (L->q1 < n) {
        const Dims d = item(L->q1);
        Dims joined = L->dims;
        joined.join(d);
        if (L->q1 > q0 && L->dims.grown_by(d)) {
            const unsigned long long g = std::min<unsigned long long>(static_cast<unsigned long long>(L->q1 - q0) + 1, first_slots);
            if (g * joined.scratch_bytes() > budget) break;
        }
        L->dims = joined; ++L->q1;
        if (L->q1 == q0 + 1) first_slots = slots(L->dims.lds_bytes());
    }
    L->per_wg = L->dims.scratch_bytes();
    if (L->per_wg > SCRATCH_ITEM_MAX) return BATCH_PLAN_SCRATCH;
    L->lds = L->dims.lds_bytes();
    L->grid = budget_grid(static_cast<unsigned>(L->q1 - q0), slots(L->lds), budget, L->per_wg);
    return BATCH_PLAN_OK;
}

// ps_align_batch: the traceback block B -- as many rows as fit in ~48 KB of LDS next to the 9 working rows; 12 KB when the
// batch is large enough to want many resident workgroups per CU instead --, the dynamic LDS, the scratch of one workgroup
// (score, skip_score and backslip_score of the longest sequence, in doubles) and the workgroups 2 GiB of scratch allow (one at
// least: unless one sequence needs more).  BATCH_PLAN_SCRATCH: one sequence needs more than SCRATCH_ITEM_MAX.
struct AlignPlan {
    int B = 0;
    size_t lds = 0;
    unsigned long long per_wg = 0;              // doubles
    unsigned grid_cap = 0;
};
constexpr unsigned long long ALIGN_SCRATCH_BUDGET = 2ull << 30;
inline BatchPlanError align_plan(int32_t m, int32_t n_seq, int64_t s_max, AlignPlan *P)
{
    const size_t blk_budget = n_seq > 512 ? (12u << 10) : (48u << 10);
    P->B = static_cast<int>(std::max<size_t>(1, std::min<size_t>(ALIGN_B_MAX, blk_budget / (3u * m * sizeof(double)))));
    P->lds = align_lds_doubles(m, P->B) * sizeof(double);
    P->per_wg = 3ull * static_cast<unsigned long long>(std::max<int64_t>(s_max, 1)) * m;
    if (P->per_wg * sizeof(double) > SCRATCH_ITEM_MAX) return BATCH_PLAN_SCRATCH;
    P->grid_cap = budget_grid(UINT32_MAX, UINT32_MAX, ALIGN_SCRATCH_BUDGET, P->per_wg * sizeof(double));
    return BATCH_PLAN_OK;
}

// ---- per-event tables ----------------------------------------------------------------------------------------------------------

// ps_statsplit_f64's tables, after check_events (its refusals are this plan's): tab = six columns of n_ev entries -- start, len,
// pre (the event's first prefix sum: the events packed back to back), lo, hi (default: the whole event), slot (its first boundary
// slot) -- and the end of the slots; an event takes 2 * (span / mw) + 2 slots, span = max(0, hi - lo); stack_cap = the
// interval stack of the longest span.
struct StatsplitTables {
    std::vector<int64_t> tab;
    int64_t total_len = 0, slots = 0, stack_cap = 0;
};
inline BatchPlanError plan_statsplit_tables(const int64_t *start, const int64_t *len, int32_t n_ev, const int64_t *lo, const int64_t *hi,
                                            int64_t mw, StatsplitTables *T, int32_t *bad)
{
    if (const BatchPlanError err = check_events(start, len, n_ev, lo, hi, 0, &T->total_len, bad)) return err;
    const size_t n = static_cast<size_t>(n_ev);
    T->tab.assign(6 * n + 1, 0);
    int64_t *t = T->tab.data(), pre = 0, longest = 0;
    T->slots = 0;
    for (size_t e = 0; e < n; ++e) {
        const int64_t l = lo ? lo[e] : 0, h = hi ? hi[e] : len[e], span = std::max<int64_t>(0, h - l);
        t[e] = start[e]; t[n + e] = len[e]; t[2 * n + e] = pre; t[3 * n + e] = l; t[4 * n + e] = h; t[5 * n + e] = T->slots;
        pre += len[e];
        T->slots += 2 * (span / mw) + 2;
        longest = std::max(longest, span);
    }
    t[6 * n] = T->slots;
    T->stack_cap = longest / mw + 2;
    return BATCH_PLAN_OK;
}

// One compaction's tile table: tab = start, npos, tile_off (n_ev + 1 entries); event e has ceil(npos[e] / SP_TILE) tiles.
// BATCH_PLAN_TOO_MANY: more than INT32_MAX tiles.
inline BatchPlanError plan_tile_table(const int64_t *start, const int64_t *npos, int32_t n_ev, std::vector<int64_t> *tab, int64_t *n_tiles)
{
    const size_t n = static_cast<size_t>(n_ev);
    tab->assign(3 * n + 1, 0);
    int64_t tiles = 0;
    for (size_t e = 0; e < n; ++e) {
        (*tab)[e] = start[e]; (*tab)[n + e] = npos[e]; (*tab)[2 * n + e] = tiles;
        tiles += (npos[e] + SP_TILE - 1) / SP_TILE;
    }
    (*tab)[3 * n] = tiles;
    *n_tiles = tiles;
    return tiles > INT32_MAX ? BATCH_PLAN_TOO_MANY : BATCH_PLAN_OK;
}

// off[0 .. n] from n counts (off[0] = 0); *total = off[n].  BATCH_PLAN_CAPACITY: the total exceeds cap.
template <class Count>
BatchPlanError offsets_from_counts(const Count *counts, size_t n, int64_t cap, int64_t *off, int64_t *total)
{
    off[0] = 0;
    for (size_t e = 0; e < n; ++e) off[e + 1] = off[e] + counts[e];
    *total = off[n];
    return *total > cap ? BATCH_PLAN_CAPACITY : BATCH_PLAN_OK;
}

}  // namespace ps
