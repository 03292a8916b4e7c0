// seg_plan.hpp -- the host's planning of a segment call: which scan route a call takes, how its events are cut into tiles on
// either stitch route, the host stitch of the tile lists, which seams get a second chance.  Plain host C++, no HIP and no
// context: poreseg.hip includes it and acts on what it returns (buffers, uploads, launches), and so does the stand-alone
// program tests/native/seg_plan_check.cpp, which runs it on the CPU, plain and under the address and undefined-behaviour
// sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "seg_types.hpp"

namespace ps {

// ---- the scan route -----------------------------------------------------------------------------------------------------------
// block-sum scan: candidates must avoid the ragged ends of a window (min_width >= 8) and a window must fit the single-wave
// sweep (at most 64 digest chunks: W <= 64 512); otherwise the LDS-window kernels take the call
inline bool scan_route_bs(bool scan_bs_option, int mw, int W, bool exact_mode, bool d_f64)
{
    return scan_bs_option && mw >= 8 && W <= 63 * 1024 && !exact_mode && !d_f64;
}

// Counts too wide for the 32-bit digest (K0 says so): the call is redone on the 64-bit digest, and if that refuses too
// (|k - m| >= 2^23) on the LDS-window kernels.  The next WIDE_MEMORY calls on the same grid start where this one ended.
// bs_mode: 1 block-sum scan on the 32-bit digest, 2 on the 64-bit digest, 0 LDS-window scan; redo, as the call's counters
// report it: 0 none, 1 = 64-bit digest, 2 = LDS-window scan.
constexpr int WIDE_MEMORY = 16;
struct WideRedo {
    double quantum = 0;       // quantum of the last call K0 refused ...
    int skip = 0;             // ... and the number of calls with that quantum that still start where that call ended:
    int mode = 0;             // ... 2 = block-sum scan on the 64-bit digest, 0 = LDS-window scan
    int bs_mode = 0, redo = 0;    // the current call's route
    bool remembers(double q) const { return skip > 0 && q == quantum; }
    void forget() { skip = 0; }
    // the route a call starts on
    int begin(bool use_bs, double q)
    {
        bs_mode = use_bs ? 1 : 0;
        redo = 0;
        if (use_bs && remembers(q)) { bs_mode = mode; --skip; redo = bs_mode == 2 ? 1 : 2; }
        return bs_mode;
    }
    // ... and the one it goes on with after K0 refused it
    int refused(bool wide_bs_option, double q)
    {
        bs_mode = (bs_mode == 1 && wide_bs_option) ? 2 : 0;
        redo = bs_mode == 2 ? 1 : 2;
        quantum = q;
        mode = bs_mode;
        skip = WIDE_MEMORY;
        return bs_mode;
    }
};

// ---- tiles ---------------------------------------------------------------------------------------------------------------------
struct Anchor { int32_t pos, kind; };

struct TileList {
    int32_t start = 0;
    std::vector<Anchor> a;
    bool ended = false;
};

// position of `pos` in a tile list (exact match), -1 if the tile starts there, -2 if absent
inline int find_in(const TileList &t, int32_t pos)
{
    if (pos == t.start) return -1;
    auto it = std::lower_bound(t.a.begin(), t.a.end(), pos, [](const Anchor &x, int32_t v) { return x.pos < v; });
    if (it != t.a.end() && it->pos == pos) return static_cast<int>(it - t.a.begin());
    return -2;
}

// anchors of one chain are >= min_width apart and at most one lies at or beyond `stop`
inline int64_t spine_cap(int64_t start, int64_t stop, int mw) { return (stop - start) / mw + 4; }

// The spine job of tile [start, stop) of event `ev` (`len` samples at `base` of the sample array), its anchor list at out_off.
// TilePlace: where the tile stands among the tiles of its event (device stitch); the halo tiles of the host stitch and its
// seam repairs stand alone.
struct TilePlace { int64_t first_tile = 0, ntiles = 1, tile_len = 0x7fffffff, vbase = 0; };
inline SpineJob make_spine_job(int64_t base, int32_t ev, int64_t len, int64_t start, int64_t stop, int mw, int64_t out_off,
                               const TilePlace &place = TilePlace())
{
    SpineJob j;
    j.base = base;
    j.start = static_cast<int32_t>(start);
    j.end = static_cast<int32_t>(len);
    j.stop = static_cast<int32_t>(stop);
    j.out_cap = static_cast<int32_t>(std::min<int64_t>(spine_cap(start, stop, mw), 0x7fffffff));
    j.out_off = out_off;
    j.first_tile = static_cast<int32_t>(place.first_tile);
    j.ntiles = static_cast<int32_t>(place.ntiles);
    j.tile_len = static_cast<int32_t>(place.tile_len);
    j.ev = ev;
    j.vbase = place.vbase;
    return j;
}

// The device route's tile length for a call of total_len samples (tile_len_option > 0: the caller's).
// block-sum scan: one tile per wave slot of the scan kernels (4 096 at four waves per SIMD) when the tiles stay
// long (>= 8 W: a 1e9-sample trace, 3.05 -> 2.70 ms), else 1 536 tiles of at least 4 W (shorter tiles only add
// speculative windows and seams: measured on the 1e8-sample trace; round 4, with the lighter windows
// of the coarse pass: 2 048 -> 1 536 tiles, 0.2298 -> 0.2247 ms per step in five interleaved rounds, one call unchanged)
inline int64_t device_tile_len(int64_t total_len, int W, int64_t tile_len_option, bool use_bs)
{
    int64_t Lt = tile_len_option;
    if (Lt <= 0) Lt = use_bs ? ((total_len + 4095) / 4096 >= 8LL * W ? (total_len + 4095) / 4096
                                                                     : std::max<int64_t>(4LL * W, (total_len + 1535) / 1536))
                             : std::max<int64_t>(8LL * W, (total_len + 1023) / 1024);
    Lt = (Lt + 7) & ~7LL;
    return std::min<int64_t>(Lt, 0x7fffffff);
}

// The tile tables of the device stitch: tiles without halo, every event cut evenly.
struct DeviceTilePlan {
    bool too_many = false;                       // more tiles than a launch takes (nothing else is filled in): the host stitch takes the call
    std::vector<SpineJob> jobs;                  // one per tile, events in order
    std::vector<int64_t> ev_first_tile, boff;    // n_ev + 1 each: first tile of every event, first 8-sample block of every event (K0)
    int64_t list_entries = 0;                    // anchors the tiles' lists hold in all (the running sum of out_cap)
    int64_t total_len = 0, sample_end = 0;       // samples of the events; one past the last sample any event reads
    // one upload: [jobs | ev_first_tile | ev_start | ev_len | boff] -> one device blob the five arrays point into
    size_t jobs_bytes() const { return (jobs.size() * sizeof(SpineJob) + 15) & ~static_cast<size_t>(15); }
    static size_t table_bytes(int32_t n_ev) { return (static_cast<size_t>(n_ev) + 1) * sizeof(int64_t); }
    size_t up_bytes(int32_t n_ev) const { return jobs_bytes() + 4 * table_bytes(n_ev); }
    void stage(char *up, const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev) const
    {
        const size_t jb = jobs_bytes(), evb = table_bytes(n_ev);
        if (!jobs.empty()) std::memcpy(up, jobs.data(), jobs.size() * sizeof(SpineJob));
        std::memcpy(up + jb, ev_first_tile.data(), evb);
        if (n_ev) std::memcpy(up + jb + evb, ev_start, evb - sizeof(int64_t));
        if (n_ev) std::memcpy(up + jb + 2 * evb, ev_len, evb - sizeof(int64_t));
        std::memcpy(up + jb + 3 * evb, boff.data(), evb);
    }
};

inline DeviceTilePlan plan_device_tiles(const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, int mw, int W,
                                        int64_t tile_len_option, bool use_bs)
{
    DeviceTilePlan p;
    for (int e = 0; e < n_ev; ++e) { p.total_len += ev_len[e]; p.sample_end = std::max(p.sample_end, ev_start[e] + ev_len[e]); }
    const int64_t Lt = device_tile_len(p.total_len, W, tile_len_option, use_bs);
    p.ev_first_tile.assign(static_cast<size_t>(n_ev) + 1, 0);
    int64_t vb_run = 0;
    for (int e = 0; e < n_ev; ++e) {
        p.ev_first_tile[e] = static_cast<int64_t>(p.jobs.size());
        const int64_t len = ev_len[e];
        if (len == 0) continue;
        const int64_t vbase = vb_run;
        vb_run += len;
        // tiles of one event share one length: the event is cut evenly.  An event of up to 1.5 tile lengths stays ONE tile
        // (round 6: a 50k event with L = 40k used to be 2 x 25k -- two chains of three windows, a seam, a bridge and a stitch
        // entry for nothing: every event start is a true anchor.  BASELINE config 2, 1 024 x 50 000: 0.338-0.355 -> 0.309 ms
        // for a lone call, 2 048 -> 1 024 tiles, 15 459 -> 14 435 windows; profiles/r06_experiments/r6_config2_tile.txt)
        const int64_t nt0 = use_bs ? std::max<int64_t>(1, (len + Lt / 2) / Lt) : (len + Lt - 1) / Lt;
        const int64_t Le = std::min<int64_t>(((len + nt0 - 1) / nt0 + 7) & ~7LL, 0x7fffffff);
        const int64_t nt = (len + Le - 1) / Le;
        if (static_cast<int64_t>(p.jobs.size()) + nt > 0x7ffffff0) { DeviceTilePlan none; none.too_many = true; return none; }
        for (int64_t t = 0; t < nt; ++t) {
            p.jobs.push_back(make_spine_job(ev_start[e], e, len, t * Le, t == nt - 1 ? len : (t + 1) * Le, mw, p.list_entries,
                                            {p.ev_first_tile[e], nt, Le, vbase}));
            p.list_entries += p.jobs.back().out_cap;
        }
    }
    p.ev_first_tile[n_ev] = static_cast<int64_t>(p.jobs.size());
    p.boff.assign(static_cast<size_t>(n_ev) + 1, 0);
    for (int e = 0; e < n_ev; ++e) p.boff[e + 1] = p.boff[e] + (ev_len[e] + 7) / 8;
    return p;
}

// What a device tile plan was made for: a call that repeats the layout and the parameters reuses the plan and the tables that
// are still on the device.
struct DeviceTileKey {
    int32_t n_ev = 0;
    int mw = 0, W = 0;
    int64_t L = 0;
    bool use_bs = false;
    std::vector<int64_t> ev_start, ev_len;
    bool matches(const int64_t *s, const int64_t *l, int32_t n, int mw_, int W_, int64_t L_, bool use_bs_) const
    {
        return n_ev == n && mw == mw_ && W == W_ && L == L_ && use_bs == use_bs_ &&
               std::equal(s, s + n, ev_start.begin()) && std::equal(l, l + n, ev_len.begin());
    }
    void set(const int64_t *s, const int64_t *l, int32_t n, int mw_, int W_, int64_t L_, bool use_bs_)
    {
        n_ev = n; mw = mw_; W = W_; L = L_; use_bs = use_bs_;
        ev_start.assign(s, s + n);
        ev_len.assign(l, l + n);
    }
};

// The tiles of the host stitch: tile t of an event is [t L, min(len, (t + 1) L + H)), one tile when len <= L + H.
// Default: as many tiles as the chip keeps resident at once (2 workgroups of 512 threads per CU on 256 CUs) so the grid runs
// as a single wave of blocks, but never shorter than 8 windows (the halo is pure overhead).
struct HostTilePlan {
    int64_t L = 0, H = 0;                        // tile length and halo the plan was cut with
    std::vector<SpineJob> jobs;
    std::vector<int64_t> ev_first_tile;          // n_ev + 1
    int64_t scratch = 0;                         // anchors the tiles' lists hold in all
};

inline HostTilePlan plan_host_tiles(const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, int mw, int W,
                                    int64_t tile_len_option, int64_t halo_option)
{
    HostTilePlan p;
    int64_t total_len = 0;
    for (int e = 0; e < n_ev; ++e) total_len += ev_len[e];
    p.H = halo_option > 0 ? halo_option : 4LL * W;
    p.L = tile_len_option;
    if (p.L <= 0) {
        const int64_t resident = 512;
        p.L = std::max<int64_t>(8LL * W, (total_len + resident - 1) / resident);
    }
    p.ev_first_tile.assign(static_cast<size_t>(n_ev) + 1, 0);
    for (int e = 0; e < n_ev; ++e) {
        p.ev_first_tile[e] = static_cast<int64_t>(p.jobs.size());
        const int64_t len = ev_len[e];
        if (len == 0) continue;
        const int64_t nt = len <= p.L + p.H ? 1 : (len + p.L - 1) / p.L;
        for (int64_t t = 0; t < nt; ++t) {
            const int64_t stop = (t == nt - 1) ? len : std::min(len, (t + 1) * p.L + p.H);
            p.jobs.push_back(make_spine_job(ev_start[e], e, len, t * p.L, stop, mw, p.scratch));
            p.scratch += p.jobs.back().out_cap;
        }
    }
    p.ev_first_tile[n_ev] = static_cast<int64_t>(p.jobs.size());
    return p;
}

// ---- the host stitch: true spine per event ------------------------------------------------------------------------------------
// The subtree job of a true anchor of kind HIT / LATE: rec(prev, pos) of the event at `base`, its output at out_off
inline TreeJob make_tree_job(int64_t base, int32_t prev, int32_t pos, int mw, int W, int64_t out_off)
{
    TreeJob tj;
    tj.base = base;
    tj.start = prev;
    tj.end = pos;
    const int64_t d = static_cast<int64_t>(pos) - W - prev;
    tj.j0 = d < 0 ? 0 : static_cast<int32_t>(d / (W / 2)) + 1;
    tj.out_cap = (pos - prev) / mw + 1;
    tj.out_off = out_off;
    tj.m = 0; tj.pad_ = 0; tj.boff = 0;
    return tj;
}

enum StitchStatus : int { STITCH_OK = 0, STITCH_REPAIR_FAILED = 1, STITCH_NO_PROGRESS = 2 };
struct HostStitch {
    std::vector<Item> items;                     // the true anchors of every event, in order
    std::vector<TreeJob> tjobs;                  // one per anchor of kind HIT / LATE: the subtree to its left
    std::vector<int64_t> first_item;             // n_ev + 1
    int64_t tscratch = 0;                        // boundaries the subtree jobs may write in all
};

// Walks the tile lists of every event from its start: an anchor that a later tile's speculative list holds as well moves the
// walk to that tile (the latest one wins).  A list that stops short of its end without having met a later tile is continued
// from its last (true) anchor z -- "seam repair": repair(event, z, stop, &ext) runs the chain over [z, stop) into ext and says
// whether it could (false: STITCH_REPAIR_FAILED, the callable knows why); a repair that neither adds an anchor nor ends the
// event is STITCH_NO_PROGRESS.  `lists` are extended in place by the repairs.
template <class Repair>
StitchStatus stitch_lists(const HostTilePlan &plan, std::vector<TileList> &lists, const int64_t *ev_start, const int64_t *ev_len,
                          int32_t n_ev, int mw, int W, Repair &&repair, HostStitch *out)
{
    const int64_t L = plan.L, H = plan.H;
    out->items.clear();
    out->tjobs.clear();
    out->first_item.assign(static_cast<size_t>(n_ev) + 1, 0);
    out->tscratch = 0;
    for (int e = 0; e < n_ev; ++e) {
        out->first_item[e] = static_cast<int64_t>(out->items.size());
        const int64_t len = ev_len[e];
        const int64_t t0 = plan.ev_first_tile[e], t1 = plan.ev_first_tile[e + 1];
        if (t0 == t1) continue;
        int64_t cur = t0;
        size_t idx = 0;
        int32_t prev = 0;
        for (;;) {
            TileList &Lc = lists[cur];
            if (idx >= Lc.a.size()) {
                if (Lc.ended) break;
                const int32_t z = Lc.a.empty() ? Lc.start : Lc.a.back().pos;
                const int64_t stop = std::min<int64_t>(len, static_cast<int64_t>(z) + L + H);
                TileList ext;
                if (!repair(e, z, stop, &ext)) return STITCH_REPAIR_FAILED;
                Lc.a.insert(Lc.a.end(), ext.a.begin(), ext.a.end());
                Lc.ended = ext.ended;
                if (ext.a.empty() && !ext.ended) return STITCH_NO_PROGRESS;
                continue;
            }
            const Anchor an = Lc.a[idx];
            // emit this true anchor
            Item it;
            it.anchor = an.pos;
            it.job = -1;
            if (an.kind == KIND_HIT || an.kind == KIND_LATE) {
                it.job = static_cast<int32_t>(out->tjobs.size());
                out->tjobs.push_back(make_tree_job(ev_start[e], prev, an.pos, mw, W, out->tscratch));
                out->tscratch += out->tjobs.back().out_cap;
            }
            out->items.push_back(it);
            prev = an.pos;
            ++idx;
            // does a later tile's speculative spine contain this anchor?  (latest tile wins)
            if (cur + 1 < t1 && an.pos >= lists[cur + 1].start) {
                int64_t u = t0 + std::min<int64_t>(an.pos / L, t1 - t0 - 1);
                for (; u > cur; --u) {
                    const int f = find_in(lists[u], an.pos);
                    if (f != -2) { cur = u; idx = static_cast<size_t>(f + 1); break; }
                }
            }
        }
    }
    out->first_item[n_ev] = static_cast<int64_t>(out->items.size());
    return STITCH_OK;
}

// ---- the second chance of the device stitch ----------------------------------------------------------------------------------
// After a stitch that failed, from the bridges' (bmeta) and the tiles' (spine_meta) records -- any struct with int members
// x, y, z, w: bmeta = (anchors added, next window / join tile, join index, BR_* status), spine_meta = (anchors, ended, ..) --
// which seams the look-ahead kernel continues in the side buffer.
//   resume_deferred   the call issued no look-ahead launch and has not made up for it: if its bridges left seams deferred,
//                     they are counted (n_deferred) and nothing else is chosen -- the look-ahead kernel takes them all first
//   otherwise         on the true path: whatever failed there (a seam out of anchors, an open tile entered at its start);
//                     elsewhere: the seams that ran out of anchors (few; they may lie on the path once the first ones are
//                     mended).  hopeless: a seam on the true path that was extended before and still has not joined, or for
//                     which the side buffer has no slot left -- the host stitch takes the call.
// ext_stride: the side buffer's stride per seam, fixed by the first round that chooses (stride_set: it is fixed already) --
// few seams: long extensions; many (a batch of events): shorter ones.
struct SecondChance {
    int64_t n_deferred = 0;
    std::vector<int> list;
    bool hopeless = false;
    int ext_stride = EXT_MAX;
};

template <class Meta>
SecondChance pick_second_chance(const Meta *bmeta, const Meta *spine_meta, size_t nj, int bridge_budget, int slots_used,
                                bool stride_set, int ext_stride, bool resume_deferred)
{
    SecondChance sc;
    sc.ext_stride = ext_stride;
    if (resume_deferred) {
        for (size_t g = 0; g < nj; ++g) sc.n_deferred += bmeta[g].w == BR_DEFER || bmeta[g].w == BR_DEFER_REACHED;
        if (sc.n_deferred) return sc;
    }
    if (!stride_set) {
        size_t n_fail = 0;
        for (size_t g = 0; g < nj; ++g) n_fail += bmeta[g].w == BR_FAIL_REACHED || (bmeta[g].w == BR_FAIL && bmeta[g].x == bridge_budget);
        sc.ext_stride = n_fail <= static_cast<size_t>(EXT_SLOTS) ? EXT_MAX : EXT_MAX_MANY;
    }
    const int slot_cap = EXT_SLOTS * (EXT_MAX / sc.ext_stride);
    for (size_t g = 0; g < nj; ++g) {
        const bool reached = bmeta[g].w == BR_FAIL_REACHED;
        const bool gave_up = bmeta[g].x == bridge_budget;                     // (out of anchors in the first pass)
        if (!reached && !(bmeta[g].w == BR_FAIL && gave_up)) continue;
        const bool open_tile = spine_meta[g].x == 0 && bmeta[g].x == 0;
        if (!gave_up && !open_tile) { if (reached) sc.hopeless = true; continue; }   // (extended before and still not joined)
        if (slots_used + static_cast<int>(sc.list.size()) < slot_cap) sc.list.push_back(static_cast<int>(g));
        else if (reached) sc.hopeless = true;
    }
    return sc;
}

}  // namespace ps
