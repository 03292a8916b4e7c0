// Stand-alone check of pypore_amd/csrc/seg_plan.hpp (the host's planning of a segment call): host code only, no GPU, no HIP.
// tests/test_seg_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   seg_plan_check                                      every check below; exit status 0 when all hold
//   seg_plan_check tiles MW W TILE_LEN USE_BS LEN...    prints the tiles the device route plans for events of these lengths
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "seg_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

struct Layout { std::vector<int64_t> start, len; };
// events of these lengths one after the other, `gap` samples apart
static Layout layout_of(const std::vector<int64_t> &lens, int64_t gap = 0)
{
    Layout l;
    int64_t at = 0;
    for (int64_t n : lens) { l.start.push_back(at); l.len.push_back(n); at += n + gap; }
    return l;
}

// ---- device tile plan -----------------------------------------------------------------------------------------------------------
// Every property the kernels rely on, recomputed from the layout alone; returns the tiles per event.
static std::vector<int64_t> check_device_plan(const char *name, const Layout &l, int mw, int W, int64_t tile_len_option, bool use_bs)
{
    const int32_t n_ev = static_cast<int32_t>(l.len.size());
    const DeviceTilePlan p = plan_device_tiles(l.start.data(), l.len.data(), n_ev, mw, W, tile_len_option, use_bs);
    std::vector<int64_t> per_event(static_cast<size_t>(n_ev), 0);
    CHECK(!p.too_many, "%s", name);
    CHECK(p.ev_first_tile.size() == static_cast<size_t>(n_ev) + 1 && p.boff.size() == static_cast<size_t>(n_ev) + 1, "%s: table sizes", name);
    if (p.ev_first_tile.size() != static_cast<size_t>(n_ev) + 1 || p.boff.size() != static_cast<size_t>(n_ev) + 1) return per_event;
    int64_t total = 0, end = 0, vbase = 0, out_off = 0, blocks = 0;
    size_t g = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        const int64_t len = l.len[e];
        CHECK(p.ev_first_tile[e] == static_cast<int64_t>(g), "%s: event %d first tile %lld, expected %zu", name, e, static_cast<long long>(p.ev_first_tile[e]), g);
        CHECK(p.boff[e] == blocks, "%s: event %d first block %lld, expected %lld", name, e, static_cast<long long>(p.boff[e]), static_cast<long long>(blocks));
        blocks += (len + 7) / 8;
        total += len;
        if (l.start[e] + len > end) end = l.start[e] + len;
        const size_t first = g;
        int64_t at = 0;
        while (len > 0 && at < len && g < p.jobs.size() && p.jobs[g].ev == e) {
            const SpineJob &j = p.jobs[g];
            CHECK(j.start == at, "%s: event %d tile %zu starts at %d, the one before it stopped at %lld", name, e, g - first, j.start, static_cast<long long>(at));
            CHECK(j.start % 8 == 0, "%s: event %d tile %zu starts at %d", name, e, g - first, j.start);
            CHECK(j.stop > j.start && j.stop <= len, "%s: event %d tile %zu [%d, %d) of %lld", name, e, g - first, j.start, j.stop, static_cast<long long>(len));
            CHECK(j.base == l.start[e] && j.end == len, "%s: event %d tile %zu base %lld end %d", name, e, g - first, static_cast<long long>(j.base), j.end);
            CHECK(j.first_tile == static_cast<int32_t>(first), "%s: event %d tile %zu first_tile %d", name, e, g - first, j.first_tile);
            CHECK(j.tile_len == p.jobs[first].tile_len && j.tile_len % 8 == 0, "%s: event %d tile %zu tile_len %d", name, e, g - first, j.tile_len);
            CHECK(j.start == static_cast<int64_t>(g - first) * j.tile_len, "%s: event %d tile %zu starts at %d with tile_len %d", name, e, g - first, j.start, j.tile_len);
            CHECK(j.vbase == vbase, "%s: event %d vbase %lld, expected %lld", name, e, static_cast<long long>(j.vbase), static_cast<long long>(vbase));
            CHECK(j.out_cap == spine_cap(j.start, j.stop, mw), "%s: event %d tile %zu out_cap %d", name, e, g - first, j.out_cap);
            CHECK(j.out_off == out_off, "%s: event %d tile %zu out_off %lld, expected %lld", name, e, g - first, static_cast<long long>(j.out_off), static_cast<long long>(out_off));
            out_off += j.out_cap;
            at = j.stop;
            ++g;
        }
        CHECK(at == len, "%s: event %d is covered up to %lld of %lld", name, e, static_cast<long long>(at), static_cast<long long>(len));
        per_event[e] = static_cast<int64_t>(g - first);
        for (size_t t = first; t < g; ++t) CHECK(p.jobs[t].ntiles == static_cast<int32_t>(g - first), "%s: event %d ntiles %d, it has %zu", name, e, p.jobs[t].ntiles, g - first);
        if (len == 0) CHECK(g == first, "%s: empty event %d owns a tile", name, e);
        vbase += len;
    }
    CHECK(g == p.jobs.size() && p.ev_first_tile[n_ev] == static_cast<int64_t>(g), "%s: %zu tiles, %zu belong to events", name, p.jobs.size(), g);
    CHECK(p.boff[n_ev] == blocks, "%s: %lld blocks, expected %lld", name, static_cast<long long>(p.boff[n_ev]), static_cast<long long>(blocks));
    CHECK(p.list_entries == out_off && p.total_len == total && p.sample_end == end, "%s: list_entries %lld total_len %lld sample_end %lld", name,
          static_cast<long long>(p.list_entries), static_cast<long long>(p.total_len), static_cast<long long>(p.sample_end));
    // the upload blob: [jobs | ev_first_tile | ev_start | ev_len | boff], the jobs padded to 16 bytes
    const size_t jb = p.jobs_bytes(), evb = DeviceTilePlan::table_bytes(n_ev);
    CHECK(jb % 16 == 0 && jb >= p.jobs.size() * sizeof(SpineJob) && jb < p.jobs.size() * sizeof(SpineJob) + 16 && p.up_bytes(n_ev) == jb + 4 * evb, "%s: blob sizes", name);
    std::vector<char> up(p.up_bytes(n_ev) + 64, 0x5a);
    p.stage(up.data(), l.start.data(), l.len.data(), n_ev);
    CHECK(p.jobs.empty() || std::memcmp(up.data(), p.jobs.data(), p.jobs.size() * sizeof(SpineJob)) == 0, "%s: jobs in the blob", name);
    CHECK(std::memcmp(up.data() + jb, p.ev_first_tile.data(), evb) == 0 && std::memcmp(up.data() + jb + 3 * evb, p.boff.data(), evb) == 0, "%s: tables in the blob", name);
    CHECK(n_ev == 0 || (std::memcmp(up.data() + jb + evb, l.start.data(), evb - 8) == 0 && std::memcmp(up.data() + jb + 2 * evb, l.len.data(), evb - 8) == 0), "%s: events in the blob", name);
    for (size_t i = p.up_bytes(n_ev); i < up.size(); ++i) CHECK(up[i] == 0x5a, "%s: the blob is written beyond its size", name);
    return per_event;
}

static int64_t sum(const std::vector<int64_t> &v) { int64_t s = 0; for (int64_t x : v) s += x; return s; }

// The batch the GPU test runs as well (tests/test_seg_plan_gpu.py): W 64, min_width 8, tiles of 256 samples
static const std::vector<int64_t> MIXED = {0, 9, 383, 0, 0, 384, 385, 1, 7, 8, 0, 2000, 0};

static void device_plan_checks()
{
    const int mw = 8, W = 64;
    check_device_plan("no event", layout_of({}), mw, W, 0, true);
    for (int64_t n : {0, 1, 7, 8, 9}) {
        const std::string name = "one event of " + std::to_string(n);
        for (bool bs : {true, false}) {
            const std::vector<int64_t> t = check_device_plan(name.c_str(), layout_of({n}), mw, W, 0, bs);
            CHECK(t[0] == (n ? 1 : 0), "%s: %lld tiles", name.c_str(), static_cast<long long>(t[0]));
        }
    }
    // tile_len 256 on the block-sum route: an event of up to 1.5 tile lengths stays one tile -- (len + 128) / 256 is 1 at 383, 2 at 384
    CHECK(check_device_plan("383", layout_of({383}), mw, W, 256, true)[0] == 1, "383 samples: one tile");
    CHECK(check_device_plan("384", layout_of({384}), mw, W, 256, true)[0] == 2, "384 samples: two tiles");
    CHECK(check_device_plan("385", layout_of({385}), mw, W, 256, true)[0] == 2, "385 samples: two tiles");
    // (the LDS-window route cuts at every tile length)
    CHECK(check_device_plan("257, LDS-window route", layout_of({257}), mw, W, 256, false)[0] == 2, "257 samples: two tiles");
    CHECK(check_device_plan("256, LDS-window route", layout_of({256}), mw, W, 256, false)[0] == 1, "256 samples: one tile");
    const std::vector<int64_t> mixed = check_device_plan("mixed batch", layout_of(MIXED, 3), mw, W, 256, true);
    const std::vector<int64_t> want = {0, 1, 1, 0, 0, 2, 2, 1, 1, 1, 0, 8, 0};
    CHECK(mixed == want, "mixed batch: tiles per event");
    check_device_plan("mixed batch, LDS-window route", layout_of(MIXED), mw, W, 256, false);
    check_device_plan("mixed batch, default tile length", layout_of(MIXED), mw, W, 0, true);
    // an explicit tile length that is no multiple of 8 is rounded up to one: 250 -> 256
    CHECK(device_tile_len(1000, W, 250, true) == 256, "tile_len 250 -> %lld", static_cast<long long>(device_tile_len(1000, W, 250, true)));
    CHECK(check_device_plan("tile_len 250", layout_of({1000, 0, 333}), mw, W, 250, true) == (std::vector<int64_t>{4, 0, 1}), "tile_len 250: tiles per event");
    // the two shapes the documents quote: min_width 100, W 10 000, default tile length
    CHECK(sum(check_device_plan("1e8 samples", layout_of({100000000}), 100, 10000, 0, true)) == 1536, "one event of 1e8 samples: 1 536 tiles");
    CHECK(sum(check_device_plan("1024 x 50000", layout_of(std::vector<int64_t>(1024, 50000)), 100, 10000, 0, true)) == 1024, "1 024 events of 50 000 samples: 1 024 tiles");
    // the length rule: 4 096 tiles when they stay >= 8 W, else 1 536 tiles of at least 4 W; the LDS-window route 1 024 of at least 8 W
    CHECK(device_tile_len(4096LL * 8 * W, W, 0, true) == 8 * W, "4 096 tiles of 8 W");
    CHECK(device_tile_len(4096LL * 8 * W - 4096, W, 0, true) == ((4096LL * 8 * W - 4096 + 1535) / 1536 + 7) / 8 * 8, "just below: 1 536 tiles");
    CHECK(device_tile_len(1000, W, 0, true) == 4 * W && device_tile_len(1000, W, 0, false) == 8 * W, "short calls: 4 W, 8 W");
    // the key a plan is reused under
    const Layout a = layout_of(MIXED), b = layout_of(MIXED, 1);
    const int32_t n = static_cast<int32_t>(MIXED.size());
    DeviceTileKey key;
    key.set(a.start.data(), a.len.data(), n, mw, W, 256, true);
    CHECK(key.matches(a.start.data(), a.len.data(), n, mw, W, 256, true), "the same call");
    CHECK(!key.matches(b.start.data(), a.len.data(), n, mw, W, 256, true) && !key.matches(a.start.data(), a.len.data(), n - 1, mw, W, 256, true) &&
          !key.matches(a.start.data(), a.len.data(), n, mw + 1, W, 256, true) && !key.matches(a.start.data(), a.len.data(), n, mw, W + 1, 256, true) &&
          !key.matches(a.start.data(), a.len.data(), n, mw, W, 0, true) && !key.matches(a.start.data(), a.len.data(), n, mw, W, 256, false), "another call");
}

// ---- host tile plan -------------------------------------------------------------------------------------------------------------
static std::vector<int64_t> check_host_plan(const char *name, const Layout &l, int mw, int W, int64_t tile_len_option, int64_t halo_option, int64_t L, int64_t H)
{
    const int32_t n_ev = static_cast<int32_t>(l.len.size());
    const HostTilePlan p = plan_host_tiles(l.start.data(), l.len.data(), n_ev, mw, W, tile_len_option, halo_option);
    std::vector<int64_t> per_event(static_cast<size_t>(n_ev), 0);
    CHECK(p.L == L && p.H == H, "%s: L %lld H %lld", name, static_cast<long long>(p.L), static_cast<long long>(p.H));
    CHECK(p.ev_first_tile.size() == static_cast<size_t>(n_ev) + 1, "%s: table size", name);
    if (p.ev_first_tile.size() != static_cast<size_t>(n_ev) + 1) return per_event;
    size_t g = 0;
    int64_t scratch = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        const int64_t len = l.len[e];
        CHECK(p.ev_first_tile[e] == static_cast<int64_t>(g), "%s: event %d first tile", name, e);
        const size_t first = g;
        const int64_t nt = len == 0 ? 0 : len <= L + H ? 1 : (len + L - 1) / L;
        for (int64_t t = 0; t < nt && g < p.jobs.size(); ++t, ++g) {
            const SpineJob &j = p.jobs[g];
            const int64_t stop = t == nt - 1 ? len : std::min<int64_t>(len, (t + 1) * L + H);
            CHECK(j.ev == e && j.base == l.start[e] && j.end == len, "%s: event %d tile %lld", name, e, static_cast<long long>(t));
            CHECK(j.start == t * L && j.stop == stop, "%s: event %d tile %lld is [%d, %d), expected [%lld, %lld)", name, e, static_cast<long long>(t), j.start, j.stop,
                  static_cast<long long>(t * L), static_cast<long long>(stop));
            // the halo: a tile reaches at least to the start of the next one -- no gap
            if (t + 1 < nt) CHECK(j.stop >= (t + 1) * L && j.stop > j.start, "%s: event %d tile %lld stops at %d", name, e, static_cast<long long>(t), j.stop);
            CHECK(j.out_cap == spine_cap(j.start, j.stop, mw) && j.out_off == scratch, "%s: event %d tile %lld out_cap %d out_off %lld", name, e, static_cast<long long>(t), j.out_cap, static_cast<long long>(j.out_off));
            scratch += j.out_cap;
        }
        if (nt) CHECK(g > first && p.jobs[g - 1].stop == len && p.jobs[first].start == 0, "%s: event %d is not covered", name, e);
        per_event[e] = static_cast<int64_t>(g - first);
    }
    CHECK(g == p.jobs.size() && p.ev_first_tile[n_ev] == static_cast<int64_t>(g) && p.scratch == scratch, "%s: %zu tiles, scratch %lld", name, p.jobs.size(), static_cast<long long>(p.scratch));
    return per_event;
}

static void host_plan_checks()
{
    const int mw = 8, W = 64;
    check_host_plan("no event", layout_of({}), mw, W, 256, 64, 256, 64);
    // on both sides of len == L + H
    CHECK(check_host_plan("L + H - 1", layout_of({319}), mw, W, 256, 64, 256, 64)[0] == 1, "319 samples: one tile");
    CHECK(check_host_plan("L + H", layout_of({320}), mw, W, 256, 64, 256, 64)[0] == 1, "320 samples: one tile");
    CHECK(check_host_plan("L + H + 1", layout_of({321}), mw, W, 256, 64, 256, 64)[0] == 2, "321 samples: two tiles");
    CHECK(check_host_plan("mixed batch", layout_of(MIXED, 5), mw, W, 256, 64, 256, 64) == (std::vector<int64_t>{0, 1, 2, 0, 0, 2, 2, 1, 1, 1, 0, 8, 0}), "mixed batch: tiles per event");
    // the defaults: halo 4 W; 512 tiles, none shorter than 8 W
    check_host_plan("default tiling, short", layout_of({5000, 0, 300}), mw, W, 0, 0, 8 * W, 4 * W);
    check_host_plan("default tiling, long", layout_of({700000, 324001}), mw, W, 0, 0, 2001, 4 * W);
}

// ---- host stitch ----------------------------------------------------------------------------------------------------------------
// A deterministic "next anchor" function per event: from position p the chain goes to p + gap[p] (>= mw further), the anchor there
// has kind[p + gap[p]]; a step that leaves the event ends the chain.
struct Chain {
    std::vector<int32_t> gap, kind;
    Chain(int64_t len, int mw, int spread, unsigned seed) : gap(static_cast<size_t>(len)), kind(static_cast<size_t>(len))
    {
        unsigned s = seed * 2654435761u + 12345u;
        const int kinds[4] = {KIND_HIT, KIND_EARLY, KIND_LATE, KIND_HIT};
        for (size_t p = 0; p < gap.size(); ++p) {
            s = s * 1664525u + 1013904223u;
            gap[p] = mw + static_cast<int32_t>((s >> 16) % static_cast<unsigned>(spread));
            kind[p] = kinds[(s >> 8) & 3];
        }
    }
    // the list of a chain started at `start` that stops behind its first anchor >= stop
    TileList run(int32_t start, int64_t stop) const
    {
        TileList t;
        t.start = start;
        int64_t p = start;
        for (;;) {
            const int64_t q = p + gap[static_cast<size_t>(p)];
            if (q >= static_cast<int64_t>(gap.size())) { t.ended = true; break; }
            t.a.push_back({static_cast<int32_t>(q), kind[static_cast<size_t>(q)]});
            if (q >= stop) break;
            p = q;
        }
        return t;
    }
};

struct StitchCase {
    Layout l;
    std::vector<Chain> chains;
    HostTilePlan plan;
    std::vector<TileList> lists;
    int mw, W;
};

static StitchCase stitch_case(const std::vector<int64_t> &lens, int mw, int W, int64_t L, int64_t H, int spread, unsigned seed)
{
    StitchCase c;
    c.l = layout_of(lens, 11);
    c.mw = mw;
    c.W = W;
    for (size_t e = 0; e < lens.size(); ++e) c.chains.emplace_back(lens[e], mw, spread, seed + static_cast<unsigned>(e));
    c.plan = plan_host_tiles(c.l.start.data(), c.l.len.data(), static_cast<int32_t>(lens.size()), mw, W, L, H);
    return c;
}
static void run_tiles(StitchCase &c)
{
    c.lists.clear();
    for (const SpineJob &j : c.plan.jobs) c.lists.push_back(c.chains[static_cast<size_t>(j.ev)].run(j.start, j.stop));
}

// stitch_lists must give exactly the iterates from 0 of every event, a subtree job for each of kind HIT / LATE; returns the repairs
static int check_stitch(const char *name, StitchCase &c)
{
    const int32_t n_ev = static_cast<int32_t>(c.l.len.size());
    int repairs = 0;
    auto repair = [&](int32_t e, int32_t z, int64_t stop, TileList *ext) {
        ++repairs;
        CHECK(stop <= c.l.len[e] && stop > z, "%s: repair of event %d over [%d, %lld)", name, e, z, static_cast<long long>(stop));
        *ext = c.chains[static_cast<size_t>(e)].run(z, stop);
        return true;
    };
    HostStitch st;
    const StitchStatus status = stitch_lists(c.plan, c.lists, c.l.start.data(), c.l.len.data(), n_ev, c.mw, c.W, repair, &st);
    CHECK(status == STITCH_OK, "%s: status %d", name, static_cast<int>(status));
    CHECK(st.first_item.size() == static_cast<size_t>(n_ev) + 1, "%s: first_item", name);
    if (status != STITCH_OK || st.first_item.size() != static_cast<size_t>(n_ev) + 1) return repairs;
    size_t i = 0, k = 0;
    int64_t tscratch = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        CHECK(st.first_item[e] == static_cast<int64_t>(i), "%s: event %d first item %lld, expected %zu", name, e, static_cast<long long>(st.first_item[e]), i);
        if (c.l.len[e] == 0) continue;
        const TileList all = c.chains[static_cast<size_t>(e)].run(0, c.l.len[e]);       // the iterates from 0
        int32_t prev = 0;
        for (const Anchor &an : all.a) {
            CHECK(i < st.items.size() && st.items[i].anchor == an.pos, "%s: event %d item %zu is %d, expected %d", name, e, i, i < st.items.size() ? st.items[i].anchor : -1, an.pos);
            if (i >= st.items.size()) return repairs;
            if (an.kind == KIND_HIT || an.kind == KIND_LATE) {
                CHECK(st.items[i].job == static_cast<int32_t>(k) && k < st.tjobs.size(), "%s: event %d item %zu job %d, expected %zu", name, e, i, st.items[i].job, k);
                if (k >= st.tjobs.size()) return repairs;
                const TreeJob &tj = st.tjobs[k];
                const int64_t d = static_cast<int64_t>(an.pos) - c.W - prev;
                const int32_t j0 = d < 0 ? 0 : static_cast<int32_t>(d / (c.W / 2)) + 1;
                CHECK(tj.base == c.l.start[e] && tj.start == prev && tj.end == an.pos, "%s: job %zu is [%d, %d), expected [%d, %d)", name, k, tj.start, tj.end, prev, an.pos);
                CHECK(tj.j0 == j0 && tj.out_cap == (an.pos - prev) / c.mw + 1 && tj.out_off == tscratch, "%s: job %zu j0 %d out_cap %d out_off %lld", name, k, tj.j0, tj.out_cap, static_cast<long long>(tj.out_off));
                CHECK(tj.m == 0 && tj.pad_ == 0 && tj.boff == 0, "%s: job %zu digest fields", name, k);
                tscratch += tj.out_cap;
                ++k;
            } else {
                CHECK(st.items[i].job == -1, "%s: event %d item %zu of kind %d has job %d", name, e, i, an.kind, st.items[i].job);
            }
            prev = an.pos;
            ++i;
        }
    }
    CHECK(i == st.items.size() && k == st.tjobs.size() && st.first_item[n_ev] == static_cast<int64_t>(i) && st.tscratch == tscratch,
          "%s: %zu items (expected %zu), %zu jobs (expected %zu), tscratch %lld", name, st.items.size(), i, st.tjobs.size(), k, static_cast<long long>(st.tscratch));
    return repairs;
}

static void stitch_checks()
{
    const int mw = 8, W = 64;
    // seeded chains: a single tile, empty events, many tiles; gaps of 8 .. 23 samples make the tiles' chains meet within the halo
    for (unsigned seed = 1; seed <= 20; ++seed) {
        StitchCase c = stitch_case({0, 100, 0, 0, 3000, 320, 321, 0}, mw, W, 256, 64, 16, seed);
        run_tiles(c);
        const std::string name = "seeded chains " + std::to_string(seed);
        check_stitch(name.c_str(), c);
        // ... and gaps of 8 .. 207: anchors more than W apart (first windows j0 > 0), chains that often miss each other (repairs)
        StitchCase far = stitch_case({0, 100, 0, 0, 3000, 320, 321, 0}, mw, W, 256, 64, 200, seed);
        run_tiles(far);
        check_stitch((name + ", far apart").c_str(), far);
    }
    {
        // one anchor exactly at a later tile's start: steps of 16 from 0 reach 256, where tile 1 begins -- find_in says -1
        StitchCase c = stitch_case({1500}, mw, W, 256, 64, 16, 77);
        for (int p = 0; p <= 256; ++p) c.chains[0].gap[static_cast<size_t>(p)] = 16;
        run_tiles(c);
        CHECK(c.lists.size() == 6 && find_in(c.lists[1], 256) == -1 && find_in(c.lists[0], 256) == 15 && find_in(c.lists[0], 250) == -2, "anchor at a tile's start");
        check_stitch("anchor at a tile's start", c);
    }
    // Two lattices that do not meet: steps of 16 everywhere, the chain from 0 starts with a step of 24 (anchors = 8 mod 16), every
    // tile's own chain walks on multiples of 16.  Tile 0's list stops behind 320 without having met tile 1's: a repair continues
    // it.  From 808 a step of 24 puts the true chain on the tiles' lattice: the walk moves to tile 3's list and needs no more repairs.
    auto lattices = [&]() {
        StitchCase c = stitch_case({0, 2000, 40}, mw, W, 256, 64, 16, 5);
        for (int32_t &g : c.chains[1].gap) g = 16;
        c.chains[1].gap[0] = 24;
        c.chains[1].gap[808] = 24;
        run_tiles(c);
        return c;
    };
    {
        StitchCase c = lattices();
        CHECK(c.lists[0].a.back().pos == 328 && !c.lists[0].ended && find_in(c.lists[1], 328) == -2, "two lattices: tile 0 stops at %d", c.lists[0].a.back().pos);
        const int repairs = check_stitch("two lattices", c);
        CHECK(repairs == 2, "two lattices: %d repairs (expected [328, 648) and [648, 968))", repairs);
    }
    {
        // a repair that adds nothing and does not end the event; one that could not run
        StitchCase c = lattices();
        HostStitch st;
        auto nothing = [](int32_t, int32_t, int64_t, TileList *ext) { *ext = TileList(); return true; };
        CHECK(stitch_lists(c.plan, c.lists, c.l.start.data(), c.l.len.data(), 3, mw, W, nothing, &st) == STITCH_NO_PROGRESS, "a repair without progress");
        c = lattices();
        auto broken = [](int32_t, int32_t, int64_t, TileList *) { return false; };
        CHECK(stitch_lists(c.plan, c.lists, c.l.start.data(), c.l.len.data(), 3, mw, W, broken, &st) == STITCH_REPAIR_FAILED, "a repair that failed");
        // ... and one that only ends the event is progress
        c = lattices();
        auto ends = [](int32_t, int32_t, int64_t, TileList *ext) { *ext = TileList(); ext->ended = true; return true; };
        CHECK(stitch_lists(c.plan, c.lists, c.l.start.data(), c.l.len.data(), 3, mw, W, ends, &st) == STITCH_OK && st.first_item[2] == 20, "a repair that ends the event");
    }
}

// ---- second-chance pick ---------------------------------------------------------------------------------------------------------
struct M4 { int x, y, z, w; };

static void second_chance_checks()
{
    const int B = BR_MAX;
    const M4 some = {5, 0, 0, 0};                // a tile with anchors of its own
    const M4 open = {0, 0, 7, 0};                // an open tile: no anchor yet
    {
        // deferred seams are counted and nothing else is chosen
        const std::vector<M4> bm = {{3, 9, 0, BR_DEFER}, {B, 0, 0, BR_FAIL_REACHED}, {0, 2, 0, BR_DEFER_REACHED}, {1, 2, 3, BR_JOINED}, {B, 0, 0, BR_FAIL}};
        const std::vector<M4> mt(bm.size(), some);
        SecondChance sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, false, EXT_MAX, true);
        CHECK(sc.n_deferred == 2 && sc.list.empty() && !sc.hopeless && sc.ext_stride == EXT_MAX, "deferred seams: %lld counted, %zu chosen", static_cast<long long>(sc.n_deferred), sc.list.size());
        // ... unless the look-ahead kernel has had them already
        sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, false, EXT_MAX, false);
        CHECK(sc.n_deferred == 0 && sc.list == (std::vector<int>{1, 4}) && !sc.hopeless && sc.ext_stride == EXT_MAX, "no deferral: seams 1 and 4");
    }
    {
        // seams that gave up with x == bridge_budget, on the true path or not; with a lowered budget
        const std::vector<M4> bm = {{B, 0, 0, BR_FAIL}, {5, 0, 0, BR_FAIL}, {B, 0, 0, BR_FAIL_REACHED}, {B, 1, 2, BR_JOINED}, {B, 0, 0, BR_ENDED}, {10, 0, 0, BR_FAIL}, {0, 0, 0, BR_NONE}};
        const std::vector<M4> mt(bm.size(), some);
        SecondChance sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, false, EXT_MAX, true);
        CHECK(sc.n_deferred == 0 && sc.list == (std::vector<int>{0, 2}) && !sc.hopeless, "gave up at the budget: seams 0 and 2");
        sc = pick_second_chance(bm.data(), mt.data(), bm.size(), 10, 0, false, EXT_MAX, false);
        CHECK(sc.list == (std::vector<int>{5}) && sc.hopeless, "budget 10: seam 5; seam 2, on the path, went beyond it");
    }
    {
        // an open tile entered at its start; a seam extended once that still failed on the true path, and one off it
        const std::vector<M4> bm = {{0, 0, 0, BR_FAIL_REACHED}, {0, 0, 0, BR_FAIL_REACHED}, {0, 0, 0, BR_FAIL}};
        const std::vector<M4> mt = {open, some, open};
        SecondChance sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, false, EXT_MAX, false);
        CHECK(sc.list == (std::vector<int>{0}) && sc.hopeless, "open tile 0 chosen; tile 1 has anchors and no bridge: hopeless");
        sc = pick_second_chance(bm.data(), mt.data(), 1, B, 0, false, EXT_MAX, false);
        CHECK(sc.list == (std::vector<int>{0}) && !sc.hopeless, "open tile entered at its start");
        const std::vector<M4> ext = {{B + 100, 0, 0, BR_FAIL_REACHED}}, ext_off = {{B + 100, 0, 0, BR_FAIL}};
        sc = pick_second_chance(ext.data(), mt.data() + 1, 1, B, 1, true, EXT_MAX, false);
        CHECK(sc.list.empty() && sc.hopeless, "extended before, on the path: hopeless");
        sc = pick_second_chance(ext_off.data(), mt.data() + 1, 1, B, 1, true, EXT_MAX, false);
        CHECK(sc.list.empty() && !sc.hopeless, "extended before, off the path: left alone");
    }
    for (int n : {EXT_SLOTS, EXT_SLOTS + 1}) {
        // the stride: long extensions for up to EXT_SLOTS seams, shorter ones for more -- fixed by the first round that chooses
        std::vector<M4> bm(static_cast<size_t>(n), M4{B, 0, 0, BR_FAIL});
        bm[3].w = BR_FAIL_REACHED;
        bm.push_back({7, 0, 0, BR_FAIL});                 // (not at the budget: does not count)
        const std::vector<M4> mt(bm.size(), some);
        SecondChance sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, false, EXT_MAX, false);
        CHECK(sc.ext_stride == (n <= EXT_SLOTS ? EXT_MAX : EXT_MAX_MANY) && sc.list.size() == static_cast<size_t>(n) && !sc.hopeless, "%d seams: stride %d, %zu chosen", n, sc.ext_stride, sc.list.size());
        sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, true, EXT_MAX_MANY, false);
        CHECK(sc.ext_stride == EXT_MAX_MANY && sc.list.size() == static_cast<size_t>(n), "%d seams, stride fixed at %d", n, EXT_MAX_MANY);
        // fixed at the long stride, EXT_SLOTS slots in all: the seam beyond them waits, off the path ...
        sc = pick_second_chance(bm.data(), mt.data(), bm.size(), B, 0, true, EXT_MAX, false);
        CHECK(sc.ext_stride == EXT_MAX && sc.list.size() == static_cast<size_t>(EXT_SLOTS) && !sc.hopeless, "%d seams, stride fixed at %d: %zu chosen", n, EXT_MAX, sc.list.size());
    }
    {
        // the slot cap: one slot left, two seams want it
        const std::vector<M4> off = {{B, 0, 0, BR_FAIL}, {B, 0, 0, BR_FAIL}}, on = {{B, 0, 0, BR_FAIL}, {B, 0, 0, BR_FAIL_REACHED}};
        const std::vector<M4> mt(2, some);
        SecondChance sc = pick_second_chance(off.data(), mt.data(), 2, B, EXT_SLOTS - 1, true, EXT_MAX, false);
        CHECK(sc.list == (std::vector<int>{0}) && !sc.hopeless, "no slot for a seam off the path: skipped");
        sc = pick_second_chance(on.data(), mt.data(), 2, B, EXT_SLOTS - 1, true, EXT_MAX, false);
        CHECK(sc.list == (std::vector<int>{0}) && sc.hopeless, "no slot for a seam on the path: hopeless");
        sc = pick_second_chance(on.data(), mt.data(), 2, B, EXT_SLOTS * (EXT_MAX / EXT_MAX_MANY) - 2, true, EXT_MAX_MANY, false);
        CHECK(sc.list == (std::vector<int>{0, 1}) && !sc.hopeless, "the short stride has eight times the slots");
    }
}

// ---- route ------------------------------------------------------------------------------------------------------------------------
static void route_checks()
{
    CHECK(!scan_route_bs(true, 7, 1000, false, false) && scan_route_bs(true, 8, 1000, false, false), "min_width 7 / 8");
    CHECK(scan_route_bs(true, 8, 64512, false, false) && !scan_route_bs(true, 8, 64513, false, false), "W 64 512 / 64 513");
    CHECK(!scan_route_bs(false, 8, 1000, false, false) && !scan_route_bs(true, 8, 1000, true, false) && !scan_route_bs(true, 8, 1000, false, true), "option, exact mode, float64 input");
    const double q = 0.25, q2 = 0.5;
    {
        // narrow -> wide, remembered for 16 calls on that grid
        WideRedo w;
        CHECK(w.begin(true, q) == 1 && w.redo == 0, "a first call starts on the 32-bit digest");
        CHECK(w.refused(true, q) == 2 && w.redo == 1 && w.remembers(q) && !w.remembers(q2), "refused: the 64-bit digest");
        CHECK(w.begin(true, q2) == 1 && w.redo == 0 && w.skip == WIDE_MEMORY, "another quantum starts narrow and uses up nothing");
        CHECK(w.begin(false, q) == 0 && w.redo == 0 && w.skip == WIDE_MEMORY, "a call off the block-sum route uses up nothing");
        for (int i = 0; i < WIDE_MEMORY; ++i) CHECK(w.begin(true, q) == 2 && w.redo == 1 && w.skip == WIDE_MEMORY - 1 - i, "call %d after the refusal starts wide", i + 1);
        CHECK(!w.remembers(q) && w.begin(true, q) == 1 && w.redo == 0, "the call after those starts narrow again");
    }
    {
        // narrow -> wide -> LDS-window
        WideRedo w;
        w.begin(true, q);
        CHECK(w.refused(true, q) == 2 && w.refused(true, q) == 0 && w.redo == 2 && w.mode == 0 && w.skip == WIDE_MEMORY, "refused twice: the LDS-window scan");
        CHECK(w.begin(true, q) == 0 && w.redo == 2 && w.skip == WIDE_MEMORY - 1, "the next call starts there");
        CHECK(w.refused(true, q) == 0, "(nothing beyond it)");
        w.forget();
        CHECK(w.begin(true, q) == 1 && w.redo == 0, "forgotten: narrow again");
    }
    {
        // option wide_bs off: straight to the LDS-window scan
        WideRedo w;
        w.begin(true, q);
        CHECK(w.refused(false, q) == 0 && w.redo == 2 && w.begin(true, q) == 0 && w.redo == 2, "wide_bs off");
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "tiles") == 0) {
        if (argc < 6) { std::fprintf(stderr, "usage: seg_plan_check tiles MW W TILE_LEN USE_BS LEN...\n"); return 2; }
        std::vector<int64_t> lens;
        for (int i = 6; i < argc; ++i) lens.push_back(std::atoll(argv[i]));
        const Layout l = layout_of(lens);
        const DeviceTilePlan p = plan_device_tiles(l.start.data(), l.len.data(), static_cast<int32_t>(lens.size()), std::atoi(argv[2]), std::atoi(argv[3]),
                                                   std::atoll(argv[4]), std::atoi(argv[5]) != 0);
        std::printf("%zu\n", p.jobs.size());
        return 0;
    }
    device_plan_checks();
    host_plan_checks();
    stitch_checks();
    second_chance_checks();
    route_checks();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("seg plan ok\n");
    return failures ? 1 : 0;
}
