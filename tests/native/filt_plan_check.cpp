// Stand-alone check of pypore_amd/csrc/filt_plan.hpp (the host's planning of a batched Bessel filter call): host code only, no
// GPU, no HIP.  tests/test_filter_batch_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   filt_plan_check                          every check below; exit status 0 when all hold
//   filt_plan_check route ALPHA FUSED        prints "H T" of the order-1 route for the pole ALPHA (H = 0: the scan route)
//   filt_plan_check units PAD UNIT LEN...    prints the units the plan gives events of these lengths, one number per event
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "filt_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

struct Layout { std::vector<int64_t> start, len; };
// events of these lengths; starts that overlap, touch and descend do not matter to the plan, so they are made to
static Layout layout_of(const std::vector<int64_t> &lens)
{
    Layout l;
    int64_t at = 1000003;
    for (size_t k = 0; k < lens.size(); ++k) { l.start.push_back(at); l.len.push_back(lens[k]); at = at > lens[k] / 2 ? at - lens[k] / 2 : at + 7; }
    return l;
}

// Every property the kernels rely on, recomputed from the lengths alone; returns the units per event.
static std::vector<int64_t> check_plan(const char *name, const Layout &l, int pad, int64_t unit, int64_t row_bytes, int64_t cap)
{
    const int32_t n_ev = static_cast<int32_t>(l.len.size());
    std::vector<int64_t> per_event(static_cast<size_t>(n_ev), 0);
    FiltPlan p;
    const FiltPlanError err = plan_filter_batch(l.start.data(), l.len.data(), n_ev, pad, unit, row_bytes, cap, &p);
    CHECK(err == FILT_PLAN_OK, "%s: error %d", name, static_cast<int>(err));
    if (err != FILT_PLAN_OK) return per_event;
    CHECK(p.ev.size() == static_cast<size_t>(n_ev), "%s: %zu event records", name, p.ev.size());
    int64_t u = 0, off = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        const int64_t m = l.len[e] + 2 * pad;
        const FiltEvent &r = p.ev[e];
        CHECK(r.start == l.start[e] && r.n == l.len[e], "%s: event %d range", name, e);
        CHECK(r.out_off == off, "%s: event %d output at %lld, expected %lld", name, e, static_cast<long long>(r.out_off), static_cast<long long>(off));
        CHECK(r.unit0 == u, "%s: event %d first unit %lld, expected %lld", name, e, static_cast<long long>(r.unit0), static_cast<long long>(u));
        // the units of the event, in order: [idx * unit, (idx + 1) * unit) cut to [0, m) -- exactly once, no gap, none empty
        int64_t covered = 0, k = 0;
        while (static_cast<size_t>(u + k) < p.unit.size() && p.unit[u + k].ev == e) {
            CHECK(p.unit[u + k].idx == k, "%s: event %d unit %lld has index %d", name, e, static_cast<long long>(k), p.unit[u + k].idx);
            const int64_t lo = k * unit, hi = lo + unit < m ? lo + unit : m;
            CHECK(lo == covered && hi > lo, "%s: event %d unit %lld covers [%lld, %lld)", name, e, static_cast<long long>(k), static_cast<long long>(lo),
                  static_cast<long long>(hi));
            covered = hi;
            ++k;
        }
        CHECK(covered == m, "%s: event %d covered to %lld of %lld", name, e, static_cast<long long>(covered), static_cast<long long>(m));
        CHECK(k == (m + unit - 1) / unit, "%s: event %d has %lld units", name, e, static_cast<long long>(k));
        per_event[e] = k;
        u += k; off += l.len[e];
    }
    CHECK(static_cast<size_t>(u) == p.unit.size(), "%s: %zu table entries for %lld units", name, p.unit.size(), static_cast<long long>(u));
    CHECK(p.total_len == off, "%s: total length", name);
    // the groups: in order, every event in exactly one, their units the events' units, each within the cap unless it is one event
    int32_t next_ev = 0;
    int64_t next_unit = 0;
    for (size_t g = 0; g < p.group.size(); ++g) {
        const FiltGroup &G = p.group[g];
        CHECK(G.ev0 == next_ev && G.ev1 > G.ev0 && G.ev1 <= n_ev, "%s: group %zu holds events [%d, %d)", name, g, G.ev0, G.ev1);
        CHECK(G.unit0 == next_unit, "%s: group %zu first unit", name, g);
        int64_t units = 0;
        for (int32_t e = G.ev0; e < G.ev1 && e < n_ev; ++e) units += per_event[e];
        CHECK(G.units == units, "%s: group %zu has %lld units, its events %lld", name, g, static_cast<long long>(G.units), static_cast<long long>(units));
        if (row_bytes > 0) {
            CHECK(G.units * row_bytes <= cap || G.ev1 - G.ev0 == 1, "%s: group %zu of %d events takes %lld bytes", name, g, G.ev1 - G.ev0,
                  static_cast<long long>(G.units * row_bytes));
            // (greedy: the next event would not have fitted)
            if (G.ev1 < n_ev) CHECK((G.units + per_event[G.ev1]) * row_bytes > cap, "%s: group %zu closed early", name, g);
        }
        next_ev = G.ev1; next_unit += G.units;
    }
    CHECK(next_ev == n_ev && next_unit == u, "%s: groups end at event %d", name, next_ev);
    if (row_bytes == 0) CHECK(p.group.size() == (n_ev ? 1u : 0u), "%s: %zu groups without scratch", name, p.group.size());
    return per_event;
}

static void check_refusal(const char *name, const Layout &l, int pad, FiltPlanError want, int want_event)
{
    FiltPlan p;
    const FiltPlanError err = plan_filter_batch(l.start.data(), l.len.data(), static_cast<int32_t>(l.len.size()), pad, 3328, 0, 0, &p);
    CHECK(err == want && p.bad_event == want_event, "%s: error %d names event %d", name, static_cast<int>(err), p.bad_event);
    CHECK(p.ev.empty() && p.unit.empty() && p.group.empty(), "%s: tables of a refused batch", name);
}

static void check_requant(const std::vector<int64_t> &lens)
{
    RequantPlan p;
    plan_requant_batch(lens.data(), static_cast<int32_t>(lens.size()), &p);
    int64_t off = 0, poff = 0;
    size_t u = 0;
    for (size_t e = 0; e < lens.size(); ++e) {
        int64_t g = (lens[e] + 2047) / 2048;
        if (g > 1024) g = 1024;
        CHECK(p.ev[e].off == off && p.ev[e].n == lens[e] && p.ev[e].poff == poff && p.ev[e].grid == g, "requant event %zu", e);
        for (int64_t i = 0; i < g; ++i, ++u)
            CHECK(u < p.unit.size() && p.unit[u].ev == static_cast<int32_t>(e) && p.unit[u].idx == i, "requant unit %zu", u);
        off += lens[e]; poff += g;
    }
    CHECK(u == p.unit.size(), "requant: %zu units", p.unit.size());
}

static int run_checks()
{
    const int64_t T = 3328;                              // (any tile: the route's own values come from the `route` mode)
    // unit counts around the tile: n + 12 = T - 1, T, T + 1, 2 T, 2 T + 1, and the shortest event
    {
        const std::vector<int64_t> lens = {T - 13, T - 12, T - 11, 2 * T - 12, 2 * T - 11, 7};
        const std::vector<int64_t> k = check_plan("around the tile", layout_of(lens), FILT_PAD, T, 0, 0);
        const int64_t want[] = {1, 1, 2, 2, 3, 1};
        for (size_t e = 0; e < lens.size(); ++e) CHECK(k[e] == want[e], "n = %lld: %lld units", static_cast<long long>(lens[e]), static_cast<long long>(k[e]));
    }
    check_plan("no events", layout_of({}), FILT_PAD, T, 0, 0);
    check_plan("one event", layout_of({50000}), FILT_PAD, T, 0, 0);
    {
        const std::vector<int64_t> k = check_plan("100 000 short events", layout_of(std::vector<int64_t>(100000, 7)), FILT_PAD, T, 0, 0);
        for (int64_t v : k) CHECK(v == 1, "a 7-sample event has %lld units", static_cast<long long>(v));
    }
    check_plan("tiles of 2048 and 3968", layout_of({7, 2036, 2037, 100000, 3957, 8}), FILT_PAD, 2048, 0, 0);
    check_plan("tiles of 3968", layout_of({7, 3956, 3957, 100000, 8}), FILT_PAD, 3968, 0, 0);
    // the order-n route: segments of S per thread, rows of (S + H) doubles, groups under a cap
    {
        const int pad = filt_padlen(2), S = 1024, H = 128;
        const int64_t row = (S + H) * 8;
        const std::vector<int64_t> lens = {S - 2 * pad, S - 2 * pad + 1, 2 * S - 2 * pad, 2 * S - 2 * pad + 1, 70000, 10, 5000, 5000, 300};
        const Layout l = layout_of(lens);
        const std::vector<int64_t> k = check_plan("order 2, one group", l, pad, S, row, FILT_BATCH_SCRATCH_DEFAULT);
        CHECK(k[0] == 1 && k[1] == 2 && k[2] == 2 && k[3] == 3 && k[4] == 69, "segments per event");
        for (int64_t rows : {1, 2, 3, 5, 8, 68, 69, 70, 85, 1000}) check_plan("order 2, capped", l, pad, S, row, rows * row);
        FiltPlan p;
        plan_filter_batch(l.start.data(), l.len.data(), static_cast<int32_t>(lens.size()), pad, S, row, FILT_BATCH_SCRATCH_DEFAULT, &p);
        CHECK(p.group.size() == 1, "default cap: %zu groups", p.group.size());
        plan_filter_batch(l.start.data(), l.len.data(), static_cast<int32_t>(lens.size()), pad, S, row, 1, &p);
        CHECK(p.group.size() == lens.size(), "a small cap: %zu groups for %zu events", p.group.size(), lens.size());
        plan_filter_batch(l.start.data(), l.len.data(), static_cast<int32_t>(lens.size()), pad, S, row, 69 * row, &p);
        CHECK(p.group.size() == 3 && p.group[1].ev0 == 4 && p.group[1].ev1 == 5, "the long event alone: %zu groups", p.group.size());
    }
    CHECK(filt_padlen(1) == 6 && filt_padlen(2) == 9 && filt_padlen(8) == 27, "padlen");
    // refusals: the first offender is named, whatever comes behind it
    {
        Layout l = layout_of({100, 6, 200, 5});
        check_refusal("6 samples", l, FILT_PAD, FILT_PLAN_SHORT, 1);
        l = layout_of({100, 200, 9, 300});
        check_refusal("9 samples at order 2", l, filt_padlen(2), FILT_PLAN_SHORT, 2);
        l = layout_of({100, 200, 300});
        l.start[2] = -1;
        check_refusal("negative start", l, FILT_PAD, FILT_PLAN_RANGE, 2);
        l = layout_of({100, 0, 6});
        check_refusal("empty", l, FILT_PAD, FILT_PLAN_RANGE, 1);
        l = layout_of({100, -5, 6});
        check_refusal("negative length", l, FILT_PAD, FILT_PLAN_RANGE, 1);
        l = layout_of({6, -5});
        check_refusal("short before empty", l, FILT_PAD, FILT_PLAN_SHORT, 0);
        // more than INT32_MAX units: refused before a table is allocated
        l = layout_of({100, int64_t(3328) * 2147483647ll, 100});
        check_refusal("too many tiles", l, FILT_PAD, FILT_PLAN_TOO_MANY, -1);
        l = layout_of({int64_t(1) << 62, int64_t(1) << 62, int64_t(1) << 62});
        check_refusal("lengths that overflow", l, FILT_PAD, FILT_PLAN_TOO_MANY, -1);
    }
    // the route's fixed points
    CHECK(filt_route1(0.5, 0) == 0 && filt_route1(0.0, 1) == 0 && filt_route1(1.0, 1) == 0 && filt_route1(-0.2, 1) == 0, "no fused route");
    CHECK(filt_route1(1e-9, 1) == 64 && filt_route1(0.5, 1) == 64, "the smallest halo");
    for (double a = 0.01; a < 0.999; a += 0.003) {
        const int H = filt_route1(a, 1);
        if (H) {
            CHECK(H % 64 == 0 && H >= 64 && H <= FILT_H_MAX && std::pow(a, H) <= std::ldexp(1.0, -60) * 1.000001, "alpha %g: H %d", a, H);
            CHECK(H == 64 || std::pow(a, H - 64) > std::ldexp(1.0, -60), "alpha %g: H %d is not the smallest", a, H);
            CHECK(filt_tile(H) == FILT_CHUNK - 2 * H && filt_tile(H) >= 2048, "alpha %g: tile", a);
        } else {
            CHECK(std::pow(a, FILT_H_MAX) > std::ldexp(1.0, -60) * 0.999999, "alpha %g takes the scan route", a);
        }
    }
    check_requant({1, 2047, 2048, 2049, 7, 1024 * 2048, 1024 * 2048 + 1, 50000});
    check_requant({});
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("filt plan ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "route")) {
        const int H = filt_route1(std::strtod(argv[2], nullptr), std::atoi(argv[3]));
        std::printf("%d %d\n", H, H ? filt_tile(H) : 0);
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "units")) {
        Layout l;
        for (int i = 4; i < argc; ++i) { l.start.push_back(i); l.len.push_back(std::atoll(argv[i])); }
        FiltPlan p;
        const FiltPlanError err = plan_filter_batch(l.start.data(), l.len.data(), static_cast<int32_t>(l.len.size()), std::atoi(argv[2]), std::atoll(argv[3]),
                                                    0, 0, &p);
        if (err != FILT_PLAN_OK) { std::printf("refused %d %d\n", static_cast<int>(err), p.bad_event); return 0; }
        for (size_t e = 0; e < p.ev.size(); ++e)
            std::printf("%lld%c", static_cast<long long>((e + 1 < p.ev.size() ? p.ev[e + 1].unit0 : static_cast<int64_t>(p.unit.size())) - p.ev[e].unit0),
                        e + 1 < p.ev.size() ? ' ' : '\n');
        return 0;
    }
    return run_checks();
}
