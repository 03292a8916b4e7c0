// Stand-alone check of pypore_amd/csrc/range_plan.hpp (the host's planning of ps_range_stats): host code only, no GPU, no HIP.
// tests/test_range_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   range_plan_check                       every check below; exit status 0 when all hold
//   range_plan_check units UNIT LEN...     prints the units the plan gives ranges of these lengths, one number per range
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "range_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

typedef long long ll;
struct Table { std::vector<int64_t> start, end; };

// Every property the kernels rely on, recomputed from the ranges alone; returns the units per range.
static std::vector<int64_t> check_plan(const char *name, const Table &t, int64_t n, int64_t unit)
{
    const int64_t nr = static_cast<int64_t>(t.start.size());
    std::vector<int64_t> per_range(static_cast<size_t>(nr), 0);
    RangePlan p;
    int64_t bad = 12345;
    const RangePlanError err = plan_ranges(t.start.data(), t.end.data(), nr, n, unit, &p, &bad);
    CHECK(err == RANGE_PLAN_OK && bad == -1, "%s: error %d at %lld", name, static_cast<int>(err), static_cast<ll>(bad));
    if (err != RANGE_PLAN_OK) return per_range;
    CHECK(p.row.size() == static_cast<size_t>(nr), "%s: %zu rows", name, p.row.size());
    int64_t u = 0;
    for (int64_t r = 0; r < nr; ++r) {
        const RangeRow &row = p.row[static_cast<size_t>(r)];
        const int64_t len = t.end[r] - t.start[r], k = (len + unit - 1) / unit;
        CHECK(row.start == t.start[r] && row.n == len, "%s: range %lld is [%lld, + %d)", name, static_cast<ll>(r), static_cast<ll>(row.start), row.n);
        CHECK(row.unit0 == u && row.units == k, "%s: range %lld has units %d + %d, expected %lld + %lld", name, static_cast<ll>(r), row.unit0, row.units,
              static_cast<ll>(u), static_cast<ll>(k));
        // the units of the range, in order: they cover [start, end) exactly once, without a gap, none empty, none above `unit`
        int64_t at = t.start[r];
        for (int64_t i = 0; i < k && static_cast<size_t>(u + i) < p.unit.size(); ++i) {
            const RangeUnit &w = p.unit[static_cast<size_t>(u + i)];
            CHECK(w.range == r && w.unit0 == u, "%s: unit %lld names range %d, first unit %d", name, static_cast<ll>(u + i), w.range, w.unit0);
            CHECK(w.first == at && w.len >= 1 && w.len <= unit, "%s: unit %lld is [%lld, + %d), expected from %lld", name, static_cast<ll>(u + i),
                  static_cast<ll>(w.first), w.len, static_cast<ll>(at));
            CHECK(w.len == unit || i == k - 1, "%s: unit %lld of %lld is short", name, static_cast<ll>(i), static_cast<ll>(k));
            CHECK(w.first >= 0 && w.first + w.len <= n, "%s: unit %lld leaves the buffer", name, static_cast<ll>(u + i));
            at += w.len;
        }
        CHECK(at == t.end[r], "%s: range %lld covered to %lld of %lld", name, static_cast<ll>(r), static_cast<ll>(at), static_cast<ll>(t.end[r]));
        per_range[static_cast<size_t>(r)] = k;
        u += k;
    }
    CHECK(static_cast<size_t>(u) == p.unit.size(), "%s: %zu table entries for %lld units", name, p.unit.size(), static_cast<ll>(u));
    return per_range;
}

static void check_refusal(const char *name, const Table &t, int64_t n, int64_t unit, RangePlanError want, int64_t want_bad)
{
    RangePlan p;
    p.row.resize(3); p.unit.resize(5);                   // (what an earlier call left behind)
    int64_t bad = 12345;
    const RangePlanError err = plan_ranges(t.start.data(), t.end.data(), static_cast<int64_t>(t.start.size()), n, unit, &p, &bad);
    CHECK(err == want && bad == want_bad, "%s: error %d names range %lld", name, static_cast<int>(err), static_cast<ll>(bad));
    CHECK(p.row.empty() && p.unit.empty(), "%s: tables of a refused call", name);
    int64_t bad2 = 12345;
    if (want != RANGE_PLAN_TOO_MANY)
        CHECK(check_ranges(t.start.data(), t.end.data(), static_cast<int64_t>(t.start.size()), n, &bad2) == want && bad2 == want_bad, "%s: check_ranges", name);
}

static int run_checks()
{
    const int64_t N = 1 << 20;
    for (int64_t T : {int64_t(64), int64_t(512), RANGE_TILE_DEFAULT}) {
        // 1, T - 1, T, T + 1 and 2 T + 3 samples, at starts of every alignment
        Table t;
        const int64_t lens[] = {1, T - 1, T, T + 1, 2 * T + 3};
        const int64_t want[] = {1, 1, 1, 2, 3};
        for (int a = 0; a < 8; ++a)
            for (int64_t len : lens) { t.start.push_back(1000 + a); t.end.push_back(1000 + a + len); }
        const std::vector<int64_t> k = check_plan("around the tile", t, N, T);
        for (size_t r = 0; r < k.size(); ++r) CHECK(k[r] == want[r % 5], "T = %lld, %lld samples: %lld units", static_cast<ll>(T),
                                                     static_cast<ll>(t.end[r] - t.start[r]), static_cast<ll>(k[r]));
    }
    {
        // overlapping, identical, nested and descending ranges; the buffer's two ends; the whole buffer
        Table t;
        t.start = {5000, 5000, 4000, 4500, 3000, 100, 0, N - 1, 0, 5000};
        t.end = {9000, 9000, 6000, 4600, 3001, 200, 1, N, N, 9000};
        const std::vector<int64_t> k = check_plan("overlapping and repeated", t, N, 512);
        CHECK(k[0] == 8 && k[1] == 8 && k[9] == 8 && k[8] == N / 512 && k[6] == 1 && k[7] == 1, "units of the repeated ranges");
    }
    {
        Table t;
        check_plan("no ranges", t, N, 512);
        check_plan("no ranges, no samples", t, 0, 512);
        RangePlan p;
        int64_t bad = 7;
        CHECK(plan_ranges(nullptr, nullptr, 0, N, 512, &p, &bad) == RANGE_PLAN_OK && bad == -1 && p.row.empty() && p.unit.empty(), "n_ranges = 0");
    }
    {
        Table t;
        for (int64_t i = 0; i < 70000; ++i) { t.start.push_back(i); t.end.push_back(i + 1); }
        const std::vector<int64_t> k = check_plan("70 000 one-sample ranges", t, 70000, RANGE_TILE_DEFAULT);
        for (int64_t v : k) CHECK(v == 1, "a one-sample range has %lld units", static_cast<ll>(v));
    }
    // refusals: the first offender is named, whatever stands behind it
    {
        const int64_t MIN = INT64_MIN, MAX = INT64_MAX;
        check_refusal("negative start", {{10, -1, -5}, {20, 5, 2}}, N, 512, RANGE_PLAN_START, 1);
        check_refusal("end behind the buffer", {{10, 20, 30}, {20, N + 1, N + 2}}, N, 512, RANGE_PLAN_END, 1);
        check_refusal("end at the buffer's end + 1, last", {{0, N - 1}, {N, N + 1}}, N, 512, RANGE_PLAN_END, 1);
        check_refusal("empty", {{10, 20, 30}, {20, 20, 40}}, N, 512, RANGE_PLAN_EMPTY, 1);
        check_refusal("reversed", {{10, 20}, {20, 19}}, N, 512, RANGE_PLAN_EMPTY, 1);
        check_refusal("start before end before range", {{-1}, {N + 5}}, N, 512, RANGE_PLAN_START, 0);
        check_refusal("INT64_MIN start", {{0, MIN}, {1, 5}}, N, 512, RANGE_PLAN_START, 1);
        check_refusal("INT64_MIN start, INT64_MAX end", {{MIN}, {MAX}}, N, 512, RANGE_PLAN_START, 0);
        check_refusal("INT64_MAX end", {{0, 0}, {1, MAX}}, N, 512, RANGE_PLAN_END, 1);
        check_refusal("INT64_MAX start", {{MAX}, {MAX}}, MAX, 512, RANGE_PLAN_EMPTY, 0);
        check_refusal("INT64_MIN end", {{0}, {MIN}}, N, 512, RANGE_PLAN_EMPTY, 0);
        // end - start would overflow were the signs not tested first
        check_refusal("end - start overflows", {{MIN + 1}, {MAX}}, MAX, 512, RANGE_PLAN_START, 0);
        check_refusal("the whole of int64", {{0}, {MAX}}, MAX, 512, RANGE_PLAN_LONG, 0);
        check_refusal("2^31 samples", {{5, 0}, {6, int64_t(1) << 31}}, MAX, 1 << 20, RANGE_PLAN_LONG, 1);
        // the longest range there is: 2^31 - 1 samples are 2 048 units of 2^20, and too many of 64
        Table t = {{7}, {7 + int64_t(INT32_MAX)}};
        const std::vector<int64_t> k = check_plan("2^31 - 1 samples", t, int64_t(1) << 32, RANGE_TILE_MAX);
        CHECK(k[0] == 2048, "2^31 - 1 samples: %lld units", static_cast<ll>(k[0]));
        check_refusal("too many units", t, int64_t(1) << 32, 64, RANGE_PLAN_TOO_MANY, -1);
        Table many;
        for (int64_t i = 0; i < 3; ++i) { many.start.push_back(0); many.end.push_back(RANGE_UNITS_MAX / 2 * 64); }
        check_refusal("too many units over several ranges", many, int64_t(1) << 32, 64, RANGE_PLAN_TOO_MANY, -1);
    }
    CHECK(range_tile_ok(RANGE_TILE_MIN) && range_tile_ok(RANGE_TILE_MAX) && range_tile_ok(512) && range_tile_ok(RANGE_TILE_DEFAULT), "tiles accepted");
    CHECK(!range_tile_ok(RANGE_TILE_MIN - 1) && !range_tile_ok(RANGE_TILE_MAX + 1) && !range_tile_ok(0) && !range_tile_ok(-512) && !range_tile_ok(INT64_MIN) &&
          !range_tile_ok(INT64_MAX), "tiles refused");
    CHECK(range_unit(false, 512) == 512 && range_unit(true, 512) == 512 && range_unit(false, RANGE_TILE_MAX) == RANGE_TILE_MAX &&
          range_unit(true, RANGE_TILE_MAX) == RANGE_TILE_F32_MAX, "units per sample type");
    // the arithmetic contract's sizes: a unit's sums are exact in int64, a range's too for int16 counts
    CHECK(static_cast<double>(RANGE_TILE_F32_MAX) * 281474976710656.0 < 9223372036854775808.0, "float32 unit: y^2 < 2^48 summed stays below 2^63");
    CHECK(static_cast<double>(RANGE_LEN_MAX) * 65535.0 * 65535.0 < 9223372036854775808.0, "int16 range: y^2 <= 65535^2 summed stays below 2^63");
    CHECK(sizeof(RangeRow) == 24 && sizeof(RangeUnit) == 24 && sizeof(RangePart) == 24, "table layouts");
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("range plan ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "units")) {
        Table t;
        int64_t at = 3;
        for (int i = 3; i < argc; ++i) { t.start.push_back(at); t.end.push_back(at + std::atoll(argv[i])); at += 5; }
        RangePlan p;
        int64_t bad = -1;
        const RangePlanError err = plan_ranges(t.start.data(), t.end.data(), static_cast<int64_t>(t.start.size()), INT64_MAX, std::atoll(argv[2]), &p, &bad);
        if (err != RANGE_PLAN_OK) { std::printf("refused %d %lld\n", static_cast<int>(err), static_cast<ll>(bad)); return 0; }
        for (size_t r = 0; r < p.row.size(); ++r) std::printf("%d%c", p.row[r].units, r + 1 < p.row.size() ? ' ' : '\n');
        return 0;
    }
    return run_checks();
}
