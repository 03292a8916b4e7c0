// Stand-alone check of pypore_amd/csrc/batch_plan.hpp (the host's planning of the batch entry points): host code only, no GPU,
// no HIP.  tests/test_batch_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   batch_plan_check                                          every check below; exit status 0 when all hold
//   batch_plan_check trf BUDGET DEFAULT [LDS:SLOTS...] -- N...     the repeat splitter's launches for sequences of N segments
//   batch_plan_check pw BUDGET DEFAULT [LDS:SLOTS...] -- MxN...    the pairwise aligner's launches for pairs of M x N elements
//                                                             one line "q0 q1 grid per_wg lds" per launch, or "refused Q0"
//   batch_plan_check chunk BUDGET ROW_BYTES LEN...            next_chunk's launches: one line "q0 q1 bytes" each
// The slots of a launch are a fake resident_slots: SLOTS for a dynamic LDS of LDS bytes, DEFAULT for any other.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "batch_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

struct FakeSlots {
    std::vector<std::pair<size_t, unsigned>> table;
    unsigned other = 1;
    std::vector<size_t> asked;                              // every LDS size asked for, in order
    unsigned operator()(size_t lds)
    {
        asked.push_back(lds);
        for (const auto &p : table) if (p.first == lds) return p.second;
        return other;
    }
};

template <class Dims> static std::vector<ScratchLaunch<Dims>> plan_all(const std::vector<Dims> &items, unsigned long long budget, FakeSlots &slots,
                                                                       int32_t *refused)
{
    std::vector<ScratchLaunch<Dims>> out;
    const int32_t n = static_cast<int32_t>(items.size());
    *refused = -1;
    ScratchLaunch<Dims> L;
    for (int32_t q0 = 0; q0 < n; q0 = L.q1) {
        if (next_scratch_launch(q0, n, budget, [&](int32_t q) { return items[q]; }, slots, &L)) { *refused = q0; break; }
        out.push_back(L);
    }
    return out;
}

static bool same(const PwDims &a, const PwDims &b) { return a.cells == b.cells && a.rows == b.rows && a.n_cap == b.n_cap; }
static bool same(const TrfDims &a, const TrfDims &b) { return a.n_cap == b.n_cap; }

// The properties of the scratch planner, from the items alone
template <class Dims> static void check_launches(const char *name, const std::vector<Dims> &items, unsigned long long budget, unsigned n_slots)
{
    FakeSlots slots;
    slots.other = n_slots;
    int32_t refused;
    const std::vector<ScratchLaunch<Dims>> Ls = plan_all(items, budget, slots, &refused);
    const int32_t n = static_cast<int32_t>(items.size());
    CHECK(refused < 0, "%s: refused at %d", name, refused);
    CHECK(slots.asked.size() == 2 * Ls.size(), "%s: %zu slot lookups for %zu launches", name, slots.asked.size(), Ls.size());
    int32_t next = 0;
    for (size_t k = 0; k < Ls.size(); ++k) {
        const ScratchLaunch<Dims> &L = Ls[k];
        CHECK(L.q0 == next && L.q1 > L.q0 && L.q1 <= n, "%s: launch %zu holds [%d, %d), expected from %d", name, k, L.q0, L.q1, next);
        next = L.q1;
        Dims d, first;
        first.join(items[L.q0]);
        for (int32_t q = L.q0; q < L.q1 && q < n; ++q) d.join(items[q]);
        CHECK(same(d, L.dims), "%s: launch %zu: dims are not the maximum of its items", name, k);
        CHECK(L.per_wg == d.scratch_bytes() && L.lds == d.lds_bytes(), "%s: launch %zu: %llu bytes, LDS %zu", name, k, L.per_wg, L.lds);
        CHECK(L.grid >= 1 && (L.grid == 1 || L.grid * L.per_wg <= budget), "%s: launch %zu: grid %u of %llu bytes", name, k, L.grid, L.per_wg);
        CHECK(L.grid <= static_cast<unsigned>(L.q1 - L.q0) && L.grid <= n_slots, "%s: launch %zu: grid %u", name, k, L.grid);
        CHECK(L.grid == std::max<unsigned long long>(1, std::min<unsigned long long>(std::min<unsigned>(L.q1 - L.q0, n_slots), budget / L.per_wg)),
              "%s: launch %zu: grid %u is not the clamp", name, k, L.grid);
        // the lookups: the first item's LDS, then the launch's
        CHECK(slots.asked[2 * k] == first.lds_bytes() && slots.asked[2 * k + 1] == L.lds, "%s: launch %zu: lookups at %zu and %zu", name, k,
              slots.asked[2 * k], slots.asked[2 * k + 1]);
        // greedy: the item behind a cut enlarged the launch, and joining would have broken the budget test
        if (L.q1 < n) {
            Dims joined = d;
            joined.join(items[L.q1]);
            const unsigned long long g = std::min<unsigned long long>(static_cast<unsigned long long>(L.q1 - L.q0) + 1, n_slots);
            CHECK(d.grown_by(items[L.q1]) && g * joined.scratch_bytes() > budget, "%s: launch %zu closed early at %d", name, k, L.q1);
        }
        // ... and no item inside it would have
        Dims run;
        for (int32_t q = L.q0; q < L.q1 && q < n; ++q) {
            Dims joined = run;
            joined.join(items[q]);
            if (q > L.q0 && run.grown_by(items[q])) {
                const unsigned long long g = std::min<unsigned long long>(static_cast<unsigned long long>(q - L.q0) + 1, n_slots);
                CHECK(g * joined.scratch_bytes() <= budget, "%s: launch %zu took item %d over the budget", name, k, q);
            }
            run = joined;
        }
    }
    CHECK(next == n, "%s: launches end at %d of %d", name, next, n);
}

template <class Dims, class Make> static void sweep(const char *name, Make &&make)
{
    std::mt19937_64 rng(20240611);
    for (int n : {0, 1, 1000}) {
        std::vector<Dims> items;
        Dims all;
        for (int q = 0; q < n; ++q) { items.push_back(make(rng)); all.join(items.back()); }
        for (unsigned s : {1u, 3u, 1000000u}) {
            const unsigned long long fit = std::min<unsigned long long>(std::max(n, 1), s) * all.scratch_bytes();   // everything in one launch, exactly
            for (unsigned long long budget : {1ull, 3 * all.scratch_bytes() / 2, fit, fit - 1, 1ull << 62}) check_launches(name, items, std::max(budget, 1ull), s);
            FakeSlots slots;
            slots.other = s;
            int32_t refused;
            const auto Ls = plan_all(items, fit, slots, &refused);
            CHECK(Ls.size() == (n ? 1u : 0u), "%s: %zu launches at the exact fit (n %d, slots %u)", name, Ls.size(), n, s);
            if (n) CHECK(Ls[0].grid == std::min<unsigned>(n, s) && Ls[0].grid * Ls[0].per_wg == fit, "%s: grid %u at the exact fit", name, Ls[0].grid);
        }
    }
}

static std::vector<TrfDims> trf_items(const std::vector<int> &lens)
{
    std::vector<TrfDims> v;
    for (int n : lens) v.push_back(TrfDims{n});
    return v;
}

static void check_pinned()
{
    CHECK(trf_scratch_bytes(65) == 4704 && trf_scratch_bytes(129) == 12416 && trf_scratch_bytes(130) == 12512, "trf scratch");
    CHECK(trf_lds_bytes(129) == 3104 && trf_lds_bytes(130) == 3128 && trf_row_words(65) == 3 && trf_row_words(129) == 4, "trf LDS and words");
    const std::vector<TrfDims> items = trf_items({65, 65, 129, 3, 129, 65, 2, 130});
    FakeSlots slots;
    slots.other = 8;
    int32_t refused;
    auto Ls = plan_all(items, 40000, slots, &refused);
    CHECK(Ls.size() == 2 && refused < 0, "trf, 40 000 bytes: %zu launches", Ls.size());
    if (Ls.size() == 2) {
        CHECK(Ls[0].q0 == 0 && Ls[0].q1 == 7 && Ls[0].grid == 3 && Ls[0].per_wg == 12416 && Ls[0].lds == 3104, "trf launch 0: [%d, %d) grid %u, %llu, %zu",
              Ls[0].q0, Ls[0].q1, Ls[0].grid, Ls[0].per_wg, Ls[0].lds);
        CHECK(Ls[1].q0 == 7 && Ls[1].q1 == 8 && Ls[1].grid == 1 && Ls[1].per_wg == 12512 && Ls[1].lds == 3128, "trf launch 1: [%d, %d) grid %u, %llu, %zu",
              Ls[1].q0, Ls[1].q1, Ls[1].grid, Ls[1].per_wg, Ls[1].lds);
    }
    Ls = plan_all(items, 1, slots, &refused);
    CHECK(Ls.size() == 3, "trf, 1 byte: %zu launches", Ls.size());
    if (Ls.size() == 3)
        CHECK(Ls[0].q1 == 2 && Ls[1].q1 == 7 && Ls[2].q1 == 8 && Ls[0].grid == 1 && Ls[1].grid == 1 && Ls[2].grid == 1, "trf, 1 byte: cuts at %d, %d, %d",
              Ls[0].q1, Ls[1].q1, Ls[2].q1);
    // the pairwise sizes against the formulas of tests/pairwise_geometry.py; a longer y alone never cuts
    for (unsigned long long rows : {0ull, 1ull, 7ull, 200ull, 46341ull})
        for (unsigned long long n : {0ull, 1ull, 64ull, 8190ull})
            CHECK(pw_scratch_bytes(rows * n, rows) == ((8 * rows * n + 12 * rows + rows * n + 15) & ~15ull), "pw scratch %llu x %llu", rows, n);
    for (int n : {1, 2, 64, 8190}) CHECK(pw_lds_bytes(n) == (2 * static_cast<size_t>(n) + 2) * 8, "pw LDS %d", n);
    {
        const std::vector<PwDims> pairs = {PwDims{8000, 100, 80}, PwDims{8000, 1, 8000}, PwDims{4000, 100, 40}, PwDims{8001, 3, 2667}};
        auto Lp = plan_all(pairs, 1, slots, &refused);
        CHECK(Lp.size() == 2 && Lp[0].q1 == 3 && Lp[0].dims.n_cap == 8000 && Lp[0].lds == pw_lds_bytes(8000), "pairwise: a longer y joined, more cells cut");
        // one pair beyond 32 GiB of scratch is refused, and named
        const std::vector<PwDims> big = {PwDims{64, 8, 8}, PwDims{1ull << 32, 1ull << 19, 8190}};
        Lp = plan_all(big, 1, slots, &refused);
        CHECK(Lp.size() == 1 && refused == 1, "pairwise: %zu launches, refused at %d", Lp.size(), refused);
    }
    // next_chunk: (len + 1) rows each
    {
        const int64_t off[] = {0, 3, 6, 9, 19, 20};
        long long bytes = 0;
        CHECK(next_chunk(off, 0, 5, 8, 100, &bytes) == 3 && bytes == 96, "chunk 0: %lld bytes", bytes);
        CHECK(next_chunk(off, 3, 5, 8, 100, &bytes) == 4 && bytes == 88, "chunk 1: %lld bytes", bytes);
        CHECK(next_chunk(off, 4, 5, 8, 100, &bytes) == 5 && bytes == 16, "chunk 2: %lld bytes", bytes);
        for (int32_t q = 0; q < 5; ++q) CHECK(next_chunk(off, q, 5, 8, 1, &bytes) == q + 1 && bytes == (off[q + 1] - off[q] + 1) * 8, "budget 1: sequence %d", q);
        CHECK(next_chunk(off, 0, 5, 8, 96 + 88 + 16, &bytes) == 5 && bytes == 200, "one launch at the exact fit");
        CHECK(next_chunk(off, 0, 5, 8, 199, &bytes) == 4 && bytes == 184, "one byte short");
    }
    // budget_grid: the clamp
    CHECK(budget_grid(10, 4, 100, 30) == 3 && budget_grid(10, 4, 100, 101) == 1 && budget_grid(2, 4, 1ull << 40, 1) == 2 && budget_grid(10, 4, 1ull << 40, 1) == 4,
          "budget_grid");
    CHECK(HMM_NT == 64 && HMM_EXPECT_LDS == 65536 && HMM_EXPECT_ROWS == 268435456 && budget_grid(1000, 2048, HMM_EXPECT_ROWS, 8u << 20) == 32, "HMM caps");
    // align_plan against tests/launch_geometry.py:align_geometry
    for (int m : {1, 7, 1024})
        for (int n_seq : {1, 512, 513})
            for (int64_t s_max : {int64_t(0), int64_t(1), int64_t(1000000)}) {
                const unsigned long long blk = n_seq > 512 ? 12u << 10 : 48u << 10;
                const unsigned long long B = std::max<unsigned long long>(1, std::min<unsigned long long>(32, blk / (24ull * m)));
                const unsigned long long lds = ((9 + 3 * B + 1) * m + 3 * 64 + 2) * 8;
                const unsigned long long cap = std::max<unsigned long long>(1, (2ull << 30) / (24ull * std::max<int64_t>(s_max, 1) * m));
                AlignPlan A;
                CHECK(align_plan(m, n_seq, s_max, &A) == BATCH_PLAN_OK, "align_plan(%d, %d, %lld) refused", m, n_seq, static_cast<long long>(s_max));
                CHECK(static_cast<unsigned long long>(A.B) == B && A.lds == lds && A.grid_cap == cap && A.per_wg == 3ull * std::max<int64_t>(s_max, 1) * m,
                      "align_plan(%d, %d, %lld): B %d, LDS %zu, cap %u", m, n_seq, static_cast<long long>(s_max), A.B, A.lds, A.grid_cap);
            }
    {
        AlignPlan A;
        CHECK(ALIGN_NT == 64 && ALIGN_M_MAX == 1024 && ALIGN_B_MAX == 32 && align_lds_doubles(7, 32) == 106 * 7 + 194, "aligner caps");
        CHECK(align_plan(1024, 1, (int64_t(32) << 30) / (24 * 1024), &A) == BATCH_PLAN_OK && A.grid_cap == 1, "32 GiB exactly");
        CHECK(align_plan(1024, 1, (int64_t(32) << 30) / (24 * 1024) + 1, &A) == BATCH_PLAN_SCRATCH, "one row above 32 GiB");
    }
}

static void check_offset_tables()
{
    const int64_t MAXLEN = INT32_MAX / 2;
    int64_t longest = -1;
    int32_t bad = -2;
    {
        const int64_t off[] = {0, 5, 5, 12, 12 + MAXLEN};
        CHECK(check_offsets(off, 4, &longest, &bad) == BATCH_PLAN_OK && longest == MAXLEN && bad == -1, "good offsets: longest %lld", static_cast<long long>(longest));
        CHECK(check_offsets(off, 0, &longest, &bad) == BATCH_PLAN_OK && longest == 0, "no sequences");
        CHECK(check_slot_offsets(off, 4, &bad) == BATCH_PLAN_OK && check_slot_offsets(off, 0, &bad) == BATCH_PLAN_OK, "good slots");
    }
    {
        const int64_t off[] = {0, 5, 6 + MAXLEN, 6 + MAXLEN};
        CHECK(check_offsets(off, 3, &longest, &bad) == BATCH_PLAN_LONG && bad == 1, "too long: names %d", bad);
        CHECK(check_slot_offsets(off, 3, &bad) == BATCH_PLAN_OK, "slots have no length cap");
    }
    {
        const int64_t off[] = {0, 5, 4, 9};
        CHECK(check_offsets(off, 3, &longest, &bad) == BATCH_PLAN_ORDER && bad == 1, "descending: names %d", bad);
        bad = -2;
        CHECK(check_slot_offsets(off, 3, &bad) == BATCH_PLAN_ORDER && bad == 1, "descending slots: names %d", bad);
        CHECK(slot_ok(off, 0) && !slot_ok(off, 1) && slot_ok(off, 2), "slot_ok");
    }
    {
        const int64_t off[] = {0, 3, -1, 9};
        CHECK(check_offsets(off, 3, &longest, &bad) == BATCH_PLAN_ORDER && bad == 1, "negative entry: names %d", bad);
    }
    // hostile tables: refused without a signed overflow (the sanitized build would stop here)
    const int64_t hostile[][2] = {{-1, INT64_MAX}, {INT64_MIN, 0}, {0, INT64_MAX}, {INT64_MIN, INT64_MAX}, {INT64_MAX, INT64_MIN}};
    const BatchPlanError want[] = {BATCH_PLAN_ORDER, BATCH_PLAN_ORDER, BATCH_PLAN_LONG, BATCH_PLAN_ORDER, BATCH_PLAN_ORDER};
    for (int k = 0; k < 5; ++k) {
        CHECK(check_offsets(hostile[k], 1, &longest, &bad) == want[k] && bad == 0, "hostile table %d", k);
        CHECK((check_slot_offsets(hostile[k], 1, &bad) == BATCH_PLAN_ORDER) == (want[k] == BATCH_PLAN_ORDER), "hostile slot table %d", k);
    }
}

static void check_event_tables()
{
    const int64_t P30 = int64_t(1) << 30;
    int64_t total = -1;
    int32_t bad = -2;
    {
        const int64_t start[] = {0, 7, 7, INT64_MAX}, len[] = {10, 0, P30, 3};
        CHECK(check_events(start, len, 4, nullptr, nullptr, 0, &total, &bad) == BATCH_PLAN_OK && total == 13 + P30 && bad == -1, "good events");
        CHECK(check_events(start, len, 0, nullptr, nullptr, 0, &total, &bad) == BATCH_PLAN_OK && total == 0, "no events");
    }
    {
        const int64_t start[] = {0, 7, 9}, len[] = {10, P30 + 1, -1};
        CHECK(check_events(start, len, 3, nullptr, nullptr, 0, &total, &bad) == BATCH_PLAN_LONG && bad == 1, "2^30 + 1: names %d", bad);
    }
    {
        const int64_t start[] = {0, -7, 9}, len[] = {10, 5, -1}, len2[] = {10, 5, INT64_MIN};
        CHECK(check_events(start, len, 3, nullptr, nullptr, 0, &total, &bad) == BATCH_PLAN_NEGATIVE && bad == 1, "negative start: names %d", bad);
        CHECK(check_events(start + 2, len + 2, 1, nullptr, nullptr, 0, &total, &bad) == BATCH_PLAN_NEGATIVE && bad == 0, "negative length");
        CHECK(check_events(start + 2, len2 + 2, 1, nullptr, nullptr, 100, &total, &bad) == BATCH_PLAN_NEGATIVE && bad == 0, "INT64_MIN");
    }
    {   // min_len: the filter-derivative parser asks for more than padlen = 6 samples
        const int64_t start[] = {0, 0, 0}, len[] = {100, 7, 6};
        CHECK(check_events(start, len, 2, nullptr, nullptr, 7, &total, &bad) == BATCH_PLAN_OK && total == 107, "padlen + 1 samples pass");
        CHECK(check_events(start, len, 3, nullptr, nullptr, 7, &total, &bad) == BATCH_PLAN_SHORT && bad == 2, "padlen samples: names %d", bad);
        CHECK(check_events(start, len, 3, nullptr, nullptr, 6, &total, &bad) == BATCH_PLAN_OK, "min_len padlen");
    }
    {   // StatSplit's ranges: within [0, len] each, hi below lo is an empty range
        const int64_t start[] = {0, 0, 0, 0}, len[] = {10, 10, 10, 0};
        const int64_t lo[] = {0, 10, 7, 0}, hi[] = {10, 10, 3, 0};
        CHECK(check_events(start, len, 4, lo, hi, 0, &total, &bad) == BATCH_PLAN_OK && total == 30, "ranges at the edges, hi < lo");
        const int64_t lo_bad[] = {0, 11, 7, 0}, hi_bad[] = {10, 10, 11, 0}, neg[] = {0, 0, -1, 0};
        CHECK(check_events(start, len, 4, lo_bad, hi, 0, &total, &bad) == BATCH_PLAN_RANGE && bad == 1, "lo > len: names %d", bad);
        CHECK(check_events(start, len, 4, lo, hi_bad, 0, &total, &bad) == BATCH_PLAN_RANGE && bad == 2, "hi > len: names %d", bad);
        CHECK(check_events(start, len, 4, neg, nullptr, 0, &total, &bad) == BATCH_PLAN_RANGE && bad == 2, "lo < 0");
        CHECK(check_events(start, len, 4, nullptr, neg, 0, &total, &bad) == BATCH_PLAN_RANGE && bad == 2, "hi < 0");
        CHECK(check_events(start, len, 4, lo, nullptr, 0, &total, &bad) == BATCH_PLAN_OK && check_events(start, len, 4, nullptr, hi, 0, &total, &bad) == BATCH_PLAN_OK,
              "one of the two tables");
    }
}

static void check_statsplit_tables(int64_t mw, const std::vector<int64_t> &len, const std::vector<int64_t> &lo, const std::vector<int64_t> &hi)
{
    const int32_t n_ev = static_cast<int32_t>(len.size());
    const size_t n = len.size();
    std::vector<int64_t> start;
    for (size_t e = 0; e < n; ++e) start.push_back(1000 - static_cast<int64_t>(e));
    StatsplitTables T;
    int32_t bad = -2;
    const BatchPlanError err = plan_statsplit_tables(start.data(), len.data(), n_ev, lo.empty() ? nullptr : lo.data(), hi.empty() ? nullptr : hi.data(), mw, &T, &bad);
    CHECK(err == BATCH_PLAN_OK && T.tab.size() == 6 * n + 1, "statsplit tables (mw %lld): error %d, %zu entries", static_cast<long long>(mw), static_cast<int>(err), T.tab.size());
    if (err || T.tab.size() != 6 * n + 1) return;
    int64_t pre = 0, slots = 0, longest = 0;
    for (size_t e = 0; e < n; ++e) {
        const int64_t l = lo.empty() ? 0 : lo[e], h = hi.empty() ? len[e] : hi[e], span = h > l ? h - l : 0;
        CHECK(T.tab[e] == start[e] && T.tab[n + e] == len[e] && T.tab[2 * n + e] == pre && T.tab[3 * n + e] == l && T.tab[4 * n + e] == h && T.tab[5 * n + e] == slots,
              "statsplit tables (mw %lld): event %zu", static_cast<long long>(mw), e);
        pre += len[e]; slots += 2 * (span / mw) + 2; longest = std::max(longest, span);
    }
    CHECK(T.tab[6 * n] == slots && T.slots == slots && T.total_len == pre && T.stack_cap == longest / mw + 2, "statsplit tables (mw %lld): totals", static_cast<long long>(mw));
}

static void check_tables()
{
    check_statsplit_tables(1, {0, 1, 5, 1 << 20}, {}, {});
    for (int64_t mw : {int64_t(1), int64_t(5), int64_t(64)}) {
        check_statsplit_tables(mw, {}, {}, {});
        check_statsplit_tables(mw, {3 * mw - 1, 3 * mw, 3 * mw + 1, 0, mw - 1, mw, mw + 1}, {}, {});
        // spans of 2 mw - 1, 2 mw, 2 mw + 1 inside longer events, an empty and a reversed range
        check_statsplit_tables(mw, {4 * mw, 4 * mw, 4 * mw, 4 * mw, 4 * mw}, {1, 1, 1, mw, 3 * mw}, {2 * mw, 2 * mw + 1, 2 * mw + 2, mw, mw});
    }
    {
        const int64_t start[] = {0, 0}, len[] = {10, (int64_t(1) << 30) + 1};
        StatsplitTables T;
        int32_t bad = -2;
        CHECK(plan_statsplit_tables(start, len, 2, nullptr, nullptr, 1, &T, &bad) == BATCH_PLAN_LONG && bad == 1 && T.tab.empty(), "statsplit tables: 2^30 + 1");
        const int64_t ok[] = {int64_t(1) << 30, int64_t(1) << 30};
        CHECK(plan_statsplit_tables(start, ok, 2, nullptr, nullptr, 1, &T, &bad) == BATCH_PLAN_OK && T.slots == (int64_t(1) << 32) + 4 && T.stack_cap == (int64_t(1) << 30) + 2,
              "statsplit tables: 2^30 twice");
    }
    // tile tables: ceil(npos / SP_TILE) tiles per event
    CHECK(SP_TILE == 2048 && SP_NT * SP_ROUNDS == SP_TILE, "SP_TILE");
    {
        const std::vector<int64_t> npos = {0, 1, 2047, 2048, 2049, 0, 5 * 2048}, start = {9, 8, 7, 6, 5, 4, 3}, want = {0, 1, 1, 1, 2, 0, 5};
        std::vector<int64_t> tab;
        int64_t tiles = -1, at = 0;
        const size_t n = npos.size();
        CHECK(plan_tile_table(start.data(), npos.data(), static_cast<int32_t>(n), &tab, &tiles) == BATCH_PLAN_OK && tab.size() == 3 * n + 1, "tile table");
        for (size_t e = 0; e < n && tab.size() == 3 * n + 1; ++e) {
            CHECK(tab[e] == start[e] && tab[n + e] == npos[e] && tab[2 * n + e] == at, "tile table: event %zu starts at tile %lld", e, static_cast<long long>(tab[2 * n + e]));
            at += want[e];
        }
        CHECK(tiles == at && tab[3 * n] == at, "tile table: %lld tiles", static_cast<long long>(tiles));
        CHECK(plan_tile_table(start.data(), npos.data(), 0, &tab, &tiles) == BATCH_PLAN_OK && tiles == 0 && tab.size() == 1 && tab[0] == 0, "empty tile table");
        // INT32_MAX tiles pass, one more is refused (events of 2^30 positions: 2^19 tiles each)
        std::vector<int64_t> big(4096, int64_t(1) << 30), zeros(4096, 0);
        big.back() -= 2048;
        CHECK(plan_tile_table(zeros.data(), big.data(), 4096, &tab, &tiles) == BATCH_PLAN_OK && tiles == INT32_MAX, "INT32_MAX tiles");
        big.back() += 1;
        CHECK(plan_tile_table(zeros.data(), big.data(), 4096, &tab, &tiles) == BATCH_PLAN_TOO_MANY && tiles == int64_t(INT32_MAX) + 1, "one tile more");
    }
    // offsets from counts
    {
        const int32_t c32[] = {3, 0, 4, 1};
        const int64_t c64[] = {3, 0, 4, 1};
        int64_t off[5] = {-1, -1, -1, -1, -1}, total = -1;
        CHECK(offsets_from_counts(c32, 4, 8, off, &total) == BATCH_PLAN_OK && total == 8 && off[0] == 0 && off[1] == 3 && off[2] == 3 && off[3] == 7 && off[4] == 8,
              "offsets at the exact capacity");
        CHECK(offsets_from_counts(c64, 4, 7, off, &total) == BATCH_PLAN_CAPACITY && total == 8 && off[4] == 8, "one short: required %lld", static_cast<long long>(total));
        CHECK(offsets_from_counts(c64, 0, 0, off, &total) == BATCH_PLAN_OK && total == 0 && off[0] == 0, "no counts");
    }
}

static int run_checks()
{
    sweep<TrfDims>("trf", [](std::mt19937_64 &rng) { return TrfDims{static_cast<int>(rng() % 301)}; });
    sweep<PwDims>("pairwise", [](std::mt19937_64 &rng) {
        const unsigned long long m = rng() % 301, n = rng() % 201;
        return PwDims{m * n, m, static_cast<int>(n)};
    });
    check_pinned();
    check_offset_tables();
    check_event_tables();
    check_tables();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("batch plan ok\n");
    return 0;
}

template <class Dims> static int print_launches(const std::vector<Dims> &items, unsigned long long budget, FakeSlots &slots)
{
    int32_t refused;
    for (const ScratchLaunch<Dims> &L : plan_all(items, budget, slots, &refused)) std::printf("%d %d %u %llu %zu\n", L.q0, L.q1, L.grid, L.per_wg, L.lds);
    if (refused >= 0) std::printf("refused %d\n", refused);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && (!std::strcmp(argv[1], "trf") || !std::strcmp(argv[1], "pw"))) {
        FakeSlots slots;
        const unsigned long long budget = std::strtoull(argv[2], nullptr, 10);
        slots.other = static_cast<unsigned>(std::strtoul(argv[3], nullptr, 10));
        int i = 4;
        for (; i < argc && std::strcmp(argv[i], "--"); ++i) {
            char *end = nullptr;
            const size_t lds = std::strtoull(argv[i], &end, 10);
            if (*end != ':') { std::fprintf(stderr, "expected LDS:SLOTS, got %s\n", argv[i]); return 2; }
            slots.table.push_back({lds, static_cast<unsigned>(std::strtoul(end + 1, nullptr, 10))});
        }
        if (!std::strcmp(argv[1], "trf")) {
            std::vector<int> lens;
            for (++i; i < argc; ++i) lens.push_back(std::atoi(argv[i]));
            return print_launches(trf_items(lens), budget, slots);
        }
        std::vector<PwDims> pairs;
        for (++i; i < argc; ++i) {
            char *end = nullptr;
            const unsigned long long m = std::strtoull(argv[i], &end, 10);
            if (*end != 'x') { std::fprintf(stderr, "expected MxN, got %s\n", argv[i]); return 2; }
            const unsigned long long n = std::strtoull(end + 1, nullptr, 10);
            pairs.push_back(PwDims{m * n, m, static_cast<int>(n)});
        }
        return print_launches(pairs, budget, slots);
    }
    if (argc >= 4 && !std::strcmp(argv[1], "chunk")) {
        std::vector<int64_t> off(1, 0);
        for (int i = 4; i < argc; ++i) off.push_back(off.back() + std::atoll(argv[i]));
        const int32_t n = static_cast<int32_t>(off.size()) - 1;
        for (int32_t q0 = 0, q1; q0 < n; q0 = q1) {
            long long bytes = 0;
            q1 = next_chunk(off.data(), q0, n, static_cast<size_t>(std::atoll(argv[3])), std::atoll(argv[2]), &bytes);
            std::printf("%d %d %lld\n", q0, q1, bytes);
        }
        return 0;
    }
    return run_checks();
}
