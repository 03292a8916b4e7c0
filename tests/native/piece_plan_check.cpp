// Stand-alone check of pypore_amd/csrc/piece_plan.hpp (the host's planning of ps_detect_pieces): host code only, no GPU, no HIP.
// tests/test_piece_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   piece_plan_check                  every check below; exit status 0 when all hold
//   piece_plan_check plan N CAP F32   prints "chunks scan_per_thread span_max bytes" of the plan, or "refused CODE"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "piece_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

typedef long long ll;
typedef unsigned __int128 u128;

static void check_sizes(int64_t n, int64_t want_chunks)
{
    for (int f32 = 0; f32 < 2; ++f32) {
        PiecePlan p;
        const PiecePlanError err = plan_pieces(n, 5, f32 != 0, &p);
        CHECK(err == PIECE_PLAN_OK, "n = %lld: error %d", static_cast<ll>(n), static_cast<int>(err));
        CHECK(p.chunks == want_chunks, "n = %lld: %d chunks, expected %lld", static_cast<ll>(n), p.chunks, static_cast<ll>(want_chunks));
        CHECK(p.n == n && p.cap == 5, "n = %lld: the plan names n and cap", static_cast<ll>(n));
        // every sample lies in exactly one chunk, the last chunk is not empty
        CHECK(static_cast<int64_t>(p.chunks) * PIECE_CHUNK >= n && (p.chunks == 0 || static_cast<int64_t>(p.chunks - 1) * PIECE_CHUNK < n),
              "n = %lld: the chunks do not cover the samples exactly", static_cast<ll>(n));
        // the one scan workgroup reaches every chunk, and no thread takes more than its share
        CHECK(static_cast<int64_t>(p.scan_per_thread) * PIECE_SCAN_NT >= p.chunks, "n = %lld: the scan leaves chunks out", static_cast<ll>(n));
        CHECK(p.chunks == 0 || static_cast<int64_t>(p.scan_per_thread - 1) * PIECE_SCAN_NT < p.chunks, "n = %lld: scan share too large", static_cast<ll>(n));
        // scratch: a word of bits per thread, four ints and two parts per chunk; every sub-buffer starts on a 16-byte boundary
        const size_t c = static_cast<size_t>(p.chunks);
        CHECK(p.b_bits >= c * PIECE_NT * 2 && p.b_bits < c * PIECE_NT * 2 + 16 && p.b_bits % 16 == 0, "n = %lld: bits", static_cast<ll>(n));
        for (size_t b : {p.b_cnt, p.b_last, p.b_base, p.b_open}) CHECK(b >= c * 4 && b < c * 4 + 16 && b % 16 == 0, "n = %lld: int table", static_cast<ll>(n));
        CHECK(p.b_head == c * sizeof(PiecePart) && p.b_tail == p.b_head, "n = %lld: parts", static_cast<ll>(n));
        CHECK(p.bytes() == p.b_bits + 4 * p.b_cnt + 2 * p.b_head, "n = %lld: total", static_cast<ll>(n));
        CHECK((n == 0) == (p.bytes() == 0), "n = %lld: %zu bytes", static_cast<ll>(n), p.bytes());
    }
}

static int run_checks()
{
    const int64_t C = PIECE_CHUNK;
    CHECK(C == 4096 && PIECE_PER == 16, "a thread's start bits are one 16-bit word, a chunk 4096 samples");
    check_sizes(0, 0);
    check_sizes(1, 1);
    check_sizes(C - 1, 1);
    check_sizes(C, 1);
    check_sizes(C + 1, 2);
    check_sizes(3 * C + 5, 4);
    check_sizes(INT32_MAX, (int64_t(1) << 19));
    {
        PiecePlan p;
        CHECK(plan_pieces(INT32_MAX, 0, false, &p) == PIECE_PLAN_OK && p.scan_per_thread == 512, "2^31 - 1 samples: %d chunks per scan thread", p.scan_per_thread);
    }
    // refusals, and what a refused call leaves
    {
        PiecePlan p;
        p.chunks = 7; p.b_bits = 99;
        CHECK(plan_pieces(-1, 0, false, &p) == PIECE_PLAN_NEGATIVE && p.chunks == 0 && p.bytes() == 0, "n = -1");
        CHECK(plan_pieces(INT64_MIN, 0, false, &p) == PIECE_PLAN_NEGATIVE, "n = INT64_MIN");
        CHECK(plan_pieces(int64_t(INT32_MAX) + 1, 0, false, &p) == PIECE_PLAN_LONG && p.bytes() == 0, "n = 2^31");
        CHECK(plan_pieces(INT64_MAX, 0, true, &p) == PIECE_PLAN_LONG, "n = INT64_MAX");
        CHECK(plan_pieces(10, -1, false, &p) == PIECE_PLAN_CAP && p.bytes() == 0, "cap = -1");
        CHECK(plan_pieces(10, INT64_MIN, true, &p) == PIECE_PLAN_CAP, "cap = INT64_MIN");
        CHECK(plan_pieces(-1, -1, false, &p) == PIECE_PLAN_NEGATIVE, "n is judged first");
        CHECK(plan_pieces(0, 0, false, &p) == PIECE_PLAN_OK && plan_pieces(10, INT64_MAX, false, &p) == PIECE_PLAN_OK, "cap = 0 and a huge cap are taken");
    }
    // the overflow bound: with |y| <= span_max, n y^2 and n |y| fit int64 -- in 128-bit arithmetic, no floating point
    for (int64_t n : {int64_t(1), int64_t(2), int64_t(3), C, int64_t(1) << 15, (int64_t(1) << 15) + 1, int64_t(100000000), int64_t(1) << 30, int64_t(INT32_MAX)}) {
        const int64_t b = piece_span_bound(n);
        CHECK(static_cast<u128>(n) * static_cast<u128>(b) * static_cast<u128>(b) <= static_cast<u128>(INT64_MAX), "n = %lld: bound %lld overflows", static_cast<ll>(n), static_cast<ll>(b));
        CHECK(static_cast<u128>(n) * static_cast<u128>(b + 1) * static_cast<u128>(b + 1) > static_cast<u128>(INT64_MAX), "n = %lld: bound %lld is not the largest", static_cast<ll>(n), static_cast<ll>(b));
        const int32_t f = piece_span_max(true, n), i = piece_span_max(false, n);
        CHECK(i == 65535, "int16 span %d", i);
        CHECK(f >= 1 && f <= PIECE_SPAN_F32_MAX && f <= b, "float32 span %d at n = %lld", f, static_cast<ll>(n));
        CHECK(static_cast<u128>(n) * static_cast<u128>(f) * static_cast<u128>(f) <= static_cast<u128>(INT64_MAX), "float32 span %d at n = %lld overflows", f, static_cast<ll>(n));
        CHECK(static_cast<u128>(n) * static_cast<u128>(i) * static_cast<u128>(i) <= static_cast<u128>(INT64_MAX), "int16 span at n = %lld overflows", static_cast<ll>(n));
    }
    // short traces are not restricted at all: any two float32 counts on the grid (|k| < 2^23) lie within the span
    CHECK(piece_span_max(true, 1 << 15) == PIECE_SPAN_F32_MAX && piece_span_max(true, 0) == PIECE_SPAN_F32_MAX, "float32, n <= 2^15: the type's own span");
    CHECK(piece_span_max(true, 100000000) >= (1 << 18), "float32, 1e8 samples: at least 2^18 counts from the piece's first");
    CHECK(piece_span_max(true, INT32_MAX) >= 65536, "float32, 2^31 - 1 samples: at least the int16 span");
    // the capacity rule: P pieces need room for P rows (and P + 1 edges)
    CHECK(piece_capacity_ok(0, 0) && piece_capacity_ok(5, 5) && piece_capacity_ok(5, 6) && !piece_capacity_ok(6, 5) && !piece_capacity_ok(1, 0) &&
          !piece_capacity_ok(-1, 5) && piece_capacity_ok(INT32_MAX, INT64_MAX), "capacity rule");
    CHECK(sizeof(PiecePart) == 32, "part layout");
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("piece plan ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !std::strcmp(argv[1], "plan")) {
        PiecePlan p;
        const PiecePlanError err = plan_pieces(std::atoll(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]) != 0, &p);
        if (err != PIECE_PLAN_OK) { std::printf("refused %d\n", static_cast<int>(err)); return 0; }
        std::printf("%d %d %d %zu\n", p.chunks, p.scan_per_thread, p.span_max, p.bytes());
        return 0;
    }
    return run_checks();
}
