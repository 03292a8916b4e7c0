// Stand-alone check of pypore_amd/csrc/pool_plan.hpp (ps_pool_plan, the parsing of GPU_MAX_HW_QUEUES): host code only, no GPU,
// no HIP.  tests/test_pool_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.
//   pool_plan_check          the table's properties; exit status 0 when all hold
//   pool_plan_check env      prints the hardware queues read from this process's GPU_MAX_HW_QUEUES
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pool_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

static int share(int v) { return v == 0 ? INT_MAX : v; }      // k0_waves 0: every slot; k0_admit 0: no limit

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "env") == 0) {
        std::printf("%d\n", ps::hw_queues_parse(std::getenv("GPU_MAX_HW_QUEUES")));
        return 0;
    }
    const int ns[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 64};
    const int qs[] = {1, 4, 16, 32};
    for (int n : ns)
        for (int q : qs) {
            ps_pool_plan_t p = {};
            CHECK(ps::pool_plan(n, q, &p) == PS_OK, "n %d q %d", n, q);
            const int n_eff = n < q ? n : q;
            CHECK(p.n_eff == n_eff, "n %d q %d: n_eff %d", n, q, p.n_eff);
            if (n <= 1 || n_eff <= 1) CHECK(p.k0_waves == 0 && p.k0_admit == 0 && p.lat_help == 1, "lone row, n %d q %d: %d %d %d", n, q, p.k0_waves, p.k0_admit, p.lat_help);
            if (n_eff >= 16) CHECK(p.k0_waves == 1 && p.k0_admit == 3 && p.lat_help == 0, "row >= 16, n %d q %d: %d %d %d", n, q, p.k0_waves, p.k0_admit, p.lat_help);
            if (n_eff > 1) CHECK(p.lat_help == 0 && p.k0_waves >= 0 && p.k0_waves <= 16 && p.k0_admit >= 0, "n %d q %d", n, q);
            // min(n, queues) only: the same plan from (n_eff, any q' >= n_eff) and from (any n' >= n_eff, n_eff)
            for (int other : {n_eff, n_eff + 1, 32, 4096}) {
                ps_pool_plan_t a = {}, b = {};
                if (n_eff >= 1 && n_eff <= 32) {
                    CHECK(ps::pool_plan(other, n_eff, &a) == PS_OK && std::memcmp(&a, &p, sizeof p) == 0, "n %d q %d against n' %d q' %d", n, q, other, n_eff);
                    if (other <= 32) CHECK(ps::pool_plan(n_eff, other, &b) == PS_OK && std::memcmp(&b, &p, sizeof p) == 0, "n %d q %d against n' %d q' %d", n, q, n_eff, other);
                }
            }
        }
    // monotone in n_eff: down the table a call never gets a larger share of the chip
    ps_pool_plan_t prev = {};
    ps::pool_plan(0, 32, &prev);
    for (int n = 1; n <= 64; ++n) {
        ps_pool_plan_t p = {};
        ps::pool_plan(n, 32, &p);
        CHECK(p.n_eff == (n < 32 ? n : 32), "n %d", n);
        CHECK(share(p.k0_waves) <= share(prev.k0_waves), "k0_waves grows at n_eff %d: %d after %d", n, p.k0_waves, prev.k0_waves);
        CHECK(share(p.k0_admit) <= share(prev.k0_admit), "k0_admit grows at n_eff %d: %d after %d", n, p.k0_admit, prev.k0_admit);
        CHECK(p.lat_help <= prev.lat_help, "lat_help comes back at n_eff %d", n);
        prev = p;
    }
    // hardware queues out of range, and bad arguments
    ps_pool_plan_t a = {}, b = {};
    ps::pool_plan(16, 0, &a);  ps::pool_plan(16, 4, &b);   CHECK(std::memcmp(&a, &b, sizeof a) == 0, "queues 0 is HIP's default of 4");
    ps::pool_plan(16, -3, &a);                             CHECK(std::memcmp(&a, &b, sizeof a) == 0, "queues < 0 is HIP's default of 4");
    CHECK(ps::pool_plan(4, 4, nullptr) == PS_ERR_ARG, "null plan");
    CHECK(ps::pool_plan(-1, 4, &a) == PS_ERR_ARG, "negative count");
    // GPU_MAX_HW_QUEUES as text
    struct { const char *text; int want; } env[] = {{nullptr, 4}, {"4", 4}, {"16", 16}, {"0", 1}, {"abc", 4}, {"99", 32}, {"", 4}, {"-2", 1},
                                                    {" 8", 8}, {"8 ", 8}, {"8x", 4}, {"1", 1}, {"32", 32},
                                                    {"-99999999999999999999999", 1}};
    for (const auto &e : env)
        CHECK(ps::hw_queues_parse(e.text) == e.want, "GPU_MAX_HW_QUEUES %s: %d, expected %d", e.text ? e.text : "(unset)", ps::hw_queues_parse(e.text), e.want);
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("pool plan ok\n");
    return failures ? 1 : 0;
}
