// Stand-alone check of pypore_amd/csrc/ctx_options.hpp (the context's options: one struct, one table): host code only, no GPU, no HIP.
// tests/test_ctx_options_host.py builds it plain and with -fsanitize=address,undefined, each with and without -DPS_DIAG, and runs all four.
//   ctx_options_check          every check below; exit status 0 when all hold
//   ctx_options_check table    one line per row: name variable lowest highest default diagnostic-only normalisation
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "ctx_options.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

typedef long long ll;

// The defaults of the library before the table, copied once from ps_ctx; which rows are the diagnostic library's; which are bools.
struct Want { const char *name; int64_t dflt; bool diag; };
static const Want WANT[] = {
    {"mode", 0, false}, {"spine_nt", 512, false}, {"tree_nt", 256, false}, {"prune", 1, false}, {"scan_bs", 1, false}, {"groups", 1, false},
    {"wide_bs", 1, false}, {"stitch_host", 0, false}, {"timing", 1, false}, {"debug", 0, false}, {"noise_k_ppm", 100000, false},
    {"near_tie_log", 65536, false}, {"k0_waves", 0, false}, {"k0_admit", 0, false}, {"k0_shared", 0, false}, {"k0_unaligned", 1, false},
    {"upload_by_kernel", 1, false}, {"download_by_kernel", 1, false}, {"single_pass", 1, false}, {"gather_fused", 1, false}, {"tree_mw", 0, false},
    {"tree_par", 1, false}, {"tree_tail_pct", 0, false}, {"tree_jobs_per_wave", 4, false}, {"tree_screen", 1, false}, {"slots_pct", 100, false},
    {"bridge_single", 1 << 30, false}, {"bridge_budget", 256, false}, {"bridge_ext", 1, false}, {"bridge_patience", 16, false}, {"lat_help", 1, false},
    {"short_chain", 1, false}, {"shared_device", 0, false}, {"hw_queues", 0, false}, {"filter_fused", 1, false},
    {"filt_batch_scratch", 256ll << 20, false}, {"range_tile", 16384, false}, {"pairwise_budget", 2ll << 30, false}, {"trf_budget", 2ll << 30, false},
    {"hmm_bp_budget", 512ll << 20, false}, {"hmm_fb_budget", 4ll << 30, false}, {"hmm_expect_lds", 1, false},
    {"dbg_phase", 0, true}, {"dbg_k0_nogrp", 0, true}, {"k0_sets", 2, true}, {"scan_lds_pad", 0, true}, {"rep_eval", 1, true}, {"rep_stage", 1, true},
    {"rep_sum", 1, true}, {"cu_mask", 0, true},
};
// The ranges of ps_set_option's chain as it stood (bools, timing and the sets apart), and the bounds decided for the ints that had none.
struct Range { const char *name; int64_t lo, hi; };
static const Range RANGES[] = {
    {"mode", 0, 2}, {"near_tie_log", 0, int64_t(1) << 30}, {"k0_waves", 0, 16}, {"k0_admit", 0, INT32_MAX}, {"bridge_ext", 0, 1}, {"lat_help", 0, 2},
    {"shared_device", 0, 4096}, {"hw_queues", 0, 32}, {"hmm_bp_budget", 1, INT64_MAX}, {"hmm_fb_budget", 1, INT64_MAX}, {"pairwise_budget", 1, INT64_MAX},
    {"trf_budget", 1, INT64_MAX}, {"slots_pct", 1, 100}, {"tree_jobs_per_wave", 0, 1024}, {"short_chain", 0, 3}, {"bridge_patience", 1, 4096},
    {"noise_k_ppm", 0, INT32_MAX}, {"bridge_budget", 1, 256}, {"bridge_single", 1, INT32_MAX}, {"tree_tail_pct", 0, 100},
    {"filt_batch_scratch", 1, INT64_MAX}, {"range_tile", 64, 1 << 20}, {"spine_nt", 256, 1024}, {"tree_nt", 256, 512},
    {"dbg_phase", 0, 2}, {"k0_sets", 2, 4}, {"scan_lds_pad", 0, 65536}, {"rep_eval", 1, INT32_MAX}, {"rep_stage", 1, INT32_MAX}, {"rep_sum", 1, INT32_MAX},
    {"cu_mask", INT64_MIN, INT64_MAX},
};
static const char *const BOOLS[] = {"stitch_host", "prune", "scan_bs", "groups", "tree_par", "k0_shared", "hmm_expect_lds", "single_pass", "gather_fused",
                                    "download_by_kernel", "debug", "k0_unaligned", "tree_screen", "dbg_k0_nogrp", "wide_bs", "filter_fused",
                                    "upload_by_kernel", "tree_mw"};

static bool same(const CtxOptions &a, const CtxOptions &b)     // every member has a row
{
    for (const OptRow &r : OPT_ROWS)
        if (r.read(a) != r.read(b)) return false;
    return true;
}

static int64_t get(const CtxOptions &o, const char *name)
{
    int64_t v = -777;
    CHECK(opt_get(o, name, &v) == OPT_OK, "get %s", name);
    return v;
}

// value is taken and reads back as `stored`
static void accepted(const char *name, int64_t value, int64_t stored)
{
    CtxOptions o;
    const OptRow *row = nullptr;
    CHECK(opt_set(&o, name, value, &row) == OPT_OK && row && !std::strcmp(row->name, name), "%s = %lld is not taken", name, static_cast<ll>(value));
    CHECK(get(o, name) == stored, "%s = %lld reads back %lld, expected %lld", name, static_cast<ll>(value), static_cast<ll>(get(o, name)), static_cast<ll>(stored));
}

// value is refused, and the option keeps what it had: its default, and a value set before
static void refused(const char *name, int64_t value, int64_t keep)
{
    CtxOptions o;
    const int64_t dflt = get(o, name);
    CHECK(opt_set(&o, name, value) == OPT_REFUSED && get(o, name) == dflt, "%s = %lld is not refused", name, static_cast<ll>(value));
    CHECK(opt_set(&o, name, keep) == OPT_OK && opt_set(&o, name, value) == OPT_REFUSED && get(o, name) == keep, "%s = %lld after %lld", name,
          static_cast<ll>(value), static_cast<ll>(keep));
}

static void check_rows()
{
    std::set<std::string> names, vars, known;
    for (const OptRow &r : OPT_ROWS) {
        CHECK(names.insert(r.name).second, "two rows named %s", r.name);
        if (r.env) CHECK(vars.insert(r.env).second && !std::strncmp(r.env, "PORESEG_", 8), "variable %s", r.env);
    }
    CHECK(names.size() == sizeof WANT / sizeof WANT[0], "%zu rows, %zu expected", names.size(), sizeof WANT / sizeof WANT[0]);
    const CtxOptions fresh;
    for (const Want &w : WANT) {
        CHECK(names.count(w.name) == 1, "no row %s", w.name);
        const OptRow *r = opt_find(w.name);
        if (w.diag && !OPT_DIAG_BUILD) {
            CtxOptions o;
            int64_t v = 5;
            CHECK(!r && opt_set(&o, w.name, 1) == OPT_UNKNOWN && opt_get(o, w.name, &v) == OPT_UNKNOWN && v == 5, "%s in the product", w.name);
            continue;
        }
        CHECK(r && r->diag == w.diag, "row %s", w.name);
        if (!r) continue;
        known.insert(w.name);
        CHECK(get(fresh, w.name) == w.dflt, "default of %s: %lld, expected %lld", w.name, static_cast<ll>(get(fresh, w.name)), static_cast<ll>(w.dflt));
    }
    size_t seen = 0;
    for (const Range &g : RANGES) {
        if (!known.count(g.name)) continue;
        ++seen;
        const OptRow *r = opt_find(g.name);
        CHECK(r->lo == g.lo && r->hi == g.hi && r->norm == OPT_AS_GIVEN, "%s: %lld .. %lld", g.name, static_cast<ll>(r->lo), static_cast<ll>(r->hi));
        accepted(g.name, g.lo, g.lo);
        accepted(g.name, g.hi, g.hi);
        if (g.lo > INT64_MIN) refused(g.name, g.lo - 1, g.lo);
        if (g.hi < INT64_MAX) refused(g.name, g.hi + 1, g.hi);
        if (g.lo > INT64_MIN) refused(g.name, INT64_MIN, g.hi);
        if (g.hi < INT64_MAX) refused(g.name, INT64_MAX, g.lo);
    }
    for (const char *b : BOOLS) {
        if (!known.count(b)) continue;
        ++seen;
        CHECK(opt_find(b)->norm == OPT_BOOL, "%s is no bool", b);
        accepted(b, 0, 0);
        accepted(b, 1, 1);
        accepted(b, -1, 1);
        accepted(b, int64_t(1) << 40, 1);
    }
    // the sets: every member, and what stands next to it
    for (int64_t v : {256, 512, 1024}) { accepted("spine_nt", v, v); refused("spine_nt", v - 1, v); refused("spine_nt", v + 1, v); }
    for (int64_t v : {256, 512}) { accepted("tree_nt", v, v); refused("tree_nt", v - 1, v); refused("tree_nt", v + 1, v); }
    refused("spine_nt", 768, 512); refused("spine_nt", 0, 512); refused("tree_nt", 1024, 256); refused("tree_nt", 384, 256);
    // 2^32 + 1 wrapped to 1 in an int: refused now
    for (const char *n : {"k0_admit", "bridge_single", "noise_k_ppm"}) refused(n, (int64_t(1) << 32) + 1, 7);
    // timing clamps and never refuses
    ++seen;
    CHECK(opt_find("timing")->norm == OPT_CLAMP, "timing clamps");
    accepted("timing", -5, 0); accepted("timing", 9, 2); accepted("timing", 0, 0); accepted("timing", 1, 1); accepted("timing", 2, 2);
    accepted("timing", INT64_MIN, 0); accepted("timing", INT64_MAX, 2);
    CHECK(seen == known.size(), "%zu rows checked of %zu", seen, known.size());
    // names the table does not have
    CtxOptions o;
    int64_t v = 5;
    const OptRow *row = &OPT_ROWS[0];
    CHECK(opt_set(&o, "no_such_option", 1, &row) == OPT_UNKNOWN && !row && opt_set(&o, "", 1) == OPT_UNKNOWN && opt_set(&o, nullptr, 1) == OPT_UNKNOWN, "unknown names");
    CHECK(opt_get(o, "no_such_option", &v) == OPT_UNKNOWN && opt_get(o, "", &v) == OPT_UNKNOWN && v == 5 && opt_set(&o, "Mode", 1) == OPT_UNKNOWN &&
          opt_set(&o, "mode ", 1) == OPT_UNKNOWN && opt_set(&o, "PORESEG_MODE", 1) == OPT_UNKNOWN, "unknown names");
    CHECK(same(o, fresh), "a refused name changed the options");
    // the side effects are on these rows and no other
    const std::map<std::string, OptEffect> fx = {{"shared_device", FX_SHARED_DEVICE}, {"short_chain", FX_SHORT_CHAIN}, {"bridge_patience", FX_BRIDGE_PATIENCE},
                                                 {"wide_bs", FX_WIDE_BS}, {"k0_unaligned", FX_K0_UNALIGNED}, {"cu_mask", FX_CU_MASK}};
    for (const OptRow &r : OPT_ROWS) CHECK(r.effect == (fx.count(r.name) ? fx.at(r.name) : FX_NONE), "effect of %s", r.name);
}

static void check_mappings()
{
    const int bits[4] = {0, SC_ALL, SC_NO_LA, SC_NO_UPLOAD};
    for (int v = 0; v < 4; ++v) CHECK(opt_short_chain_bits(v) == bits[v] && opt_short_chain_of_bits(bits[v]) == v, "short_chain %d", v);
    CHECK(SC_NO_LA == 1 && SC_NO_UPLOAD == 2 && SC_ALL == (SC_NO_LA | SC_NO_UPLOAD) && opt_short_chain_of_bits(4) == -1, "short_chain bits");
    CHECK(opt_short_chain_bits(CtxOptions().short_chain) == SC_ALL, "short_chain by default");
    const float tenth = opt_noise_k(100000), zero = opt_noise_k(0), lit = 0.1f, z = 0.0f;
    CHECK(!std::memcmp(&tenth, &lit, sizeof lit) && !std::memcmp(&zero, &z, sizeof z), "noise_k: %a, %a", static_cast<double>(tenth), static_cast<double>(zero));
    CHECK(opt_noise_k(CtxOptions().noise_k_ppm) == 0.1f && opt_noise_k(250000) == 0.25f, "noise_k");
}

// A getenv that has every variable of the table: good values, bad values, or what `over` says for single ones.
struct FakeEnv {
    bool good = true, all = true;
    std::map<std::string, std::string> over;
    std::map<std::string, std::string> text;      // (keeps what it handed out alive)
    const char *operator()(const char *var)
    {
        if (over.count(var)) return over[var].c_str();
        if (!all) return nullptr;
        for (const OptRow &r : OPT_ROWS) {
            if (!r.env || std::strcmp(r.env, var)) continue;
            std::string &t = text[var];
            if (r.env_text == ENV_MILLIONTHS) t = good ? "0.25" : "-0.5";
            else if (r.norm != OPT_AS_GIVEN) t = good ? "7" : "seven";        // (a bool or timing takes any NUMBER)
            else t = std::to_string(good ? r.hi : r.hi + 1);
            return t.c_str();
        }
        return nullptr;
    }
};

static void check_env()
{
    size_t with_var = 0;
    for (const OptRow &r : OPT_ROWS) with_var += r.env && (OPT_DIAG_BUILD || !r.diag);
    {
        CtxOptions o;
        FakeEnv env;
        const std::vector<const char *> bad = opt_apply_env(&o, env);
        CHECK(bad.empty(), "%zu good variables refused, first %s", bad.size(), bad.empty() ? "" : bad[0]);
        for (const OptRow &r : OPT_ROWS) {
            if (!r.env || (r.diag && !OPT_DIAG_BUILD)) continue;
            const int64_t want = r.env_text == ENV_MILLIONTHS ? 250000 : r.norm == OPT_BOOL ? 1 : r.norm == OPT_CLAMP ? r.hi : r.hi;
            CHECK(get(o, r.name) == want, "%s=... gave %s %lld", r.env, r.name, static_cast<ll>(get(o, r.name)));
        }
        CHECK(o.noise_k_ppm == 250000 && o.shared_device == 0 && o.hw_queues == 0 && o.range_tile == CtxOptions().range_tile, "options without a variable");
        if (!OPT_DIAG_BUILD) CHECK(o.dbg_phase == 0 && o.k0_sets == 2 && o.rep_eval == 1 && o.scan_lds_pad == 0, "the product read a diagnostic variable");
    }
    {
        CtxOptions o;
        const CtxOptions fresh;
        FakeEnv env;
        env.good = false;
        const std::vector<const char *> bad = opt_apply_env(&o, env);
        std::set<std::string> got(bad.begin(), bad.end());
        CHECK(got.size() == bad.size() && bad.size() == with_var, "%zu refused of %zu", bad.size(), with_var);
        for (const OptRow &r : OPT_ROWS)
            if (r.env && (OPT_DIAG_BUILD || !r.diag)) CHECK(got.count(r.name) == 1, "%s not among the refused", r.name);
        CHECK(same(o, fresh), "a refused variable changed the options");
    }
    {
        // absent and empty variables; exactly the bad ones are named; text around a number
        CtxOptions o;
        const CtxOptions fresh;
        FakeEnv env;
        env.all = false;
        CHECK(opt_apply_env(&o, env).empty() && same(o, fresh), "no variables");
        env.over = {{"PORESEG_MODE", ""}, {"PORESEG_DEBUG", ""}, {"PORESEG_NOISE_K", ""}};
        CHECK(opt_apply_env(&o, env).empty() && same(o, fresh), "empty variables");
        env.over = {{"PORESEG_MODE", "3"}, {"PORESEG_K0_WAVES", "17"}, {"PORESEG_TREE_NT", "512"}, {"PORESEG_LAT_HELP", " 2 "}, {"PORESEG_SLOTS_PCT", "50%"},
                    {"PORESEG_TIMING", "9"}, {"PORESEG_PRUNE", "-1"}, {"PORESEG_NOISE_K", "nan"}, {"PORESEG_BRIDGE_BUDGET", "1e2"},
                    {"PORESEG_K0_MAX", "99999999999999999999"}, {"PORESEG_SHARED_DEVICE", "4"}, {"PORESEG_TILE", "x"}};
        const std::vector<const char *> bad = opt_apply_env(&o, env);
        const std::set<std::string> got(bad.begin(), bad.end()), want = {"mode", "k0_waves", "slots_pct", "noise_k_ppm", "bridge_budget", "k0_admit"};
        CHECK(got == want && bad.size() == want.size(), "%zu refused", bad.size());
        CHECK(o.mode == 0 && o.k0_waves == 0 && o.tree_nt == 512 && o.lat_help == 2 && o.slots_pct == 100 && o.timing == 2 && o.prune == 1 &&
              o.noise_k_ppm == 100000 && o.bridge_budget == 256 && o.k0_admit == 0 && o.shared_device == 0, "what the mixed variables left");
        env.over = {{"PORESEG_NOISE_K", "0.25"}};
        CHECK(opt_apply_env(&o, env).empty() && o.noise_k_ppm == 250000, "PORESEG_NOISE_K=0.25: %d", o.noise_k_ppm);
        env.over = {{"PORESEG_NOISE_K", "1e300"}};
        CHECK(opt_apply_env(&o, env).size() == 1 && o.noise_k_ppm == 250000, "PORESEG_NOISE_K=1e300");
        env.over = {{"PORESEG_NOISE_K", "inf"}};
        CHECK(opt_apply_env(&o, env).size() == 1 && o.noise_k_ppm == 250000, "PORESEG_NOISE_K=inf");
    }
}

static void print_table()
{
    const CtxOptions fresh;
    for (const OptRow &r : OPT_ROWS)
        std::printf("%s %s %lld %lld %lld %d %s\n", r.name, r.env ? r.env : "-", static_cast<ll>(r.lo), static_cast<ll>(r.hi), static_cast<ll>(r.read(fresh)),
                    r.diag ? 1 : 0, r.norm == OPT_BOOL ? "bool" : r.norm == OPT_CLAMP ? "clamp" : "given");
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "table")) { print_table(); return 0; }
    check_rows();
    check_mappings();
    check_env();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ctx options ok (%s)\n", OPT_DIAG_BUILD ? "diagnostic" : "product");
    return 0;
}
