// Stand-alone check of pypore_amd/csrc/hmm_plan.hpp (the host's planning of the ps_hmm_* entry points): host code only, no
// GPU, no HIP.  tests/test_hmm_plan_host.py builds it plain and with -fsanitize=address,undefined and runs both.  Every model
// lives in exactly sized heap arrays, so that one element read too many is the address sanitizer's finding.
//   hmm_plan_check                         every check below; exit status 0 when all hold
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "hmm_plan.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) { ++failures; std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

typedef long long ll;
static const double INF = std::numeric_limits<double>::infinity();

// ---- models in exactly sized heap arrays ---------------------------------------------------------------------------------------

struct Edge { int src, dst; };

// What a model is made from.  Values are told apart by table and index, so a table read through a pointer into another one
// cannot compare equal.
struct Spec {
    std::vector<int32_t> kind;                  // emitting states first
    std::vector<int32_t> level_ptr;
    std::vector<Edge> edges;
    int start = 0, end = 0, finite = 1, n_dim = 0, points = 2, comps = 2;
};

static double value(int table, size_t i) { return table * 1000.0 + static_cast<double>(i) + 0.5; }

template <typename T> static T *exact(const std::vector<T> &v)
{
    if (v.empty()) return nullptr;
    T *p = static_cast<T *>(std::malloc(v.size() * sizeof(T)));
    std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Built {
    ps_hmm_model m;
    ps_hmm_sample_tables t;
    int32_t *kind, *level_ptr, *in_ptr, *in_src, *out_ptr, *out_dst, *kde_ptr, *comp_kind, *mix_ptr, *mix_kind;
    double *param, *in_lp, *out_lp, *kde_pt, *kde_lw, *comp_param, *comp_w, *mix_param, *mix_lw, *mix_cdf, *mix_draw;
    double *out_cdf, *emit_param, *kde_cdf;
    int S, NE, E;
    Built(const Built &) = delete;
    Built &operator=(const Built &) = delete;

    // a row of a cdf table: n entries ascending to exactly 1.0
    static void cdf_rows(const std::vector<int32_t> &ptr, std::vector<double> *cdf)
    {
        cdf->assign(static_cast<size_t>(ptr.back()), 0.0);
        for (size_t k = 0; k + 1 < ptr.size(); ++k)
            for (int i = ptr[k]; i < ptr[k + 1]; ++i) (*cdf)[i] = static_cast<double>(i - ptr[k] + 1) / (ptr[k + 1] - ptr[k]);
    }

    explicit Built(const Spec &s)
    {
        S = static_cast<int>(s.kind.size());
        NE = 0;
        bool kde = false, vec = false, mix = false;
        for (int k : s.kind) { NE += k != HMM_SILENT; kde |= k == HMM_KDE; vec |= k == HMM_VECTOR; mix |= k == HMM_MIXTURE; }
        E = static_cast<int>(s.edges.size());
        std::vector<int32_t> inp(S + 1, 0), outp(S + 1, 0), src(E), dst(E);
        std::vector<double> ilp(E), olp(E);
        for (const Edge &e : s.edges) { ++inp[e.dst + 1]; ++outp[e.src + 1]; }
        for (int k = 0; k < S; ++k) { inp[k + 1] += inp[k]; outp[k + 1] += outp[k]; }
        std::vector<int32_t> ifill(inp.begin(), inp.end() - 1), ofill(outp.begin(), outp.end() - 1);
        for (int e = 0; e < E; ++e) {
            const int i = ifill[s.edges[e].dst]++, o = ofill[s.edges[e].src]++;
            src[i] = s.edges[e].src; ilp[i] = -value(1, e);
            dst[o] = s.edges[e].dst; olp[o] = -value(2, e);
        }
        std::vector<double> par(3 * static_cast<size_t>(S));
        for (size_t i = 0; i < par.size(); ++i) par[i] = value(0, i);
        std::vector<int32_t> kptr, ckind, mptr, mkind;
        std::vector<double> kpt, klw, cpar, cw, mpar, mlw, mcdf, mdraw, kcdf;
        if (kde) {
            kptr.assign(1, 0);
            for (int k = 0; k < NE; ++k) kptr.push_back(kptr.back() + (s.kind[k] == HMM_KDE ? s.points : 0));
            for (int i = 0; i < kptr.back(); ++i) { kpt.push_back(value(3, i)); klw.push_back(-value(4, i)); }
            cdf_rows(kptr, &kcdf);
        }
        if (vec) {
            const int kinds[4] = {HMM_NORMAL, HMM_UNIFORM, HMM_LOGNORMAL, HMM_EXPONENTIAL};
            for (int i = 0; i < NE * s.n_dim; ++i) { ckind.push_back(kinds[i & 3]); cw.push_back(value(6, i)); }
            for (int i = 0; i < 3 * NE * s.n_dim; ++i) cpar.push_back(value(5, i));
        }
        if (mix) {
            mptr.assign(1, 0);
            for (int k = 0; k < NE; ++k) mptr.push_back(mptr.back() + (s.kind[k] == HMM_MIXTURE ? s.comps : 0));
            for (int i = 0; i < mptr.back(); ++i) { mkind.push_back(i & 1 ? HMM_LOGNORMAL : HMM_NORMAL); mlw.push_back(-value(8, i)); }
            for (int i = 0; i < 3 * mptr.back(); ++i) mpar.push_back(value(7, i));
            for (int i = 0; i < 2 * mptr.back(); ++i) mdraw.push_back(value(9, i));
            cdf_rows(mptr, &mcdf);
        }
        std::vector<double> ocdf, epar(2 * static_cast<size_t>(NE) * (vec ? s.n_dim : 1));
        cdf_rows(outp, &ocdf);
        for (size_t i = 0; i < epar.size(); ++i) epar[i] = value(10, i);
        kind = exact(s.kind); level_ptr = exact(s.level_ptr); in_ptr = exact(inp); in_src = exact(src); out_ptr = exact(outp); out_dst = exact(dst);
        param = exact(par); in_lp = exact(ilp); out_lp = exact(olp);
        kde_ptr = exact(kptr); kde_pt = exact(kpt); kde_lw = exact(klw);
        comp_kind = exact(ckind); comp_param = exact(cpar); comp_w = exact(cw);
        mix_ptr = exact(mptr); mix_kind = exact(mkind); mix_param = exact(mpar); mix_lw = exact(mlw); mix_cdf = exact(mcdf); mix_draw = exact(mdraw);
        out_cdf = exact(ocdf); emit_param = exact(epar); kde_cdf = exact(kcdf);
        m = ps_hmm_model{S, NE, static_cast<int32_t>(s.level_ptr.size()) - 1, s.start, s.end, s.finite, kind, level_ptr, in_ptr, in_src, out_ptr,
                         out_dst, param, in_lp, out_lp, kde_ptr, kde_pt, kde_lw, s.n_dim, comp_kind, comp_param, comp_w, mix_ptr, mix_kind,
                         mix_param, mix_lw, mix_cdf, mix_draw};
        t = ps_hmm_sample_tables{out_cdf, emit_param, kde_cdf, E, static_cast<int64_t>(epar.size()), static_cast<int64_t>(kcdf.size())};
    }
    ~Built()
    {
        void *all[] = {kind, level_ptr, in_ptr, in_src, out_ptr, out_dst, kde_ptr, comp_kind, mix_ptr, mix_kind, param, in_lp, out_lp, kde_pt,
                       kde_lw, comp_param, comp_w, mix_param, mix_lw, mix_cdf, mix_draw, out_cdf, emit_param, kde_cdf};
        for (void *p : all) std::free(p);
    }
};

// Two emitting states of the kinds given, then start (level 0) and end (level 1): 4 states, 7 edges, one of them silent
static Spec small(int k0, int k1, int n_dim = 0)
{
    Spec s;
    s.kind = {k0, k1, HMM_SILENT, HMM_SILENT};
    s.level_ptr = {2, 3, 4};
    s.edges = {{0, 0}, {0, 1}, {0, 3}, {1, 3}, {2, 0}, {2, 1}, {2, 3}};
    s.start = 2; s.end = 3; s.n_dim = n_dim;
    return s;
}

// ---- the round trip ------------------------------------------------------------------------------------------------------------

template <typename A, typename B> static bool same(const A *got, const B *want, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(got[i] == want[i])) return false;
    return true;
}

static void round_trip(const char *name, const Built &b)
{
    const ps_hmm_model &m = b.m;
    HmmModelInfo I;
    std::string why;
    const bool ok = hmm_model_check(&m, &I, &why);
    CHECK(ok && why.empty(), "%s: refused: %s", name, why.c_str());
    if (!ok) return;
    const size_t S = static_cast<size_t>(m.n_states), NE = static_cast<size_t>(m.n_emit), NL = static_cast<size_t>(m.n_levels), E = static_cast<size_t>(b.E);
    CHECK(I.S == m.n_states && I.NE == m.n_emit && I.NL == m.n_levels && I.E == b.E, "%s: counts", name);
    int max_in = 0;
    for (size_t k = 0; k < S; ++k) max_in = std::max(max_in, m.in_ptr[k + 1] - m.in_ptr[k]);
    CHECK(I.max_in == max_in, "%s: max_in %d, expected %d", name, I.max_in, max_in);
    CHECK(I.kde == (b.kde_ptr != nullptr) && I.vec == (b.comp_kind != nullptr) && I.mix == (b.mix_ptr != nullptr), "%s: flags", name);
    const size_t NP = I.kde ? static_cast<size_t>(m.kde_ptr[NE]) : 0, NC = I.vec ? NE * m.n_dim : 0, NM = I.mix ? static_cast<size_t>(m.mix_ptr[NE]) : 0;
    CHECK(static_cast<size_t>(I.NP) == NP && static_cast<size_t>(I.NC) == NC && static_cast<size_t>(I.n_mix) == NM, "%s: table counts", name);
    CHECK(I.dim() == (I.vec ? m.n_dim : 1) && I.n_stats() == static_cast<ll>((1 + 2 * I.dim()) * NE + 3 * NM) && I.n_acc() == static_cast<ll>(E) + I.n_stats() + 1,
          "%s: derived sizes", name);

    // the layout: the tables in their order, disjoint and without a gap, the doubles first and aligned, the total the sum of the parts
    const HmmBlobLayout L = hmm_blob_layout(I);
    size_t at = 0;
    for (int t = 0; t < HMM_T_COUNT; ++t) {
        CHECK(L.byte_off(t) == at, "%s: table %d at byte %zu, expected %zu", name, t, L.byte_off(t), at);
        CHECK(L.byte_off(t) % HmmBlobLayout::width(t) == 0, "%s: table %d misaligned", name, t);
        CHECK(HmmBlobLayout::width(t) == (t < HMM_T_INT ? 8u : 4u), "%s: width of table %d", name, t);
        at += L.n[t] * HmmBlobLayout::width(t);
        if (t == HMM_T_INT - 1) CHECK(at == L.nd * 8, "%s: %zu bytes of doubles, nd %zu", name, at, L.nd);
    }
    CHECK(at == L.bytes && L.bytes == L.nd * 8 + L.ni * 4, "%s: %zu bytes, the parts add up to %zu", name, L.bytes, at);
    // the blob as it was before the layout was written once: the same sums, spelled out
    const size_t nd0 = 3 * S + 2 * E, nd1 = nd0 + 2 * NP + 4 * NC, nd = nd1 + 4 * NM;
    const size_t ni0 = S + (NL + 1) + 2 * (S + 1) + 2 * E + 3, ni1 = ni0 + (I.kde ? NE + 1 : 0) + (I.vec ? NC + 1 : 0), ni = ni1 + (I.mix ? NE + 1 + NM : 0);
    CHECK(L.nd == nd && L.ni == ni, "%s: %zu doubles and %zu ints, expected %zu and %zu", name, L.nd, L.ni, nd, ni);
    CHECK(L.off[HMM_T_IN_LP] == 3 * S && L.off[HMM_T_OUT_LP] == 3 * S + E && L.off[HMM_T_MIX_PARAM] == nd1 && L.off[HMM_T_MIX_LW] == nd1 + 3 * NM,
          "%s: offsets of the doubles", name);
    if (I.kde) CHECK(L.off[HMM_T_KDE_PT] == nd0 && L.off[HMM_T_KDE_LW] == nd0 + NP && L.off[HMM_T_KDE_PTR] == ni0, "%s: offsets of the kde tables", name);
    if (I.vec) CHECK(L.off[HMM_T_COMP_PARAM] == nd0 && L.off[HMM_T_COMP_W] == nd0 + 3 * NC && L.off[HMM_T_COMP_KIND] == ni0 && L.off[HMM_T_N_DIM] == ni0 + NC,
                     "%s: offsets of the component tables", name);
    CHECK(L.off[HMM_T_LEVEL_PTR] == S && L.off[HMM_T_IN_PTR] == S + NL + 1 && L.off[HMM_T_OUT_PTR] == 2 * S + NL + 2 && L.off[HMM_T_IN_SRC] == 3 * S + NL + 3 &&
          L.off[HMM_T_OUT_DST] == 3 * S + NL + 3 + E && L.off[HMM_T_TAIL] == ni0 - 3 && L.off[HMM_T_MIX_PTR] == ni1 && L.off[HMM_T_MIX_KIND] == ni1 + (I.mix ? NE + 1 : 0),
          "%s: offsets of the ints", name);

    std::vector<char> blob, again(7, 'x');
    hmm_blob_pack(&m, L, &blob);
    hmm_blob_pack(&m, L, &again);
    CHECK(blob.size() == L.bytes && blob == again, "%s: packing twice", name);

    // every table through the structs the kernels get, aimed at the host blob
    HmmDevK K; HmmDevV V; HmmDevM M;
    hmm_blob_resolve(blob.data(), L, I, &K, &V, &M);
    const HmmDev *devs[3] = {&K, &V, &M};
    const std::vector<double> zeros(3 * S, 0.0);
    for (const HmmDev *D : devs) {
        CHECK(same(D->param, I.vec ? zeros.data() : m.param, 3 * S), "%s: param", name);
        CHECK(same(D->in_lp, m.in_lp, E) && same(D->out_lp, m.out_lp, E), "%s: edge log probabilities", name);
        CHECK(same(D->kind, m.kind, S) && same(D->level_ptr, m.level_ptr, NL + 1), "%s: kind, level_ptr", name);
        CHECK(same(D->in_ptr, m.in_ptr, S + 1) && same(D->out_ptr, m.out_ptr, S + 1), "%s: edge offsets", name);
        CHECK(same(D->in_src, m.in_src, E) && same(D->out_dst, m.out_dst, E), "%s: edge ends", name);
        CHECK(D->S == m.n_states && D->n_emit == m.n_emit && D->n_levels == m.n_levels && D->start == m.start && D->end == m.end &&
              D->finite == (m.finite != 0), "%s: scalars", name);
        CHECK(D->out_dst[E] == m.start && D->out_dst[E + 1] == m.end && D->out_dst[E + 2] == m.finite, "%s: start, end, finite behind out_dst", name);
    }
    const HmmDevK *ks[2] = {&K, &M};
    for (const HmmDevK *D : ks) {
        if (I.kde) CHECK(same(D->kde_ptr, m.kde_ptr, NE + 1) && same(D->kde_pt, m.kde_pt, NP) && same(D->kde_lw, m.kde_lw, NP), "%s: kde tables", name);
        else CHECK(!D->kde_ptr && !D->kde_pt && !D->kde_lw, "%s: kde tables of a model without any", name);
    }
    if (I.vec) CHECK(same(V.comp_kind, m.comp_kind, NC) && same(V.comp_param, m.comp_param, 3 * NC) && same(V.comp_w, m.comp_w, NC) &&
                     V.D == m.n_dim && V.comp_kind[NC] == m.n_dim, "%s: component tables", name);
    else CHECK(!V.comp_kind && !V.comp_param && !V.comp_w && V.D == 1, "%s: component tables of a model without any", name);
    if (I.mix) CHECK(same(M.mix_ptr, m.mix_ptr, NE + 1) && same(M.mix_kind, m.mix_kind, NM) && same(M.mix_param, m.mix_param, 3 * NM) &&
                     same(M.mix_lw, m.mix_lw, NM), "%s: mixture tables", name);
    else CHECK(!M.mix_ptr && !M.mix_kind && !M.mix_param && !M.mix_lw, "%s: mixture tables of a model without any", name);
    CHECK(!M.mix_cdf && !M.mix_draw, "%s: the sampling tables are ps_hmm_sample's", name);

    // the sampling tables and their upload: accepted, staged back to back as the entry point does, read back through the pointers
    const bool ok_s = hmm_sample_check(&m, &b.t, I, 3, 100, &why);
    CHECK(ok_s && why.empty(), "%s: sampling refused: %s", name, why.c_str());
    const int64_t h_off[3] = {0, 4, 9}, h_path_off[3] = {0, 10, 30};
    for (int paths = 0; paths < 2; ++paths) {
        const HmmSampleLayout U = hmm_sample_layout(&m, &b.t, I, h_off, paths ? h_path_off : nullptr, 2);
        std::vector<char> up(U.total + 8, 'y');
        size_t pos = 0;
        for (int t = 0; t < HMM_U_COUNT; ++t) {
            CHECK(U.off[t] == pos && U.bytes[t] % 8 == 0, "%s: upload table %d at %zu, expected %zu", name, t, U.off[t], pos);
            if (U.bytes[t]) std::memcpy(up.data() + pos, U.src[t], U.bytes[t]);
            pos += U.bytes[t];
        }
        CHECK(pos == U.total, "%s: upload of %zu bytes, the parts add up to %zu", name, U.total, pos);
        HmmSampleDev T;
        const long long *off = nullptr, *path_off = nullptr;
        hmm_sample_resolve(up.data(), U, &T, &M, &off, &path_off);
        CHECK(same(T.out_cdf, b.out_cdf, E) && same(T.emit_param, b.emit_param, 2 * NE * I.dim()) && same(T.kde_cdf, b.kde_cdf, NP), "%s: sampling tables", name);
        CHECK(same(M.mix_cdf, b.mix_cdf, NM) && same(M.mix_draw, b.mix_draw, 2 * NM), "%s: mixture sampling tables", name);
        CHECK(same(off, h_off, 3) && (paths ? same(path_off, h_path_off, 3) : !path_off), "%s: offsets of the upload", name);
        CHECK(reinterpret_cast<const char *>(off + 3 + (paths ? 3 : 0)) == up.data() + U.total, "%s: end of the upload", name);
    }
}

static std::vector<char> packed(const char *name, const ps_hmm_model &m)
{
    HmmModelInfo I;
    std::string why;
    std::vector<char> blob;
    const bool ok = hmm_model_check(&m, &I, &why);
    CHECK(ok, "%s: refused: %s", name, why.c_str());
    if (ok) hmm_blob_pack(&m, hmm_blob_layout(I), &blob);
    return blob;
}

// changing one value of the model changes the blob, whichever it is
static void blob_identity()
{
    Built a(small(HMM_MIXTURE, HMM_KDE)), v(small(HMM_VECTOR, HMM_VECTOR, 3));
    const std::vector<char> base_a = packed("identity", a.m), base_v = packed("identity (vector)", v.m);
    CHECK(base_a == packed("identity", a.m), "the same model, the same blob");
    struct Change { const char *what; bool vector; std::function<void(Built &)> apply; };
    const Change changes[] = {
        {"a parameter", false, [](Built &b) { b.param[4] += 1.0; }},
        {"an in-edge probability", false, [](Built &b) { b.in_lp[b.E - 1] -= 1.0; }},
        {"an out-edge probability", false, [](Built &b) { b.out_lp[0] -= 1.0; }},
        {"a mixture weight", false, [](Built &b) { b.mix_lw[1] -= 1.0; }},
        {"a mixture parameter", false, [](Built &b) { b.mix_param[5] += 1.0; }},
        {"a mixture component's kind", false, [](Built &b) { b.mix_kind[0] = HMM_EXPONENTIAL; }},
        {"a kde point", false, [](Built &b) { b.kde_pt[1] += 1.0; }},
        {"a kde weight", false, [](Built &b) { b.kde_lw[0] -= 1.0; }},
        {"finite", false, [](Built &b) { b.m.finite = 0; }},
        {"start", false, [](Built &b) { b.m.start = 3; }},
        {"end", false, [](Built &b) { b.m.end = 2; }},
        {"a component's weight", true, [](Built &b) { b.comp_w[5] += 1.0; }},
        {"a component's parameter", true, [](Built &b) { b.comp_param[17] += 1.0; }},
        {"a component's kind", true, [](Built &b) { b.comp_kind[2] = HMM_NORMAL; }},
        {"n_dim", true, [](Built &b) { b.m.n_dim = 2; }},
    };
    for (const Change &c : changes) {
        Built changed(c.vector ? small(HMM_VECTOR, HMM_VECTOR, 3) : small(HMM_MIXTURE, HMM_KDE));
        c.apply(changed);
        CHECK(packed(c.what, changed.m) != (c.vector ? base_v : base_a), "%s changed, the blob did not", c.what);
    }
}

// ---- refusals --------------------------------------------------------------------------------------------------------------------

static void refused(const char *name, const ps_hmm_model &m, const std::string &text)
{
    HmmModelInfo I;
    std::string why;
    const bool ok = hmm_model_check(&m, &I, &why);
    CHECK(!ok && why == text, "%s: %s \"%s\", expected \"%s\"", name, ok ? "accepted" : "refused with", why.c_str(), text.c_str());
}
static void refused(const char *name, const Spec &s, const std::function<void(Built &)> &change, const std::string &text)
{
    Built b(s);
    change(b);
    refused(name, b.m, text);
}

static void model_refusals()
{
    const Spec plain = small(HMM_NORMAL, HMM_UNIFORM), kde = small(HMM_KDE, HMM_NORMAL), vec = small(HMM_VECTOR, HMM_VECTOR, 2),
               mix = small(HMM_MIXTURE, HMM_NORMAL);
    // hostile counts: nothing is read of a model whose counts are wrong -- its arrays are not even there
    ps_hmm_model none;
    std::memset(&none, 0, sizeof none);
    for (int S : {0, -1, INT32_MIN, HMM_S_MAX + 1, INT32_MAX}) {
        none.n_states = S;
        refused("states", none, "model of " + std::to_string(S) + " states: the device HMM kernels take 1..4096");
    }
    none.n_states = 4;
    const int counts[][2] = {{5, 0}, {-1, 1}, {INT32_MAX, 1}, {2, -1}, {2, 3}, {2, INT32_MAX}, {2, 0}, {4, 1}};
    for (const int *c : counts) { none.n_emit = c[0]; none.n_levels = c[1]; refused("state / level counts", none, "bad state / level counts"); }
    none.n_emit = 2; none.n_levels = 2;
    const int ends[][2] = {{1, 3}, {4, 3}, {2, 0}, {2, INT32_MAX}, {-1, 3}};
    for (const int *c : ends) { none.start = c[0]; none.end = c[1]; refused("start / end", none, "start and end must be silent states"); }
    none.start = 2; none.end = 3;
    refused("no arrays", none, "null model array");

    refused("kind", plain, [](Built &b) { b.m.kind = nullptr; }, "null model array");
    refused("param", plain, [](Built &b) { b.m.param = nullptr; }, "null model array");
    refused("silent state among the emitting", plain, [](Built &b) { b.kind[1] = HMM_SILENT; }, "state 1: emitting states first, then silent ones");
    refused("emitting state among the silent", plain, [](Built &b) { b.kind[3] = HMM_NORMAL; }, "state 3: emitting states first, then silent ones");
    refused("unknown kind", plain, [](Built &b) { b.kind[0] = 8; }, "state 0: emitting states first, then silent ones");
    // a vector model
    for (int other : {HMM_NORMAL, HMM_UNIFORM, HMM_KDE, HMM_MIXTURE})
        refused("kind 4 beside another", vec, [&](Built &b) { b.kind[1] = other; },
                "a vector model's emitting states are all kind 4: kinds 1..3 cannot be mixed with it");
    refused("n_dim 0", vec, [](Built &b) { b.m.n_dim = 0; }, "n_dim 0: a vector model takes 1..16 components");
    refused("n_dim 17", vec, [](Built &b) { b.m.n_dim = 17; }, "n_dim 17: a vector model takes 1..16 components");
    refused("comp_w", vec, [](Built &b) { b.m.comp_w = nullptr; }, "a vector model needs comp_kind, comp_param and comp_w");
    refused("component kind", vec, [](Built &b) { b.comp_kind[3] = HMM_KDE; }, "component 3: unknown component kind 3");
    refused("component weight 0", vec, [](Built &b) { b.comp_w[2] = 0.0; }, "component 2: a weight must be finite and > 0");
    refused("component weight inf", vec, [](Built &b) { b.comp_w[1] = INF; }, "component 1: a weight must be finite and > 0");
    refused("a vector model's param is not read", vec, [](Built &b) { b.m.param = nullptr; b.in_ptr[0] = 1; }, "edge lists must start at 0");
    // kernel-density states
    refused("kde_pt", kde, [](Built &b) { b.m.kde_pt = nullptr; }, "a kernel-density state needs kde_ptr, kde_pt and kde_lw");
    refused("kde_ptr[0]", kde, [](Built &b) { b.kde_ptr[0] = 1; }, "kde_ptr must start at 0");
    refused("negative kde_ptr step", kde, [](Built &b) { b.kde_ptr[2] = -5; }, "descending kde_ptr at state 1");
    refused("INT32_MIN kde_ptr step", kde, [](Built &b) { b.kde_ptr[1] = INT32_MIN; }, "descending kde_ptr at state 0");
    refused("kde state without a point", kde, [](Built &b) { b.kde_ptr[1] = 0; },
            "state 0: a kernel-density state has at least one point, any other state none");
    refused("normal state with points", kde, [](Built &b) { b.kde_ptr[2] = 3; },
            "state 1: a kernel-density state has at least one point, any other state none");
    refused("too many kde points", kde, [](Built &b) { b.kde_ptr[1] = b.kde_ptr[2] = INT32_MAX; },
            "2147483647 kernel-density points: the device HMM kernels take at most 16777216");
    refused("kde point nan", kde, [](Built &b) { b.kde_pt[1] = NAN; }, "kernel-density point 1: points must be finite and log weights <= 0");
    refused("kde weight > 0", kde, [](Built &b) { b.kde_lw[0] = 0.5; }, "kernel-density point 0: points must be finite and log weights <= 0");
    // mixture states
    refused("mix_kind", mix, [](Built &b) { b.m.mix_kind = nullptr; }, "a mixture state needs mix_ptr, mix_kind, mix_param and mix_lw");
    refused("mix_ptr[0]", mix, [](Built &b) { b.mix_ptr[0] = 1; }, "mix_ptr must start at 0");
    refused("descending mix_ptr", mix, [](Built &b) { b.mix_ptr[2] = 1; }, "descending mix_ptr at state 1");
    refused("mixture state without a component", mix, [](Built &b) { b.mix_ptr[1] = 0; },
            "state 0: a mixture state has at least one component, any other state none");
    refused("normal state with components", mix, [](Built &b) { b.mix_ptr[2] = 3; },
            "state 1: a mixture state has at least one component, any other state none");
    refused("too many components", mix, [](Built &b) { b.mix_ptr[1] = b.mix_ptr[2] = INT32_MAX; },
            "2147483647 mixture components: the device HMM kernels take at most 16777216");
    refused("mixture kind", mix, [](Built &b) { b.mix_kind[1] = HMM_MIXTURE; }, "mixture component 1: unknown component kind 7");
    refused("mixture weight nan", mix, [](Built &b) { b.mix_lw[0] = NAN; }, "mixture component 0: a log weight must be <= 0");
    // levels
    refused("level_ptr[0]", plain, [](Built &b) { b.level_ptr[0] = 1; }, "levels must cover the silent states");
    refused("level_ptr[NL]", plain, [](Built &b) { b.level_ptr[2] = INT32_MAX; }, "levels must cover the silent states");
    refused("empty level", plain, [](Built &b) { b.level_ptr[1] = 2; }, "empty or descending level 0");
    refused("INT32_MAX level", plain, [](Built &b) { b.level_ptr[1] = INT32_MAX; }, "empty or descending level 1");
    // edges
    refused("in_ptr[0]", plain, [](Built &b) { b.in_ptr[0] = 1; }, "edge lists must start at 0");
    refused("out_ptr[0]", plain, [](Built &b) { b.out_ptr[0] = -1; }, "edge lists must start at 0");
    refused("descending in_ptr", plain, [](Built &b) { b.in_ptr[2] = 1; }, "descending edge offsets");
    refused("descending out_ptr", plain, [](Built &b) { b.out_ptr[4] = INT32_MIN; }, "descending edge offsets");
    refused("in_src", plain, [](Built &b) { b.m.in_src = nullptr; }, "null edge array");
    refused("out_lp", plain, [](Built &b) { b.m.out_lp = nullptr; }, "null edge array");
    refused("edge from state S", plain, [](Built &b) { b.in_src[0] = 4; }, "edge to a state out of range");
    refused("edge to state -1", plain, [](Built &b) { b.out_dst[6] = -1; }, "edge to a state out of range");
    refused("silent edge down", plain, [](Built &b) { b.in_src[b.in_ptr[3] + 2] = 3; }, "silent edge 3 -> 3 does not go up a level");
    refused("silent edge down (out)", plain, [](Built &b) { b.out_dst[6] = 2; }, "silent edge 2 -> 2 does not go up a level");
    refused("edge lists of different length", plain, [](Built &b) { b.out_ptr[3] = b.out_ptr[4] = 6; }, "in- and out-edge lists differ in length");
    {
        Spec many = plain;                                  // 65 536 edges into state 1: 65 535 from state 0, one from start
        many.edges.insert(many.edges.begin() + 2, 65534, Edge{0, 1});
        Built b(many);
        refused("65536 in-edges", b.m, "a state with 65536 in-edges: the device HMM kernels take at most 65535");
        many.edges.erase(many.edges.begin() + 2);
        Built c(many);
        HmmModelInfo I;
        std::string why;
        CHECK(hmm_model_check(&c.m, &I, &why) && I.max_in == 65535 && hmm_bp_wide(I), "65535 in-edges: %s", why.c_str());
    }
    // a caller built against the struct as it was before kinds 3, 4 and 7: the fields behind out_lp are not read
    {
        Built b(plain);
        const size_t old_size = offsetof(ps_hmm_model, kde_ptr);
        ps_hmm_model *old = static_cast<ps_hmm_model *>(std::malloc(old_size));
        std::memcpy(static_cast<void *>(old), &b.m, old_size);
        ps_hmm_model *volatile as_given = old;
        CHECK(!packed("the shorter struct", *as_given).empty(), "the shorter struct");
        std::free(old);
    }
}

static void sample_refused(const char *name, const Spec &s, const std::function<void(Built &)> &change, int32_t length, int32_t max_length,
                           const std::string &text)
{
    Built b(s);
    HmmModelInfo I;
    std::string why;
    const bool model_ok = hmm_model_check(&b.m, &I, &why);
    CHECK(model_ok, "%s: the model is refused: %s", name, why.c_str());
    if (!model_ok) return;
    change(b);
    const bool ok = hmm_sample_check(&b.m, &b.t, I, length, max_length, &why);
    if (text.empty()) CHECK(ok && why.empty(), "%s: refused with \"%s\"", name, why.c_str());
    else CHECK(!ok && why == text, "%s: %s \"%s\", expected \"%s\"", name, ok ? "accepted" : "refused with", why.c_str(), text.c_str());
}

static void sample_refusals()
{
    const Spec plain = small(HMM_NORMAL, HMM_UNIFORM), kde = small(HMM_KDE, HMM_NORMAL), vec = small(HMM_VECTOR, HMM_VECTOR, 2),
               mix = small(HMM_MIXTURE, HMM_NORMAL);
    const auto nothing = [](Built &) {};
    sample_refused("no end, no length", plain, [](Built &b) { b.m.finite = 0; }, 0, 10,
                   "a model without an edge into end never ends a walk: a length must be given");
    sample_refused("no end, a length", plain, [](Built &b) { b.m.finite = 0; }, 1, 10, "");
    // the longest path there can be, (max_length + 1) (n_levels + 1) + 2, within int32
    const int NL = 2, largest = (INT32_MAX - 2) / (NL + 1) - 1;
    CHECK((largest + 1ll) * (NL + 1) + 2 <= INT32_MAX && INT32_MAX < (largest + 2ll) * (NL + 1) + 2, "largest %d", largest);
    sample_refused("max_length largest", plain, nothing, 0, largest, "");
    sample_refused("max_length largest + 1", plain, nothing, 0, largest + 1,
                   "max_length " + std::to_string(largest + 1) + " with 2 silent levels: a path could exceed int32");
    sample_refused("max_length INT32_MAX", plain, nothing, 0, INT32_MAX, "max_length 2147483647 with 2 silent levels: a path could exceed int32");
    sample_refused("mix_cdf", mix, [](Built &b) { b.m.mix_cdf = nullptr; }, 0, 10, "sampling a mixture state needs mix_cdf and mix_draw");
    sample_refused("mix_draw", mix, [](Built &b) { b.m.mix_draw = nullptr; }, 0, 10, "sampling a mixture state needs mix_cdf and mix_draw");
    sample_refused("n_cdf", plain, [](Built &b) { b.t.n_cdf = 6; }, 0, 10, "sampling tables of 6 / 4 / 0 entries, the model takes 7 / 4 / 0");
    sample_refused("n_param", vec, [](Built &b) { b.t.n_param = 4; }, 0, 10, "sampling tables of 7 / 4 / 0 entries, the model takes 7 / 8 / 0");
    sample_refused("n_kde", kde, [](Built &b) { b.t.n_kde = INT64_MAX; }, 0, 10,
                   "sampling tables of 7 / 4 / 9223372036854775807 entries, the model takes 7 / 4 / 2");
    sample_refused("out_cdf", plain, [](Built &b) { b.t.out_cdf = nullptr; }, 0, 10, "null sampling table");
    sample_refused("emit_param", plain, [](Built &b) { b.t.emit_param = nullptr; }, 0, 10, "null sampling table");
    sample_refused("kde_cdf", kde, [](Built &b) { b.t.kde_cdf = nullptr; }, 0, 10, "null sampling table");
    // the rows: state 0 has the out-edges 0, 1, 2 (cdf 1/3, 2/3, 1), state 2 the out-edges 4, 5, 6
    const std::string row0 = "out_cdf of state 0: ascending from >= 0 with the last entry 1.0", row2 = "out_cdf of state 2: ascending from >= 0 with the last entry 1.0";
    sample_refused("a row that descends", plain, [](Built &b) { b.out_cdf[1] = 0.25; }, 0, 10, row0);
    sample_refused("a row from below 0", plain, [](Built &b) { b.out_cdf[4] = -0.5; }, 0, 10, row2);
    sample_refused("a row with a nan", plain, [](Built &b) { b.out_cdf[0] = NAN; }, 0, 10, row0);
    sample_refused("a row with inf", plain, [](Built &b) { b.out_cdf[1] = INF; }, 0, 10, row0);
    sample_refused("a row that closes below 1.0", plain, [](Built &b) { b.out_cdf[6] = std::nextafter(1.0, 0.0); }, 0, 10, row2);
    sample_refused("a row that closes above 1.0", plain, [](Built &b) { b.out_cdf[2] = std::nextafter(1.0, 2.0); }, 0, 10, row0);
    sample_refused("a row that passes 1.0 by an ulp and steps back", plain,
                   [](Built &b) { b.out_cdf[0] = std::nextafter(1.0, 2.0); b.out_cdf[1] = 1.0; }, 0, 10, "");
    sample_refused("a row that passes 1.0 by an ulp before it closes", plain,
                   [](Built &b) { b.out_cdf[0] = 0.5; b.out_cdf[1] = std::nextafter(1.0, 2.0); }, 0, 10, "");
    sample_refused("a row that steps back to 1.0 from 1.0", plain, [](Built &b) { b.out_cdf[0] = b.out_cdf[1] = 1.0; }, 0, 10, "");
    sample_refused("a row that steps back below 1.0", plain,
                   [](Built &b) { b.out_cdf[4] = std::nextafter(1.0, 2.0); b.out_cdf[5] = std::nextafter(1.0, 0.0); }, 0, 10, row2);
    sample_refused("mass on a -inf edge", plain, [](Built &b) { b.out_lp[5] = -INF; }, 0, 10,
                   "out_cdf of state 2: entry 1 rises above its predecessor, its log probability is -inf");
    sample_refused("mass on a -inf first edge", plain, [](Built &b) { b.out_lp[0] = -INF; }, 0, 10,
                   "out_cdf of state 0: entry 0 rises above its predecessor, its log probability is -inf");
    sample_refused("no mass on a -inf edge", plain, [](Built &b) { b.out_lp[5] = -INF; b.out_cdf[5] = b.out_cdf[4]; }, 0, 10, "");
    sample_refused("a kde row from below 0", kde, [](Built &b) { b.kde_cdf[0] = -1.0; }, 0, 10,
                   "kde_cdf of state 0: ascending from >= 0 with the last entry 1.0");
    sample_refused("mass on a -inf point", kde, [](Built &b) { b.kde_lw[1] = -INF; }, 0, 10,
                   "kde_cdf of state 0: entry 1 rises above its predecessor, its log probability is -inf");
    sample_refused("a mixture row that closes below 1.0", mix, [](Built &b) { b.mix_cdf[1] = 0.75; }, 0, 10,
                   "mix_cdf of state 0: ascending from >= 0 with the last entry 1.0");
    sample_refused("mass on a -inf component", mix, [](Built &b) { b.mix_lw[0] = -INF; }, 0, 10,
                   "mix_cdf of state 0: entry 0 rises above its predecessor, its log probability is -inf");
    sample_refused("mix_draw", mix, [](Built &b) { b.mix_draw[3] = INF; }, 0, 10, "mix_draw 3 is not finite");
    sample_refused("emit_param", vec, [](Built &b) { b.emit_param[7] = NAN; }, 0, 10, "emit_param 7 is not finite");
}

// ---- sizes and decisions at their edges --------------------------------------------------------------------------------------------

static void decisions()
{
    HmmModelInfo I;
    std::string why;
    I.S = 4; I.NE = 2; I.NL = 2;
    CHECK(hmm_lds_bytes(1) == 16 && hmm_lds_bytes(HMM_S_MAX) == HMM_EXPECT_LDS && hmm_lds_bytes(4, 3) == 88, "LDS of the forward-type kernels");
    // the accumulators: E + n_stats + 1
    I.E = (1 << 26) - 1 - 6;
    CHECK(I.n_acc() == 1ll << 26 && hmm_acc_check(I, true, &why) && hmm_acc_check(I, false, &why) && why.empty(), "2^26 accumulators: %s", why.c_str());
    ++I.E;
    CHECK(I.n_acc() == (1ll << 26) + 1 && !hmm_acc_check(I, true, &why) && why == "model of 67108858 edges: the E-step takes at most 2^26 accumulators",
          "2^26 + 1 accumulators: %s", why.c_str());
    CHECK(!hmm_acc_check(I, false, &why) && why == "model of 67108858 edges: at most 2^26 accumulators", "2^26 + 1 accumulators: %s", why.c_str());
    I.E = INT32_MAX;
    CHECK(!hmm_acc_check(I, true, &why), "INT32_MAX edges");
    // the sizes of the four model types
    I.E = 7; I.vec = true; I.n_dim = 3;
    CHECK(I.dim() == 3 && I.n_stats() == 14 && I.n_acc() == 22, "a vector model's sizes");
    I.vec = false; I.mix = true; I.n_mix = 5;
    CHECK(I.dim() == 1 && I.n_stats() == 21 && I.n_acc() == 29, "a mixture model's sizes");
    I.mix = false; I.n_mix = 0; I.n_dim = 1;
    CHECK(I.n_stats() == 6 && I.n_acc() == 14, "a plain model's sizes");
    // the E-step's row in LDS: 16 S + 8 n_acc against HMM_EXPECT_LDS
    I.E = static_cast<int>(HMM_EXPECT_LDS / 8) - 2 * I.S - 6 - 1;
    CHECK(hmm_lds_bytes(I.S, I.n_acc()) == HMM_EXPECT_LDS && hmm_expect_in_lds(I, true) && !hmm_expect_in_lds(I, false), "a row that fills the LDS");
    ++I.E;
    CHECK(hmm_lds_bytes(I.S, I.n_acc()) == HMM_EXPECT_LDS + 8 && !hmm_expect_in_lds(I, true), "a row 8 bytes above the LDS");
    // the posterior's counts row: 16 S + 8 E
    I.E = static_cast<int>(HMM_EXPECT_LDS / 8) - 2 * I.S;
    CHECK(hmm_posterior_cnt(I, true, true) == 2 && hmm_posterior_cnt(I, true, false) == 1 && hmm_posterior_cnt(I, false, true) == 0, "a counts row that fills the LDS");
    ++I.E;
    CHECK(hmm_posterior_cnt(I, true, true) == 1 && hmm_posterior_cnt(I, false, false) == 0, "a counts row 8 bytes above the LDS");
    I.E = 0;
    CHECK(hmm_posterior_cnt(I, true, true) == 0, "no edges, no counts");
    // backpointers
    I.max_in = 255;
    CHECK(!hmm_bp_wide(I), "255 in-edges");
    I.max_in = 256;
    CHECK(hmm_bp_wide(I), "256 in-edges");
    why.clear();
    CHECK(hmm_launch_check(3, 8ll << 30, true, &why) && hmm_launch_check(3, 16ll << 30, false, &why) && why.empty(), "launches at the caps");
    CHECK(!hmm_launch_check(3, (8ll << 30) + 1, true, &why) && why == "sequence 3 needs 8589934593 bytes of backpointers (8 GiB at most)", "%s", why.c_str());
    CHECK(!hmm_launch_check(5, (16ll << 30) + 1, false, &why) && why == "sequence 5 needs 17179869185 bytes of forward matrix (16 GiB at most)", "%s", why.c_str());
}

static void short_slots()
{
    const int64_t off[5] = {0, 3, 3, 8, 8}, path_off[5] = {0, 5, 6, 6, 20};
    int64_t so = -1, sp = -1;
    const int32_t fit[4] = {3, 0, 5, 0}, pfit[4] = {5, 1, 0, 14};
    hmm_short_slots(fit, off, pfit, path_off, 4, &so, &sp);
    CHECK(so == 0 && sp == 0, "slots that fit exactly: %lld, %lld", static_cast<ll>(so), static_cast<ll>(sp));
    const int32_t over[4] = {4, 1, 5, 1}, pover[4] = {5, 2, 1, 15};
    hmm_short_slots(over, off, pover, path_off, 4, &so, &sp);
    CHECK(so == 3 && sp == 3, "short slots: %lld, %lld", static_cast<ll>(so), static_cast<ll>(sp));
    hmm_short_slots(over, off, nullptr, nullptr, 4, &so, &sp);
    CHECK(so == 3 && sp == 0, "no paths: %lld, %lld", static_cast<ll>(so), static_cast<ll>(sp));
    hmm_short_slots(nullptr, off, nullptr, nullptr, 0, &so, &sp);
    CHECK(so == 0 && sp == 0, "no sequences");
}

int main()
{
    round_trip("plain", Built(small(HMM_NORMAL, HMM_UNIFORM)));
    round_trip("kernel density", Built(small(HMM_KDE, HMM_KDE)));
    round_trip("kernel density beside normal", Built(small(HMM_NORMAL, HMM_KDE)));
    for (int D : {1, 3, 16}) round_trip("vector", Built(small(HMM_VECTOR, HMM_VECTOR, D)));
    round_trip("mixture beside kernel density", Built(small(HMM_MIXTURE, HMM_KDE)));
    round_trip("mixture", Built(small(HMM_UNIFORM, HMM_MIXTURE)));
    {
        Spec one;                                           // S = 1, NE = 0: start = end, nothing to emit
        one.kind = {HMM_SILENT}; one.level_ptr = {0, 1};
        round_trip("one silent state", Built(one));
        Spec apart = small(HMM_NORMAL, HMM_KDE);
        apart.edges.clear();
        round_trip("no edges", Built(apart));
        Spec emitting;                                      // no silent level: refused as to start and end, whatever they are
        emitting.kind = {HMM_NORMAL}; emitting.level_ptr = {1};
        refused("no silent state", Built(emitting).m, "start and end must be silent states");
        Spec big;                                           // HMM_S_MAX states: a chain of emitting ones between start and end
        big.kind.assign(HMM_S_MAX - 2, HMM_NORMAL);
        big.kind[7] = HMM_KDE; big.kind[4000] = HMM_MIXTURE;
        big.kind.push_back(HMM_SILENT); big.kind.push_back(HMM_SILENT);
        big.level_ptr = {HMM_S_MAX - 2, HMM_S_MAX - 1, HMM_S_MAX};
        big.start = HMM_S_MAX - 2; big.end = HMM_S_MAX - 1;
        for (int k = 0; k < HMM_S_MAX - 2; ++k) { if (k + 1 < HMM_S_MAX - 2) big.edges.push_back({k, k + 1}); big.edges.push_back({k, big.end}); }
        for (int k = 0; k < HMM_S_MAX - 2; ++k) big.edges.push_back({big.start, k});
        round_trip("HMM_S_MAX states", Built(big));
    }
    blob_identity();
    model_refusals();
    sample_refusals();
    decisions();
    short_slots();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("hmm plan ok\n");
    return 0;
}
