// hmm_plan.hpp -- the host's planning of the sequence-model entry points (ps_hmm_batch, ps_hmm_expect, ps_hmm_posterior,
// ps_hmm_sample): what they refuse in a ps_hmm_model and in the sampling tables, the layout of the model's blob on the device --
// written once, and read by the packing, by the pointers the kernels get and by the check program alike --, the layout of
// ps_hmm_sample's upload, and the sizes and decisions derived from a model.  Plain host C++ on <stdint.h>, the standard library,
// include/poreseg.h (plain C: the two structs) and batch_plan.hpp (HMM_EXPECT_LDS), no HIP: poreseg.hip and seg_hmm.hpp include
// it and define none of it again, and so does the stand-alone program tests/native/hmm_plan_check.cpp, which runs it under the
// address and undefined-behaviour sanitizers on models in exactly sized heap arrays.  A refusal is `false` and its text in *why
// -- the entry points hand it to fail() as it is; nothing is written to *why on the way to `true`.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "batch_plan.hpp"                  // HMM_EXPECT_LDS
#include "poreseg.h"

namespace ps {

constexpr int HMM_S_MAX = 4096;            // states: two fp64 rows of S in LDS = 64 KiB at most
constexpr int HMM_VITERBI = 0, HMM_FORWARD = 1, HMM_BACKWARD = 2;   // include/poreseg.h PS_HMM_*
constexpr int HMM_SILENT = 0, HMM_NORMAL = 1, HMM_UNIFORM = 2, HMM_KDE = 3;   // include/poreseg.h ps_hmm_model.kind
constexpr int HMM_VECTOR = 4;              // ... kind: a state of D components (a vector model)
constexpr int HMM_LOGNORMAL = 5, HMM_EXPONENTIAL = 6;   // ps_hmm_model.comp_kind, beside HMM_NORMAL and HMM_UNIFORM
constexpr int HMM_D_MAX = 16;              // components of a vector model's observation
constexpr int HMM_MIXTURE = 7;             // ... kind: a weighted choice between component distributions (HmmDevM)
constexpr int64_t HMM_KDE_POINTS_MAX = 1 << 24;
constexpr int64_t HMM_MIX_COMPONENTS_MAX = 1 << 24;
constexpr int HMM_IN_MAX = 65535;          // in-edges of a state: a backpointer is 1 byte, or 2 from HMM_BP_NARROW_MAX + 1 on
constexpr int HMM_BP_NARROW_MAX = 255;
constexpr long long HMM_ACC_MAX = 1ll << 26;       // accumulators of the E-step and the posterior's counts
constexpr long long HMM_BP_BYTES_MAX = 8ll << 30, HMM_FMAT_BYTES_MAX = 16ll << 30;   // one launch's backpointers / forward matrix

struct HmmDev {                 // device pointers into one upload of the baked model (include/poreseg.h ps_hmm_model)
    const double *param;        // 3 per state: normal (mean, 1 / (2 std^2), -log(std sqrt(2 pi))), uniform (low, high, -log(high - low))
    const double *in_lp, *out_lp;
    const int *kind, *level_ptr, *in_ptr, *in_src, *out_ptr, *out_dst;
    int S, n_emit, n_levels, start, end, finite;
};

// A model with kernel-density states (kind 3): state k's points are [kde_ptr[k], kde_ptr[k+1]) of kde_pt (the points) and
// kde_lw (their log weights, the weights summing to 1), and its param is (weighted mean of the points, 1 / (2 h^2),
// -log(h sqrt(2 pi))) for the bandwidth h.  The kernels are instantiated once per model type: a model without such states
// runs the HmmDev instantiations, whose code knows nothing of these tables.
struct HmmDevK : HmmDev {
    const int *kde_ptr;
    const double *kde_pt, *kde_lw;
};

// A vector model (every emitting state is kind 4): an observation is a row of D doubles, and state k scores it with the D
// independent components [k D, (k + 1) D) of comp_kind / comp_param (3 per component: normal and uniform as param,
// log-normal (mu, 1 / (2 sigma^2), -log(sigma sqrt(2 pi))), exponential (0, rate, log rate)) / comp_w (weights > 0).  Its
// `param` is not read.  A third set of instantiations: the HmmDev and HmmDevK code knows nothing of these tables.
struct HmmDevV : HmmDev {
    const int *comp_kind;
    const double *comp_param, *comp_w;
    int D;
};

// A model with mixture states (kind 7), beside normal, uniform and kernel-density ones: state k's components are
// [mix_ptr[k], mix_ptr[k+1]) of mix_kind (1, 2, 5, 6 as comp_kind), mix_param (3 per component, as comp_param) and mix_lw
// (their log weights, the weights summing to 1; -inf: the component is skipped), and its param is (0, 0, 0).  A fourth set
// of instantiations: the HmmDev, HmmDevK and HmmDevV code knows nothing of these tables.  The two sampling tables of
// ps_hmm_model ride here as well (HmmSampleDev stays the struct the other instantiations were compiled with): they are set
// by ps_hmm_sample alone, which uploads them per call, and are null in every other call.
struct HmmDevM : HmmDevK {
    const int *mix_ptr, *mix_kind;
    const double *mix_param, *mix_lw;
    const double *mix_cdf;      // per component: the running sum of the state's weights; 1.0 from the last positive weight on
    const double *mix_draw;     // 2 per component, as HmmSampleDev.emit_param
};

struct HmmSampleDev {           // device copies of ps_hmm_sample_tables (include/poreseg.h)
    const double *out_cdf;      // per out-edge: the running sum of the state's edge probabilities, its last entry 1.0
    const double *emit_param;   // 2 per emitting state (per component k D + d of a vector model)
    const double *kde_cdf;      // per kernel-density point: the running sum of the state's weights, its last entry 1.0
};

// a refusal's text, formatted as fail() formats it
inline bool hmm_refuse(std::string *why, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *why = buf;
    return false;
}

// ---- the model ---------------------------------------------------------------------------------------------------------------

// What hmm_model_check learns of a model it accepts: the counts the layout is made of, and the sizes derived from them.
struct HmmModelInfo {
    int S = 0, NE = 0, NL = 0;              // states, emitting states, silent levels
    int start = 0, end = 0, finite = 0;
    int n_dim = 1;                          // doubles per observation of a vector model (else 1)
    int E = 0, max_in = 0;                  // edges of the model (in- and out-lists alike), most in-edges of a state
    int64_t NP = 0, NC = 0, n_mix = 0;      // kernel-density points, components of a vector model (NE * n_dim), mixture components
    bool kde = false, vec = false, mix = false;     // some state of kind 3 / every emitting state of kind 4 / some state of kind 7
    int dim() const { return vec ? n_dim : 1; }                                  // doubles per observation
    long long n_stats() const { return (1ll + 2 * dim()) * NE + 3ll * n_mix; }   // doubles of ps_hmm_expect's d_stats
    long long n_acc() const { return E + n_stats() + 1; }                        // hmm_expect_kernel's accumulators
};

inline bool hmm_component_kind(int ck) { return ck == HMM_NORMAL || ck == HMM_UNIFORM || ck == HMM_LOGNORMAL || ck == HMM_EXPONENTIAL; }

// The model's arrays against its counts, the counts first: no array is read beyond what the counts checked so far allow.
// Only a model with a state of kind 3 has its kde_* fields read, only a vector model (kind 4) n_dim and the comp_* fields,
// only one with mixture states (kind 7) mix_ptr, mix_kind, mix_param and mix_lw; mix_cdf and mix_draw are hmm_sample_check's.
inline bool hmm_model_check(const ps_hmm_model *m, HmmModelInfo *I, std::string *why)
{
    const int S = m->n_states, NE = m->n_emit, NL = m->n_levels;
    if (S < 1 || S > HMM_S_MAX) return hmm_refuse(why, "model of %d states: the device HMM kernels take 1..%d", S, HMM_S_MAX);
    if (NE < 0 || NE > S || NL < 0 || NL > S - NE || (NL == 0) != (NE == S)) return hmm_refuse(why, "bad state / level counts");
    if (m->start < NE || m->start >= S || m->end < NE || m->end >= S) return hmm_refuse(why, "start and end must be silent states");
    if (!m->kind || !m->level_ptr || !m->in_ptr || !m->out_ptr) return hmm_refuse(why, "null model array");
    bool kde = false, vec = false, plain = false, mix = false;
    for (int k = 0; k < S; ++k) {
        const int kd = m->kind[k];
        if ((k < NE) != (kd == HMM_NORMAL || kd == HMM_UNIFORM || kd == HMM_KDE || kd == HMM_VECTOR || kd == HMM_MIXTURE) || (k >= NE && kd != HMM_SILENT))
            return hmm_refuse(why, "state %d: emitting states first, then silent ones", k);
        kde = kde || kd == HMM_KDE;
        vec = vec || kd == HMM_VECTOR;
        mix = mix || kd == HMM_MIXTURE;
        plain = plain || (k < NE && kd != HMM_VECTOR);
    }
    if (!vec && !m->param) return hmm_refuse(why, "null model array");      // (a vector model's param is not read)
    int64_t NC = 0;
    if (vec) {
        if (plain) return hmm_refuse(why, "a vector model's emitting states are all kind 4: kinds 1..3 cannot be mixed with it");
        if (m->n_dim < 1 || m->n_dim > HMM_D_MAX) return hmm_refuse(why, "n_dim %d: a vector model takes 1..%d components", m->n_dim, HMM_D_MAX);
        if (!m->comp_kind || !m->comp_param || !m->comp_w) return hmm_refuse(why, "a vector model needs comp_kind, comp_param and comp_w");
        NC = static_cast<int64_t>(NE) * m->n_dim;
        for (int64_t i = 0; i < NC; ++i) {
            const int ck = m->comp_kind[i];
            if (!hmm_component_kind(ck)) return hmm_refuse(why, "component %lld: unknown component kind %d", static_cast<long long>(i), ck);
            if (!std::isfinite(m->comp_w[i]) || !(m->comp_w[i] > 0.0))
                return hmm_refuse(why, "component %lld: a weight must be finite and > 0", static_cast<long long>(i));
        }
    }
    int64_t NP = 0;
    if (kde) {
        if (!m->kde_ptr || !m->kde_pt || !m->kde_lw) return hmm_refuse(why, "a kernel-density state needs kde_ptr, kde_pt and kde_lw");
        if (m->kde_ptr[0] != 0) return hmm_refuse(why, "kde_ptr must start at 0");
        for (int k = 0; k < NE; ++k) {
            if (m->kde_ptr[k + 1] < m->kde_ptr[k]) return hmm_refuse(why, "descending kde_ptr at state %d", k);
            if ((m->kde_ptr[k + 1] > m->kde_ptr[k]) != (m->kind[k] == HMM_KDE))
                return hmm_refuse(why, "state %d: a kernel-density state has at least one point, any other state none", k);
        }
        NP = m->kde_ptr[NE];
        if (NP > HMM_KDE_POINTS_MAX)
            return hmm_refuse(why, "%lld kernel-density points: the device HMM kernels take at most %lld",
                              static_cast<long long>(NP), static_cast<long long>(HMM_KDE_POINTS_MAX));
        for (int64_t i = 0; i < NP; ++i)
            if (!std::isfinite(m->kde_pt[i]) || !(m->kde_lw[i] <= 0.0))
                return hmm_refuse(why, "kernel-density point %lld: points must be finite and log weights <= 0", static_cast<long long>(i));
    }
    int64_t NM = 0;
    if (mix) {                                           // (never beside kind 4: refused above)
        if (!m->mix_ptr || !m->mix_kind || !m->mix_param || !m->mix_lw)
            return hmm_refuse(why, "a mixture state needs mix_ptr, mix_kind, mix_param and mix_lw");
        if (m->mix_ptr[0] != 0) return hmm_refuse(why, "mix_ptr must start at 0");
        for (int k = 0; k < NE; ++k) {
            if (m->mix_ptr[k + 1] < m->mix_ptr[k]) return hmm_refuse(why, "descending mix_ptr at state %d", k);
            if ((m->mix_ptr[k + 1] > m->mix_ptr[k]) != (m->kind[k] == HMM_MIXTURE))
                return hmm_refuse(why, "state %d: a mixture state has at least one component, any other state none", k);
        }
        NM = m->mix_ptr[NE];
        if (NM > HMM_MIX_COMPONENTS_MAX)
            return hmm_refuse(why, "%lld mixture components: the device HMM kernels take at most %lld",
                              static_cast<long long>(NM), static_cast<long long>(HMM_MIX_COMPONENTS_MAX));
        for (int64_t i = 0; i < NM; ++i) {
            const int ck = m->mix_kind[i];
            if (!hmm_component_kind(ck)) return hmm_refuse(why, "mixture component %lld: unknown component kind %d", static_cast<long long>(i), ck);
            if (!(m->mix_lw[i] <= 0.0)) return hmm_refuse(why, "mixture component %lld: a log weight must be <= 0", static_cast<long long>(i));
        }
    }
    if (m->level_ptr[0] != NE || m->level_ptr[NL] != S) return hmm_refuse(why, "levels must cover the silent states");
    for (int L = 0; L < NL; ++L) if (m->level_ptr[L + 1] <= m->level_ptr[L]) return hmm_refuse(why, "empty or descending level %d", L);
    std::vector<int> level(S, -1);
    for (int L = 0; L < NL; ++L) for (int k = m->level_ptr[L]; k < m->level_ptr[L + 1]; ++k) level[k] = L;
    const int32_t *ptrs[2] = {m->in_ptr, m->out_ptr}, *idx[2] = {m->in_src, m->out_dst};
    int64_t n_edge[2];
    int max_in = 0;
    for (int d = 0; d < 2; ++d) {
        if (ptrs[d][0] != 0) return hmm_refuse(why, "edge lists must start at 0");
        for (int k = 0; k < S; ++k) {
            if (ptrs[d][k + 1] < ptrs[d][k]) return hmm_refuse(why, "descending edge offsets");
            if (d == 0) max_in = std::max(max_in, ptrs[d][k + 1] - ptrs[d][k]);
        }
        n_edge[d] = ptrs[d][S];
        if (n_edge[d] > 0 && (!idx[d] || !(d ? m->out_lp : m->in_lp))) return hmm_refuse(why, "null edge array");
        for (int k = 0; k < S; ++k)
            for (int e = ptrs[d][k]; e < ptrs[d][k + 1]; ++e) {
                const int o = idx[d][e];
                if (o < 0 || o >= S) return hmm_refuse(why, "edge to a state out of range");
                const int src = d ? k : o, dst = d ? o : k;
                if (dst >= NE && src >= NE && level[src] >= level[dst]) return hmm_refuse(why, "silent edge %d -> %d does not go up a level", src, dst);
            }
    }
    if (n_edge[0] != n_edge[1]) return hmm_refuse(why, "in- and out-edge lists differ in length");
    if (max_in > HMM_IN_MAX) return hmm_refuse(why, "a state with %d in-edges: the device HMM kernels take at most %d", max_in, HMM_IN_MAX);
    I->S = S; I->NE = NE; I->NL = NL;
    I->start = m->start; I->end = m->end; I->finite = m->finite;
    I->n_dim = vec ? m->n_dim : 1;
    I->E = static_cast<int>(n_edge[0]); I->max_in = max_in;
    I->NP = NP; I->NC = NC; I->n_mix = NM;
    I->kde = kde; I->vec = vec; I->mix = mix;
    return true;
}

// ---- the blob ----------------------------------------------------------------------------------------------------------------

// The tables of the blob in their order: the doubles, then (from HMM_T_INT on) the int32s.  The device copy is reused while
// the blob is unchanged, so whatever the kernels read of a model is in it: HMM_T_TAIL holds (start, end, finite) and
// HMM_T_N_DIM a vector model's n_dim for the comparison alone.  A table the model does not have (kde_* without kind 3, comp_*
// and n_dim without kind 4 -- the two exclude each other --, mix_* without kind 7) takes no room.
enum HmmTable {
    HMM_T_PARAM, HMM_T_IN_LP, HMM_T_OUT_LP, HMM_T_KDE_PT, HMM_T_KDE_LW, HMM_T_COMP_PARAM, HMM_T_COMP_W, HMM_T_MIX_PARAM, HMM_T_MIX_LW,
    HMM_T_INT,
    HMM_T_KIND = HMM_T_INT, HMM_T_LEVEL_PTR, HMM_T_IN_PTR, HMM_T_OUT_PTR, HMM_T_IN_SRC, HMM_T_OUT_DST, HMM_T_TAIL, HMM_T_KDE_PTR,
    HMM_T_COMP_KIND, HMM_T_N_DIM, HMM_T_MIX_PTR, HMM_T_MIX_KIND,
    HMM_T_COUNT
};

struct HmmBlobLayout {
    size_t off[HMM_T_COUNT], n[HMM_T_COUNT];    // of table t: its first entry and its entries, in doubles or in int32s
    size_t nd, ni, bytes;                       // doubles and int32s in all; the blob: nd doubles, then ni int32s
    static size_t width(int t) { return t < HMM_T_INT ? sizeof(double) : sizeof(int32_t); }
    size_t byte_off(int t) const { return t < HMM_T_INT ? off[t] * sizeof(double) : nd * sizeof(double) + off[t] * sizeof(int32_t); }
    template <typename T> const T *at(const void *base, int t) const { return reinterpret_cast<const T *>(static_cast<const char *>(base) + byte_off(t)); }
    // a table only some models have: null where this one has none of it
    template <typename T> const T *opt(const void *base, int t) const { return n[t] ? at<T>(base, t) : nullptr; }
};

inline HmmBlobLayout hmm_blob_layout(const HmmModelInfo &I)
{
    const size_t S = static_cast<size_t>(I.S), NE = static_cast<size_t>(I.NE), E = static_cast<size_t>(I.E),
                 NP = static_cast<size_t>(I.NP), NC = static_cast<size_t>(I.NC), NM = static_cast<size_t>(I.n_mix);
    HmmBlobLayout L;
    for (int t = 0; t < HMM_T_COUNT; ++t) L.n[t] = 0;
    L.n[HMM_T_PARAM] = 3 * S; L.n[HMM_T_IN_LP] = E; L.n[HMM_T_OUT_LP] = E;
    L.n[HMM_T_KIND] = S; L.n[HMM_T_LEVEL_PTR] = static_cast<size_t>(I.NL) + 1; L.n[HMM_T_IN_PTR] = S + 1; L.n[HMM_T_OUT_PTR] = S + 1;
    L.n[HMM_T_IN_SRC] = E; L.n[HMM_T_OUT_DST] = E; L.n[HMM_T_TAIL] = 3;
    if (I.kde) { L.n[HMM_T_KDE_PT] = NP; L.n[HMM_T_KDE_LW] = NP; L.n[HMM_T_KDE_PTR] = NE + 1; }
    if (I.vec) { L.n[HMM_T_COMP_PARAM] = 3 * NC; L.n[HMM_T_COMP_W] = NC; L.n[HMM_T_COMP_KIND] = NC; L.n[HMM_T_N_DIM] = 1; }
    if (I.mix) { L.n[HMM_T_MIX_PARAM] = 3 * NM; L.n[HMM_T_MIX_LW] = NM; L.n[HMM_T_MIX_PTR] = NE + 1; L.n[HMM_T_MIX_KIND] = NM; }
    L.nd = L.ni = 0;
    for (int t = 0; t < HMM_T_INT; ++t) { L.off[t] = L.nd; L.nd += L.n[t]; }
    for (int t = HMM_T_INT; t < HMM_T_COUNT; ++t) { L.off[t] = L.ni; L.ni += L.n[t]; }
    L.bytes = L.nd * sizeof(double) + L.ni * sizeof(int32_t);
    return L;
}

// The blob of a model hmm_model_check accepted, by the layout made from its HmmModelInfo.  A vector model's `param` is not
// read: its slots stay 0.  The fields appended to ps_hmm_model for a kind are read only for a model that has the kind (a
// caller built against the shorter struct never sets it).
inline void hmm_blob_pack(const ps_hmm_model *m, const HmmBlobLayout &L, std::vector<char> *blob)
{
    blob->assign(L.bytes, 0);
    const bool kde = L.n[HMM_T_KDE_PTR] != 0, vec = L.n[HMM_T_N_DIM] != 0, mix = L.n[HMM_T_MIX_PTR] != 0;
    const int32_t tail[3] = {m->start, m->end, m->finite};
    const void *src[HMM_T_COUNT] = {};
    src[HMM_T_PARAM] = vec ? nullptr : m->param; src[HMM_T_IN_LP] = m->in_lp; src[HMM_T_OUT_LP] = m->out_lp;
    src[HMM_T_KIND] = m->kind; src[HMM_T_LEVEL_PTR] = m->level_ptr; src[HMM_T_IN_PTR] = m->in_ptr; src[HMM_T_OUT_PTR] = m->out_ptr;
    src[HMM_T_IN_SRC] = m->in_src; src[HMM_T_OUT_DST] = m->out_dst; src[HMM_T_TAIL] = tail;
    if (kde) { src[HMM_T_KDE_PT] = m->kde_pt; src[HMM_T_KDE_LW] = m->kde_lw; src[HMM_T_KDE_PTR] = m->kde_ptr; }
    if (vec) { src[HMM_T_COMP_PARAM] = m->comp_param; src[HMM_T_COMP_W] = m->comp_w; src[HMM_T_COMP_KIND] = m->comp_kind; src[HMM_T_N_DIM] = &m->n_dim; }
    if (mix) { src[HMM_T_MIX_PARAM] = m->mix_param; src[HMM_T_MIX_LW] = m->mix_lw; src[HMM_T_MIX_PTR] = m->mix_ptr; src[HMM_T_MIX_KIND] = m->mix_kind; }
    for (int t = 0; t < HMM_T_COUNT; ++t)
        if (L.n[t] && src[t]) std::memcpy(blob->data() + L.byte_off(t), src[t], L.n[t] * HmmBlobLayout::width(t));
}

// The three structs the kernels take, aimed at a copy of the blob at `base` (the device's, or in the check program the host
// blob itself): null where the model has no such table, V->D = 1 for a model that is no vector model.  M's mix_cdf and
// mix_draw are ps_hmm_sample's (hmm_sample_resolve) and null here.
inline void hmm_blob_resolve(const void *base, const HmmBlobLayout &L, const HmmModelInfo &I, HmmDevK *K, HmmDevV *V, HmmDevM *M)
{
    K->param = L.at<double>(base, HMM_T_PARAM); K->in_lp = L.at<double>(base, HMM_T_IN_LP); K->out_lp = L.at<double>(base, HMM_T_OUT_LP);
    K->kind = L.at<int>(base, HMM_T_KIND); K->level_ptr = L.at<int>(base, HMM_T_LEVEL_PTR);
    K->in_ptr = L.at<int>(base, HMM_T_IN_PTR); K->in_src = L.at<int>(base, HMM_T_IN_SRC);
    K->out_ptr = L.at<int>(base, HMM_T_OUT_PTR); K->out_dst = L.at<int>(base, HMM_T_OUT_DST);
    K->S = I.S; K->n_emit = I.NE; K->n_levels = I.NL; K->start = I.start; K->end = I.end; K->finite = I.finite != 0;
    K->kde_ptr = L.opt<int>(base, HMM_T_KDE_PTR); K->kde_pt = L.opt<double>(base, HMM_T_KDE_PT); K->kde_lw = L.opt<double>(base, HMM_T_KDE_LW);
    static_cast<HmmDev &>(*V) = *K;
    V->comp_kind = L.opt<int>(base, HMM_T_COMP_KIND); V->comp_param = L.opt<double>(base, HMM_T_COMP_PARAM); V->comp_w = L.opt<double>(base, HMM_T_COMP_W);
    V->D = I.dim();
    static_cast<HmmDevK &>(*M) = *K;
    M->mix_ptr = L.opt<int>(base, HMM_T_MIX_PTR); M->mix_kind = L.opt<int>(base, HMM_T_MIX_KIND);
    M->mix_param = L.opt<double>(base, HMM_T_MIX_PARAM); M->mix_lw = L.opt<double>(base, HMM_T_MIX_LW);
    M->mix_cdf = M->mix_draw = nullptr;
}

// ---- sizes and decisions -----------------------------------------------------------------------------------------------------

// dynamic LDS of the forward-type kernels: the two score rows, and `extra` doubles behind them (an accumulator or a counts row)
inline size_t hmm_lds_bytes(int S, long long extra = 0) { return (2 * static_cast<size_t>(S) + static_cast<size_t>(extra)) * sizeof(double); }
// `option`: the context's hmm_expect_lds (0: the rows stay in global memory)
inline bool hmm_fits_lds(int S, long long extra, bool option) { return hmm_lds_bytes(S, extra) <= HMM_EXPECT_LDS && option; }
// ps_hmm_expect: the accumulator row of a workgroup in LDS, or in global memory
inline bool hmm_expect_in_lds(const HmmModelInfo &I, bool option) { return hmm_fits_lds(I.S, I.n_acc(), option); }
// ps_hmm_posterior: the counts row of a sequence -- 0 none asked for (or no edges), 2 in LDS when it fits beside the score
// rows, else 1 in place
inline int hmm_posterior_cnt(const HmmModelInfo &I, bool want_counts, bool option)
{
    return !want_counts || I.E == 0 ? 0 : hmm_fits_lds(I.S, I.E, option) ? 2 : 1;
}
// Viterbi's backpointers: the ordinal of the winning in-edge in one byte, or in two
inline bool hmm_bp_wide(const HmmModelInfo &I) { return I.max_in > HMM_BP_NARROW_MAX; }

inline bool hmm_acc_check(const HmmModelInfo &I, bool e_step, std::string *why)
{
    if (I.n_acc() <= HMM_ACC_MAX) return true;
    return e_step ? hmm_refuse(why, "model of %d edges: the E-step takes at most 2^26 accumulators", I.E)
                  : hmm_refuse(why, "model of %d edges: at most 2^26 accumulators", I.E);
}
// the scratch of the launch that begins with sequence q0 (next_chunk, batch_plan.hpp): Viterbi's backpointers, or a forward matrix
inline bool hmm_launch_check(int32_t q0, long long bytes, bool backpointers, std::string *why)
{
    if (bytes <= (backpointers ? HMM_BP_BYTES_MAX : HMM_FMAT_BYTES_MAX)) return true;
    return backpointers ? hmm_refuse(why, "sequence %d needs %lld bytes of backpointers (8 GiB at most)", q0, bytes)
                        : hmm_refuse(why, "sequence %d needs %lld bytes of forward matrix (16 GiB at most)", q0, bytes);
}

// ---- sampling ----------------------------------------------------------------------------------------------------------------

// One row [ptr[k], ptr[k + 1]) of a cdf table beside the model's log probabilities lp of its entries.  A rounded running sum
// may pass 1.0 by an ulp, and the entries stored as 1.0 behind it then step back onto 1.0: both are above every u the kernel
// draws, so the bisection still finds the linear scan's entry.  An entry above its predecessor (the first: above 0) owns an
// interval of u; where the model says -inf the row gives mass to an impossible entry.
inline bool hmm_cdf_row(const char *what, const double *cdf, const double *lp, const int32_t *ptr, int k, std::string *why)
{
    const int lo = ptr[k], hi = ptr[k + 1];
    double prev = 0.0;
    for (int i = lo; i < hi; ++i) {
        const double v = cdf[i];
        const bool closes = i == hi - 1;
        if (closes ? v != 1.0 : !std::isfinite(v) || !(v >= prev || (v == 1.0 && prev > 1.0)))
            return hmm_refuse(why, "%s of state %d: ascending from >= 0 with the last entry 1.0", what, k);
        if (v > prev && lp[i] == -INFINITY)
            return hmm_refuse(why, "%s of state %d: entry %d rises above its predecessor, its log probability is -inf", what, k, i - lo);
        prev = v;
    }
    return true;
}

// What ps_hmm_sample checks once the model stands (I: hmm_model_check's): a walk that can end, the longest path there can be
// within int32, then the tables against the model -- sizes, every state's cdf ascending within [0, 1] and closed by exactly 1.0.
inline bool hmm_sample_check(const ps_hmm_model *model, const ps_hmm_sample_tables *tables, const HmmModelInfo &I, int32_t length,
                             int32_t max_length, std::string *why)
{
    if (!model->finite && length == 0) return hmm_refuse(why, "a model without an edge into end never ends a walk: a length must be given");
    if ((static_cast<long long>(max_length) + 1) * (I.NL + 1) + 2 > INT32_MAX)
        return hmm_refuse(why, "max_length %d with %d silent levels: a path could exceed int32", max_length, I.NL);
    const int64_t n_param = 2 * static_cast<int64_t>(I.NE) * I.dim(), n_kde = I.NP;
    if (I.mix && (!model->mix_cdf || !model->mix_draw)) return hmm_refuse(why, "sampling a mixture state needs mix_cdf and mix_draw");
    if (tables->n_cdf != I.E || tables->n_param != n_param || tables->n_kde != n_kde)
        return hmm_refuse(why, "sampling tables of %lld / %lld / %lld entries, the model takes %d / %lld / %lld",
                          static_cast<long long>(tables->n_cdf), static_cast<long long>(tables->n_param), static_cast<long long>(tables->n_kde),
                          I.E, static_cast<long long>(n_param), static_cast<long long>(n_kde));
    if ((I.E > 0 && !tables->out_cdf) || (n_param > 0 && !tables->emit_param) || (n_kde > 0 && !tables->kde_cdf))
        return hmm_refuse(why, "null sampling table");
    for (int k = 0; k < I.S; ++k)
        if (!hmm_cdf_row("out_cdf", tables->out_cdf, model->out_lp, model->out_ptr, k, why)) return false;
    for (int k = 0; I.kde && k < I.NE; ++k)
        if (!hmm_cdf_row("kde_cdf", tables->kde_cdf, model->kde_lw, model->kde_ptr, k, why)) return false;
    for (int k = 0; I.mix && k < I.NE; ++k)
        if (!hmm_cdf_row("mix_cdf", model->mix_cdf, model->mix_lw, model->mix_ptr, k, why)) return false;
    for (int64_t i = 0; i < 2 * I.n_mix; ++i)
        if (!std::isfinite(model->mix_draw[i])) return hmm_refuse(why, "mix_draw %lld is not finite", static_cast<long long>(i));
    for (int64_t i = 0; i < n_param; ++i)
        if (!std::isfinite(tables->emit_param[i])) return hmm_refuse(why, "emit_param %lld is not finite", static_cast<long long>(i));
    return true;
}

// ps_hmm_sample's upload, one transfer per call: the tables back to back in this order, 8-byte entries all.  src / bytes are
// the list the entry point stages (a table the model or the call does not have: 0 bytes), hmm_sample_resolve aims the kernel's
// arguments at a copy of it.
enum HmmSampleTable { HMM_U_CDF, HMM_U_PARAM, HMM_U_KDE_CDF, HMM_U_MIX_CDF, HMM_U_MIX_DRAW, HMM_U_OFF, HMM_U_PATH_OFF, HMM_U_COUNT };
struct HmmSampleLayout {
    const void *src[HMM_U_COUNT];
    size_t bytes[HMM_U_COUNT], off[HMM_U_COUNT], total;
    template <typename T> const T *at(const void *base, int t) const { return reinterpret_cast<const T *>(static_cast<const char *>(base) + off[t]); }
};

inline HmmSampleLayout hmm_sample_layout(const ps_hmm_model *model, const ps_hmm_sample_tables *tables, const HmmModelInfo &I,
                                         const int64_t *h_off, const int64_t *h_path_off, int32_t n_seq)
{
    const size_t n_mix = static_cast<size_t>(I.n_mix), n_off = static_cast<size_t>(n_seq) + 1;
    HmmSampleLayout U;
    const void *src[HMM_U_COUNT] = {tables->out_cdf, tables->emit_param, tables->kde_cdf, I.mix ? model->mix_cdf : nullptr,
                                    I.mix ? model->mix_draw : nullptr, h_off, h_path_off};
    const size_t n[HMM_U_COUNT] = {static_cast<size_t>(I.E), 2 * static_cast<size_t>(I.NE) * I.dim(), static_cast<size_t>(I.NP), n_mix, 2 * n_mix,
                                   n_off, h_path_off ? n_off : 0};
    U.total = 0;
    for (int t = 0; t < HMM_U_COUNT; ++t) { U.src[t] = src[t]; U.bytes[t] = n[t] * 8; U.off[t] = U.total; U.total += U.bytes[t]; }
    return U;
}

inline void hmm_sample_resolve(const void *base, const HmmSampleLayout &U, HmmSampleDev *T, HmmDevM *M, const long long **off,
                               const long long **path_off)
{
    T->out_cdf = U.at<double>(base, HMM_U_CDF); T->emit_param = U.at<double>(base, HMM_U_PARAM); T->kde_cdf = U.at<double>(base, HMM_U_KDE_CDF);
    M->mix_cdf = U.at<double>(base, HMM_U_MIX_CDF); M->mix_draw = U.at<double>(base, HMM_U_MIX_DRAW);
    *off = U.at<long long>(base, HMM_U_OFF);
    *path_off = U.bytes[HMM_U_PATH_OFF] ? U.at<long long>(base, HMM_U_PATH_OFF) : nullptr;
}

// The lengths the kernel reported against the slots (plens and h_path_off null: no paths asked for)
inline void hmm_short_slots(const int32_t *lens, const int64_t *h_off, const int32_t *plens, const int64_t *h_path_off, int32_t n_seq,
                            int64_t *short_obs, int64_t *short_path)
{
    *short_obs = *short_path = 0;
    for (int32_t q = 0; q < n_seq; ++q) {
        *short_obs += lens[q] > h_off[q + 1] - h_off[q];
        if (plens) *short_path += plens[q] > h_path_off[q + 1] - h_path_off[q];
    }
}

}  // namespace ps
