// seg_hmm.hpp -- hidden Markov model decoding (pypore_amd.hmm): Viterbi, forward and backward for a batch of observation
// sequences against one baked model, on gfx950.
//
// States are ordered as pypore_amd.hmm.Model.bake leaves them: emitting states [0, n_emit), then the silent states
// [n_emit, S) grouped by topological level (a silent state's silent predecessors all lie in lower levels).  A time step t
// of the forward-type passes runs in two phases:
//   1. every emitting state combines its in-edges from row t-1 and adds its emission log density of observation t-1;
//   2. the silent states, level by level, combine their in-edges from row t (emitting states of step t and silent states
//      of lower levels).
// The backward pass runs the mirror image over the out-edges (levels descending, then the emitting states); it is written
// once (hmm_bwd_sweep, hmm_bwd_state) for the three kernels that run it: backward, E-step and posterior.  Viterbi takes
// the maximum over the in-edges, scanned in ascending source index and updated only on a strictly greater score, so the
// lowest source wins a tie; forward and backward take log-sum-exp, accumulated online as  max + log1p(sum of the other
// terms' exp(v - max)),  which keeps values near log(1) accurate.
//
// One workgroup of one wave per sequence: the lanes spread over the states, the previous and current score rows live in
// LDS (16 * S bytes, S <= 4096), and the steps between phases and levels need only a wave-level fence, no s_barrier.  The
// model arrays are read from global memory: every workgroup reads the same few KB, which stay in L2 / L1.  Viterbi stores
// one backpointer per (step, state) -- the ordinal of the winning in-edge, 1 or 2 bytes -- in global memory, and a second
// kernel walks them back with one lane per sequence.  fp64 throughout, no FMA contraction.
#pragma once

#include "batch_plan.hpp"                  // HMM_NT
#include "hmm_plan.hpp"                    // the limits, the state kinds and modes; HmmDev, HmmDevK, HmmDevV, HmmDevM, HmmSampleDev

namespace ps {

// The observation as the kernels hand it to hmm_emit: doubles per observation, and observation t of the sequence that
// starts at x -- the double itself, or for a vector model the row of D doubles (one address for the whole wave).
template <typename MD> __device__ __forceinline__ int hmm_dim(const MD &) { return 1; }
__device__ __forceinline__ int hmm_dim(const HmmDevV &M) { return M.D; }
template <typename MD> __device__ __forceinline__ double hmm_obs(const MD &, const double *x, int t) { return x[t]; }
__device__ __forceinline__ const double *hmm_obs(const HmmDevV &M, const double *x, int t)
{
    return x + static_cast<long long>(t) * M.D;
}

__device__ __forceinline__ void hm_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double hmm_emit(const HmmDev &M, int k, double x)
{
#pragma clang fp contract(off)
    const double a = M.param[3 * k], b = M.param[3 * k + 1], c = M.param[3 * k + 2];
    if (M.kind[k] == HMM_NORMAL) {
        const double d = x - a;
        return c - (d * d) * b;
    }
    return (x >= a && x <= b) ? c : -__builtin_inf();
}

// log-sum-exp of a stream of terms: m = the largest so far, r = sum of exp(v - m) over the others
struct HmmLse {
    double m = -__builtin_inf(), r = 0.0;
    __device__ __forceinline__ void add(double v)
    {
        if (!(v > -__builtin_inf())) return;
        if (v > m) { r = (r + 1.0) * exp(m - v); m = v; }
        else r += exp(v - m);
    }
    __device__ __forceinline__ double get() const { return m > -__builtin_inf() ? m + log1p(r) : -__builtin_inf(); }
};

// Kernel-density emission  c + log sum_i w_i exp(-(x - p_i)^2 / (2 h^2)):  the lane that owns the state streams its
// points through HmmLse in ascending index (the largest term plus log1p of the others, so an observation far from every
// point gives a finite value).  The other kinds take the HmmDev code.
__device__ __forceinline__ double hmm_emit(const HmmDevK &M, int k, double x)
{
#pragma clang fp contract(off)
    if (M.kind[k] != HMM_KDE) return hmm_emit(static_cast<const HmmDev &>(M), k, x);
    const double b = M.param[3 * k + 1], c = M.param[3 * k + 2];
    HmmLse acc;
    const int i1 = M.kde_ptr[k + 1];
    for (int i = M.kde_ptr[k]; i < i1; ++i) {
        const double d = x - M.kde_pt[i];
        acc.add(M.kde_lw[i] - (d * d) * b);
    }
    return c + acc.get();
}

// Vector emission  w_0 l_0(x_0) + w_1 l_1(x_1) + ...:  the lane that owns the state walks its D components in ascending d,
// the sum starting from the first product, so one component of weight 1 gives that component's own bits.  A weight is
// finite and > 0: an impossible component makes the sum -inf, never NaN.
__device__ __forceinline__ double hmm_emit(const HmmDevV &M, int k, const double *x)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int d = 0, i = k * M.D; d < M.D; ++d, ++i) {
        const double a = M.comp_param[3 * i], b = M.comp_param[3 * i + 1], c = M.comp_param[3 * i + 2];
        const double xd = x[d];
        const int kd = M.comp_kind[i];
        double l;
        if (kd == HMM_NORMAL) {
            const double u = xd - a;
            l = c - (u * u) * b;
        } else if (kd == HMM_UNIFORM) {
            l = (xd >= a && xd <= b) ? c : -__builtin_inf();
        } else if (kd == HMM_LOGNORMAL) {
            if (xd > 0.0) {
                const double y = log(xd), u = y - a;
                l = (c - (u * u) * b) - y;
            } else l = -__builtin_inf();
        } else {
            l = xd >= 0.0 ? c - xd * b : -__builtin_inf();
        }
        const double wl = M.comp_w[i] * l;
        s = d ? s + wl : wl;
    }
    return s;
}

// The log density of one mixture component of kind kd with its triple (a, b, c) at x: the formulas of the vector emission's
// component switch above (include/poreseg.h comp_kind).  The vector emission keeps its own body: routed through this
// function the HmmDevV kernels compile to other code than they did, and their E-step measured slower.
__device__ __forceinline__ double hmm_comp_logp(int kd, double a, double b, double c, double x)
{
#pragma clang fp contract(off)
    if (kd == HMM_NORMAL) {
        const double u = x - a;
        return c - (u * u) * b;
    }
    if (kd == HMM_UNIFORM) return (x >= a && x <= b) ? c : -__builtin_inf();
    if (kd == HMM_LOGNORMAL) {
        if (x > 0.0) {
            const double y = log(x), u = y - a;
            return (c - (u * u) * b) - y;
        }
        return -__builtin_inf();
    }
    return x >= 0.0 ? c - x * b : -__builtin_inf();
}

// Term i of a mixture state's density at x:  log w_i + l_i(x),  -inf for a component of weight 0 or one that excludes x.
__device__ __forceinline__ double hmm_mix_term(const HmmDevM &M, int i, double x)
{
#pragma clang fp contract(off)
    return M.mix_lw[i] + hmm_comp_logp(M.mix_kind[i], M.mix_param[3 * i], M.mix_param[3 * i + 1], M.mix_param[3 * i + 2], x);
}

// Mixture emission  log sum_i w_i p_i(x):  the lane that owns the state streams its components' terms through HmmLse in
// ascending index, as the kernel-density loop does its points: -inf when no term is finite, never NaN, and one component
// of weight 1 gives that component's own bits (0.0 + l = l, l + log1p(0) = l).  The other kinds take the HmmDevK code.
__device__ __forceinline__ double hmm_emit(const HmmDevM &M, int k, double x)
{
#pragma clang fp contract(off)
    if (M.kind[k] != HMM_MIXTURE) return hmm_emit(static_cast<const HmmDevK &>(M), k, x);
    HmmLse acc;
    const int i1 = M.mix_ptr[k + 1];
    for (int i = M.mix_ptr[k]; i < i1; ++i) acc.add(hmm_mix_term(M, i, x));
    return acc.get();
}

// What the E-step's statistics sum for component d of emitting state k: y - c, with y the observation (its logarithm for
// a log-normal component) and c the component's shift (slot 0 of its parameters).  Called only where the state's posterior
// is positive, so a log-normal component sees x > 0.
template <typename MD> __device__ __forceinline__ double hmm_stat(const MD &M, int k, int, double x)
{
    return x - M.param[3 * k];
}
__device__ __forceinline__ double hmm_stat(const HmmDevV &M, int k, int d, const double *x)
{
    const int i = k * M.D + d;
    const double y = M.comp_kind[i] == HMM_LOGNORMAL ? log(x[d]) : x[d];
    return y - M.comp_param[3 * i];
}

// The E-step's rows of a mixture state's components (rows: one (W_i, A_i, B_i) per component in table order, behind the
// states' rows): state k's posterior g > 0 at observation x is shared out by the responsibilities  r_i = exp(v_i - e)  of
// the terms v_i > -inf, e = the state's emission (finite here), and component i sums  w = g r_i,  w d  and  (w d) d  with
// d = y - mix_param[3 i],  y = log x  for a log-normal component (its term is finite only for x > 0).  The rows belong to
// the lane that owns the state.  Models without mixture states have no such rows.
template <typename MD, typename X> __device__ __forceinline__ void hmm_mix_stat(const MD &, int, X, double, double *) {}
__device__ __forceinline__ void hmm_mix_stat(const HmmDevM &M, int k, double x, double g, double *rows)
{
#pragma clang fp contract(off)
    if (M.kind[k] != HMM_MIXTURE) return;
    const double e = hmm_emit(M, k, x);
    const int i1 = M.mix_ptr[k + 1];
    for (int i = M.mix_ptr[k]; i < i1; ++i) {
        const double v = hmm_mix_term(M, i, x);
        if (!(v > -__builtin_inf())) continue;
        const double w = g * exp(v - e);
        const double y = M.mix_kind[i] == HMM_LOGNORMAL ? log(x) : x;
        const double d = y - M.mix_param[3 * i];
        const double wd = w * d;
        double *s = rows + 3 * i;
        s[0] += w;
        s[1] += wd;
        s[2] += wd * d;
    }
}

// Viterbi / forward over one sequence per workgroup.  Rows of sequence q: mat (optional, row off[q] + q - mat_row0) and bp
// (backpointers, Viterbi only, row off[q] + q - bp_row0 of this launch).  Writes logp[q] and, for Viterbi, last[q]: the
// state the path ends in (end for a finite model, else the best state of step n, lowest index on a tie).
template <int MODE, typename BP, typename MD = HmmDev>
__global__ __launch_bounds__(HMM_NT) void hmm_fwd_kernel(MD M, const double *obs, const long long *off, int q0,
                                                         double *logp, double *mat, long long mat_row0, BP *bp,
                                                         long long bp_row0, int *last)
{
#pragma clang fp contract(off)
    extern __shared__ double hm_lds[];
    const int S = M.S, NE = M.n_emit, lane = threadIdx.x;
    const int q = q0 + blockIdx.x;
    const long long base = off[q];
    const int n = static_cast<int>(off[q + 1] - base);
    const double *x = obs + base * hmm_dim(M);
    const long long row0 = base + q;
    double *prev = hm_lds, *cur = hm_lds + S;
    constexpr double NEG = -__builtin_inf();

    // silent states of step t, level by level, from row `cur`
    auto silent_phase = [&](int t) {
        BP *bprow = MODE == HMM_VITERBI ? bp + (row0 - bp_row0 + t) * S : nullptr;
        for (int L = 0; L < M.n_levels; ++L) {
            const int hi = M.level_ptr[L + 1];
            for (int k = M.level_ptr[L] + lane; k < hi; k += HMM_NT) {
                const int e0 = M.in_ptr[k], e1 = M.in_ptr[k + 1];
                const bool init = t == 0 && k == M.start;
                if (MODE == HMM_VITERBI) {
                    double best = init ? 0.0 : NEG; int arg = 0;
                    for (int e = e0; e < e1; ++e) {
                        const double v = cur[M.in_src[e]] + M.in_lp[e];
                        if (v > best) { best = v; arg = e - e0; }
                    }
                    cur[k] = best;
                    bprow[k] = static_cast<BP>(arg);
                } else {
                    HmmLse acc;
                    if (init) acc.add(0.0);
                    for (int e = e0; e < e1; ++e) acc.add(cur[M.in_src[e]] + M.in_lp[e]);
                    cur[k] = acc.get();
                }
            }
            hm_sync();
        }
    };
    auto store_row = [&](int t) {
        if (mat) {
            double *dst = mat + (row0 - mat_row0 + t) * S;
            for (int k = lane; k < S; k += HMM_NT) dst[k] = cur[k];
        }
    };

    for (int k = lane; k < NE; k += HMM_NT) {
        cur[k] = NEG;
        if (MODE == HMM_VITERBI) bp[(row0 - bp_row0) * S + k] = 0;
    }
    hm_sync();
    silent_phase(0);
    store_row(0);
    for (int t = 1; t <= n; ++t) {
        double *tmp = prev; prev = cur; cur = tmp;
        const auto xt = hmm_obs(M, x, t - 1);
        BP *bprow = MODE == HMM_VITERBI ? bp + (row0 - bp_row0 + t) * S : nullptr;
        for (int k = lane; k < NE; k += HMM_NT) {
            const int e0 = M.in_ptr[k], e1 = M.in_ptr[k + 1];
            double v;
            if (MODE == HMM_VITERBI) {
                double best = NEG; int arg = 0;
                for (int e = e0; e < e1; ++e) {
                    const double c = prev[M.in_src[e]] + M.in_lp[e];
                    if (c > best) { best = c; arg = e - e0; }
                }
                bprow[k] = static_cast<BP>(arg);
                v = best;
            } else {
                HmmLse acc;
                for (int e = e0; e < e1; ++e) acc.add(prev[M.in_src[e]] + M.in_lp[e]);
                v = acc.get();
            }
            cur[k] = v > NEG ? v + hmm_emit(M, k, xt) : NEG;
        }
        hm_sync();
        silent_phase(t);
        store_row(t);
    }

    // the result of the sequence
    if (M.finite) {
        if (lane == 0) {
            logp[q] = cur[M.end];
            if (MODE == HMM_VITERBI) last[q] = M.end;
        }
        return;
    }
    double m = NEG; int am = 0x7fffffff;
    for (int k = lane; k < S; k += HMM_NT) if (cur[k] > m) { m = cur[k]; am = k; }
    for (int d = 32; d; d >>= 1) {
        const double om = __shfl_xor(m, d); const int oa = __shfl_xor(am, d);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    if (MODE == HMM_VITERBI) {
        if (lane == 0) { logp[q] = m; last[q] = am; }
        return;
    }
    double r = 0.0;
    if (m > NEG)
        for (int k = lane; k < S; k += HMM_NT) if (k != am) r += exp(cur[k] - m);
    for (int d = 32; d; d >>= 1) r += __shfl_xor(r, d);
    if (lane == 0) logp[q] = m > NEG ? m + log1p(r) : NEG;
}

// The backward recursion, written once for hmm_bwd_kernel, hmm_expect_kernel and hmm_posterior_kernel:  b[n][k] starts from
// log 1 at end (finite model) or at every state (infinite),  b[t][k] = logsumexp over out-edges k -> l of  lp + (l emitting ?
// e_l(x_t) + b[t+1][l] : b[t][l]).  The kernels differ only in their hooks (generic lambdas, inlined):
//   fwd(k, t)            what the kernel folds in for state k at step t (f[t][k]; hmm_bwd_kernel: nothing), handed to
//   term(e, v, fk)       every term v the sum of state k forms for out-edge e, in edge order, right after it is added;
//   emitted(k, t, fk, b) an emitting state whose b[t][k] = b is finished (same lane, right after its last term);
//   row(t, cur)          row t finished and fenced.

// b[t][k] from rows nxt (row t+1 with the emission of observation t added: emitting successors) and cur (row t: silent ones)
template <typename MD, typename Term>
__device__ __forceinline__ double hmm_bwd_state(const MD &M, const double *nxt, double *cur, int k, int t, int n, double fk,
                                                Term &&term)
{
#pragma clang fp contract(off)
    const int NE = M.n_emit;
    HmmLse acc;
    if (t == n && (!M.finite || k == M.end)) acc.add(0.0);
    const int e0 = M.out_ptr[k], e1 = M.out_ptr[k + 1];
    for (int e = e0; e < e1; ++e) {
        const int l = M.out_dst[e];
        if (l < NE && t >= n) continue;
        const double v = (l < NE ? nxt[l] : cur[l]) + M.out_lp[e];
        acc.add(v);
        term(e, v, fk);
    }
    const double b = acc.get();
    cur[k] = b;
    return b;
}

// Steps t = n .. 0 of one sequence x[0, n) with the two score rows in rows[0, 2 S): the silent levels from the top down, then
// the emitting states.  Returns row 0.
template <typename MD, typename Fwd, typename Term, typename Emitted, typename Row>
__device__ __forceinline__ const double *hmm_bwd_sweep(const MD &M, const double *x, int n, double *rows, Fwd &&fwd, Term &&term,
                                                       Emitted &&emitted, Row &&row)
{
#pragma clang fp contract(off)
    const int NE = M.n_emit, lane = threadIdx.x;
    double *nxt = rows, *cur = rows + M.S;
    constexpr double NEG = -__builtin_inf();
    for (int t = n; t >= 0; --t) {
        if (t < n) {
            double *tmp = nxt; nxt = cur; cur = tmp;
            const auto xt = hmm_obs(M, x, t);
            for (int l = lane; l < NE; l += HMM_NT) nxt[l] = nxt[l] > NEG ? nxt[l] + hmm_emit(M, l, xt) : NEG;
            hm_sync();
        }
        for (int L = M.n_levels - 1; L >= 0; --L) {
            const int hi = M.level_ptr[L + 1];
            for (int k = M.level_ptr[L] + lane; k < hi; k += HMM_NT) hmm_bwd_state(M, nxt, cur, k, t, n, fwd(k, t), term);
            hm_sync();
        }
        for (int k = lane; k < NE; k += HMM_NT) {
            const double fk = fwd(k, t);
            emitted(k, t, fk, hmm_bwd_state(M, nxt, cur, k, t, n, fk, term));
        }
        hm_sync();
        row(t, cur);
    }
    return cur;
}

// Backward over one sequence per workgroup.  Row t of sequence q goes to mat (optional) at row off[q] + q + t;
// logp[q] = b[0][start].
template <typename MD = HmmDev>
__global__ __launch_bounds__(HMM_NT) void hmm_bwd_kernel(MD M, const double *obs, const long long *off, int q0,
                                                         double *logp, double *mat)
{
#pragma clang fp contract(off)
    extern __shared__ double hm_lds[];
    const int S = M.S, lane = threadIdx.x;
    const int q = q0 + blockIdx.x;
    const long long base = off[q];
    const int n = static_cast<int>(off[q + 1] - base);
    const long long row0 = base + q;
    const double *b0 = hmm_bwd_sweep(
        M, obs + base * hmm_dim(M), n, hm_lds, [](int, int) { return 0.0; }, [](int, double, double) {},
        [](int, int, double, double) {},
        [&](int t, const double *cur) {
            if (mat) {
                double *dst = mat + (row0 + t) * S;
                for (int k = lane; k < S; k += HMM_NT) dst[k] = cur[k];
            }
        });
    if (lane == 0) logp[q] = b0[M.start];
}

// E-step of Baum-Welch (ps_hmm_expect): the backward recursion with the expectations folded in.  The forward matrix of the
// launch's sequences is in HBM (fmat, sequence q at row off[q] + q - f_row0, from hmm_fwd_kernel); the backward rows stay in
// LDS and are never written out.  With w = f[t][k] - logp[q], every out-edge term the recursion forms for state k at step t
// -- nxt[l] + lp (l emitting, b[t+1][l] + e_l(x_t) + lp) or cur[l] + lp (l silent) -- adds exp(w + term) to the count of
// that edge, and an emitting state k adds its posterior exp(f[t][k] + b[t][k] - logp[q]) to (W, A, B) with the observation
// x[t-1] shifted by c_k = param[3k]; a vector model's state adds it to W once and to (A_d, B_d) per component (hmm_stat).
//
// Accumulators: one row of n_acc = E + (1 + 2 D) NE + 3 n_mix + 1 doubles per workgroup (edge counts in out-edge order, W
// and (A_d, B_d) for d < D per emitting state -- D = 1, so (W, A, B), unless the model is a vector model --, one (W, A, B)
// per mixture component of a model with mixture states (hmm_mix_stat), the number of sequences skipped for logp = -inf).  Workgroup g takes the sequences q = g (mod gridDim.x)
// of [q0, q1), in ascending order, so its row sums the same sequences in the same order however the batch is cut into
// launches.  An edge belongs to the lane that owns its source state (and a state's statistics to the lane that owns the
// state) in every step, so a row needs no atomics.  ACC_LDS: the row is loaded into LDS next to the two score rows and
// stored back at the end; otherwise it is updated in place in global memory.
template <bool ACC_LDS, typename MD = HmmDev>
__global__ __launch_bounds__(HMM_NT) void hmm_expect_kernel(MD M, const double *obs, const long long *off, int q0, int q1,
                                                            const double *logp, const double *fmat, long long f_row0,
                                                            double *acc_rows, int n_acc)
{
#pragma clang fp contract(off)
    extern __shared__ double hm_lds[];
    const int S = M.S, lane = threadIdx.x, G = gridDim.x;
    const int E = M.out_ptr[S];
    double *acc_g = acc_rows + static_cast<long long>(blockIdx.x) * n_acc;
    double *acc = ACC_LDS ? hm_lds + 2 * S : acc_g;
    double *cnt = acc, *st = acc + E;
    constexpr double NEG = -__builtin_inf();
    if (ACC_LDS) {
        for (int i = lane; i < n_acc; i += HMM_NT) acc[i] = acc_g[i];
        hm_sync();
    }
    int qs = q0 + static_cast<int>((static_cast<long long>(blockIdx.x) - q0 % G + G) % G);
    for (int q = qs; q < q1; q += G) {
        const double lq = logp[q];
        if (!(lq > NEG)) {
            if (lane == 0) acc[n_acc - 1] += 1.0;
            continue;
        }
        const long long base = off[q];
        const int n = static_cast<int>(off[q + 1] - base);
        const double *x = obs + base * hmm_dim(M);
        const double *f = fmat + (base + q - f_row0) * S;
        hmm_bwd_sweep(
            M, x, n, hm_lds, [&](int k, int t) { return f[static_cast<long long>(t) * S + k]; },
            [&](int e, double v, double fk) {
                const double w = fk - lq;
                if (w > NEG && v > NEG) cnt[e] += exp(w + v);
            },
            [&](int k, int t, double fk, double bk) {
                if (t > 0 && fk > NEG && bk > NEG) {
                    const double g = exp(fk + bk - lq);
                    const int D = hmm_dim(M);
                    double *s = st + (1 + 2 * D) * k;
                    const auto xt = hmm_obs(M, x, t - 1);
                    s[0] += g;
                    for (int c = 0; c < D; ++c) {
                        const double d = hmm_stat(M, k, c, xt);
                        const double gd = g * d;
                        s[1 + 2 * c] += gd;
                        s[2 + 2 * c] += gd * d;
                    }
                    hmm_mix_stat(M, k, xt, g, st + (1 + 2 * D) * M.n_emit);
                }
            },
            [](int, const double *) {});
    }
    if (ACC_LDS) {
        hm_sync();
        for (int i = lane; i < n_acc; i += HMM_NT) acc_g[i] = acc[i];
    }
}

// The per-workgroup rows of hmm_expect_kernel summed in workgroup order (one thread per entry: a fixed order, so the same
// rows give the same bits): counts[E], stats[(1 + 2 D) NE], *skipped.
__global__ __launch_bounds__(256) void hmm_expect_reduce_kernel(const double *acc_rows, int G, int n_acc, int E,
                                                                double *counts, double *stats, double *skipped)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_acc) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += acc_rows[static_cast<long long>(g) * n_acc + i];
    if (i < E) counts[i] = s;
    else if (i < n_acc - 1) stats[i - E] = s;
    else *skipped = s;
}

// Posterior decoding (ps_hmm_posterior): the two passes of the E-step with every per-step value kept per observation
// instead of summed over the batch.  One workgroup of one wave per sequence q of [q0, q0 + gridDim.x); the forward matrix
// of the launch is in HBM (fmat, as for hmm_expect_kernel), the two backward rows stay in LDS.  For observation t (0 <= t
// < n) and emitting state k the log posterior is  (f[t+1][k] + b[t+1][k]) - logp[q],  -inf where either term is -inf.
// Every output is optional (null: skipped) and belongs to one sequence, so nothing is accumulated across workgroups:
//   post       row off[q] + t, NE doubles: the log posteriors of observation t (stores coalesced over k);
//   map_state  at off[q] + t: the emitting state of the largest entry of that row.  A lane keeps the maximum of its states
//              k = lane, lane + 64, ... (ascending, replaced only by a strictly greater value), the lanes' maxima are
//              combined by an xor butterfly that prefers the lower state on equal values: the lowest index wins a tie;
//   map_logp   [q]: the sum of those maxima in ascending t.  The butterfly leaves the maximum in every lane; lane t % 64
//              parks it in pmax[off[q] + t] (a scratch of one double per observation), and after the last step each lane
//              reads back the entries it wrote, 64 at a time, and the wave adds them in order of t;
//   counts_seq row q of E doubles: the sequence's expected count of every out-edge, formed as hmm_expect_kernel forms
//              cnt[e], zeroed here by the lane that owns the edge's source state (CNT 1: the row is updated in place in
//              global memory, CNT 2: in LDS behind the score rows and stored at the end; CNT 0: no counts).
// logp[q] = -inf: the rows of post are -inf, map_state -1, map_logp -inf, the counts row 0.  n = 0: no rows, map_logp 0.0,
// and the counts row holds the silent edges of step 0.
template <int CNT, typename MD = HmmDev>
__global__ __launch_bounds__(HMM_NT) void hmm_posterior_kernel(MD M, const double *obs, const long long *off, int q0,
                                                               const double *logp, const double *fmat, long long f_row0,
                                                               double *post, int *map_state, double *map_logp,
                                                               double *pmax, double *counts_seq)
{
#pragma clang fp contract(off)
    extern __shared__ double hm_lds[];
    const int S = M.S, NE = M.n_emit, lane = threadIdx.x;
    const int E = M.out_ptr[S];
    const int q = q0 + blockIdx.x;
    const long long base = off[q];
    const int n = static_cast<int>(off[q + 1] - base);
    const double lq = logp[q];
    constexpr double NEG = -__builtin_inf();
    double *crow = CNT ? counts_seq + static_cast<long long>(q) * E : nullptr;
    double *cnt = CNT == 2 ? hm_lds + 2 * S : crow;

    if (!(lq > NEG)) {
        if (post)
            for (long long i = lane, m = static_cast<long long>(n) * NE; i < m; i += HMM_NT) post[base * NE + i] = NEG;
        if (map_state)
            for (int t = lane; t < n; t += HMM_NT) map_state[base + t] = -1;
        if (map_logp && lane == 0) map_logp[q] = NEG;
        if (CNT)
            for (int e = lane; e < E; e += HMM_NT) crow[e] = 0.0;
        return;
    }
    if (CNT)        // (by the lane that adds to the edge in every step: no ordering between lanes is needed)
        for (int k = lane; k < S; k += HMM_NT)
            for (int e = M.out_ptr[k], e1 = M.out_ptr[k + 1]; e < e1; ++e) cnt[e] = 0.0;

    const double *f = fmat + (base + q - f_row0) * S;
    const bool want_map = map_state || map_logp;
    double m = NEG; int am = 0x7fffffff;      // the lane's largest log posterior of the step and its state
    hmm_bwd_sweep(
        M, obs + base * hmm_dim(M), n, hm_lds, [&](int k, int t) { return f[static_cast<long long>(t) * S + k]; },
        [&](int e, double v, double fk) {
            const double w = fk - lq;
            if (CNT && w > NEG && v > NEG) cnt[e] += exp(w + v);
        },
        [&](int k, int t, double fk, double bk) {
            if (t > 0) {
                const double v = (fk > NEG && bk > NEG) ? (fk + bk) - lq : NEG;
                if (post) post[(base + t - 1) * NE + k] = v;
                if (v > m) { m = v; am = k; }
            }
        },
        [&](int t, const double *) {
            if (t > 0 && want_map) {
                for (int d = 32; d; d >>= 1) {
                    const double om = __shfl_xor(m, d); const int oa = __shfl_xor(am, d);
                    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
                }
                if (lane == ((t - 1) & (HMM_NT - 1))) {
                    if (map_state) map_state[base + t - 1] = m > NEG ? am : -1;
                    if (map_logp) pmax[base + t - 1] = m;
                }
            }
            m = NEG; am = 0x7fffffff;
        });
    if (CNT == 2) {
        hm_sync();
        for (int e = lane; e < E; e += HMM_NT) crow[e] = cnt[e];
    }
    if (map_logp) {
        double s = 0.0;
        for (int c = 0; c < n; c += HMM_NT) {
            const double v = c + lane < n ? pmax[base + c + lane] : 0.0;      // (written by this lane)
            const int m = n - c < HMM_NT ? n - c : HMM_NT;
            for (int j = 0; j < m; ++j) s += __shfl(v, j);
        }
        if (lane == 0) map_logp[q] = s;
    }
}

// Viterbi traceback, one lane per sequence: from (n, last[q]) back to (0, start).  An emitting state steps back one
// observation, a silent one stays.  The path goes to path[path_off[q] ..] in forward order when it fits; path_len[q] is its
// length either way (0: the sequence is impossible).  *flags: bit 0 a path did not fit, bit 1 a walk left the model (a bug).
template <typename BP>
__global__ __launch_bounds__(HMM_NT) void hmm_trace_kernel(HmmDev M, const long long *off, int q0, int nq, const BP *bp,
                                                           long long bp_row0, const int *last, const double *logp,
                                                           const long long *path_off, int *path, int *path_len, int *flags)
{
    const int i = blockIdx.x * HMM_NT + threadIdx.x;
    if (i >= nq) return;
    const int q = q0 + i, S = M.S;
    const long long base = off[q];
    const int n = static_cast<int>(off[q + 1] - base);
    const BP *b = bp + (base + q - bp_row0) * S;
    if (!(logp[q] > -__builtin_inf())) { path_len[q] = 0; return; }
    const long long bound = static_cast<long long>(n + 1) * S + 1;
    long long len = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int t = n, k = last[q];
        long long w = path_off[q] + len - 1;
        for (long long c = 0;; ++c) {
            if (c >= bound || k < 0 || k >= S || (k < M.n_emit && t == 0)) { atomicOr(flags, 2); path_len[q] = 0; return; }
            if (pass) path[w - c] = k;
            if (t == 0 && k == M.start) { if (!pass) len = c + 1; break; }
            const int e0 = M.in_ptr[k], e = e0 + static_cast<int>(b[static_cast<long long>(t) * S + k]);
            if (e >= M.in_ptr[k + 1]) { atomicOr(flags, 2); path_len[q] = 0; return; }
            if (k < M.n_emit) --t;
            k = M.in_src[e];
        }
        if (!pass) {
            path_len[q] = static_cast<int>(len);
            if (len > path_off[q + 1] - path_off[q]) { atomicOr(flags, 1); return; }
        }
    }
}

// ---- sampling (ps_hmm_sample) ----------------------------------------------------------------------------------------
// A walk from `start` along the out-edges, an observation drawn on entering an emitting state.  The decoding kernels above
// spread one sequence's states over a wave; a walk touches one state per step, so here it is one lane per sequence: lane l
// of workgroup g owns sequence q = g * HMM_NT + l, keeps (k, j, emitted, path_len) in registers, reads the model and the
// sampling tables through global memory and writes its own slots.  No LDS, no atomics, no barrier.
//
// The random stream is counter-based, Philox4x32-10 with key (seed low, seed high): sequence Q = first + q owns the blocks
// j = 0, 1, 2, ... at counter (j low, j high, Q low, Q high); a block of four words gives two doubles in [0, 1) and the
// walk consumes blocks strictly in walk order (one per transition, one per component of an emission, two for a
// kernel-density or a mixture state), so a walk's path and length depend on (seed, Q, out_cdf) alone, never on the values drawn.

struct HmmPhilox {
    unsigned r[4];
    __device__ __forceinline__ HmmPhilox(unsigned long long seed, unsigned long long Q, unsigned long long j)
    {
        unsigned c0 = static_cast<unsigned>(j), c1 = static_cast<unsigned>(j >> 32);
        unsigned c2 = static_cast<unsigned>(Q), c3 = static_cast<unsigned>(Q >> 32);
        unsigned k0 = static_cast<unsigned>(seed), k1 = static_cast<unsigned>(seed >> 32);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
            const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<unsigned>(p0 >> 32) ^ c3 ^ k1;
            c1 = static_cast<unsigned>(p1); c3 = static_cast<unsigned>(p0); c0 = n0; c2 = n2;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
    }
    // 53 bits of two words: a multiple of 2^-53 in [0, 1), so 1 - u is exact and > 0
    __device__ __forceinline__ static double unit(unsigned a, unsigned b)
    {
        return static_cast<double>((static_cast<unsigned long long>(a >> 5) << 26) | (b >> 6)) * 0x1p-53;
    }
    __device__ __forceinline__ double u0() const { return unit(r[0], r[1]); }
    __device__ __forceinline__ double u1() const { return unit(r[2], r[3]); }
    // a standard normal from the block's two doubles (Box-Muller, the cosine branch)
    __device__ __forceinline__ double normal() const
    {
#pragma clang fp contract(off)
        return sqrt(-2.0 * log(1.0 - u0())) * cos(6.283185307179586 * u1());
    }
};

// The first i of [lo, hi) with u < cdf[i], by bisection.  cdf ascends over [lo, hi - 1) and cdf[hi - 1] = 1.0 > u, so
// "u < cdf[i]" is false up to some i and true from there on: bisection finds the index a linear scan would.  hi > lo.
__device__ __forceinline__ int hmm_cdf_pick(const double *cdf, int lo, int hi, double u)
{
    --hi;                                   // (the last entry is never read: it is 1.0)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (u < cdf[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One draw of kind kd with the table's two parameters (a, b): normal (mean, std), uniform (low, high - low), log-normal
// (mu, sigma), exponential (0, rate).
__device__ __forceinline__ double hmm_draw(int kd, double a, double b, const HmmPhilox &R)
{
#pragma clang fp contract(off)
    if (kd == HMM_UNIFORM) return a + R.u0() * b;
    if (kd == HMM_EXPONENTIAL) return -log(1.0 - R.u0()) / b;
    const double v = a + b * R.normal();
    return kd == HMM_LOGNORMAL ? exp(v) : v;
}

// The emission of state k: its values go to x (null: drawn and dropped, the slot is full); j counts the blocks taken.
__device__ __forceinline__ void hmm_sample_emit(const HmmDev &M, const HmmSampleDev &T, int k, unsigned long long seed,
                                                unsigned long long Q, unsigned long long &j, double *x)
{
    const double v = hmm_draw(M.kind[k], T.emit_param[2 * k], T.emit_param[2 * k + 1], HmmPhilox(seed, Q, j++));
    if (x) *x = v;
}
__device__ __forceinline__ void hmm_sample_emit(const HmmDevK &M, const HmmSampleDev &T, int k, unsigned long long seed,
                                                unsigned long long Q, unsigned long long &j, double *x)
{
#pragma clang fp contract(off)
    if (M.kind[k] != HMM_KDE) return hmm_sample_emit(static_cast<const HmmDev &>(M), T, k, seed, Q, j, x);
    const int i = hmm_cdf_pick(T.kde_cdf, M.kde_ptr[k], M.kde_ptr[k + 1], HmmPhilox(seed, Q, j++).u0());
    const double v = M.kde_pt[i] + T.emit_param[2 * k + 1] * HmmPhilox(seed, Q, j++).normal();
    if (x) *x = v;
}
// a mixture state takes two blocks: the first component i with u0 < mix_cdf[i] (never one of weight 0), then its draw
__device__ __forceinline__ void hmm_sample_emit(const HmmDevM &M, const HmmSampleDev &T, int k, unsigned long long seed,
                                                unsigned long long Q, unsigned long long &j, double *x)
{
    if (M.kind[k] != HMM_MIXTURE) return hmm_sample_emit(static_cast<const HmmDevK &>(M), T, k, seed, Q, j, x);
    const int i = hmm_cdf_pick(M.mix_cdf, M.mix_ptr[k], M.mix_ptr[k + 1], HmmPhilox(seed, Q, j++).u0());
    const double v = hmm_draw(M.mix_kind[i], M.mix_draw[2 * i], M.mix_draw[2 * i + 1], HmmPhilox(seed, Q, j++));
    if (x) *x = v;
}
__device__ __forceinline__ void hmm_sample_emit(const HmmDevV &M, const HmmSampleDev &T, int k, unsigned long long seed,
                                                unsigned long long Q, unsigned long long &j, double *x)
{
    for (int d = 0, i = k * M.D; d < M.D; ++d, ++i) {
        const double v = hmm_draw(M.comp_kind[i], T.emit_param[2 * i], T.emit_param[2 * i + 1], HmmPhilox(seed, Q, j++));
        if (x) x[d] = v;
    }
}

// Sequence q of [0, nq): observations (hmm_dim(M) doubles each) into obs[off[q] .. off[q+1]), the path -- every state
// visited from start on, silent ones included; path null: none -- into path[path_off[q] .. path_off[q+1]).  What does not
// fit its slot is counted and not written: len[q] and path_len[q] (null: not kept) are the full lengths whatever the slots
// hold.  flags[q]: 0 the walk entered end or made its `length` emissions (length 0: no such stop), 1 it stopped at
// max_length emissions, 2 it stood in a state without out-edges.
//
// Termination: bake rejects cycles of silent states and the library checks that every silent edge goes up a level, so
// between two emissions a walk takes at most n_levels silent steps and one emitting step: at most
// (max_length + 1) * (n_levels + 1) + 1 transitions in all.  The loop is bounded by that as well.
template <typename MD = HmmDev>
__global__ __launch_bounds__(HMM_NT) void hmm_sample_kernel(MD M, HmmSampleDev T, unsigned long long seed, long long first,
                                                            int nq, int length, int max_length, double *obs,
                                                            const long long *off, int *len, int *flags, int *path,
                                                            const long long *path_off, int *path_len)
{
    const int q = blockIdx.x * HMM_NT + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long Q = static_cast<unsigned long long>(first) + static_cast<unsigned long long>(q);
    const int D = hmm_dim(M), NE = M.n_emit;
    const long long cap = off[q + 1] - off[q], pcap = path ? path_off[q + 1] - path_off[q] : 0;
    double *x = obs + off[q] * D;
    int *p = path ? path + path_off[q] : nullptr;
    const long long bound = (static_cast<long long>(max_length) + 1) * (M.n_levels + 1) + 1;
    unsigned long long j = 0;
    int k = M.start, emitted = 0, flag = 1;
    long long plen = 1;
    if (pcap > 0) p[0] = k;
    for (long long step = 0; step < bound; ++step) {
        if (k == M.end || (length > 0 && emitted >= length)) { flag = 0; break; }
        if (emitted >= max_length) break;
        const int e0 = M.out_ptr[k], e1 = M.out_ptr[k + 1];
        if (e0 == e1) { flag = 2; break; }
        k = M.out_dst[hmm_cdf_pick(T.out_cdf, e0, e1, HmmPhilox(seed, Q, j++).u0())];
        if (plen < pcap) p[plen] = k;
        ++plen;
        if (k < NE) {
            hmm_sample_emit(M, T, k, seed, Q, j, emitted < cap ? x + static_cast<long long>(emitted) * D : nullptr);
            ++emitted;
        }
    }
    len[q] = emitted;
    flags[q] = flag;
    if (path_len) path_len[q] = static_cast<int>(plen);
}

}  // namespace ps
