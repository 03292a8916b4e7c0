// seg_pairwise.hpp -- PairwiseAligner of the reference (PyPore/alignment.py:97-313) on gfx950: Needleman-Wunsch
// (global), Smith-Waterman (local) and the repeated local traceback, for batches of pairs and for all-vs-all scores.
//
// A cell is the maximum of three or four two-operand fp64 sums, first candidate winning a tie; there is no running
// chain whose rounding depends on the order, so the anti-diagonals run in parallel and stay bit-reproducible.  One
// 64-lane wave per pair; the rows go in stripes of 64, lane r owns row r of the stripe and at step t computes cell
// (r, t - r) from its own previous value (left), the previous value of lane r-1 (up) and the value lane r-1 held a step
// earlier (diagonal).  y and the stripe's last row (the next stripe's top border) live in LDS.  The workgroup is one
// wave: al_sync() (seg_align.hpp), no s_barrier.
//
// Score-only route (pw_score_kernel): nothing but the result leaves the chip.  Traceback route (pw_batch_kernel): the
// fp64 score matrix and one pointer byte per cell stream row-major to a per-workgroup scratch in HBM -- the repeated
// traceback rewrites cells, mirrored ones (j, i) included, and takes arg-maxima over rows, which row-major keeps
// coalesced -- together with the maximum of every row and its first column.  Lane 0 walks, the wave takes each arg-max
// over the row maxima and refreshes only the rows a walk touched.  fp64 throughout, no FMA contraction.
#pragma once

#include "batch_plan.hpp"                       // PW_NT, PW_N_MAX, pw_lds_bytes, pw_scratch_bytes

namespace ps {

constexpr double PW_NEGINF = -999999999.0;      // alignment.py NEGINF: the mark of a walked cell
constexpr int PW_GLOBAL = 0, PW_LOCAL = 1, PW_REPEATED = 2;
constexpr int PW_OK = 0, PW_INDEX = 1;          // per-pair status (include/poreseg.h)

// _score (alignment.py:112-115): 0 for the gap marker (uploaded as NaN), else 3 - |x - y|^2 with the square by product
__device__ __forceinline__ double pw_match(double x, double y)
{
#pragma clang fp contract(off)
    if (x != x || y != y) return 0.0;
    const double d = fabs(x - y);
    return 3.0 - d * d;
}

struct PwBest { double v; int i, j; };          // local mode: the maximum and its row-major-first cell (1-based; 0, 0: the border)

// The fill.  x: m row elements (global), ly: n column elements (LDS), top: n + 1 doubles of LDS.  TRACE: scores and
// pointer bytes of the m x n interior go to g_score / g_ptr (row-major), for LOCAL also every row's maximum and its
// first column (1-based).  Returns score[m][n]; for LOCAL without TRACE *best is the matrix maximum.
template <bool LOCAL, bool TRACE>
__device__ __forceinline__ double pw_fill(const double *x, int m, int n, double penalty, const double *ly, double *top,
                                          double *g_score, unsigned char *g_ptr, double *g_rowmax, int *g_rowcol, PwBest *best)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    for (int j = lane; j <= n; j += PW_NT) top[j] = LOCAL ? 0.0 : static_cast<double>(j) * penalty;
    al_sync();
    double bv = 0.0; int bi = 0, bj = 0;
    double cur = 0.0;
    for (int i0 = 0; i0 < m; i0 += PW_NT) {
        const int row = i0 + lane;
        const bool valid = row < m;
        const double xi = valid ? x[row] : 0.0;
        cur = LOCAL ? 0.0 : static_cast<double>(row + 1) * penalty;          // score[i][0]
        double diag = top[0];
        double rv = -__builtin_inf(); int rc = 0;
        const int steps = n + min(PW_NT, m - i0) - 1;
        const bool feeds = lane == PW_NT - 1 && i0 + PW_NT < m;              // this row is the next stripe's top border
        const long long ro = static_cast<long long>(row) * n;
        for (int t = 0; t < steps; ++t) {
            double up = __shfl_up(cur, 1);
            const double tv = top[min(t + 1, n)];
            if (lane == 0) up = tv;
            const int j = t - lane;
            if (valid && j >= 0 && j < n) {
                const double a = diag + pw_match(xi, ly[j]), b = cur + penalty, c = up + penalty;
                double v; int p;
                if (LOCAL) {
                    v = 0.0; p = 0;
                    if (a > v) { v = a; p = 1; }
                    if (b > v) { v = b; p = 2; }
                    if (c > v) { v = c; p = 3; }
                    if (TRACE) { if (v > rv) { rv = v; rc = j + 1; } }
                    else if (v > bv) { bv = v; bi = row + 1; bj = j + 1; }
                } else {
                    v = a; p = 0;
                    if (b > v) { v = b; p = 1; }
                    if (c > v) { v = c; p = 2; }
                }
                cur = v;
                if (TRACE) { g_score[ro + j] = v; g_ptr[ro + j] = static_cast<unsigned char>(p); }
                if (feeds) top[j + 1] = v;
            }
            diag = up;
        }
        if (TRACE && LOCAL && valid) { g_rowmax[row] = rv; g_rowcol[row] = rc; }
        if (i0 + PW_NT < m) {
            al_sync();
            if (lane == 0) top[0] = LOCAL ? 0.0 : static_cast<double>(i0 + PW_NT) * penalty;
            al_sync();
        }
    }
    if (LOCAL && !TRACE) {
        for (int d = 32; d; d >>= 1) {
            const double ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d), oj = __shfl_xor(bj, d);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; bj = oj; }
        }
        best->v = bv; best->i = bi; best->j = bj;
    }
    return __shfl(cur, (m - 1) & (PW_NT - 1));
}

// all pairs of A x B, scores only.  d_pos (local mode, may be null): 2 ints per pair, the cell of the maximum (0, 0: none above 0)
template <bool LOCAL>
__global__ __launch_bounds__(PW_NT) void pw_score_kernel(const double *a, const long long *a_off, int n_a, const double *b,
                                                         const long long *b_off, int n_b, double penalty, int n_cap,
                                                         double *scores, int *pos)
{
#pragma clang fp contract(off)
    extern __shared__ double pw_lds[];
    double *ly = pw_lds, *top = ly + n_cap;
    const int lane = threadIdx.x;
    const long long n_jobs = static_cast<long long>(n_a) * n_b;
    for (long long q = blockIdx.x; q < n_jobs; q += gridDim.x) {
        const int ia = static_cast<int>(q / n_b), ib = static_cast<int>(q % n_b);
        const double *x = a + a_off[ia], *y = b + b_off[ib];
        const int m = static_cast<int>(a_off[ia + 1] - a_off[ia]), n = static_cast<int>(b_off[ib + 1] - b_off[ib]);
        al_sync();
        for (int j = lane; j < n; j += PW_NT) ly[j] = y[j];
        double s; PwBest best = {0.0, 0, 0};
        if (m == 0 || n == 0) s = LOCAL ? 0.0 : static_cast<double>(m == 0 ? n : m) * penalty;
        else {
            s = pw_fill<LOCAL, false>(x, m, n, penalty, ly, top, nullptr, nullptr, nullptr, nullptr, &best);
            if (LOCAL) s = best.v;
        }
        if (lane == 0) {
            scores[q] = s;
            if (LOCAL && pos) { pos[2 * q] = best.i; pos[2 * q + 1] = best.j; }
        }
    }
}

struct PwBatch {
    const double *a, *b;
    const long long *a_off, *b_off, *col_off, *aln_off;       // col_off / aln_off: the pair's slots of columns / alignments
    const int *pair_a, *pair_b;
    int mode, min_length;
    double penalty;
    double *scores; int *status;
    int *cols_i, *cols_j;                                     // index columns in walk order (alignment end first), -1: gap
    int *col_need;                                            // columns the pair's alignments take
    double *aln_score; int *aln_start, *aln_len;              // per alignment: score, first column within the pair's slot, columns
    int *aln_count;                                           // alignments completed (before the error, if any)
    int *flag;                                                // 1: some slot was too small
};

template <bool LOCAL>
__global__ __launch_bounds__(PW_NT) void pw_batch_kernel(PwBatch P, int q0, int nq, int n_cap, unsigned char *scratch,
                                                         unsigned long long stride, unsigned long long cells_cap,
                                                         unsigned long long rows_cap)
{
#pragma clang fp contract(off)
    extern __shared__ double pw_lds[];
    double *ly = pw_lds, *top = ly + n_cap;
    const int lane = threadIdx.x;
    unsigned char *wg = scratch + static_cast<unsigned long long>(blockIdx.x) * stride;
    double *g_score = reinterpret_cast<double *>(wg), *g_rowmax = g_score + cells_cap;
    int *g_rowcol = reinterpret_cast<int *>(g_rowmax + rows_cap);
    unsigned char *g_ptr = reinterpret_cast<unsigned char *>(g_rowcol + rows_cap);

    for (int q = q0 + blockIdx.x; q < q0 + nq; q += gridDim.x) {
        const int ia = P.pair_a[q], ib = P.pair_b[q];
        const double *x = P.a + P.a_off[ia], *y = P.b + P.b_off[ib];
        const int m = static_cast<int>(P.a_off[ia + 1] - P.a_off[ia]), n = static_cast<int>(P.b_off[ib + 1] - P.b_off[ib]);
        const long long cbase = P.col_off[q], ccap = P.col_off[q + 1] - cbase;
        const long long abase = P.aln_off[q], acap = P.aln_off[q + 1] - abase;
        al_sync();
        for (int j = lane; j < n; j += PW_NT) ly[j] = y[j];
        double s = 0.0;
        if (m == 0 || n == 0) {
            // global: the border cell, no columns (:167 loops while i > 0 and j > 0); local: xalign[-1] of an empty list;
            // repeated: the arg-max is the border's 0 with pointer 0, nothing is yielded
            if (lane == 0) {
                P.scores[q] = LOCAL ? 0.0 : static_cast<double>(m == 0 ? n : m) * P.penalty;
                P.status[q] = P.mode == PW_LOCAL ? PW_INDEX : PW_OK;
                P.col_need[q] = 0;
                P.aln_count[q] = P.mode == PW_GLOBAL ? 1 : 0;
                if (P.mode == PW_GLOBAL) {
                    if (acap >= 1) { P.aln_score[abase] = P.scores[q]; P.aln_start[abase] = 0; P.aln_len[abase] = 0; }
                    else *P.flag = 1;
                }
            }
            continue;
        }
        s = pw_fill<LOCAL, true>(x, m, n, P.penalty, ly, top, g_score, g_ptr, g_rowmax, g_rowcol, nullptr);
        __threadfence();            // the fill's stores have arrived and the vector L1 holds no line of the pair before

        if (!LOCAL) {
            if (lane == 0) {        // :157-181
                int i = m, j = n; long long k = 0;
                while (i > 0 && j > 0) {
                    const int p = g_ptr[static_cast<long long>(i - 1) * n + (j - 1)];
                    if (k < ccap) { P.cols_i[cbase + k] = p == 1 ? -1 : i - 1; P.cols_j[cbase + k] = p == 2 ? -1 : j - 1; }
                    ++k;
                    if (p == 0) { --i; --j; } else if (p == 1) --j; else --i;
                }
                P.scores[q] = s; P.status[q] = PW_OK; P.col_need[q] = static_cast<int>(k); P.aln_count[q] = 1;
                if (acap >= 1) { P.aln_score[abase] = s; P.aln_start[abase] = 0; P.aln_len[abase] = static_cast<int>(k); }
                if (k > ccap || acap < 1) *P.flag = 1;
            }
            continue;
        }

        // local (:214-249) and local repeated (:251-294)
        long long kpos = 0; int count = 0, err = 0; double first_score = 0.0;
        for (int round = 0;; ++round) {
            // arg-max of the matrix: the first row holding the largest row maximum, its first column.  Nothing above 0:
            // the row-major-first maximum is the border cell (0, 0), whose pointer is 0
            double bv = -__builtin_inf(); int bi = 0x7fffffff;
            for (int r = lane; r < m; r += PW_NT) { const double v = g_rowmax[r]; if (v > bv) { bv = v; bi = r; } }
            for (int d = 32; d; d >>= 1) {
                const double ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (!(bv > 0.0)) {
                if (P.mode == PW_LOCAL) err = 1;            // :246 xalign[-1] of the empty list
                break;
            }
            if (round == 0) first_score = bv;
            const int i_start = bi + 1, j_start = g_rowcol[bi];
            int i_lo = i_start, j_lo = j_start, emit = 0;
            if (lane == 0) {
                int i = i_start, j = j_start, L = 0, clean = 0;
                while (i > 0 && j > 0) {                    // (a border cell's pointer is 0)
                    const long long idx = static_cast<long long>(i - 1) * n + (j - 1);
                    const int p = g_ptr[idx];
                    if (p == 0) break;
                    g_ptr[idx] = 0;
                    if (j > m || i > n) { err = 1; break; } // pointer[j, i] out of bounds: IndexError
                    const long long mid = static_cast<long long>(j - 1) * n + (i - 1);
                    g_ptr[mid] = 0; g_score[idx] = PW_NEGINF; g_score[mid] = PW_NEGINF;
                    i_lo = i; j_lo = j;
                    const long long k = kpos + L;
                    if (k < ccap) { P.cols_i[cbase + k] = p == 2 ? -1 : i - 1; P.cols_j[cbase + k] = p == 3 ? -1 : j - 1; }
                    ++L;
                    // :246-248 trims the alignment's start while either side is '-': a gap, or the caller's own marker
                    if (p == 1 && x[i - 1] == x[i - 1] && ly[j - 1] == ly[j - 1]) clean = L;
                    if (p == 1) { --i; --j; } else if (p == 2) --j; else --i;
                }
                if (!err && !(P.mode == PW_REPEATED && L < P.min_length)) {
                    if (clean == 0) err = 1;                // trimmed to nothing: xalign[-1] of the empty list
                    else {
                        if (count < acap) { P.aln_score[abase + count] = bv; P.aln_start[abase + count] = static_cast<int>(kpos); P.aln_len[abase + count] = clean; }
                        emit = clean;
                    }
                }
            }
            err = __shfl(err, 0); emit = __shfl(emit, 0); i_lo = __shfl(i_lo, 0); j_lo = __shfl(j_lo, 0);
            if (emit) { kpos += emit; ++count; }
            if (err || P.mode == PW_LOCAL) break;
            // the rows the walk touched: its own (i_lo .. i_start) and the mirrored ones (j_lo .. j_start)
            __threadfence();
            for (int part = 0; part < 2; ++part) {
                const int lo = part ? j_lo : i_lo, hi = part ? j_start : i_start;
                for (int r = lo; r <= hi; ++r) {
                    if (part && r >= i_lo && r <= i_start) continue;
                    const double *row = g_score + static_cast<long long>(r - 1) * n;
                    double rv = -__builtin_inf(); int rc = 0x7fffffff;
                    for (int c = lane; c < n; c += PW_NT) { const double v = row[c]; if (v > rv) { rv = v; rc = c + 1; } }
                    for (int d = 32; d; d >>= 1) {
                        const double ov = __shfl_xor(rv, d); const int oc = __shfl_xor(rc, d);
                        if (ov > rv || (ov == rv && oc < rc)) { rv = ov; rc = oc; }
                    }
                    if (lane == 0) { g_rowmax[r - 1] = rv; g_rowcol[r - 1] = rc; }
                }
            }
            __threadfence();
        }
        if (lane == 0) {
            P.scores[q] = first_score; P.status[q] = err ? PW_INDEX : PW_OK;
            P.col_need[q] = static_cast<int>(kpos); P.aln_count[q] = count;
            if (kpos > ccap || count > acap) *P.flag = 1;
        }
        __threadfence();            // the next pair of this workgroup rewrites the scratch
    }
}

}  // namespace ps
