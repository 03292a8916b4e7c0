// seg_trf.hpp -- NaiveSplitter, the inner generator of the reference's NaiveTRF (PyPore/alignment.py:806-870), on gfx950:
// a local self-alignment of one sequence of segments (mean, std) whose best off-diagonal path is pulled out, masked and
// the matrix filled again, until nothing scores above min_score.  DESIGN.md 7n has the semantics and their proofs.
//
// One 64-lane wave per sequence, the whole fill -> arg-max -> walk -> mask loop in one launch.  Only the strict upper
// triangle (j > i) is computed: with penalty < 0 and min_score >= 0 the diagonal is never a source (the identity mask
// covers it) nor the arg-max, and the lower triangle mirrors the upper.  The rows go in stripes of 64; lane r owns row
// i = i0 + r + 1 of the stripe and at step t computes cell (i, i0 + 1 + t - r) from its own previous value (left), the
// previous value of lane r-1 (up) and the value lane r-1 held a step earlier (diagonal), all moved by __shfl_up.  What
// moves is the cell's value AS A SOURCE: -inf for a masked cell, so a masked source loses every strict comparison
// against the candidate 0 (the reference's -999 does no more than that).  The column operands and the stripe's last row
// (the next stripe's top border; at first row 0 of the matrix: 0, or -inf where an end cell was marked) live in LDS.
// The workgroup is one wave: al_sync() (seg_align.hpp), no s_barrier.
//
// No score is stored.  The arg-max is tracked per lane as (value, i, j) with strict >, so the first cell of a row and
// the first stripe win a tie, and reduced over the wave to the row-major-first cell.  The walk needs the pointer (2
// bits) and the mask (1 bit) of a cell: they live in a per-workgroup scratch in HBM in SKEWED coordinates -- bit t of
// row i, t the step at which the row's lane computed the cell -- so that every lane loads one aligned 64-bit mask word
// per 64 steps and stores one aligned 128-bit pointer block per 64 steps, all lanes at the same step.  Row 0 keeps its
// mask bits by column.  Lane 0 walks, sets mask bits and appends (score, length, i, j) to the sequence's slot.
// fp64 throughout, no FMA contraction, IEEE division.
#pragma once

#include "batch_plan.hpp"                       // TRF_NT, TRF_N_MAX, trf_lds_bytes, trf_row_words, trf_scratch_bytes

namespace ps {

constexpr int TRF_DONE = 0, TRF_MAX_REPEATS = 1;    // per-sequence status (include/poreseg.h)

// _score (alignment.py:812): 2 - |x.mean - y.mean| ** 2 / (x.std * y.std), the square by product
__device__ __forceinline__ double trf_match(double mi, double si, double mj, double sj)
{
#pragma clang fp contract(off)
    const double d = fabs(mi - mj);
    const double q = (d * d) / (si * sj);
    return 2.0 - q;
}

struct TrfBatch {
    const double *mean, *std;
    const long long *off, *slot_off;
    double penalty, min_score;
    long long max_repeats;                                    // 0: no cap
    double *score; int *len, *i, *j;                          // the yields, sequence q's in slot [slot_off[q], slot_off[q+1])
    int *count, *status;
    int *flag;                                                // 1: some slot was too small
};

// skewed position of cell (i, j), 1 <= i < j: the row's lane computes it at step t of its stripe
__device__ __forceinline__ int trf_step(int i, int j) { return j - 1 - (((i - 1) >> 6) << 6) + ((i - 1) & 63); }

// One fill of the strict upper triangle with the mask as it stands.  lm / ls: the n means / stds (LDS), top: n + 1
// doubles of LDS.  g_mask: row 0 by column, rows 1 .. n by step; g_ptr: rows 1 .. n by step, 2 bits per cell.
// Returns in (*out_v, *out_i, *out_j), on every lane, the row-major-first maximum; (0, 0, 0) when no cell is above 0.
__device__ __forceinline__ void trf_fill(int n, double penalty, const double *lm, const double *ls, double *top,
                                         const unsigned long long *g_mask, unsigned long long *g_ptr, unsigned long long W,
                                         double *out_v, int *out_i, int *out_j)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const double NEG = -__builtin_inf();
    for (int j = lane; j <= n; j += TRF_NT) top[j] = ((g_mask[j >> 6] >> (j & 63)) & 1ull) ? NEG : 0.0;
    al_sync();
    double bv = 0.0; int bi = 0, bj = 0;
    for (int i0 = 0; i0 < n; i0 += TRF_NT) {
        const int i = i0 + lane + 1, c0 = i0 + 1;
        const bool valid = i <= n;
        const double mi = valid ? lm[i - 1] : 0.0, si = valid ? ls[i - 1] : 1.0;
        const int steps = n - c0 + min(TRF_NT, n - i0);                  // the last valid lane reaches column n
        const bool feeds = lane == TRF_NT - 1 && i0 + TRF_NT < n;        // this row is the next stripe's top border
        const unsigned long long *mrow = g_mask + static_cast<unsigned long long>(valid ? i : 0) * W;
        unsigned long long *prow = g_ptr + static_cast<unsigned long long>(valid ? i - 1 : 0) * 2ull * W;
        double cur = NEG, diag = NEG;                                    // (i, i): masked by the identity
        unsigned long long mw = 0, plo = 0, phi = 0;
        for (int t = 0; t < steps; ++t) {
            double up = __shfl_up(cur, 1);
            const double tv = top[min(c0 + t, n)];
            if (lane == 0) up = tv;
            if ((t & 63) == 0) mw = valid ? mrow[t >> 6] : 0ull;
            const int j = c0 + t - lane;
            if (valid && j > i && j <= n) {
                const double a = diag + trf_match(mi, si, lm[j - 1], ls[j - 1]), b = cur + penalty, c = up + penalty;
                double v = 0.0; unsigned long long p = 0;
                if (a > v) { v = a; p = 1; }
                if (b > v) { v = b; p = 2; }
                if (c > v) { v = c; p = 3; }
                if (v > bv) { bv = v; bi = i; bj = j; }
                cur = ((mw >> (t & 63)) & 1ull) ? NEG : v;
                if (t & 32) phi |= p << (2 * (t & 31)); else plo |= p << (2 * (t & 31));
                if (feeds) top[j] = cur;
            }
            diag = up;
            if ((t & 63) == 63 || t == steps - 1) {
                if (valid) { prow[2 * (t >> 6)] = plo; prow[2 * (t >> 6) + 1] = phi; }
                plo = 0; phi = 0;
            }
        }
        al_sync();
    }
    for (int d = 32; d; d >>= 1) {
        const double ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d), oj = __shfl_xor(bj, d);
        if (ov > bv || (ov == bv && (oi < bi || (oi == bi && oj < bj)))) { bv = ov; bi = oi; bj = oj; }
    }
    *out_v = bv; *out_i = bi; *out_j = bj;
}

__global__ __launch_bounds__(TRF_NT) void trf_kernel(TrfBatch P, int q0, int nq, int n_cap, unsigned char *scratch,
                                                     unsigned long long stride)
{
#pragma clang fp contract(off)
    extern __shared__ double trf_lds[];
    double *lm = trf_lds, *ls = lm + n_cap, *top = ls + n_cap;
    const int lane = threadIdx.x;
    const unsigned long long W = trf_row_words(n_cap);
    unsigned long long *g_mask = reinterpret_cast<unsigned long long *>(scratch + static_cast<unsigned long long>(blockIdx.x) * stride);
    unsigned long long *g_ptr = g_mask + W * (static_cast<unsigned long long>(n_cap) + 1ull);

    for (int q = q0 + blockIdx.x; q < q0 + nq; q += gridDim.x) {
        const long long base = P.off[q];
        const int n = static_cast<int>(P.off[q + 1] - base);
        const long long sbase = P.slot_off[q], scap = P.slot_off[q + 1] - sbase;
        if (n > n_cap) continue;                        // (the host sized n_cap to the launch's longest sequence)
        al_sync();
        for (int k = lane; k < n; k += TRF_NT) { lm[k] = P.mean[base + k]; ls[k] = P.std[base + k]; }
        const unsigned long long mask_words = W * (static_cast<unsigned long long>(n) + 1ull);
        for (unsigned long long k = lane; k < mask_words; k += TRF_NT) g_mask[k] = 0ull;
        __threadfence();
        al_sync();
        long long count = 0; int status = TRF_DONE;
        // every repeat masks a cell that was not masked before, so (n + 1)^2 bounds the loop whatever the input
        const long long bound = (static_cast<long long>(n) + 1) * (static_cast<long long>(n) + 1);
        while (n >= 2 && count < bound) {
            if (P.max_repeats > 0 && count >= P.max_repeats) { status = TRF_MAX_REPEATS; break; }
            double bv; int bi, bj;
            trf_fill(n, P.penalty, lm, ls, top, g_mask, g_ptr, W, &bv, &bi, &bj);
            if (!(bv > P.min_score)) break;
            __threadfence();        // the fill's pointer stores have arrived before lane 0 reads them
            if (lane == 0) {
                int i = bi, j = bj, L = 0;
                while (i >= 1 && j > i && j <= n) {
                    const int t = trf_step(i, j);
                    const int p = static_cast<int>((g_ptr[(static_cast<unsigned long long>(i) - 1ull) * 2ull * W + (t >> 5)] >> (2 * (t & 31))) & 3ull);
                    if (p == 0) break;
                    ++L;
                    g_mask[static_cast<unsigned long long>(i) * W + (t >> 6)] |= 1ull << (t & 63);
                    if (p == 1) { --i; --j; } else if (p == 2) --j; else --i;
                }
                // the cell the walk ended on: in row 0 by column, else by step (a cell on the diagonal is masked already)
                if (i == 0 && j >= 0 && j <= n) g_mask[j >> 6] |= 1ull << (j & 63);
                else if (i >= 1 && j > i && j <= n) { const int t = trf_step(i, j); g_mask[static_cast<unsigned long long>(i) * W + (t >> 6)] |= 1ull << (t & 63); }
                if (count < scap) { P.score[sbase + count] = bv; P.len[sbase + count] = L; P.i[sbase + count] = i; P.j[sbase + count] = j; }
            }
            ++count;
            __threadfence();        // the mask bits have arrived and the vector L1 holds no older line of them
        }
        if (lane == 0) {
            P.count[q] = static_cast<int>(min(count, static_cast<long long>(0x7fffffff)));
            P.status[q] = status;
            if (count > scap) *P.flag = 1;
        }
        __threadfence();            // the next sequence of this workgroup rewrites the scratch
    }
}

}  // namespace ps
