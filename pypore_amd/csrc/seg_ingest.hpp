// K6: a float64 current that is already on the device finds its ADC grid there (ps_grid_check_f64, ps_grid_counts_f64,
// ps_narrow_f64; grid.affine_grid_device and engine.to_device_with_counts drive them).
//
// Three streaming kernels over a float64 buffer, one shape: 16-byte loads (two samples per lane), ING_UNROLL loads in flight
// per lane, a grid-stride loop over passes of ING_T samples per workgroup, then a reduction per wave (shuffles), per
// workgroup (LDS) and -- of one partial per workgroup -- on the host.  Every reduced quantity is a minimum, a maximum or an
// integer count, so the result does not depend on the order in which partials meet.  The arithmetic per sample is numpy's:
// x - origin, / quantum and rint are the IEEE operations (no contraction, no reciprocal, round-half-even), so the host code
// in grid.affine_grid stays the oracle of every decision taken from these numbers.
//
// A buffer that starts 8 bytes off a 16-byte boundary (a slice of a tensor) has one head sample, and a buffer whose rest is
// odd has one tail sample; lanes 0 and 1 of workgroup 0 take them, everything between is read in aligned pairs.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ps {

constexpr int ING_NT = 256;                                  // lanes per workgroup
constexpr int ING_UNROLL = 4;                                // 16-byte loads in flight per lane
constexpr int ING_T = ING_NT * 2 * ING_UNROLL;               // samples per workgroup pass (2048)
constexpr int ING_GRID_MAX = 2048;                           // workgroups: 8 per CU; longer buffers stride

struct IngestSpan {                                          // how a buffer of n doubles splits into head, pairs and tail
    const double2 *pairs;
    long long n_pairs;
    int head, tail;
};
inline IngestSpan ingest_span(const double *x, long long n)
{
    IngestSpan s;
    s.head = (reinterpret_cast<uintptr_t>(x) & 15u) && n > 0 ? 1 : 0;
    s.n_pairs = (n - s.head) / 2;
    s.tail = static_cast<int>((n - s.head) & 1);
    s.pairs = reinterpret_cast<const double2 *>(x + s.head);
    return s;
}
inline unsigned ingest_grid(long long n)
{
    const long long g = (n + ING_T - 1) / ING_T;
    return static_cast<unsigned>(g < 1 ? 1 : (g > ING_GRID_MAX ? ING_GRID_MAX : g));
}

struct GridPartial {                                         // one per workgroup (ps_grid_report's fields)
    double max_frac, min_frac_above, min_count, max_count;
    unsigned long long n_nonfinite, n_undefined;
};

struct GridAcc {
    double max_frac = 0.0, min_above = INFINITY, kmin = INFINITY, kmax = -INFINITY;
    unsigned long long nonfinite = 0, undefined = 0;
};

__device__ __forceinline__ double grid_count_of(double x, double origin, double q)
{
#pragma clang fp contract(off)
    const double d = x - origin;
    return rint(d / q);
}

__device__ __forceinline__ void grid_acc(GridAcc &a, double x, double origin, double q, double tol)
{
#pragma clang fp contract(off)
    const double d = x - origin;
    const double k = d / q;
    const double kr = rint(k);
    const double f = fabs(k - kr);
    a.max_frac = fmax(a.max_frac, f);                        // (fmax / fmin pass a NaN by: it is counted instead)
    if (f > tol) a.min_above = fmin(a.min_above, f);
    a.kmin = fmin(a.kmin, kr);
    a.kmax = fmax(a.kmax, kr);
    a.nonfinite += !(fabs(x) < INFINITY);
    a.undefined += f != f;
}

// For every sample k = (x - origin) / q and kr = rint(k): max |k - kr|, the smallest |k - kr| above tol (INFINITY: none), min
// and max kr, the samples that are NaN or infinite, and the samples whose |k - kr| is NaN.
__global__ __launch_bounds__(ING_NT) void grid_check_kernel(IngestSpan s, long long n, const double *x, double origin, double q,
                                                            double tol, GridPartial *part)
{
    __shared__ GridPartial s_part[ING_NT / 64];
    GridAcc a;
    const long long stride = static_cast<long long>(gridDim.x) * (ING_T / 2);
    for (long long base = static_cast<long long>(blockIdx.x) * (ING_T / 2); base < s.n_pairs; base += stride) {
        double2 v[ING_UNROLL];
        bool in[ING_UNROLL];
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u) {
            const long long p = base + u * ING_NT + threadIdx.x;
            in[u] = p < s.n_pairs;
            if (in[u]) v[u] = s.pairs[p];
        }
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u)
            if (in[u]) { grid_acc(a, v[u].x, origin, q, tol); grid_acc(a, v[u].y, origin, q, tol); }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && s.head) grid_acc(a, x[0], origin, q, tol);
        if (threadIdx.x == 1 && s.tail) grid_acc(a, x[n - 1], origin, q, tol);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.max_frac = fmax(a.max_frac, __shfl_down(a.max_frac, d));
        a.min_above = fmin(a.min_above, __shfl_down(a.min_above, d));
        a.kmin = fmin(a.kmin, __shfl_down(a.kmin, d));
        a.kmax = fmax(a.kmax, __shfl_down(a.kmax, d));
        a.nonfinite += __shfl_down(a.nonfinite, d);
        a.undefined += __shfl_down(a.undefined, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_part[wave] = GridPartial{a.max_frac, a.min_above, a.kmin, a.kmax, a.nonfinite, a.undefined};
    __syncthreads();
    if (threadIdx.x == 0) {
        GridPartial r = s_part[0];
        for (int w = 1; w < ING_NT / 64; ++w) {
            const GridPartial o = s_part[w];
            r.max_frac = fmax(r.max_frac, o.max_frac); r.min_frac_above = fmin(r.min_frac_above, o.min_frac_above);
            r.min_count = fmin(r.min_count, o.min_count); r.max_count = fmax(r.max_count, o.max_count);
            r.n_nonfinite += o.n_nonfinite; r.n_undefined += o.n_undefined;
        }
        part[blockIdx.x] = r;
    }
}

// out[i] = int16(rint((x[i] - origin) / q) - centre): the counts of a grid that grid_check_kernel confirmed and whose
// re-centred range the caller found inside int16.
__global__ __launch_bounds__(ING_NT) void grid_counts_kernel(IngestSpan s, long long n, const double *x, double origin, double q,
                                                             long long centre, short *out)
{
    short *body = out + s.head;
    const long long stride = static_cast<long long>(gridDim.x) * (ING_T / 2);
    for (long long base = static_cast<long long>(blockIdx.x) * (ING_T / 2); base < s.n_pairs; base += stride) {
        double2 v[ING_UNROLL];
        bool in[ING_UNROLL];
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u) {
            const long long p = base + u * ING_NT + threadIdx.x;
            in[u] = p < s.n_pairs;
            if (in[u]) v[u] = s.pairs[p];
        }
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u) {
            if (!in[u]) continue;
            const long long p = base + u * ING_NT + threadIdx.x;
            const short c0 = static_cast<short>(static_cast<long long>(grid_count_of(v[u].x, origin, q)) - centre);
            const short c1 = static_cast<short>(static_cast<long long>(grid_count_of(v[u].y, origin, q)) - centre);
            body[2 * p] = c0; body[2 * p + 1] = c1;
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && s.head) out[0] = static_cast<short>(static_cast<long long>(grid_count_of(x[0], origin, q)) - centre);
        if (threadIdx.x == 1 && s.tail) out[n - 1] = static_cast<short>(static_cast<long long>(grid_count_of(x[n - 1], origin, q)) - centre);
    }
}

// out[i] = float(x[i]) (round to nearest even, as numpy's astype); part[workgroup] = the samples with double(float(x)) != x
// (a NaN counts: numpy.array_equal refuses it too).
__global__ __launch_bounds__(ING_NT) void narrow_f64_kernel(IngestSpan s, long long n, const double *x, float *out,
                                                            unsigned long long *part)
{
    __shared__ unsigned long long s_bad[ING_NT / 64];
    unsigned long long bad = 0;
    float *body = out + s.head;
    const long long stride = static_cast<long long>(gridDim.x) * (ING_T / 2);
    for (long long base = static_cast<long long>(blockIdx.x) * (ING_T / 2); base < s.n_pairs; base += stride) {
        double2 v[ING_UNROLL];
        bool in[ING_UNROLL];
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u) {
            const long long p = base + u * ING_NT + threadIdx.x;
            in[u] = p < s.n_pairs;
            if (in[u]) v[u] = s.pairs[p];
        }
#pragma unroll
        for (int u = 0; u < ING_UNROLL; ++u) {
            if (!in[u]) continue;
            const long long p = base + u * ING_NT + threadIdx.x;
            const float f0 = static_cast<float>(v[u].x), f1 = static_cast<float>(v[u].y);
            bad += (static_cast<double>(f0) != v[u].x) + (static_cast<double>(f1) != v[u].y);
            body[2 * p] = f0; body[2 * p + 1] = f1;
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && s.head) { const float f = static_cast<float>(x[0]); bad += static_cast<double>(f) != x[0]; out[0] = f; }
        if (threadIdx.x == 1 && s.tail) { const float f = static_cast<float>(x[n - 1]); bad += static_cast<double>(f) != x[n - 1]; out[n - 1] = f; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_down(bad, d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ING_NT / 64; ++w) bad += s_bad[w];
        part[blockIdx.x] = bad;
    }
}

}  // namespace ps
