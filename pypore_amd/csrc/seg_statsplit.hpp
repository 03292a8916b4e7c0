// StatSplit (parsers.py:220-503): the reference's older, pure-Python segmenter -- variance or log-variance gains, a "stepwise"
// (two levels) or a "slanted" (two straight lines plus noise) model of each split, windows of window_width samples that
// advance by half a window, forced splits every max_width samples (ps_statsplit_f64, include/poreseg.h).
//
// Two kernels, nothing shared with the SpeedyStatSplit pipeline but ref_var_c and the tie-break (seg_device.hpp):
//   statsplit_prefix_kernel   one wave per event: c = cumsum(x), c2 = cumsum(x * x) and, for the slanted splitter,
//                             ct = cumsum(x * t) as numpy forms them -- strictly sequential chains, products rounded first
//   statsplit_kernel          one workgroup per event (grid stride): _segment_cumulative (:468-503) with an explicit interval
//                             stack in global memory; every thread scores candidates of the window at hand, a workgroup
//                             arg-max picks the split (strict '>' against the threshold, lowest index among equal gains)
// All arithmetic is fp64 without contraction, in the reference's order of operations; the one difference left is the device
// logarithm's last bit (use_log).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "seg_device.hpp"

namespace ps {

constexpr int SS_NT = 256;                 // threads of a recursion workgroup
constexpr int SS_TRIP = 512;               // samples the prefix wave moves through LDS at a time
enum : unsigned { SS_ST_STACK = 1u, SS_ST_OUT = 2u };     // status bits: interval stack / boundary slot too small

struct SsFrame { int32_t s, e, b; };       // a pending interval [s, e) and the boundary to emit when it is taken up

// Per event (device copies of the call's tables, int64 each): where its samples start, where its prefix sums start, the
// range [lo, hi) that is segmented (positions from the event's first sample), and where its boundary slot starts.
struct SsEvents {
    const int64_t *start, *len, *pre, *lo, *hi, *slot;       // (slot has n_ev + 1 entries)
    int n_ev;
};

struct SsCfg {
    const double *C, *C2, *Ct;             // prefix sums, event e at pre[e]; Ct only for the slanted splitter
    int mw, maxw, W;
    double thresh;                         // min_gain_per_sample * window_width, formed on the host
    SsFrame *stack;                        // stack_cap frames per workgroup
    int64_t stack_cap;
    int32_t *tmp;                          // boundary slots (slot[e] .. slot[e + 1])
    int32_t *count;                        // boundaries found per event (counted past the slot's end, never written there)
    unsigned *status;
};

// c, c2 (and ct) of every event.  The chains start from -0.0, the one value that leaves every first element as it is
// (numpy's accumulate copies it): the results are numpy's bit for bit, the sign of a zero included.  t is the index from the
// event's first sample as a double (np.linspace(0, n, num=n, endpoint=False): arange * 1.0, exact), so x * t is one rounding.
__global__ __launch_bounds__(64) void statsplit_prefix_kernel(const double *__restrict__ x, SsEvents ev, double *C, double *C2,
                                                              double *Ct)
{
#pragma clang fp contract(off)
    __shared__ double xs[SS_TRIP], cs[SS_TRIP], c2s[SS_TRIP], cts[SS_TRIP];
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < ev.n_ev; e += gridDim.x) {
        const int64_t base = ev.start[e], len = ev.len[e], po = ev.pre[e];
        double c = -0.0, c2 = -0.0, ct = -0.0;
        for (int64_t b = 0; b < len; b += SS_TRIP) {
            const int m = static_cast<int>(len - b < SS_TRIP ? len - b : SS_TRIP);
            for (int k = lane; k < m; k += 64) xs[k] = x[base + b + k];
            ps_sync<64>();
            if (lane == 0) {
                if (Ct) {
#pragma unroll 8
                    for (int j = 0; j < m; ++j) {
                        const double v = xs[j];
                        const double vv = v * v;
                        const double vt = v * static_cast<double>(b + j);
                        c = c + v; c2 = c2 + vv; ct = ct + vt;
                        cs[j] = c; c2s[j] = c2; cts[j] = ct;
                    }
                } else {
#pragma unroll 8
                    for (int j = 0; j < m; ++j) {
                        const double v = xs[j];
                        const double vv = v * v;
                        c = c + v; c2 = c2 + vv;
                        cs[j] = c; c2s[j] = c2;
                    }
                }
            }
            ps_sync<64>();
            for (int k = lane; k < m; k += 64) {
                C[po + b + k] = cs[k]; C2[po + b + k] = c2s[k];
                if (Ct) Ct[po + b + k] = cts[k];
            }
            ps_sync<64>();
        }
    }
}

// _mean_c / _mean_c2 / _mean_ct (:309-345) on one prefix array
__device__ __forceinline__ double ss_mean(const double *P, int a, int b)
{
#pragma clang fp contract(off)
    if (a == b) return 0.0;
    if (a == 0) return P[b - 1] / static_cast<double>(b);
    const double d = P[b - 1] - P[a - 1];
    return d / static_cast<double>(b - a);
}

// The mean square residual of _lr(a, b) (:355-371), operation for operation.  x_bar = a + (b - a - 1) / 2 is a half-integer
// and exact.  x2_bar = N / 6.0 with N = 2b^2 + b(2a - 3) + 2a^2 - 3a + 1 an exact integer (a Python int in the reference):
// b <= 2^30 keeps every term below 2^61 and N below 2^63; its conversion to double is the one rounding Python's int / float
// makes.  Above 2^53 (b > ~7e7) that rounding is the same round-to-nearest-even on both sides, but no test reaches it.
// x_bar ** 2 is C pow in the reference; for half-integers below 4.7e7 the square is exact in a double, so pow and the product
// agree; beyond that the product is used unchecked.  alpha ** 2 and beta ** 2 are pow(x, 2.0) of numpy scalars,
// which glibc rounds correctly: the same double as the product (seg_device.hpp: ref_var_c).  0 / 0 (b - a == 1) is NaN, as in
// numpy, and a NaN gain never wins.
__device__ __forceinline__ double ss_lr_var(const double *C, const double *C2, const double *Ct, int a, int b)
{
#pragma clang fp contract(off)
    const double xy_bar = ss_mean(Ct, a, b);
    const double y_bar = ss_mean(C, a, b);
    const double half = static_cast<double>(b - a - 1) / 2.0;
    const double x_bar = static_cast<double>(a) + half;
    const long long A = a, B = b;
    const long long N = 2 * B * B + B * (2 * A - 3) + 2 * A * A - 3 * A + 1;
    const double x2_bar = static_cast<double>(N) / 6.0;
    const double xx = x_bar * x_bar;
    const double xyb = x_bar * y_bar;
    const double num = xy_bar - xyb;
    const double den = x2_bar - xx;
    const double beta = num / den;
    const double bx = beta * x_bar;
    const double alpha = y_bar - bx;
    const double y2_bar = ss_mean(C2, a, b);
    const double a2 = 2.0 * alpha;
    const double b2 = 2.0 * beta;
    const double t1 = a2 * y_bar;
    const double t2 = b2 * xy_bar;
    const double t3 = alpha * alpha;
    const double t4a = a2 * beta;
    const double t4 = t4a * x_bar;
    const double t5a = beta * beta;
    const double t5 = t5a * x2_bar;
    double v = y2_bar - t1;
    v = v - t2;
    v = v + t3;
    v = v + t4;
    v = v + t5;
    return v;
}

// (b - a) * f(var(a, b)): one side's term of a gain.  MODE bit 0: use_log, bit 1: slanted.
template <int MODE>
__device__ __forceinline__ double ss_cost(const double *C, const double *C2, const double *Ct, int a, int b)
{
#pragma clang fp contract(off)
    double v;
    if constexpr (MODE & 2) v = ss_lr_var(C, C2, Ct, a, b);
    else v = ref_var_c(C, C2, a, b);
    if constexpr (MODE & 1) v = log(v);
    return static_cast<double>(b - a) * v;
}

// _best_split_stepwise / _best_split_slanted (:373-461) on the window [ps, pe), pe - ps >= 2 mw: the candidate
// ps + mw .. pe - mw (inclusive) with the largest gain above thresh, the lowest index among equal gains (the reference walks
// upwards with a strict '>'); -1: none.  Uniform over the workgroup.  wbest / widx: SS_NT / 64 LDS slots.
template <int MODE>
__device__ int ss_scan(const double *C, const double *C2, const double *Ct, int ps, int pe, int mw, double thresh,
                       double *wbest, int *widx)
{
#pragma clang fp contract(off)
    const double tot = ss_cost<MODE>(C, C2, Ct, ps, pe);
    double best = thresh;
    int bi = -1;
    const int last = pe - mw;
    for (int64_t i64 = static_cast<int64_t>(ps) + mw + threadIdx.x; i64 <= last; i64 += SS_NT) {
        const int i = static_cast<int>(i64);
        const double low = ss_cost<MODE>(C, C2, Ct, ps, i);
        const double high = ss_cost<MODE>(C, C2, Ct, i, pe);
        const double sm = low + high;
        const double gain = tot - sm;
        if (gain > best) { best = gain; bi = i; }          // (ascending i per thread: its first maximum; NaN never passes)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double og = __shfl_down(best, d);
        const int oi = __shfl_down(bi, d);
        if (beats(og, oi, best, bi)) { best = og; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                        // (the slots' readers of the scan before are through)
    if (lane == 0) { wbest[wave] = best; widx[wave] = bi; }
    __syncthreads();
    double bg = wbest[0];
    int r = widx[0];
#pragma unroll
    for (int w = 1; w < SS_NT / 64; ++w)
        if (beats(wbest[w], widx[w], bg, r)) { bg = wbest[w]; r = widx[w]; }
    return r;
}

// _segment_cumulative(lo, hi) (:468-503) per event, without recursion.  The interval at hand is [s, end); what the
// reference's recursion would still have to do afterwards sits on the stack as frames (s', e', b): emit boundary b, then
// segment [s', e').  A split x of [s, end) pushes (x, end, x) and goes on with [s, x): boundaries leave in ascending order.
// An in-loop forced split (:480-484) emits its boundary at once and goes on with the right part, as the reference does.
//
// Stack size.  A frame is pushed only for a found split (x <= pe - mw <= end - mw) or a late forced split
// (x = min(s + maxw, end - mw)): its interval [x, end) holds at least mw samples.  The frames and the interval at hand are
// disjoint pieces of [lo, hi) -- each push carves the frame out of the interval at hand.  Hence at most (hi - lo) / mw
// frames at a time; the host gives every workgroup (longest range of the call) / mw + 2.  A left part that can yield nothing
// (no window to scan: length <= 2 mw, and length <= maxw: no forced split) is not descended into: its boundary is emitted at
// once and nothing is pushed.  A push beyond the slab sets SS_ST_STACK and ends the event; nothing is written past the slab.
//
// Boundary slots.  Both parts of a found split hold >= mw samples; a late forced split leaves a right part of >= mw samples
// and, when x = end - mw < s + maxw, a left part that may be shorter than mw -- whose right neighbour then is a final segment
// of exactly mw samples (no window fits, mw <= maxw).  So every segment shorter than mw is followed by one of at least mw
// samples: at most 2 (hi - lo) / mw segments.  The host sizes the slots 2 (hi - lo) / mw + 2; the count is kept beyond the
// slot's end (SS_ST_OUT) without a store.
template <int MODE>
__global__ __launch_bounds__(SS_NT) void statsplit_kernel(SsEvents ev, SsCfg c)
{
    __shared__ double wbest[SS_NT / 64];
    __shared__ int widx[SS_NT / 64];
    SsFrame *stack = c.stack + static_cast<int64_t>(blockIdx.x) * c.stack_cap;
    const int64_t mw = c.mw, maxw = c.maxw, W = c.W, step = c.W / 2;
    for (int e = blockIdx.x; e < ev.n_ev; e += gridDim.x) {
        const int64_t po = ev.pre[e];
        const double *C = c.C + po, *C2 = c.C2 + po, *Ct = (MODE & 2) ? c.Ct + po : nullptr;
        int32_t *out = c.tmp + ev.slot[e];
        const int64_t out_cap = ev.slot[e + 1] - ev.slot[e];
        int64_t s = ev.lo[e], end = ev.hi[e];
        int64_t sp = 0, cnt = 0;
        unsigned st = 0;
        auto emit = [&](int64_t b) {
            if (cnt < out_cap) { if (threadIdx.x == 0) out[cnt] = static_cast<int32_t>(b); }
            else st |= SS_ST_OUT;
            ++cnt;
        };
        for (;;) {
            int64_t split = -1;
            bool tail = false;
            for (int64_t ps = s; ps < end - 2 * mw; ps += step) {
                if (ps > s + maxw) {                         // scanned a long way with no split (:480-484)
                    const int64_t x = s + maxw < end - mw ? s + maxw : end - mw;
                    emit(x);
                    s = x;
                    tail = true;
                    break;
                }
                const int64_t pe = end < ps + W ? end : ps + W;
                split = ss_scan<MODE>(C, C2, Ct, static_cast<int>(ps), static_cast<int>(pe), c.mw, c.thresh, wbest, widx);
                if (split >= 0) break;
            }
            if (tail) continue;
            if (split < 0 && end - s > maxw) split = s + maxw < end - mw ? s + maxw : end - mw;      // (:495)
            if (split >= 0) {
                const int64_t left = split - s;
                if (left <= 2 * mw && left <= maxw) {        // the left part yields nothing
                    emit(split);
                    s = split;
                    continue;
                }
                if (sp >= c.stack_cap) { st |= SS_ST_STACK; break; }
                if (threadIdx.x == 0) {
                    SsFrame f;
                    f.s = static_cast<int32_t>(split); f.e = static_cast<int32_t>(end); f.b = static_cast<int32_t>(split);
                    stack[sp] = f;
                }
                ++sp;
                end = split;
                continue;
            }
            if (sp == 0) break;
            __syncthreads();                                 // (thread 0's frames are visible to the workgroup)
            const SsFrame f = stack[--sp];
            __syncthreads();                                 // (... and read by all of it before thread 0 reuses the place)
            emit(f.b);
            s = f.s; end = f.e;
        }
        if (threadIdx.x == 0) {
            c.count[e] = static_cast<int32_t>(cnt < 0x7fffffff ? cnt : 0x7fffffff);
            if (st) atomicOr(c.status, st);
        }
        __syncthreads();                                     // (the next event reuses the stack slab)
    }
}

// Boundaries from the slots to the caller's array, event e at off[e]
__global__ __launch_bounds__(256) void statsplit_gather_kernel(const int32_t *__restrict__ tmp, const int64_t *__restrict__ slot,
                                                               const int64_t *__restrict__ off, int n_ev, int32_t *out)
{
    for (int e = blockIdx.x; e < n_ev; e += gridDim.x) {
        const int64_t n = off[e + 1] - off[e];
        const int32_t *src = tmp + slot[e];
        int32_t *dst = out + off[e];
        for (int64_t k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
    }
}

}  // namespace ps
