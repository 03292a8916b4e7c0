// seg_ranges.hpp -- ps_range_stats: mean / std / min / max of caller-given sample ranges of one device buffer, in two launches
// whatever the number of ranges.  The ranges may overlap, repeat and be as long as the buffer (the merged segments of HMM-guided
// segmentation are: DataTypes.merge_by_hmm), so they are not the boundaries of any segment call and segstat_kernel, one workgroup
// per segment of the call's own boundaries, does not serve them.  The host cuts every range into units (range_plan.hpp):
//   range_part_kernel   one workgroup per unit: reads its samples once -- 16-byte loads from the first 16-byte boundary on, the
//                       head before it and the tail behind the last full vector sample by sample -- and leaves the INTEGER sums
//                       of y = count - k0 and y^2, min and max of y in the unit's RangePart (k0: the count of the RANGE's first
//                       sample, so the partial rows of a range add up)
//   range_final_kernel  one lane per range: adds the range's rows in unit order and forms the ps_segstat with segstat_kernel's
//                       final expressions
// No workgroup waits on another, nothing is accumulated with atomics, no multiply-add is fused.
// Arithmetic: int16 counts give |y| <= 65535 -- y^2 fits 32 unsigned bits, the sums of a range of fewer than 2^31 samples fit
// int64 and are exact; S2 is converted to double once, to nearest.  float32 on a grid gives |y| < 2^24: the plan keeps units at
// RANGE_TILE_F32_MAX samples so that a unit's int64 sums are exact, and the units are combined in fp64 in unit order -- exact while
// the total stays below 2^53, as segstat_kernel documents for itself.  Either way the bits do not depend on how range_tile cuts.
// Included by poreseg.hip behind seg_device.hpp (DevCfg, Raw, to_count, load_count).
#pragma once

#include "range_plan.hpp"   // RANGE_NT, RangeRow, RangeUnit, RangePart: shared with the host plan

namespace ps {

template <int DT> struct RangeAcc {
    long long s1 = 0, s2 = 0;
    int mn = 0x7fffffff, mx = static_cast<int>(0x80000000);
    __device__ __forceinline__ void add(int y)
    {
        s1 += y;
        if (sdt(DT) == PS_DTYPE_I16) {
            const unsigned uy = static_cast<unsigned>(y);
            s2 += static_cast<long long>(uy * uy);          // (|y| <= 65535: the low 32 bits of the product are the square)
        } else {
            s2 += static_cast<long long>(y) * y;
        }
        mn = y < mn ? y : mn; mx = y > mx ? y : mx;
    }
};

template <int DT>
__global__ __launch_bounds__(RANGE_NT) void range_part_kernel(DevCfg c, const RangeRow *rows, const RangeUnit *units, RangePart *part,
                                                              unsigned *status)
{
    typedef typename Raw<DT>::type raw_t;
    constexpr int EPV = 16 / static_cast<int>(sizeof(raw_t));       // samples of a 16-byte load
    constexpr int NW = RANGE_NT / 64;
    __shared__ long long ws1[NW], ws2[NW];
    __shared__ int smin[NW], smax[NW];
    const RangeUnit u = units[blockIdx.x];
    const int tid = threadIdx.x;
    unsigned bad = 0;
    const int k0 = load_count<DT>(c, rows[u.range].start, bad);
    const raw_t *p = static_cast<const raw_t *>(c.samples) + u.first;
    // [0, head): up to the first 16-byte boundary; [head, head + nvec EPV): whole vectors; the rest: fewer than EPV samples
    const int to_boundary = static_cast<int>(((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(p)) & 15u)) & 15u) / sizeof(raw_t));
    const int head = to_boundary < u.len ? to_boundary : u.len;
    const int nvec = (u.len - head) / EPV;
    const int tail0 = head + nvec * EPV;
    RangeAcc<DT> a;
    if (tid < head) a.add(to_count<DT>(c, p[tid], bad) - k0);
    if (sdt(DT) == PS_DTYPE_I16) {
        const int4 *pv = reinterpret_cast<const int4 *>(p + head);
        for (int i = tid; i < nvec; i += RANGE_NT) {
            const int4 v = pv[i];
            const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a.add(static_cast<int>(static_cast<int16_t>(w[k] & 0xffff)) + c.off_counts - k0);
                a.add((w[k] >> 16) + c.off_counts - k0);
            }
        }
    } else {
        const float4 *pv = reinterpret_cast<const float4 *>(p + head);
        for (int i = tid; i < nvec; i += RANGE_NT) {
            const float4 v = pv[i];
            a.add(to_count<DT>(c, v.x, bad) - k0); a.add(to_count<DT>(c, v.y, bad) - k0);
            a.add(to_count<DT>(c, v.z, bad) - k0); a.add(to_count<DT>(c, v.w, bad) - k0);
        }
    }
    if (tail0 + tid < u.len) a.add(to_count<DT>(c, p[tail0 + tid], bad) - k0);
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.s1 += __shfl_down(a.s1, d); a.s2 += __shfl_down(a.s2, d);
        const int om = __shfl_down(a.mn, d), ox = __shfl_down(a.mx, d);
        a.mn = om < a.mn ? om : a.mn; a.mx = ox > a.mx ? ox : a.mx;
    }
    if (lane == 0) { ws1[wave] = a.s1; ws2[wave] = a.s2; smin[wave] = a.mn; smax[wave] = a.mx; }
    __syncthreads();
    if (tid == 0) {
        RangePart r = {0, 0, 0x7fffffff, static_cast<int>(0x80000000)};
        for (int w = 0; w < NW; ++w) {
            r.s1 += ws1[w]; r.s2 += ws2[w];
            r.mn = smin[w] < r.mn ? smin[w] : r.mn; r.mx = smax[w] > r.mx ? smax[w] : r.mx;
        }
        part[blockIdx.x] = r;
    }
    if (bad) atomicOr(status, bad);
}

// The final expressions of a range's -- or a piece's (seg_pieces.hpp) -- statistics, written once: t1 = sum of y = count - k0 and
// t2 = sum of y^2 over the n samples (exact integers, converted to double by the caller), mn / mx the extremes of y.
// mean = (k0 + t1 / n) q, std = sqrt(max(0, t2 / n - (t1 / n)^2)) q, min / max from the integers; no multiply-add is fused.
__device__ __forceinline__ ps_segstat segstat_from_sums(int k0, double t1, double t2, int n, int mn, int mx, double q)
{
#pragma clang fp contract(off)
    const double dn = static_cast<double>(n);
    const double my = t1 / dn;
    double var = t2 / dn - my * my;
    if (var < 0) var = 0;
    ps_segstat s;
    s.mean = (static_cast<double>(k0) + my) * q; s.std = sqrt(var) * q;
    s.min = static_cast<double>(k0 + mn) * q; s.max = static_cast<double>(k0 + mx) * q;
    return s;
}

template <int DT>
__global__ __launch_bounds__(RANGE_NT) void range_final_kernel(DevCfg c, const RangeRow *rows, int32_t n_ranges, const RangePart *part,
                                                               ps_segstat *stats)
{
#pragma clang fp contract(off)
    const int64_t r = static_cast<int64_t>(blockIdx.x) * RANGE_NT + threadIdx.x;
    if (r >= n_ranges) return;
    const RangeRow row = rows[r];
    unsigned bad = 0;                                               // (range_part_kernel has reported it)
    const int k0 = load_count<DT>(c, row.start, bad);
    const RangePart *p = part + row.unit0;
    int mn = 0x7fffffff, mx = static_cast<int>(0x80000000);
    double t1, t2;
    if (sdt(DT) == PS_DTYPE_I16) {
        long long a1 = 0, a2 = 0;
        for (int k = 0; k < row.units; ++k) {
            a1 += p[k].s1; a2 += p[k].s2;
            mn = p[k].mn < mn ? p[k].mn : mn; mx = p[k].mx > mx ? p[k].mx : mx;
        }
        t1 = static_cast<double>(a1); t2 = static_cast<double>(a2);
    } else {
        t1 = 0; t2 = 0;
        for (int k = 0; k < row.units; ++k) {
            t1 += static_cast<double>(p[k].s1); t2 += static_cast<double>(p[k].s2);
            mn = p[k].mn < mn ? p[k].mn : mn; mx = p[k].mx > mx ? p[k].mx : mx;
        }
    }
    stats[r] = segstat_from_sums(k0, t1, t2, row.n, mn, mx, c.q);
}

}  // namespace ps
