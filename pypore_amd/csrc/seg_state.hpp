// The reference's "state parsers" (parsers.py:572-679): snakebase_parser and FilterDerivativeSegmenter (ps_snakebase_f64,
// ps_filter_derivative_f64, include/poreseg.h).  Both are one streaming pattern: a predicate on neighbouring
// samples, a stream compaction of its hits, a pairing of the hits.
//
//   sp_count_kernel<Pred>   pass 1: one workgroup per tile of SP_TILE positions of ONE event: the predicate of every position
//                           as a bit mask (one 64-bit word per wave and round: word w, bit b <-> position 64 w + b of the
//                           tile) and the tile's hit count.  The samples are read here and nowhere else.
//   sp_scan_kernel          exclusive scan of the tile counts, one workgroup (the total behind the last tile)
//   sp_event_off_kernel     hits before each event: the scan read at the event's first tile
//   sp_scatter_kernel       pass 2: the set bits of a tile as positions from the event's start, ascending, at the tile's
//                           place in the list -- from the mask, so it is the same kernel for every predicate
//   sp_judge_kernel         filter-derivative: one wave per pair of tics, the maxima of the derivative left and right of
//                           position h + 1 of the pair, a keep flag (np.argmax(deriv[s:e]) > high_threshold)
//   sp_snake_spans_kernel / sp_fd_spans_kernel   the (start, end) pairs of every event from the hit list / the kept pairs
//
// Pass 1 and pass 2 are separate launches with the scan between them: no workgroup ever waits on another.  A tile belongs
// to one event and a position j of an event of npos positions reads samples j .. j + reach <= npos - 1 + reach = n - 1: no
// difference is formed across an event's end.  Differences and comparisons only, fp64, no contraction; non-finite samples:
// a NaN difference satisfies no comparison (snakebase: no hit, as in numpy); the filter-derivative parser on non-finite
// input is undefined, as scipy's filtfilt is.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "batch_plan.hpp"                          // SP_NT, SP_ROUNDS, SP_TILE

namespace ps {

constexpr int SP_WORDS = SP_TILE / 64;             // mask words per tile

// The compaction's view of a call (device copies, int64 each): event e has npos[e] positions, its data starts at
// start[e] of the predicate's array, its tiles are tile_off[e] .. tile_off[e + 1].
struct SpEvents {
    const int64_t *start, *npos, *tile_off;        // (tile_off has n_ev + 1 entries)
    int n_ev;
};

// The entry e of an ascending offset table off[0 .. n] (off[0] = 0) with off[e] <= v < off[e + 1]; entries that repeat
// (empty events) are skipped.
__device__ __forceinline__ int sp_find(const int64_t *off, int n, int64_t v)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// snakebase (parsers.py:582-584): |x[j + 1] - x[j]| < 1e-3, j in [0, n - 1)
struct SnakePred {
    const double *x;
    __device__ __forceinline__ bool operator()(int64_t start, int64_t j) const
    {
#pragma clang fp contract(off)
        const double *p = x + start + j;
        return fabs(p[1] - p[0]) < 1e-3;
    }
};

// filter-derivative (parsers.py:637-642): blocks[j + 1] != blocks[j], blocks[j] = |y[j + 1] - y[j]| > low, j in [0, n - 2);
// the tic is j + 1
struct FdPred {
    const double *y;
    double low;
    __device__ __forceinline__ bool operator()(int64_t start, int64_t j) const
    {
#pragma clang fp contract(off)
        const double *p = y + start + j;
        const double a = p[0], b = p[1], c = p[2];
        return (fabs(c - b) > low) != (fabs(b - a) > low);
    }
};

// the keep flags of the pair judge, compacted like any other predicate
struct KeepPred {
    const uint8_t *keep;
    __device__ __forceinline__ bool operator()(int64_t start, int64_t j) const { return keep[start + j] != 0; }
};

template <class Pred>
__global__ __launch_bounds__(SP_NT) void sp_count_kernel(Pred pred, SpEvents ev, unsigned long long *__restrict__ mask,
                                                         uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t s_cnt[SP_NT / 64];
    const int64_t tile = blockIdx.x;
    const int e = sp_find(ev.tile_off, ev.n_ev, tile);
    const int64_t j0 = (tile - ev.tile_off[e]) * SP_TILE, npos = ev.npos[e], start = ev.start[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (a position beyond the event evaluates the event's last one and is masked: the loads of all rounds carry no branch and
    //  go out together)
    bool hit[SP_ROUNDS];
#pragma unroll
    for (int k = 0; k < SP_ROUNDS; ++k) {
        const int64_t j = j0 + k * SP_NT + threadIdx.x;
        hit[k] = pred(start, min(j, npos - 1)) & (j < npos);
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < SP_ROUNDS; ++k) {
        const unsigned long long b = __ballot(hit[k]);
        if (lane == 0) mask[tile * SP_WORDS + k * (SP_NT / 64) + wave] = b;
        cnt += static_cast<uint32_t>(__popcll(b));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < SP_NT / 64; ++w) t += s_cnt[w];
        tile_cnt[tile] = t;
    }
}

// excl[t] = hits in the tiles before t, excl[n_tiles] = all hits.  One workgroup: thread i sums its run of tiles, the
// 1 024 sums are scanned (wave scans, then the 16 wave totals), the run is walked again.
constexpr int SP_SCAN_NT = 1024;
__global__ __launch_bounds__(SP_SCAN_NT) void sp_scan_kernel(const uint32_t *__restrict__ cnt, int64_t n_tiles, int64_t *__restrict__ excl)
{
    __shared__ int64_t wtot[SP_SCAN_NT / 64];
    const int64_t per = (n_tiles + SP_SCAN_NT - 1) / SP_SCAN_NT;
    const int64_t t0 = min(n_tiles, static_cast<int64_t>(threadIdx.x) * per), t1 = min(n_tiles, t0 + per);
    int64_t sum = 0;
    for (int64_t t = t0; t < t1; ++t) sum += cnt[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t lo = __shfl_up(inc, d);
        if (lane >= d) inc += lo;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int64_t run = inc - sum;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (int64_t t = t0; t < t1; ++t) { excl[t] = run; run += cnt[t]; }
    if (threadIdx.x == SP_SCAN_NT - 1) excl[n_tiles] = run;        // (the last thread's run ends at n_tiles, empty or not)
}

__global__ __launch_bounds__(256) void sp_event_off_kernel(SpEvents ev, const int64_t *__restrict__ excl, int64_t *__restrict__ ev_off)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e <= ev.n_ev) ev_off[e] = excl[ev.tile_off[e]];
}

// Thread t takes byte t of the tile's mask (positions 8 t .. 8 t + 7); `add` is what a hit's position is reported with
// (filter-derivative: the tic of position j is j + 1).
__global__ __launch_bounds__(SP_NT) void sp_scatter_kernel(SpEvents ev, const unsigned long long *__restrict__ mask,
                                                           const int64_t *__restrict__ excl, int32_t add, int32_t *__restrict__ out)
{
    __shared__ uint32_t s_cnt[SP_NT / 64];
    const int64_t tile = blockIdx.x;
    const int e = sp_find(ev.tile_off, ev.n_ev, tile);
    const int64_t j0 = (tile - ev.tile_off[e]) * SP_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long word = mask[tile * SP_WORDS + (threadIdx.x >> 3)];
    unsigned bits = static_cast<unsigned>(word >> (8 * (threadIdx.x & 7))) & 0xffu;
    const uint32_t mine = static_cast<uint32_t>(__popc(bits));
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up(inc, d);
        if (lane >= d) inc += lo;
    }
    if (lane == 63) s_cnt[wave] = inc;
    __syncthreads();
    int64_t at = excl[tile] + (inc - mine);
    for (int w = 0; w < wave; ++w) at += s_cnt[w];
    const int32_t p0 = static_cast<int32_t>(j0) + static_cast<int32_t>(threadIdx.x) * 8 + add;
    while (bits) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        out[at++] = p0 + b;
    }
}

// ---- filter-derivative: the pair judge -----------------------------------------------------------------------------------
// Pair i of event e is (s, t) = (tics[2 i], tics[2 i + 1]) of the event's tic list; it is kept when the first maximum of
// deriv[s .. t) lies at an index > high_threshold, i.e. at index >= h1 = floor(high_threshold) + 1: iff
// max(deriv[s + h1 .. t)) > max(deriv[s .. s + h1)), strictly; an empty right part keeps nothing, h1 = 0 (a negative
// threshold) keeps every pair.  One wave per pair, its lanes striding over the pair: a pair may be three samples or the whole
// event (the gaps between blocks are pairs when blocks[0] is set), and an event may hold thousands; a wave reads any of them
// in 512-byte rows and the grid is as wide as the pairs are many.  Lanes per pair would save the idle lanes of short pairs at
// the price of a second kernel and a length threshold between the two; the judge reads what the blocks cover, a small part
// of what pass 1 read.
struct SpPairs {
    const int64_t *start;          // the event's first sample in y
    const int64_t *tic_off;        // its first tic in `tics` (n_ev + 1 entries)
    const int64_t *pair_off;       // its first pair (n_ev + 1 entries)
    int n_ev;
};

__global__ __launch_bounds__(256) void sp_judge_kernel(const double *__restrict__ y, SpPairs pr, const int32_t *__restrict__ tics,
                                                       int64_t n_pairs, int32_t h1, uint8_t *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4LL + (threadIdx.x >> 6), n_waves = gridDim.x * 4LL;
    for (int64_t p = wave0; p < n_pairs; p += n_waves) {
        const int e = sp_find(pr.pair_off, pr.n_ev, p);
        const int64_t i = p - pr.pair_off[e];
        const int32_t *tc = tics + pr.tic_off[e] + 2 * i;
        const int32_t s = tc[0], t = tc[1];
        const double *ye = y + pr.start[e];
        const int32_t mid = t - s > h1 ? s + h1 : t;          // left part [s, mid), right part [mid, t)
        double ml = -INFINITY, mr = -INFINITY;
        for (int32_t j = s + lane; j < t; j += 64) {
            const double d = fabs(ye[j + 1] - ye[j]);
            if (j < mid) ml = fmax(ml, d); else mr = fmax(mr, d);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { ml = fmax(ml, __shfl_down(ml, d)); mr = fmax(mr, __shfl_down(mr, d)); }
        if (lane == 0) keep[p] = (mid < t && mr > ml) ? 1 : 0;
    }
}

// ---- span assembly ---------------------------------------------------------------------------------------------------------
// snakebase (parsers.py:584, :590): tics = [0] + low + [m]; the spans are tics[i] .. tics[i + 1] for odd i: (low[0], low[1]),
// (low[2], low[3]), ... and, when the hits are odd in number, (low[-1], m).  One thread per span.
__global__ __launch_bounds__(256) void sp_snake_spans_kernel(SpEvents ev, const int32_t *__restrict__ hits, const int64_t *__restrict__ hit_off,
                                                             const int64_t *__restrict__ span_off, int64_t n_spans, int32_t *__restrict__ spans)
{
    const int64_t s = blockIdx.x * 256LL + threadIdx.x;
    if (s >= n_spans) return;
    const int e = sp_find(span_off, ev.n_ev, s);
    const int64_t i = s - span_off[e], h0 = hit_off[e], n_hits = hit_off[e + 1] - h0;
    spans[2 * s] = hits[h0 + 2 * i];
    spans[2 * s + 1] = 2 * i + 1 < n_hits ? hits[h0 + 2 * i + 1] : static_cast<int32_t>(ev.npos[e]);
}

// filter-derivative (parsers.py:646-656): with the kept pairs (s_1, t_1) .. (s_k, t_k) the spans are [0, s_1), [t_1, s_2), ...,
// [t_k, n); k = 0: [0, n).  kept: the kept pairs' indices among the event's pairs, ascending.  One thread per span.
__global__ __launch_bounds__(256) void sp_fd_spans_kernel(SpPairs pr, const int64_t *__restrict__ len, const int32_t *__restrict__ tics,
                                                          const int32_t *__restrict__ kept, const int64_t *__restrict__ kept_off,
                                                          const int64_t *__restrict__ span_off, int64_t n_spans, int32_t *__restrict__ spans)
{
    const int64_t s = blockIdx.x * 256LL + threadIdx.x;
    if (s >= n_spans) return;
    const int e = sp_find(span_off, pr.n_ev, s);
    const int64_t i = s - span_off[e], k0 = kept_off[e], k = kept_off[e + 1] - k0;
    const int32_t *tc = tics + pr.tic_off[e];
    spans[2 * s] = i == 0 ? 0 : tc[2 * kept[k0 + i - 1] + 1];
    spans[2 * s + 1] = i == k ? static_cast<int32_t>(len[e]) : tc[2 * kept[k0 + i]];
}

}  // namespace ps
