// seg_pieces.hpp -- ps_detect_pieces: EVERY piece the threshold cuts a trace into, with start, length, mean, std, min and max, on
// the device in four launches whatever the number of pieces.  The built-in detector (edge_scan_kernel) looks only at pieces longer
// than min_duration and only at their extremes; the rules of a caller's own (lambda_event_parser(rules=...)) need the general form.
// A piece START is sample 0 and every sample i >= 1 with below(i) != below(i - 1) (below_thr, the detector's own predicate); piece p
// runs from start p to start p + 1 (the last one to n).  A chunk is PIECE_CHUNK samples, a thread's share PIECE_PER (piece_plan.hpp).
//   piece_mark_kernel   one workgroup per chunk: reads the samples once (16-byte loads; sample by sample where the base is not
//                       16-byte aligned or the trace ends inside the thread's share), leaves a 16-bit word of start bits per thread,
//                       the chunk's number of starts and its last start
//   piece_scan_kernel   ONE workgroup: exclusive sum of the starts (the piece index a chunk begins with) and running maximum of
//                       the last start (where the piece begins that is open at the chunk's first sample: its k0 is the count there);
//                       writes P and edges[P] = n
//   piece_stats_kernel  one workgroup per chunk: reads the samples a second time, ranks every start (edges[p]), walks its 16
//                       samples with an accumulator that restarts at every start -- a piece that begins and ends inside one thread's
//                       share is written at once --, and combines what is open at the threads' ends with a SEGMENTED scan across
//                       lanes (shuffles) and waves (LDS).  A piece that ends in the chunk and began in it is written with plain
//                       stores; what lies before the chunk's first start and from its last start on are left as two PieceParts
//                       (a chunk without a start -- nearly every chunk of a file trace -- is one part: a plain reduction)
//   piece_seam_kernel   one workgroup per chunk that begins a piece which leaves it: adds its tail part and the head parts of the
//                       chunks behind it, up to the first one that holds a start, 256 chunks a round, and writes the row
// Every sum is an integer relative to the count of the PIECE's first sample (k0), so the parts of a piece add up and the bits do
// not depend on where the chunks cut or in what order anything ran: no atomics on results, no float accumulation, no workgroup waits
// for another.  The final expressions are segstat_from_sums (seg_ranges.hpp), the ones ps_range_stats forms.
// Arithmetic: |y| = |k - k0| <= span_max (piece_plan.hpp: 65535 for int16 by the type; for float32 the bound under which n y^2
// fits int64, checked per sample -- ST_WIDE_RANGE), so s1 and s2 are exact in int64; each is converted to double once, to nearest.
// Included by poreseg.hip behind seg_device.hpp (DevCfg, to_count, load_count, below_thr) and seg_ranges.hpp.
#pragma once

#include "piece_plan.hpp"   // PIECE_NT, PIECE_PER, PIECE_CHUNK, PIECE_SCAN_NT, PiecePart: shared with the host plan

namespace ps {

struct PieceAcc {
    long long s1, s2;
    int mn, mx, len;
    __device__ __forceinline__ void clear() { s1 = 0; s2 = 0; mn = 0x7fffffff; mx = static_cast<int>(0x80000000); len = 0; }
    __device__ __forceinline__ void add(int y)
    {
        s1 += y; s2 += static_cast<long long>(y) * y;
        mn = y < mn ? y : mn; mx = y > mx ? y : mx; ++len;
    }
    __device__ __forceinline__ void join(const PieceAcc &o)
    {
        s1 += o.s1; s2 += o.s2; mn = o.mn < mn ? o.mn : mn; mx = o.mx > mx ? o.mx : mx; len += o.len;
    }
    __device__ __forceinline__ PieceAcc up(int d) const
    {
        PieceAcc o;
        o.s1 = __shfl_up(s1, d); o.s2 = __shfl_up(s2, d); o.mn = __shfl_up(mn, d); o.mx = __shfl_up(mx, d); o.len = __shfl_up(len, d);
        return o;
    }
    __device__ __forceinline__ PieceAcc down(int d) const
    {
        PieceAcc o;
        o.s1 = __shfl_down(s1, d); o.s2 = __shfl_down(s2, d); o.mn = __shfl_down(mn, d); o.mx = __shfl_down(mx, d); o.len = __shfl_down(len, d);
        return o;
    }
    __device__ __forceinline__ PiecePart part() const { PiecePart p = {s1, s2, mn, mx, len, 0}; return p; }
    __device__ __forceinline__ void from(const PiecePart &p) { s1 = p.s1; s2 = p.s2; mn = p.mn; mx = p.mx; len = p.len; }
};

// The counts of the PIECE_PER samples from i0 on (0 behind the trace's end).  NOTE: this is edge_scan_kernel's load block
// (seg_device.hpp, K3) restated -- that kernel is left as it is --; a change to the int16 unpacking or to the alignment test in
// one of the two belongs in the other as well.
template <int DT>
__device__ __forceinline__ void piece_load(const DevCfg &c, int64_t i0, int64_t n, int (&k)[PIECE_PER], unsigned &bad)
{
    constexpr int ES = static_cast<int>(sizeof(typename Raw<DT>::type));
    const char *p = static_cast<const char *>(c.samples) + i0 * ES;
    if (i0 + PIECE_PER <= n && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        constexpr int NV = PIECE_PER * ES / 16;
        int4 raw[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) raw[v] = reinterpret_cast<const int4 *>(p)[v];
        if (sdt(DT) == PS_DTYPE_F32) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const float f[4] = {__int_as_float(raw[v].x), __int_as_float(raw[v].y), __int_as_float(raw[v].z), __int_as_float(raw[v].w)};
#pragma unroll
                for (int e = 0; e < 4; ++e) k[v * 4 + e] = to_count<DT>(c, f[e], bad);
            }
        } else {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int w[4] = {raw[v].x, raw[v].y, raw[v].z, raw[v].w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    k[v * 8 + e] = ((e & 1) ? (w[e >> 1] >> 16) : static_cast<int>(static_cast<short>(w[e >> 1] & 0xffff))) + c.off_counts;
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < PIECE_PER; ++u) k[u] = (i0 + u < n) ? load_count<DT>(c, i0 + u, bad) : 0;
    }
}

// Inclusive sum of `ns` and inclusive maximum of `lp` over the workgroup's threads in thread order; returns the EXCLUSIVE pair
// (what the threads before this one hold: 0 and -1 for the first).  lds: 2 * (NT / 64) ints; one barrier inside.
template <int NT>
__device__ __forceinline__ void block_rank_last(int ns, int lp, int &sum_excl, int &last_excl, int &sum_incl, int &last_incl, int *lds)
{
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r = ns, m = lp;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(r, d), om = __shfl_up(m, d);
        if (lane >= d) { r += o; m = om > m ? om : m; }
    }
    if (lane == 63) { lds[wave] = r; lds[NW + wave] = m; }
    __syncthreads();
    int cr = 0, cm = -1;
    for (int j = 0; j < wave; ++j) { cr += lds[j]; cm = lds[NW + j] > cm ? lds[NW + j] : cm; }
    r += cr; m = cm > m ? cm : m;
    const int pm = __shfl_up(m, 1);
    sum_incl = r; last_incl = m;
    sum_excl = r - ns;
    last_excl = lane == 0 ? cm : pm;
}

template <int DT>
__global__ __launch_bounds__(PIECE_NT) void piece_mark_kernel(DevCfg c, int64_t n, double thr, uint16_t *bits, int *cnt, int *last,
                                                              unsigned *status)
{
    __shared__ int lds[2 * (PIECE_NT / 64)];
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * PIECE_CHUNK + static_cast<int64_t>(threadIdx.x) * PIECE_PER;
    unsigned sb = 0, bad = 0;
    if (i0 < n) {
        int k[PIECE_PER];
        piece_load<DT>(c, i0, n, k, bad);
        bool prev = i0 > 0 ? below_thr<DT>(c, load_count<DT>(c, i0 - 1, bad), thr) : false;
#pragma unroll
        for (int u = 0; u < PIECE_PER; ++u) {
            if (i0 + u < n) {
                const bool m = below_thr<DT>(c, k[u], thr);
                if (i0 + u == 0 || m != prev) sb |= 1u << u;
                prev = m;
            }
        }
    }
    bits[static_cast<size_t>(blockIdx.x) * PIECE_NT + threadIdx.x] = static_cast<uint16_t>(sb);
    const int lp = sb ? static_cast<int>(i0) + (31 - __clz(static_cast<int>(sb))) : -1;
    int se, le, si, li;
    block_rank_last<PIECE_NT>(__popc(sb), lp, se, le, si, li, lds);
    if (threadIdx.x == PIECE_NT - 1) { cnt[blockIdx.x] = si; last[blockIdx.x] = li; }
    if (bad) atomicOr(status, bad);
}

// ONE workgroup.  base[c]: starts before chunk c; open[c]: the last start before chunk c (-1 for chunk 0).  *n_pieces = P, and
// edges[P] = n where the caller's table has room for it.
__global__ __launch_bounds__(PIECE_SCAN_NT) void piece_scan_kernel(const int *cnt, const int *last, int nb, int per, int *base, int *open,
                                                                   int64_t n, int64_t cap, int64_t *edges, unsigned long long *n_pieces)
{
    __shared__ int lds[2 * (PIECE_SCAN_NT / 64)];
    const int j0 = min(static_cast<int>(threadIdx.x) * per, nb), j1 = min(j0 + per, nb);     // (nb <= 2^19, per <= 2^9)
    int s = 0, m = -1;
    for (int j = j0; j < j1; ++j) { s += cnt[j]; const int l = last[j]; m = l > m ? l : m; }
    int se, le, si, li;
    block_rank_last<PIECE_SCAN_NT>(s, m, se, le, si, li, lds);
    for (int j = j0; j < j1; ++j) {
        base[j] = se; open[j] = le;
        se += cnt[j];
        const int l = last[j];
        le = l > le ? l : le;
    }
    if (threadIdx.x == PIECE_SCAN_NT - 1) {
        *n_pieces = static_cast<unsigned long long>(si);
        if (si <= cap) edges[si] = n;
    }
}

__device__ __forceinline__ void piece_row(const DevCfg &c, ps_segstat *stats, int64_t cap, int p, const PieceAcc &a, int k0)
{
    if (p < cap) stats[p] = segstat_from_sums(k0, static_cast<double>(a.s1), static_cast<double>(a.s2), a.len, a.mn, a.mx, c.q);
}

template <int DT>
__global__ __launch_bounds__(PIECE_NT) void piece_stats_kernel(DevCfg c, int64_t n, int span_max, const uint16_t *bits, const int *cnt,
                                                               const int *last, const int *base, const int *open, PiecePart *head,
                                                               PiecePart *tail, int64_t *edges, ps_segstat *stats, int64_t cap,
                                                               unsigned *status)
{
    constexpr int NW = PIECE_NT / 64;
    __shared__ int lds[2 * NW];
    __shared__ PiecePart wtot[NW];
    __shared__ int wflag[NW];
    const int chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = static_cast<int64_t>(chunk) * PIECE_CHUNK + static_cast<int64_t>(tid) * PIECE_PER;
    const int n_starts = cnt[chunk], p_base = base[chunk];
    unsigned bad = 0;
    int k[PIECE_PER];
    unsigned sb = 0;
    if (i0 < n) piece_load<DT>(c, i0, n, k, bad);
    if (n_starts == 0) {
        // The whole chunk lies inside one piece (nearly every chunk of a file trace; uniform over the workgroup, and never chunk 0,
        // which holds start 0): no bits, no ranks, no segments -- a plain reduction about the count where that piece began.
        const int k_first = load_count<DT>(c, open[chunk], bad);
        PieceAcc a;
        a.clear();
        if (i0 < n) {
#pragma unroll
            for (int u = 0; u < PIECE_PER; ++u) {
                if (i0 + u < n) {
                    const int y = k[u] - k_first;
                    if (sdt(DT) == PS_DTYPE_F32 && (y > span_max || y < -span_max)) bad |= ST_WIDE_RANGE;
                    a.add(y);
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const PieceAcc o = a.down(d); a.join(o); }
        if (lane == 0) wtot[wave] = a.part();
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NW; ++w) { PieceAcc o; o.from(wtot[w]); a.join(o); }
            head[chunk] = a.part();
        }
        if (bad) atomicOr(status, bad);
        return;
    }
    if (i0 < n) sb = bits[static_cast<size_t>(chunk) * PIECE_NT + tid];
    // the piece open at this thread's first sample: its index, and where it began (its k0 is the count there)
    const int lp = sb ? static_cast<int>(i0) + (31 - __clz(static_cast<int>(sb))) : -1;
    int rank, before, si, li;
    block_rank_last<PIECE_NT>(__popc(sb), lp, rank, before, si, li, lds);
    const int carried = open[chunk];
    const int open_at = before > carried ? before : carried;          // (-1 only for the thread that holds sample 0)
    const int k_open = (i0 < n && i0 > 0) ? load_count<DT>(c, open_at, bad) : 0;
    int p = p_base + rank - 1;
    const int p_open = p;
    // the walk: `cur` restarts at every start; what stood in it goes to `hd` at the thread's first start (the end of a piece that
    // began in an earlier thread) and to the table at every later one (a piece inside this thread's share)
    PieceAcc cur, hd;
    cur.clear(); hd.clear();
    int k0 = k_open;
    bool seen = false;
    if (i0 < n) {
#pragma unroll
        for (int u = 0; u < PIECE_PER; ++u) {
            if (i0 + u < n) {
                if (sb & (1u << u)) {
                    if (!seen) hd = cur; else piece_row(c, stats, cap, p, cur, k0);
                    seen = true;
                    cur.clear();
                    k0 = k[u];
                    ++p;
                    if (p < cap) edges[p] = i0 + u;
                }
                const int y = k[u] - k0;
                if (sdt(DT) == PS_DTYPE_F32 && (y > span_max || y < -span_max)) bad |= ST_WIDE_RANGE;
                cur.add(y);
            }
        }
    }
    // segmented inclusive scan of what is open at the threads' ends: a thread with a start begins a new segment
    PieceAcc v = cur;
    int f = seen ? 1 : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const PieceAcc o = v.up(d);
        const int of = __shfl_up(f, d);
        if (lane >= d && !f) { v.join(o); f = of; }
    }
    if (lane == 63) { wtot[wave] = v.part(); wflag[wave] = f; }
    __syncthreads();
    PieceAcc carry;
    carry.clear();
    for (int j = 0; j < wave; ++j) {
        PieceAcc w;
        w.from(wtot[j]);
        if (wflag[j]) carry = w; else carry.join(w);
    }
    if (!f) v.join(carry);
    PieceAcc ex = v.up(1);                                            // what the threads before this one leave open
    if (lane == 0) ex = carry;
    if (seen) {
        ex.join(hd);                                                  // the piece this thread's first start ends
        if (rank > 0) piece_row(c, stats, cap, p_open, ex, k_open);   // ... began in this chunk: complete
        else head[chunk] = ex.part();                                 // ... began before it (chunk 0: nothing, an empty part)
    }
    if (tid == PIECE_NT - 1) {
        if (chunk == static_cast<int>(gridDim.x) - 1) piece_row(c, stats, cap, p_base + n_starts - 1, v, load_count<DT>(c, last[chunk], bad));
        else tail[chunk] = v.part();
    }
    if (bad) atomicOr(status, bad);
}

// Workgroup c finishes the piece that begins at chunk c's last start and leaves the chunk: tail[c] and the head parts of the chunks
// behind it up to, and with, the first that holds a start (what lies before that start is the piece's end); PIECE_NT chunks a round.
template <int DT>
__global__ __launch_bounds__(PIECE_NT) void piece_seam_kernel(DevCfg c, const int *cnt, const int *last, const int *base, const PiecePart *head,
                                                              const PiecePart *tail, ps_segstat *stats, int64_t cap)
{
    constexpr int NW = PIECE_NT / 64;
    __shared__ int s_end;
    __shared__ PiecePart wtot[NW];
    const int chunk = blockIdx.x, nb = gridDim.x, tid = threadIdx.x;
    const int n_starts = cnt[chunk];
    if (n_starts == 0 || chunk == nb - 1) return;                     // (uniform: no piece begins here, or the last chunk wrote its own)
    PieceAcc a;
    a.clear();
    if (tid == 0) a.from(tail[chunk]);
    for (int b0 = chunk + 1; b0 < nb; b0 += PIECE_NT) {
        if (tid == 0) s_end = 0x7fffffff;
        __syncthreads();
        const int j = b0 + tid;
        if (j < nb && cnt[j] > 0) atomicMin(&s_end, j);
        __syncthreads();
        const int e = s_end;
        if (j < nb && j <= e) { PieceAcc h; h.from(head[j]); a.join(h); }
        __syncthreads();
        if (e != 0x7fffffff) break;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const PieceAcc o = a.down(d); a.join(o); }
    if ((tid & 63) == 0) wtot[tid >> 6] = a.part();
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) { PieceAcc o; o.from(wtot[w]); a.join(o); }
        unsigned bad = 0;                                             // (piece_mark_kernel has reported it)
        piece_row(c, stats, cap, base[chunk] + n_starts - 1, a, load_count<DT>(c, last[chunk], bad));
    }
}

}  // namespace ps
