// filt_plan.hpp -- the host's planning of a batched Bessel filter call (ps_filter_bessel_batch, and the inside of
// ps_filter_requantise_batch and ps_filter_derivative_f64): which route an order-1 filter takes, how the events of a batch are
// cut into units of work -- one tile per workgroup on the fused route, one segment per thread on the order-n route --, how the
// order-n launches are grouped under a scratch cap, what the batch refuses, and the workgroups of the batched re-quantisation.
// Plain host C++ on <stdint.h> and the standard library, no HIP: poreseg.hip and seg_filter.hpp include it and define none of it
// again, and so does the stand-alone program tests/native/filt_plan_check.cpp, which runs it under the address and
// undefined-behaviour sanitizers.
//
// The rule everything here follows: a unit of a batch is the unit the per-event launch (ps_filter_bessel) would have had -- event
// e gets ceil((n_e + 2 pad) / unit) of them, numbered from 0 within the event --, so a kernel that hands workgroup (thread) b the
// pair (event, unit) of table entry b computes what the per-event kernel computes, bit for bit.
//
// Slow order-1 filters (the halo would exceed FILT_H_MAX, or the context's filter_fused switch is off) take the three-pass scan
// and have no batched kernel: filt_route1 returns 0 for them, and the batch entry queues them per event.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace ps {

constexpr int FILT_NT = 256;
constexpr int FILT_PER = 16;                        // consecutive samples per thread
constexpr int FILT_CHUNK = FILT_NT * FILT_PER;
constexpr int FILT_PAD = 6;                         // scipy: padlen = 3 * max(len(a), len(b)) for a first-order section
constexpr int FILT_MAXORD = 8;
constexpr int FILT_H_MAX = 1024;                    // the fused route's halo at most: slower poles take the exact scan
constexpr int64_t FILT_BATCH_SCRATCH_DEFAULT = 256ll << 20;     // option filt_batch_scratch: bytes of order-n scratch rows per launch

constexpr int RQ_NT = 256;
constexpr int RQ_PER = 8;                           // samples per thread and trip the statistics grid is sized for
constexpr int RQ_GRID_MAX = 1024;

inline int filt_padlen(int order) { return order == 1 ? FILT_PAD : 3 * (order + 1); }    // scipy: 3 * max(len(a), len(b))

// The order-1 route.  alpha: the pole of the section (-a1); fused: the context's filter_fused switch.  Returns the halo H of the
// fused kernel -- the smallest multiple of 64, at least 64, with alpha^H <= 2^-60 -- or 0: the three-pass scan (H would exceed
// FILT_H_MAX, the switch is off, or the pole is not inside (0, 1)).
inline int filt_route1(double alpha, int fused)
{
    if (!fused || !(alpha > 0.0) || !(alpha < 1.0)) return 0;
    const double h_req = std::ceil(60.0 * std::log(2.0) / -std::log(alpha));
    return h_req <= static_cast<double>(FILT_H_MAX) ? std::max(64, (static_cast<int>(h_req) + 63) / 64 * 64) : 0;
}
inline int filt_tile(int H) { return FILT_CHUNK - 2 * H; }      // extended samples a fused workgroup is responsible for

// The tables the kernels read (the layout on the device is this one).
struct FiltEvent { int64_t start, n, out_off, unit0; };         // first sample, length, first output (events packed back to back), first unit
struct FiltUnit { int32_t ev, idx; };                           // event, unit within the event
struct FiltGroup { int32_t ev0, ev1; int64_t unit0, units; };   // one order-n launch: events [ev0, ev1), their units [unit0, unit0 + units)

enum FiltPlanError { FILT_PLAN_OK = 0, FILT_PLAN_RANGE, FILT_PLAN_SHORT, FILT_PLAN_TOO_MANY };

struct FiltPlan {
    std::vector<FiltEvent> ev;
    std::vector<FiltUnit> unit;
    std::vector<FiltGroup> group;       // one group when row_bytes == 0 (the fused route: no scratch)
    int64_t total_len = 0;
    int bad_event = -1;                 // FILT_PLAN_RANGE / FILT_PLAN_SHORT: the first event refused
};

inline int64_t filt_units(int64_t n, int pad, int64_t unit) { return (n + 2 * static_cast<int64_t>(pad) + unit - 1) / unit; }

// pad: filt_padlen(order); unit: filt_tile(H) (fused) or S (order n); row_bytes: scratch of one unit ((S + H) * 8 on the order-n
// route, 0 on the fused one); cap_bytes: scratch of one launch at most (an event that alone exceeds it is a group of its own).
// Refusals, events taken in order: a negative start or an empty range (FILT_PLAN_RANGE), n <= pad (FILT_PLAN_SHORT) -- bad_event
// names the event --, more than INT32_MAX units (FILT_PLAN_TOO_MANY).  Nothing is allocated for a batch that is refused.
inline FiltPlanError plan_filter_batch(const int64_t *ev_start, const int64_t *ev_len, int32_t n_ev, int pad, int64_t unit, int64_t row_bytes,
                                       int64_t cap_bytes, FiltPlan *out)
{
    out->ev.clear(); out->unit.clear(); out->group.clear();
    out->total_len = 0; out->bad_event = -1;
    int64_t units = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        if (ev_start[e] < 0 || ev_len[e] < 1) { out->bad_event = e; return FILT_PLAN_RANGE; }
        if (ev_len[e] <= pad) { out->bad_event = e; return FILT_PLAN_SHORT; }
        if (ev_len[e] > (1ll << 46)) return FILT_PLAN_TOO_MANY;     // (2^31 units of 2^15 samples, the largest: the sums stay inside int64)
        units += filt_units(ev_len[e], pad, unit);
        if (units > INT32_MAX) return FILT_PLAN_TOO_MANY;
    }
    out->ev.resize(static_cast<size_t>(n_ev));
    out->unit.resize(static_cast<size_t>(units));
    const int64_t rows_max = row_bytes > 0 ? std::max<int64_t>(1, cap_bytes / row_bytes) : INT64_MAX;
    int64_t u = 0, off = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        const int64_t k = filt_units(ev_len[e], pad, unit);
        out->ev[e] = {ev_start[e], ev_len[e], off, u};
        for (int64_t i = 0; i < k; ++i) out->unit[static_cast<size_t>(u + i)] = {e, static_cast<int32_t>(i)};
        if (out->group.empty() || out->group.back().units + k > rows_max) out->group.push_back({e, e, u, 0});
        out->group.back().ev1 = e + 1;
        out->group.back().units += k;
        u += k; off += ev_len[e];
    }
    out->total_len = off;
    return FILT_PLAN_OK;
}

// The batched re-quantisation (requant_stats_batch_kernel, requant_round_batch_kernel): event e of a packed float64 buffer gets
// grid_e = min(RQ_GRID_MAX, ceil(n_e / (RQ_PER * RQ_NT))) workgroups -- ps_requantise's grid for that event alone --, workgroup g
// of it strides the event as block g of a launch of grid_e blocks does and leaves its partial sums at part[3 * (poff_e + g)].
struct RequantEvent { int64_t off, n, poff; int32_t grid, pad_; };
struct RequantPlan {
    std::vector<RequantEvent> ev;
    std::vector<FiltUnit> unit;         // one entry per workgroup: (event, block g)
};
inline unsigned requant_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>(RQ_GRID_MAX, (n + RQ_PER * RQ_NT - 1) / (RQ_PER * RQ_NT))); }
inline void plan_requant_batch(const int64_t *ev_len, int32_t n_ev, RequantPlan *out)
{
    out->ev.resize(static_cast<size_t>(n_ev));
    out->unit.clear();
    int64_t off = 0, poff = 0;
    for (int32_t e = 0; e < n_ev; ++e) {
        const int32_t g = static_cast<int32_t>(requant_grid(ev_len[e]));
        out->ev[e] = {off, ev_len[e], poff, g, 0};
        for (int32_t i = 0; i < g; ++i) out->unit.push_back({e, i});
        off += ev_len[e]; poff += g;
    }
}

}  // namespace ps
