// pool_plan.hpp -- how a context that shares its device configures a call (ps_pool_plan, option "shared_device"), and how many
// hardware queues the process has.  Plain host C++, no HIP: poreseg.hip includes it, and so does the stand-alone program
// tests/native/pool_plan_check.cpp, which runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "poreseg.h"

namespace ps {

constexpr int HW_QUEUES_DEFAULT = 4;     // HIP's own default: what the runtime opens when GPU_MAX_HW_QUEUES is unset
constexpr int HW_QUEUES_MAX = 32;

// The value of GPU_MAX_HW_QUEUES as text -> hardware queues of the process: nullptr (unset), empty or not a whole number: the
// default; a number: itself, clamped to 1 .. HW_QUEUES_MAX.
inline int hw_queues_parse(const char *text)
{
    if (!text) return HW_QUEUES_DEFAULT;
    char *end = nullptr;
    errno = 0;
    const long v = std::strtol(text, &end, 10);
    if (end == text) return HW_QUEUES_DEFAULT;
    while (*end == ' ' || *end == '\t' || *end == '\n') ++end;
    if (*end != 0) return HW_QUEUES_DEFAULT;
    if (errno == ERANGE) return v < 0 ? 1 : HW_QUEUES_MAX;
    return static_cast<int>(std::max<long>(1, std::min<long>(HW_QUEUES_MAX, v)));
}

// Streams that share a hardware queue run their kernels one after the other: of n contexts, each on its own stream, min(n, queues)
// calls execute at a time, and that number -- not n -- is what a call shares the chip with.
inline int pool_n_eff(int n_contexts, int hw_queues)
{
    const int q = hw_queues <= 0 ? HW_QUEUES_DEFAULT : std::min(hw_queues, HW_QUEUES_MAX);
    return std::max(0, std::min(n_contexts, q));
}

// One row per n_eff.  Rows 0, 1 (a lone call) and >= 16 (round 5's measurement with sixteen calls in flight) are conditions; the
// rows between them come from the sweep of tools/pool_plan_sweep.py (profiles/pool_queues_ab.json, DESIGN.md section 6 has the
// table and the rule).  Going down the table a call never gets a larger share of the chip: K0's waves per SIMD (0 = every slot
// it can get) do not grow, the number of K0s admitted at a time (0 = all of them) does not grow, the helpers do not come back.
struct PoolRow { int n_eff_max, k0_waves, k0_admit, lat_help; };
// Measured with sixteen contexts on 2, 4, 8 and 16 queues, k0_waves 0 / 1 / 2 / 3 / 4 / 6 / 8 x k0_admit 0 / 2 / 3, eight rounds of 100
// steps each.  The rule: a row takes the setting with the lowest mean at the measured n_eff nearest to it by ratio (2: 2; 3 .. 5: 4;
// 6 .. 11: 8; 12 .. 15: 16) among those that keep the table monotone; settings within two standard errors of the difference
// from the best count as tied with it, and among tied settings the one with the fewest K0 waves per SIMD wins (0 is the most).
//   2 queues: the one-shot K0 without a gate 0.2335 ms per step, (1, 0) 0.2375, (4, 0) 0.2449, round 5's (1, 3) 0.2435
//   4 queues: (6, 0) 0.1688 and (4, 0) 0.1698 tied, (3, 0) 0.1715, (0, 0) 0.1722, (1, 0) 0.1805, (1, 3) 0.1855 -- every gated
//             setting loses: a wait in front of K0 is a barrier packet in a queue that three more contexts stand in
//   8 queues: (2, 0) 0.1698, (3, 0) 0.1701, (4, 0) 0.1709, (1, 0) 0.1713 tied, (1, 3) 0.1816
//  16 queues: (1, 3) 0.1577 and (2, 3) 0.1605 tied, (1, 0) 0.1652, (4, 0) 0.1678 -- round 5's setting holds where it was measured
constexpr PoolRow POOL_ROWS[] = {
    {1, 0, 0, 1},                        // a lone call
    {2, 0, 0, 0},                        // two calls at a time: the one-shot K0, no gate
    {5, 4, 0, 0},                        // 3 .. 5: persistent K0 at four waves per SIMD, no gate
    {11, 1, 0, 0},                       // 6 .. 11: one wave per SIMD, no gate
    {15, 1, 3, 0},                       // 12 .. 15: as sixteen calls in flight
};
constexpr PoolRow POOL_ROW_MANY = {1 << 30, 1, 3, 0};     // sixteen calls in flight and more

inline int pool_plan(int n_contexts, int hw_queues, ps_pool_plan_t *out)
{
    if (!out || n_contexts < 0) return PS_ERR_ARG;
    const int n = pool_n_eff(n_contexts, hw_queues);
    const PoolRow *row = &POOL_ROW_MANY;
    for (const PoolRow &r : POOL_ROWS)
        if (n <= r.n_eff_max) { row = &r; break; }
    out->n_eff = n;
    out->k0_waves = row->k0_waves;
    out->k0_admit = row->k0_admit;
    out->lat_help = row->lat_help;
    return PS_OK;
}

}  // namespace ps
