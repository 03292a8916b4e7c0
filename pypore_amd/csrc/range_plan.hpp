// range_plan.hpp -- the host's planning of ps_range_stats (statistics of caller-given sample ranges of one device buffer): what
// the entry refuses in its range table, how every range is cut into units of at most `range_tile` samples -- one workgroup of
// range_part_kernel each --, and the two tables the kernels read (seg_ranges.hpp).  Plain host C++ on <stdint.h> and the standard
// library, no HIP: poreseg.hip and seg_ranges.hpp include it and define none of it again, and so does the stand-alone program
// tests/native/range_plan_check.cpp, which runs it under the address and undefined-behaviour sanitizers.  A refusal is an error
// code and the index it names; the messages are the entry point's.
//
// The rule: range r = [start, end) gets ceil((end - start) / unit) units, unit k of it the samples [start + k unit, start +
// min((k + 1) unit, end - start)), numbered from RangeRow::unit0 on.  The kernels find their work in the tables alone -- no
// workgroup searches for its range --, and because the per-unit sums are exact integers the statistics of a range do not depend
// on how `unit` cuts it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ps {

constexpr int RANGE_NT = 256;                           // threads of a range_part_kernel workgroup
constexpr int64_t RANGE_TILE_MIN = 64;                  // option range_tile: samples per unit at most, RANGE_TILE_MIN .. RANGE_TILE_MAX
constexpr int64_t RANGE_TILE_MAX = 1ll << 20;           // (int16: |y| <= 65535, a unit's sum of y^2 stays below 2^52)
constexpr int64_t RANGE_TILE_DEFAULT = 16384;
// float32 on a grid: |y| < 2^24, so y^2 < 2^48 and the int64 sum of a unit is exact for up to 2^15 samples; units stay at half that
constexpr int64_t RANGE_TILE_F32_MAX = 1ll << 14;
constexpr int64_t RANGE_LEN_MAX = INT32_MAX;            // samples of one range at most
constexpr int64_t RANGE_UNITS_MAX = 0xffffff;           // units of one call at most (a launch holds fewer than 2^32 threads)

// The tables the kernels read (the layout on the device is this one).
struct RangeRow { int64_t start; int32_t n, unit0, units, pad_; };     // first sample, length, first unit, number of units
struct RangeUnit { int64_t first; int32_t range, len, unit0, pad_; };  // first sample, range, length, the range's first unit
// What range_part_kernel leaves per unit: the sums of y = count - k0 and y^2, min and max of y (k0: the count of the RANGE's
// first sample)
struct RangePart { int64_t s1, s2; int32_t mn, mx; };

enum RangePlanError {
    RANGE_PLAN_OK = 0,
    RANGE_PLAN_START,       // start < 0
    RANGE_PLAN_END,         // end > n
    RANGE_PLAN_EMPTY,       // end <= start
    RANGE_PLAN_LONG,        // more than RANGE_LEN_MAX samples
    RANGE_PLAN_TOO_MANY     // more ranges than int32 holds, or more than RANGE_UNITS_MAX units
};

struct RangePlan {
    std::vector<RangeRow> row;
    std::vector<RangeUnit> unit;
};

inline bool range_tile_ok(int64_t tile) { return tile >= RANGE_TILE_MIN && tile <= RANGE_TILE_MAX; }

// samples per unit for a sample type: the context's range_tile, capped for float32 so that a unit's integer sums are exact
inline int64_t range_unit(bool f32, int64_t tile) { return f32 ? std::min(tile, RANGE_TILE_F32_MAX) : tile; }

// The range table against a buffer of n samples, ranges taken in order; *bad names the first offender.  The signs are tested
// before anything is subtracted: with 0 <= start < end <= n the length end - start cannot overflow.
inline RangePlanError check_ranges(const int64_t *start, const int64_t *end, int64_t n_ranges, int64_t n, int64_t *bad)
{
    for (int64_t r = 0; r < n_ranges; ++r) {
        *bad = r;
        if (start[r] < 0) return RANGE_PLAN_START;
        if (end[r] > n) return RANGE_PLAN_END;
        if (end[r] <= start[r]) return RANGE_PLAN_EMPTY;
        if (end[r] - start[r] > RANGE_LEN_MAX) return RANGE_PLAN_LONG;
    }
    *bad = -1;
    return RANGE_PLAN_OK;
}

inline int64_t range_units(int64_t len, int64_t unit) { return (len + unit - 1) / unit; }

// The tables of a call.  A refused call leaves both tables empty and allocates nothing: the units are counted first.
inline RangePlanError plan_ranges(const int64_t *start, const int64_t *end, int64_t n_ranges, int64_t n, int64_t unit, RangePlan *out,
                                  int64_t *bad)
{
    out->row.clear(); out->unit.clear();
    if (const RangePlanError err = check_ranges(start, end, n_ranges, n, bad)) return err;
    if (n_ranges > INT32_MAX) return RANGE_PLAN_TOO_MANY;
    int64_t units = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        units += range_units(end[r] - start[r], unit);              // (at most 2^31 each: the sum stays inside int64)
        if (units > RANGE_UNITS_MAX) return RANGE_PLAN_TOO_MANY;
    }
    out->row.resize(static_cast<size_t>(n_ranges));
    out->unit.resize(static_cast<size_t>(units));
    int64_t u = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        const int64_t len = end[r] - start[r], k = range_units(len, unit);
        out->row[static_cast<size_t>(r)] = {start[r], static_cast<int32_t>(len), static_cast<int32_t>(u), static_cast<int32_t>(k), 0};
        for (int64_t i = 0; i < k; ++i)
            out->unit[static_cast<size_t>(u + i)] = {start[r] + i * unit, static_cast<int32_t>(r), static_cast<int32_t>(std::min(unit, len - i * unit)),
                                                     static_cast<int32_t>(u), 0};
        u += k;
    }
    return RANGE_PLAN_OK;
}

}  // namespace ps
