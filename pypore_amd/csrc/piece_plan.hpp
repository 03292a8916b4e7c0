// piece_plan.hpp -- the host's planning of ps_detect_pieces (every piece the threshold cuts a trace into, with its statistics:
// seg_pieces.hpp): what the entry refuses, how the trace is cut into chunks -- one workgroup of each streaming kernel per chunk --,
// the sizes of the context's scratch, the capacity rule, and the bound under which the kernels' int64 sums cannot overflow.
// Plain host C++ on <stdint.h>, no HIP: poreseg.hip and seg_pieces.hpp include it and define none of it again, and so does the
// stand-alone program tests/native/piece_plan_check.cpp, which runs it under the address and undefined-behaviour sanitizers.
//
// The rule: chunk c holds the samples [c PIECE_CHUNK, min((c + 1) PIECE_CHUNK, n)), thread t of its workgroup PIECE_PER of them.
// A piece START is sample 0 and every sample whose side of the threshold differs from the sample before it; piece p begins at
// start p, so a trace of n >= 1 samples has P = (number of starts) pieces and n = 0 has none.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace ps {

constexpr int PIECE_NT = 256;                           // threads of a workgroup of the streaming kernels
constexpr int PIECE_PER = 16;                           // samples per thread: one 16-bit word of start bits
constexpr int PIECE_CHUNK = PIECE_NT * PIECE_PER;       // samples per chunk
constexpr int PIECE_SCAN_NT = 1024;                     // threads of the ONE workgroup that scans the chunks
constexpr int64_t PIECE_N_MAX = INT32_MAX;              // samples of a call at most: positions and piece indices fit int32
constexpr int PIECE_SPAN_I16 = 65535;                   // |k - k0| of int16 counts, whatever offset_counts is
constexpr int PIECE_SPAN_F32_MAX = (1 << 24) - 2;       // |k - k0| of float32 on a grid (|k| < 2^23)

// What a chunk leaves for a piece that crosses one of its seams: the sums of y = count - k0 and y^2 (k0: the count of the PIECE's
// first sample, so the rows of a piece add up), min and max of y, and the samples counted.
struct PiecePart { int64_t s1, s2; int32_t mn, mx, len, pad_; };

enum PiecePlanError {
    PIECE_PLAN_OK = 0,
    PIECE_PLAN_NEGATIVE,    // n < 0
    PIECE_PLAN_LONG,        // n > PIECE_N_MAX
    PIECE_PLAN_CAP          // cap < 0
};

struct PiecePlan {
    int64_t n = 0, cap = 0;
    int32_t chunks = 0;             // workgroups of the streaming kernels, and of the seam kernel
    int32_t scan_per_thread = 0;    // chunks each thread of the scan workgroup takes
    int32_t span_max = 0;           // |count - k0| above which a call is refused ("counts too wide"): below it no sum can overflow
    // scratch, in bytes, in this order in ONE buffer (every offset a multiple of 16)
    size_t b_bits = 0;              // start bits: uint16 per thread
    size_t b_cnt = 0;               // starts per chunk, int32
    size_t b_last = 0;              // last start of the chunk, int32 (-1: none)
    size_t b_base = 0;              // starts before the chunk, int32 (the scan's output)
    size_t b_open = 0;              // last start before the chunk, int32 (the scan's output)
    size_t b_head = 0, b_tail = 0;  // a PiecePart per chunk each: before its first start, from its last start on
    size_t bytes() const { return b_bits + b_cnt + b_last + b_base + b_open + b_head + b_tail; }
};

inline size_t piece_align16(size_t b) { return (b + 15) & ~static_cast<size_t>(15); }

inline int64_t piece_chunks(int64_t n) { return (n + PIECE_CHUNK - 1) / PIECE_CHUNK; }

// The largest Y with n Y^2 <= 2^63 - 1 (integer square root, no floating point): with |y| <= Y in every sample the sum of y^2 of
// ANY piece of a trace of n samples fits int64, and so does the sum of y.  n >= 1.
inline int64_t piece_span_bound(int64_t n)
{
    const uint64_t lim = static_cast<uint64_t>(INT64_MAX) / static_cast<uint64_t>(n);
    uint64_t lo = 0, hi = 3037000499ull;                // floor(sqrt(2^63 - 1))
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (mid * mid <= lim) lo = mid; else hi = mid - 1;
    }
    return static_cast<int64_t>(lo);
}

// int16 counts: |y| <= 65535 by the type, and 65535^2 (2^31 - 1) < 2^63 -- nothing to refuse.  float32 on a grid: |y| < 2^24, so
// y^2 < 2^48 and a long piece could overflow; the kernels refuse a sample further than this from its piece's first.
inline int32_t piece_span_max(bool f32, int64_t n)
{
    if (!f32) return PIECE_SPAN_I16;
    const int64_t b = piece_span_bound(n < 1 ? 1 : n);
    return static_cast<int32_t>(b < PIECE_SPAN_F32_MAX ? b : PIECE_SPAN_F32_MAX);
}

// The capacity rule: the caller's tables hold cap + 1 edges and cap rows; the kernels write row p and edge p only for p < cap and
// edge P only for P <= cap, and the call succeeds when all P pieces found room (else PS_ERR_CAPACITY with P reported).
inline bool piece_capacity_ok(int64_t pieces, int64_t cap) { return pieces >= 0 && pieces <= cap; }

inline PiecePlanError plan_pieces(int64_t n, int64_t cap, bool f32, PiecePlan *out)
{
    *out = PiecePlan();
    if (n < 0) return PIECE_PLAN_NEGATIVE;
    if (n > PIECE_N_MAX) return PIECE_PLAN_LONG;
    if (cap < 0) return PIECE_PLAN_CAP;
    out->n = n; out->cap = cap;
    const int64_t nb = piece_chunks(n);                 // at most 2^19
    out->chunks = static_cast<int32_t>(nb);
    out->scan_per_thread = static_cast<int32_t>((nb + PIECE_SCAN_NT - 1) / PIECE_SCAN_NT);
    out->span_max = piece_span_max(f32, n);
    const size_t c = static_cast<size_t>(nb);
    out->b_bits = piece_align16(c * PIECE_NT * sizeof(uint16_t));
    out->b_cnt = out->b_last = out->b_base = out->b_open = piece_align16(c * sizeof(int32_t));
    out->b_head = out->b_tail = c * sizeof(PiecePart);
    return PIECE_PLAN_OK;
}

}  // namespace ps
