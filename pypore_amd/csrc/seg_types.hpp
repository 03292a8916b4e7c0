// seg_types.hpp -- the plain structs and constants that the host's planning (seg_plan.hpp) and the kernels (seg_device.hpp)
// share: job and item records as they lie in device memory, anchor kinds, bridge status codes, the sizes of the bridge chain
// and of its second chance.  Plain C++, <stdint.h> only: the host plan is compiled and tested without HIP
// (tests/native/seg_plan_check.cpp).  The layouts are pinned by the static_asserts below: host and device read the same bytes.
#pragma once
#include <stdint.h>

namespace ps {

constexpr int BR_MAX = 256;       // bridge chain: anchors a seam may add before it must have joined (densely stepped
                                  // data: two chains pick the best of ~10 steps per window and can take dozens of
                                  // anchors to meet; a seam that gives up sends the whole call to the host stitch)
// Round 5: seams that the bridges gave up on (BR_MAX anchors without meeting a downstream list: densely stepped data, where two
// chains can stay out of step for a long stretch) and open tiles that the true chain enters exactly at their start get a second
// chance on the device before the call falls back to the host stitch: the look-ahead kernel continues them with room for
// EXT_MAX more anchors each, in a side buffer (anchor i >= BR_MAX of seam g lives at ext[ext_slot[g] * EXT_MAX + i - BR_MAX]).
constexpr int EXT_MAX = 16384;     // further anchors of an extended seam when few seams need them (<= EXT_SLOTS) ...
constexpr int EXT_SLOTS = 64;
constexpr int EXT_MAX_MANY = 2048; // ... and when many do (a batch of events with a failed seam each): the side buffer holds
constexpr int EXT_ROUNDS = 4;      // EXT_SLOTS * EXT_MAX anchors either way; the stride is fixed by the first round of a call

enum : int { KIND_NONE = 0, KIND_HIT = 1, KIND_EARLY = 2, KIND_LATE = 3, KIND_STOP = 4 };   // STOP: gave up at stop_lim (spine tiles)

// Status of a seam's bridge, bmeta[g].w (seg_device.hpp: phase 1b): 0 nothing to do, 1 joined (continue with
// list[join_tile][join_idx+1..]), 2 the chain reached the end of the event, 3 gave up, 4 deferred to the look-ahead kernel
enum : int { BR_NONE = 0, BR_JOINED = 1, BR_ENDED = 2, BR_FAIL = 3, BR_DEFER = 4,
              BR_FAIL_REACHED = 5,                       // (set by the stitch: a failed seam that lies on the true path)
              BR_DEFER_REACHED = 6 };                    // (... a deferred seam nobody finished that does: short_chain, no look-ahead launch)

struct SpineJob {           // speculative spine of one tile: rec(start, end) without left subtrees
    int64_t base;           // offset of the event in the sample array
    int32_t start, end;     // chain anchor, event length
    int32_t stop;           // stop after the first spine anchor >= stop
    int32_t out_cap;
    int64_t out_off;        // into the anchor list storage (int2 entries)
    int32_t first_tile;     // global index of the event's first tile
    int32_t ntiles;         // tiles of this event
    int32_t tile_len;       // tile t of the event starts at t * tile_len
    int32_t ev;             // event index
    int64_t vbase;          // sum of the lengths of the preceding events (layout of the tree output regions)
};

struct TreeJob {            // full in-order traversal of rec(start, end), first window index j0
    int64_t base;
    int32_t start, end, j0;
    int32_t out_cap;
    int64_t out_off;        // into the private boundary scratch (int32) and the spill stack (int2)
    int32_t m, pad_;        // the event's centre (first count), pad_ = its phase (EvRef::ph), and first block (K0 digest; 0 on the LDS-window path)
    int64_t boff;
};

// gather: final boundary list = for every true spine anchor: [its left subtree..., anchor]
struct Item { int32_t job; int32_t anchor; };

}  // namespace ps

// Header written by assemble_tiles_kernel.  Kernels downstream of the device stitch take it as `hdr`: when
// it is non-null the item / job count is read from it on the device (no host round trip in the middle of
// the pipeline) and a failed stitch turns them into no-ops; when null the host-provided count is used.
// (Outside the namespace, where it has always stood: the kernels that take it keep their symbol names.)
struct AsmHeader { long long n_items, n_jobs, tscratch; int fail, pad; };

#define PS_LAYOUT(T, size) static_assert(sizeof(T) == size, #T ": size")
#define PS_FIELD(T, f, off) static_assert(__builtin_offsetof(T, f) == off, #T "::" #f ": offset")
PS_LAYOUT(ps::SpineJob, 56);
PS_FIELD(ps::SpineJob, base, 0);        PS_FIELD(ps::SpineJob, start, 8);      PS_FIELD(ps::SpineJob, end, 12);
PS_FIELD(ps::SpineJob, stop, 16);       PS_FIELD(ps::SpineJob, out_cap, 20);   PS_FIELD(ps::SpineJob, out_off, 24);
PS_FIELD(ps::SpineJob, first_tile, 32); PS_FIELD(ps::SpineJob, ntiles, 36);    PS_FIELD(ps::SpineJob, tile_len, 40);
PS_FIELD(ps::SpineJob, ev, 44);         PS_FIELD(ps::SpineJob, vbase, 48);
PS_LAYOUT(ps::TreeJob, 48);
PS_FIELD(ps::TreeJob, base, 0);         PS_FIELD(ps::TreeJob, start, 8);       PS_FIELD(ps::TreeJob, end, 12);
PS_FIELD(ps::TreeJob, j0, 16);          PS_FIELD(ps::TreeJob, out_cap, 20);    PS_FIELD(ps::TreeJob, out_off, 24);
PS_FIELD(ps::TreeJob, m, 32);           PS_FIELD(ps::TreeJob, pad_, 36);       PS_FIELD(ps::TreeJob, boff, 40);
PS_LAYOUT(ps::Item, 8);
PS_FIELD(ps::Item, job, 0);             PS_FIELD(ps::Item, anchor, 4);
PS_LAYOUT(AsmHeader, 32);
PS_FIELD(AsmHeader, n_items, 0);        PS_FIELD(AsmHeader, n_jobs, 8);        PS_FIELD(AsmHeader, tscratch, 16);
PS_FIELD(AsmHeader, fail, 24);          PS_FIELD(AsmHeader, pad, 28);
#undef PS_LAYOUT
#undef PS_FIELD
