"""Test-side helpers for the launch geometry of the pairwise aligner (ps_pairwise_batch, csrc/poreseg.hip): its options set
for one block and restored afterwards, the dynamic LDS of a launch and the launches the library prints under `debug`."""
import contextlib
import re

from pypore_amd import engine

LIBRARY_DEFAULTS = {"debug": 0, "slots_pct": 100, "pairwise_budget": 2 << 30}

_LAUNCH = re.compile(r"\[poreseg\] pairwise launch: pairs (\d+)\.\.(\d+), grid (\d+), (\d+) bytes of scratch per workgroup, dynamic LDS (\d+)")
_SLOTS = re.compile(r"\[poreseg\] resident slots: (\d+) \((\d+) threads, dynamic LDS (\d+), slots_pct (\d+)\)")


@contextlib.contextmanager
def options(ctx, **opts):
    """Sets the options on ctx for the block; restores every one of them to its default in `finally`."""
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        yield ctx
    finally:
        for name in opts:
            ctx.set_option(name, engine.DEFAULT_OPTIONS.get(name, LIBRARY_DEFAULTS[name]))


def lds_bytes(n_max):
    """Dynamic LDS of a launch whose longest y has n_max elements: y and the border row (csrc/seg_pairwise.hpp)."""
    return (2 * max(n_max, 1) + 2) * 8


def scratch_bytes(cells, rows):
    """Scratch of one workgroup: fp64 scores, a pointer byte per cell, row maxima and their columns."""
    return (8 * cells + 12 * rows + cells + 15) & ~15


def printed_launches(err):
    """(first pair, end pair, grid, scratch bytes per workgroup, dynamic LDS) of every launch printed in `err`."""
    return [tuple(int(g) for g in m.groups()) for m in _LAUNCH.finditer(err)]


def printed_slots(err, lds):
    """(slots, slots_pct) of every resident_slots line for 64-thread launches of dynamic LDS `lds`."""
    return [(int(m.group(1)), int(m.group(4))) for m in _SLOTS.finditer(err) if int(m.group(3)) == lds and int(m.group(2)) == 64]


def passes(launches):
    """The printed launches grouped by pass over the batch: a call whose slots were too small runs the batch again with
    the sizes the first pass reported (PS_ERR_CAPACITY), so its launches are printed twice."""
    out = []
    for l in launches:
        if l[0] == 0:
            out.append([])
        out[-1].append(l)
    return out
