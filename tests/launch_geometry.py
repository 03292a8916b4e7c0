"""Test-side helpers for the launch geometry of the batch kernels: options set for one block and restored afterwards, and
the slot counts the library prints under option `debug` (resident_slots, csrc/poreseg.hip), matched by dynamic LDS."""
import contextlib
import re

from pypore_amd import engine

# the library's own defaults (csrc/poreseg.hip ps_ctx) of the options these tests change
LIBRARY_DEFAULTS = {"debug": 0, "slots_pct": 100, "hmm_bp_budget": 512 << 20, "hmm_fb_budget": 4 << 30,
                    "hmm_expect_lds": 1, "filter_fused": 1}

_SLOTS = re.compile(r"\[poreseg\] resident slots: (\d+) \((\d+) threads, dynamic LDS (\d+), slots_pct (\d+)\)")


def default(name):
    """What a context of this process starts with (PORESEG_* modes fill engine.DEFAULT_OPTIONS)."""
    return engine.DEFAULT_OPTIONS.get(name, LIBRARY_DEFAULTS[name])


@contextlib.contextmanager
def options(ctx, **opts):
    """Sets the options on ctx for the block; restores every one of them to its default in `finally`."""
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        yield ctx
    finally:
        for name in opts:
            ctx.set_option(name, default(name))


def printed_slots(err, lds):
    """The slot counts resident_slots printed in `err` (captured stderr) for launches of dynamic LDS `lds` bytes, as
    (slots, slots_pct) in order."""
    return [(int(m.group(1)), int(m.group(4))) for m in _SLOTS.finditer(err) if int(m.group(3)) == lds]


def align_geometry(m, n_seq, s_max):
    """ps_align_batch's traceback block B, dynamic LDS bytes and scratch cap on the grid (csrc/poreseg.hip)."""
    budget = (12 << 10) if n_seq > 512 else (48 << 10)
    B = max(1, min(32, budget // (24 * m)))
    lds = ((9 + 3 * B + 1) * m + 3 * 64 + 2) * 8
    cap = max(1, (2 << 30) // (24 * max(s_max, 1) * m))
    return B, lds, cap
