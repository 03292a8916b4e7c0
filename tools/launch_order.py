#!/usr/bin/env python3
"""One context through every route of the segmentation host code, once each, on small seeded inputs -- to be run under a
kernel trace, once per library, so that the two ordered lists of launches can be compared:

    rocprofv3 --kernel-trace --output-format csv -d OUT_A -o t -- python tools/launch_order.py
    PORESEG_LIB=$PWD/pypore_amd/libporeseg_other.so rocprofv3 --kernel-trace --output-format csv -d OUT_B -o t -- python tools/launch_order.py
    python tools/launch_order.py --compare OUT_A OUT_B

--compare reads the *kernel_trace.csv under each directory and compares, launch by launch in dispatch order, kernel name,
grid, workgroup size and LDS size (whatever of these columns the trace has; it says which are missing).  Exit status 1
when the lists differ.  A refactor of the host code that leaves the device code alone must leave these lists equal.

`--tree-screen 0` (before any other argument) sets option tree_screen 0 on the context: the list of a library that has the
subtree screen is then, launch for launch, the list of one that does not (tree_screen 1, the default, adds one
tree_screen_kernel in front of every tree_kernel<64> of the narrow digest).  `--compare A B --names-only` compares the kernel
names without their parameter lists (tree_kernel gained arguments with the screen).

`--short-chain 0|1` sets option short_chain on the context (1 is the library's default): with 0 the list is, launch for launch,
the one of a library without the option.  The routes below run on a lone context, where the option only leaves out the upload
kernel of a call that repeats the layout of the call before it; `--pooled` runs them as a context that shares its device
(shared_device 16), where it also leaves out the look-ahead kernel.  Both flags go before any other argument, in any order."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES_ONLY = False        # --compare A B --names-only: kernel names without their parameter lists (a kernel that gained an argument)
COLUMNS = ["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
           "LDS_Block_Size"]


def launches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    have = [c for c in COLUMNS if rows and c in rows[0]]
    order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    return have, order, [tuple(r[c].split("(")[0] if c == "Kernel_Name" and NAMES_ONLY else r[c] for c in have) for r in rows]


def compare(dir_a, dir_b):
    have_a, order_a, a = launches(dir_a)
    have_b, order_b, b = launches(dir_b)
    print("columns compared: %s (ordered by %s / %s); missing: %s" %
          (", ".join(have_a), order_a, order_b, ", ".join(c for c in COLUMNS if c not in have_a) or "none"))
    print("launches: %d and %d" % (len(a), len(b)))
    if have_a != have_b:
        print("the two traces have different columns")
        return 1
    bad = 0
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            bad += 1
            if bad <= 10:
                print("launch %d differs:\n  %s\n  %s" % (i, x, y))
    if bad or len(a) != len(b):
        print("DIFFERENT: %d launches differ, lengths %d / %d" % (bad, len(a), len(b)))
        return 1
    print("the same %d launches in the same order" % len(a))
    return 0


def routes(tree_screen=None, short_chain=None, pooled=False):
    import numpy as np
    import torch
    from pypore_amd import _lib, engine, synth
    ctx = engine.Context(0)
    if tree_screen is not None:
        ctx.set_option("tree_screen", tree_screen)
    if short_chain is not None:
        ctx.set_option("short_chain", short_chain)
    if pooled:
        ctx.set_option("shared_device", 16)
    q = synth.QUANTUM
    p = _lib.split_params(prior_segments_per_second=10.)
    dense = _lib.split_params(min_width=100, max_width=1000000, window_width=10000, prior_segments_per_second=10., sampling_freq=1e5)
    k = synth.random_dwell_counts(300000, 11)
    f32 = torch.from_numpy(synth.counts_to_pa(k, np.float32)).cuda()
    i16 = torch.from_numpy(k.astype(np.int16)).cuda()
    one = np.array([0, k.size], dtype=np.int64)
    three = np.array([0, 90000, 90000, 300000], dtype=np.int64)       # (an empty event among them)
    done = []

    def note(name, bounds):
        done.append((name, int(bounds.numel()) if hasattr(bounds, "numel") else int(bounds)))

    def with_options(opts, fn, tiling=None):
        for o, v in opts:
            ctx.set_option(o, v)
        if tiling:
            ctx.set_tiling(*tiling)
        try:
            return fn()
        finally:
            for o, v in opts:
                ctx.set_option(o, DEFAULTS[o])
            if tiling:
                ctx.set_tiling(0, 0)

    DEFAULTS = {"stitch_host": 0, "scan_bs": 1, "tree_par": 1, "tree_mw": 0, "gather_fused": 1, "bridge_budget": 256}
    note("batch fp32", ctx.segment_batch(f32, one, p, q, want_stats=False)[0])
    note("batch int16", ctx.segment_batch(i16, three, p, q, want_stats=False)[0])
    note("multi-tile", with_options([], lambda: ctx.segment_batch(f32, one, p, q, want_stats=False)[0], tiling=(20000, 1)))
    note("stitch_host 1", with_options([("stitch_host", 1)], lambda: ctx.segment_batch(i16, one, p, q, want_stats=False)[0], tiling=(20000, 1)))
    note("scan_bs 0", with_options([("scan_bs", 0)], lambda: ctx.segment_batch(f32, three, p, q, want_stats=False)[0], tiling=(20000, 1)))
    note("tree_mw 1", with_options([("tree_mw", 1)], lambda: ctx.segment_batch(i16, one, p, q, want_stats=False)[0]))
    note("gather_fused 0", with_options([("gather_fused", 0)], lambda: ctx.segment_batch(f32, one, p, q, want_stats=False)[0]))
    note("statistics", ctx.segment_batch(i16, three, p, q, want_stats=True)[0])
    # densely stepped data with three anchors per bridge: seams give up and get their second chance on the device
    d = synth.dwell_table(77, 600000, 100, 400)
    kd = np.repeat(synth.LEVEL_COUNTS[np.arange(len(d)) % 5], d)[:600000] + synth.noise_counts(77, 0, 600000)
    td = torch.from_numpy(kd.astype(np.int16)).cuda()
    note("bridge_budget 3", with_options([("bridge_budget", 3)],
                                         lambda: ctx.segment_batch(td, np.array([0, kd.size], dtype=np.int64), dense, q, want_stats=False)[0]))
    note("  seams continued or repaired", ctx.timings()["repairs"])
    # a file trace: detector + events from one digest
    c, _ = synth.file_trace_counts(600000, 41, gap=30011, ev_lo=60000, ev_hi=200000)
    tc = torch.from_numpy(c.astype(np.int16)).cuda()
    note("ps_detect_segment_trace", ctx.detect_segment_trace(tc, q, p, threshold=90.0, min_duration=1000, want_stats=True)[2])
    w = np.array([[0, 10000], [5000, 15000], [100000, 110000]], dtype=np.int32)
    note("ps_audit_bounds", ctx.audit_bounds(f32, q, p, w)["corner"]["blocks"])
    note("ps_best_single_split", ctx.best_single_split(i16[:20000].contiguous(), q)[1])
    x64 = torch.from_numpy(synth.counts_to_pa(k[:120000], np.float64) * 1.0000001).cuda()
    note("ps_segment_exact_f64", ctx.segment_exact_f64(x64, np.array([0, 60000]), np.array([60000, 60000]), p)[0])
    # the 64-bit digest last (the context remembers the wide route for the next calls on this grid): levels more than 2^14 counts apart
    kw = np.clip((synth.random_dwell_counts(200000, 40, 400, 6000).astype(np.int64) - 1500) * 58, -32768, 32767)
    tw = torch.from_numpy(kw.astype(np.int16)).cuda()
    onew = np.array([0, kw.size], dtype=np.int64)
    for par in (1, 0):
        note("wide digest, tree_par %d" % par, with_options([("tree_par", par)], lambda: ctx.segment_batch(tw, onew, dense, q, want_stats=True)[0]))
        note("  wide_redo", ctx.timings()["wide_redo"])
    ctx.close()
    for name, n in done:
        print("%-32s %d" % (name, n))


if __name__ == "__main__":
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--compare":
        NAMES_ONLY = len(sys.argv) == 5 and sys.argv[4] == "--names-only"
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    opts, a = {}, sys.argv[1:]
    while a:
        if a[0] == "--pooled":
            opts["pooled"], a = True, a[1:]
        elif a[0] in ("--tree-screen", "--short-chain") and len(a) >= 2:
            opts[a[0][2:].replace("-", "_")], a = int(a[1]), a[2:]
        else:
            raise SystemExit("usage: launch_order.py [--tree-screen 0|1] [--short-chain 0|1] [--pooled] | --compare A B [--names-only]")
    routes(**opts)
