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


SENTINEL = -7


def batch_once(ctx, pairs, mode, penalty, min_length, col_slots, aln_slots):
    """One ps_pairwise_batch call, as engine.Context.pairwise_batch makes it, with the caller's slots and with every
    output buffer filled with SENTINEL beforehand; nothing is run again.  pairs: (x, y) of float64 arrays (NaN: the marker).
    Returns (return code, dict of the raw buffers as numpy arrays, col_off, aln_off)."""
    import ctypes

    import numpy as np
    import torch
    dev = torch.device("cuda", ctx.device)

    def pack(seqs):
        off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
        flat = np.concatenate([np.asarray(s, dtype=np.float64) for s in seqs]) if off[-1] else np.zeros(1)
        return torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float64)).to(dev), off
    a, a_off = pack([p[0] for p in pairs])
    b, b_off = pack([p[1] for p in pairs])
    n = len(pairs)
    idx = np.arange(n, dtype=np.int32)
    col_off = np.concatenate(([0], np.cumsum(col_slots))).astype(np.int64)
    aln_off = np.concatenate(([0], np.cumsum(aln_slots))).astype(np.int64)
    n_col, n_aln = int(col_off[-1]) + 16, int(aln_off[-1]) + 16          # a margin behind the last slot, watched too
    i32 = lambda k: torch.full((k,), SENTINEL, dtype=torch.int32, device=dev)
    f64 = lambda k: torch.full((k,), float(SENTINEL), dtype=torch.float64, device=dev)
    buf = {"scores": f64(n), "status": i32(n), "cols_i": i32(n_col), "cols_j": i32(n_col), "col_need": i32(n),
           "aln_score": f64(n_aln), "aln_start": i32(n_aln), "aln_len": i32(n_aln), "aln_count": i32(n)}
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda name: ctypes.c_void_p(buf[name].data_ptr())
    torch.cuda.synchronize(dev)
    with ctx.lock:
        rc = ctx.L.ps_pairwise_batch(
            ctx.handle, ctypes.c_void_p(a.data_ptr()), a_off.ctypes.data_as(i64p), n, ctypes.c_void_p(b.data_ptr()),
            b_off.ctypes.data_as(i64p), n, idx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p), n, int(mode), float(penalty),
            int(min_length), ptr("scores"), ptr("status"), col_off.ctypes.data_as(i64p), ptr("cols_i"), ptr("cols_j"),
            ptr("col_need"), aln_off.ctypes.data_as(i64p), ptr("aln_score"), ptr("aln_start"), ptr("aln_len"), ptr("aln_count"))
    return rc, {k: v.cpu().numpy() for k, v in buf.items()}, col_off, aln_off
