"""The host's planning of the batch entry points (pypore_amd/csrc/batch_plan.hpp) -- no GPU.

A stand-alone C++ program, tests/native/batch_plan_check.cpp, includes the header the library is built from and checks, on the
CPU: the scratch planner of the pairwise aligner and the repeat splitter over random batches of 0, 1 and 1 000 items, budgets of
1 byte, a small one, the exact fit (and a byte less) and a huge one, 1, 3 and 10^6 slots -- the launches tile the batch in
order, their dims are the maximum of their items, the grid is the clamp and within budget and slots, every cut is greedy, the
slots are looked up twice per launch --; the pinned launches of eight sequences and of next_chunk; the sizes against the
formulas the GPU tests restate (pairwise_geometry.py, launch_geometry.py); what check_offsets, the slot and the event checks
refuse and the index they name, hostile tables included; the StatSplit and tile tables; offsets from counts.  The program is
built twice -- plain, and with -fsanitize=address,undefined -- and both builds run; nothing is loaded into Python.

The program's command-line modes (launches of given lengths under given slots) are what tests/test_batch_plan_gpu.py compares
the library's launches with; here they are asked for the pinned cases."""
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")
TRF_PINNED = [65, 65, 129, 3, 129, 65, 2, 130]
CHUNK_PINNED = [3, 3, 3, 10, 1]


def build(tmp, name, flags):
    # (no HIP include path, not even include/: the header stands on <stdint.h> and the standard library)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("batch_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


def _rows(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
    return [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]


def planned_launches(exe, kind, budget, default_slots, slots, items):
    """(q0, q1, grid, per_wg, lds) of every launch the planner cuts `items` into -- segment counts for kind "trf", (m, n) for
    "pw" -- under a budget in bytes and a fake resident_slots: slots = {dynamic LDS: slots}, default_slots for any other."""
    items = ["%dx%d" % it for it in items] if kind == "pw" else list(items)
    return _rows(exe, [kind, budget, default_slots] + ["%d:%d" % kv for kv in sorted(slots.items())] + ["--"] + items)


def planned_chunks(exe, budget, row_bytes, lens):
    """(q0, q1, bytes) of every launch next_chunk cuts sequences of these lengths into."""
    return _rows(exe, ["chunk", budget, row_bytes] + list(lens))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "batch plan ok" in r.stdout and not r.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_pinned_launches(programs, which):
    exe = programs[which]
    for slots in (8, 1000):
        assert planned_launches(exe, "trf", 40000, slots, {}, TRF_PINNED) == [(0, 7, 3, 12416, 3104), (7, 8, 1, 12512, 3128)]
        assert [l[:3] for l in planned_launches(exe, "trf", 1, slots, {}, TRF_PINNED)] == [(0, 2, 1), (2, 7, 1), (7, 8, 1)]
    # the slots of the launch's first sequence bound the budget test, those of the finished launch the grid
    assert planned_launches(exe, "trf", 40000, 8, {3 * 65 * 8 + 8: 2}, TRF_PINNED) == [(0, 8, 3, 12512, 3128)]
    assert planned_launches(exe, "trf", 40000, 8, {3104: 2}, TRF_PINNED) == [(0, 7, 2, 12416, 3104), (7, 8, 1, 12512, 3128)]
    assert planned_chunks(exe, 100, 8, CHUNK_PINNED) == [(0, 3, 96), (3, 4, 88), (4, 5, 16)]
    assert planned_chunks(exe, 1, 8, CHUNK_PINNED) == [(q, q + 1, (n + 1) * 8) for q, n in enumerate(CHUNK_PINNED)]
    # pairwise: a larger matrix cuts, a longer y alone does not; per_wg and LDS are pairwise_geometry's formulas
    got = planned_launches(exe, "pw", 1, 4, {}, [(8, 8), (1, 60), (9, 8), (9, 7)])
    assert got == [(0, 2, 1, (9 * 64 + 12 * 8 + 15) & ~15, 122 * 8), (2, 4, 1, (9 * 72 + 12 * 9 + 15) & ~15, 18 * 8)]


def test_the_library_defines_none_of_it():
    """What the header holds is defined there alone, the header stands on the standard library, and the library keeps neither
    the greedy rule nor the grid clamp."""
    consts = ("PW_NT PW_N_MAX TRF_NT TRF_N_MAX ALIGN_NT ALIGN_M_MAX ALIGN_B_MAX HMM_NT HMM_EXPECT_LDS HMM_EXPECT_ROWS SP_NT SP_ROUNDS "
              "SP_TILE").split()
    structs = "PwDims TrfDims ScratchLaunch AlignPlan StatsplitTables".split()
    funcs = ("pw_lds_bytes pw_scratch_bytes trf_lds_bytes trf_row_words trf_scratch_bytes align_lds_doubles slot_ok check_slot_offsets "
             "check_offsets check_events budget_grid next_chunk next_scratch_launch align_plan plan_statsplit_tables plan_tile_table "
             "offsets_from_counts").split()
    moved = [r"constexpr\s+\w+\s+%s\b" % c for c in consts] + [r"struct\s+%s\b\s*\{" % t for t in structs] + \
            [r"(?m)^[\w:\s]*[\w:]\s+%s\s*\([^;{]*\)\s*\{" % f for f in funcs]         # (a definition at the start of a line)
    header = open(os.path.join(CSRC, "batch_plan.hpp")).read()
    others = {name: open(os.path.join(CSRC, name)).read() for name in
              ("poreseg.hip", "seg_pairwise.hpp", "seg_trf.hpp", "seg_align.hpp", "seg_hmm.hpp", "seg_statsplit.hpp", "seg_state.hpp")}
    for pat in moved:
        assert re.search(pat, header), pat
        for name, text in others.items():
            assert not re.search(pat, text), (name, pat)
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h or h == "poreseg.h"], included
    lib = open(os.path.join(CSRC, "poreseg.hip")).read()
    assert '#include "batch_plan.hpp"' in lib
    assert "> budget) break" not in lib and lib.count("budget / per_wg") <= 1
    assert lib.count("next_scratch_launch(") == 2 and lib.count("next_chunk(") == 3
