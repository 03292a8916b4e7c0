"""The host's planning of a segment call (pypore_amd/csrc/seg_plan.hpp, seg_types.hpp) -- no GPU.

A stand-alone C++ program, tests/native/seg_plan_check.cpp, includes the header the library is built from and checks, on the CPU:
the device route's tile plan (tiles cover every event without gap or overlap, starts on multiples of 8, one tile length per event,
first_tile / ntiles / vbase / out_cap / out_off / boff / list_entries / total_len / sample_end as the layout gives them; the 1.5-tile
rule at 383 / 384 / 385 samples with tiles of 256; 1e8 samples at W = 10 000 -> 1 536 tiles, 1 024 x 50 000 -> 1 024 tiles), the
host route's halo tiles on both sides of len == L + H, the host stitch against a seeded next-anchor function (an anchor at a later
tile's start, a list that stops short and is repaired, a repair without progress, single tiles, empty events), the choice of
seams for the second chance, and the scan route with its wide-digest memory.  The program is built twice -- plain, and with
-fsanitize=address,undefined -- and both builds run; nothing is loaded into Python.

Not exercised: the plan's refusal of a call with too many tiles (DeviceTilePlan::too_many) -- it would need 2^31 jobs."""
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "seg_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")
# the batch tests/test_seg_plan_gpu.py runs: W 64, min_width 8, tiles of 256 samples, the block-sum route
GPU_CASE = dict(mw=8, W=64, tile_len=256, lens=(0, 9, 383, 0, 0, 384, 385, 1, 7, 8, 0, 2000, 0), tiles=17)


def build(tmp, name, flags):
    # (no HIP include path, not even include/: the two headers stand on <stdint.h> and the standard library)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seg_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


def planned_tiles(exe, mw, W, tile_len, lens, use_bs=1):
    r = subprocess.run([exe, "tiles", str(mw), str(W), str(tile_len), str(use_bs)] + [str(n) for n in lens], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return int(r.stdout)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "seg plan ok" in r.stdout


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_tiles_of_a_layout(programs, which):
    c = GPU_CASE
    assert planned_tiles(programs[which], c["mw"], c["W"], c["tile_len"], c["lens"]) == c["tiles"]
    assert planned_tiles(programs[which], 100, 10000, 0, [100000000]) == 1536
    assert planned_tiles(programs[which], 100, 10000, 0, [50000] * 1024) == 1024
    assert planned_tiles(programs[which], 8, 64, 256, []) == 0


def test_the_library_defines_none_of_it():
    """What moved into the two headers is defined there alone."""
    moved = (r"struct\s+(SpineJob|TreeJob|Item|AsmHeader|Anchor|TileList|TilePlace)\b\s*\{", r"\b(find_in|spine_cap|make_spine_job)\s*\([^;]*\)\s*\{",
             r"\bKIND_HIT\s*=", r"\bBR_DEFER_REACHED\s*=", r"constexpr\s+int\s+(BR_MAX|EXT_MAX|EXT_SLOTS|EXT_MAX_MANY|EXT_ROUNDS)\b")
    for name in ("poreseg.hip", "seg_device.hpp", "seg_bs.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        for pat in moved:
            assert not re.search(pat, text), (name, pat)
    both = open(os.path.join(CSRC, "seg_types.hpp")).read() + open(os.path.join(CSRC, "seg_plan.hpp")).read()
    for pat in moved:
        assert re.search(pat, both), pat
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", both)
    assert included and not [h for h in included if "hip" in h or h == "poreseg.h"], included
