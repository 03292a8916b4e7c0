"""The host's planning of ps_range_stats (pypore_amd/csrc/range_plan.hpp) -- no GPU.

A stand-alone C++ program, tests/native/range_plan_check.cpp, includes the header the library is built from and checks, on the
CPU: the unit tables of ranges of 1, T - 1, T, T + 1 and 2 T + 3 samples at every start alignment, for T = 64, 512 and the
default; overlapping, identical, nested and descending ranges, the buffer's two ends and the whole buffer; 70 000 one-sample
ranges; n_ranges = 0; every refusal with the index it names -- a negative start, an end behind the buffer, an empty and a
reversed range, a range of 2^31 samples, hostile tables (INT64_MIN, INT64_MAX, an end - start that would overflow) -- and the
tables of a refused call (empty); too many units; the validated range of option range_tile and the unit per sample type; the
sizes the arithmetic contract rests on.  The program is built twice -- plain, and with -fsanitize=address,undefined -- and both
builds run; nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "range_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")


def build(tmp, name, flags):
    # (no HIP include path, not even include/: the header stands on <stdint.h> and the standard library)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("range_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "range plan ok" in r.stdout and not r.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_units_per_range(programs, which):
    def units(tile, lens):
        r = subprocess.run([programs[which], "units", str(tile)] + [str(n) for n in lens], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
        return [int(v) for v in r.stdout.split()]
    for T in (64, 512, 16384):
        lens = [1, T - 1, T, T + 1, 2 * T + 3, 50000]
        assert units(T, lens) == [-(-n // T) for n in lens]


def test_the_library_defines_none_of_it():
    """What the header holds is defined there alone, the header stands on the standard library, and the entry point plans
    through it."""
    header = open(os.path.join(CSRC, "range_plan.hpp")).read()
    others = {name: open(os.path.join(CSRC, name)).read() for name in ("poreseg.hip", "seg_ranges.hpp")}
    moved = [r"constexpr\s+\w+\s+%s\b" % c for c in ("RANGE_NT", "RANGE_TILE_MIN", "RANGE_TILE_MAX", "RANGE_TILE_DEFAULT",
                                                    "RANGE_TILE_F32_MAX", "RANGE_LEN_MAX", "RANGE_UNITS_MAX")] + \
            [r"struct\s+%s\b\s*\{" % t for t in ("RangeRow", "RangeUnit", "RangePart", "RangePlan")] + \
            [r"(?m)^[\w:\s]*[\w:]\s+%s\s*\([^;{]*\)\s*\{" % f for f in ("check_ranges", "plan_ranges", "range_units", "range_unit", "range_tile_ok")]
    for pat in moved:
        assert re.search(pat, header), pat
        for name, text in others.items():
            assert not re.search(pat, text), (name, pat)
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h or h == "poreseg.h"], included
    assert '#include "range_plan.hpp"' in others["seg_ranges.hpp"] and '#include "seg_ranges.hpp"' in others["poreseg.hip"]
    assert others["poreseg.hip"].count("plan_ranges(") == 1
