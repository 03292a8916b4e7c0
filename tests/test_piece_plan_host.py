"""The host's planning of ps_detect_pieces (pypore_amd/csrc/piece_plan.hpp) -- no GPU.

A stand-alone C++ program, tests/native/piece_plan_check.cpp, includes the header the library is built from and checks, on the
CPU: the chunk count, the scan's share per thread and every scratch size at n = 0, 1, chunk - 1, chunk, chunk + 1, 3 chunk + 5
and 2^31 - 1; the refusals (n < 0, n > 2^31 - 1, cap < 0, hostile values) and what a refused call leaves; the capacity rule; and
the overflow bound -- that n * span^2 fits int64 for both sample types and that the bound is the largest such, in 128-bit integer
arithmetic.  The program is built twice -- plain, and with -fsanitize=address,undefined -- and both builds run; nothing is loaded
into Python."""
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "piece_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")
CHUNK = 4096


def build(tmp, name, flags):
    # (no HIP include path, not even include/: the header stands on <stdint.h> and <stddef.h>)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("piece_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "piece plan ok" in r.stdout and not r.stderr


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_chunks_and_scratch(programs, which):
    def plan(n, cap=0, f32=0):
        r = subprocess.run([programs[which], "plan", str(n), str(cap), str(f32)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr)
        return r.stdout.split()

    def pad(b):
        return -(-b // 16) * 16

    for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 2 ** 31 - 1):
        chunks = -(-n // CHUNK)
        want_bytes = pad(chunks * 256 * 2) + 4 * pad(chunks * 4) + 2 * chunks * 32
        got = [int(v) for v in plan(n)]
        assert got[0] == chunks and got[1] == -(-chunks // 1024) and got[2] == 65535 and got[3] == want_bytes, (n, got)
        span = int(plan(n, 0, 1)[2])
        assert max(n, 1) * span * span <= 2 ** 63 - 1 and (span == 2 ** 24 - 2 or max(n, 1) * (span + 1) ** 2 > 2 ** 63 - 1), (n, span)
    assert plan(-1) == ["refused", "1"] and plan(2 ** 31) == ["refused", "2"] and plan(5, -1) == ["refused", "3"]


def test_the_library_defines_none_of_it():
    """What the header holds is defined there alone, the header stands on the standard library, and the entry point plans
    through it."""
    header = open(os.path.join(CSRC, "piece_plan.hpp")).read()
    others = {name: open(os.path.join(CSRC, name)).read() for name in ("poreseg.hip", "seg_pieces.hpp")}
    moved = [r"constexpr\s+\w+\s+%s\b" % c for c in ("PIECE_NT", "PIECE_PER", "PIECE_CHUNK", "PIECE_SCAN_NT", "PIECE_N_MAX")] + \
            [r"struct\s+%s\b\s*\{" % t for t in ("PiecePart", "PiecePlan")] + \
            [r"(?m)^[\w:\s]*[\w:]\s+%s\s*\([^;{]*\)\s*\{" % f for f in ("plan_pieces", "piece_chunks", "piece_span_max", "piece_span_bound",
                                                                        "piece_capacity_ok")]
    for pat in moved:
        assert re.search(pat, header), pat
        for name, text in others.items():
            assert not re.search(pat, text), (name, pat)
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h or h == "poreseg.h"], included
    assert '#include "piece_plan.hpp"' in others["seg_pieces.hpp"] and '#include "seg_pieces.hpp"' in others["poreseg.hip"]
    assert others["poreseg.hip"].count("plan_pieces(") == 1 and others["poreseg.hip"].count("piece_capacity_ok(") == 1
    # the final expressions of a row are written once, and both entries' kernels call them
    ranges = open(os.path.join(CSRC, "seg_ranges.hpp")).read()
    assert len(re.findall(r"ps_segstat\s+segstat_from_sums\s*\(", ranges)) == 1 and ranges.count("segstat_from_sums(") == 2
    assert "segstat_from_sums(" in others["seg_pieces.hpp"] and "sqrt(" not in others["seg_pieces.hpp"]
