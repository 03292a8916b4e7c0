"""The host's planning of a batched Bessel filter call (pypore_amd/csrc/filt_plan.hpp) -- no GPU.

A stand-alone C++ program, tests/native/filt_plan_check.cpp, includes the header the library is built from and checks, on the
CPU: every event's units cover [0, n + 2 pad) exactly once and in order; the unit counts at n + 12 = T - 1, T, T + 1, 2 T,
2 T + 1 and at n = 7; 0 events, 1 event, 100 000 events of 7 samples; the table entries against the per-event records; the
scratch groups of the order-n route (each within the cap except a lone oversized event, order kept, every event in exactly one,
greedy, a small cap gives one event per group); the refusals and the event they name; the order-1 route's halo against
alpha^H <= 2^-60 over a sweep of poles; the re-quantisation's workgroups.  The program is built twice -- plain, and with
-fsanitize=address,undefined -- and both builds run; nothing is loaded into Python.

The route function is also asked about the cutoffs the GPU tests use, against the rule restated here (filter_exact.py restates
it once more for the existing tests): 2 000 Hz at 100 kHz is the default and fused, 650 Hz the last fused cutoff of the
hundreds, 600 Hz takes the scan, 20 kHz has the smallest halo."""
import math
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "filt_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")
CHUNK, H_MAX, PAD1 = 4096, 1024, 6


def build(tmp, name, flags):
    # (no HIP include path, not even include/: the header stands on <stdint.h> and the standard library)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("filt_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


def pole(cutoff, second):
    """alpha = -a1 of scipy.signal.bessel(1, cutoff / (second / 2)): bilinear transform with pre-warping, fs = 2."""
    wo = 4.0 * math.tan(math.pi * (cutoff / (second / 2.0)) / 2.0)
    return -((wo - 4.0) / (wo + 4.0))


def rule(alpha, fused=1):
    """(H, T): the smallest multiple of 64, at least 64, with alpha^H <= 2^-60; (0, 0) beyond H_MAX -- the scan route."""
    if not fused or not 0.0 < alpha < 1.0:
        return 0, 0
    h_req = math.ceil(60.0 * math.log(2.0) / -math.log(alpha))
    if h_req > H_MAX:
        return 0, 0
    H = max(64, (int(h_req) + 63) // 64 * 64)
    return H, CHUNK - 2 * H


def route(exe, alpha, fused=1):
    r = subprocess.run([exe, "route", repr(alpha), str(fused)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    H, T = (int(v) for v in r.stdout.split())
    return H, T


def units(exe, pad, unit, lens):
    r = subprocess.run([exe, "units", str(pad), str(unit)] + [str(n) for n in lens], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return [int(v) for v in r.stdout.split()]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "filt plan ok" in r.stdout


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_route_at_the_cutoffs_in_use(programs, which):
    exe = programs[which]
    got = {}
    for cutoff in (2000., 650., 600., 20000., 700., 10., 49000.):
        alpha = pole(cutoff, 1.e5)
        got[cutoff] = route(exe, alpha)
        assert got[cutoff] == rule(alpha), (cutoff, alpha)
        assert route(exe, alpha, fused=0) == (0, 0)
    # what the rule says about them: the default is fused, 650 Hz sits on the largest halo, 600 Hz is past it, 20 kHz on the smallest
    assert 64 < got[2000.][0] < H_MAX and got[2000.][1] == CHUNK - 2 * got[2000.][0]
    assert got[650.] == (H_MAX, CHUNK - 2 * H_MAX)
    assert got[600.] == (0, 0) and got[10.] == (0, 0)
    assert got[20000.][0] == 64
    assert pole(49000., 1.e5) < 0.0 and got[49000.] == (0, 0)                 # (a pole left of zero: never fused)
    # the pole and the halo of the default, from the arithmetic alone: alpha^H <= 2^-60 < alpha^(H - 64)
    a, H = pole(2000., 1.e5), got[2000.][0]
    assert a ** H <= 2.0 ** -60 < a ** (H - 64)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_units_around_the_tile(programs, which):
    exe = programs[which]
    for cutoff in (2000., 650., 20000.):
        T = rule(pole(cutoff, 1.e5))[1]
        lens = [T - 1 - 2 * PAD1, T - 2 * PAD1, T + 1 - 2 * PAD1, 2 * T - 2 * PAD1, 2 * T + 1 - 2 * PAD1, 7, 3 * T + 5]
        assert units(exe, PAD1, T, lens) == [-(-(n + 2 * PAD1) // T) for n in lens] == [1, 1, 2, 2, 3, 1, 4]
    assert units(exe, PAD1, 3328, [7] * 1000) == [1] * 1000
    assert units(exe, 9, 1024, [1024 - 18, 1024 - 17, 70000]) == [1, 2, 69]
    r = subprocess.run([exe, "units", "6", "3328", "100", "6", "5"], capture_output=True, text=True)
    assert r.stdout.split() == ["refused", "2", "1"]                          # FILT_PLAN_SHORT, event 1


def test_the_library_defines_none_of_it():
    """What the header holds is defined there alone, and the header stands on the standard library."""
    moved = (r"constexpr\s+int\s+(FILT_NT|FILT_PER|FILT_CHUNK|FILT_PAD|FILT_MAXORD|FILT_H_MAX|RQ_NT)\b",
             r"struct\s+(FiltEvent|FiltUnit|FiltGroup|FiltPlan|RequantEvent|RequantPlan)\b\s*\{",
             r"(?m)^\s*(?:inline\s+|static\s+)*[\w:]+\s+(filt_route1|filt_tile|filt_units|filt_padlen|plan_filter_batch|plan_requant_batch|"
             r"requant_grid)\s*\([^;{]*\)\s*\{")
    header = open(os.path.join(CSRC, "filt_plan.hpp")).read()
    for pat in moved:
        assert re.search(pat, header), pat
        for name in ("poreseg.hip", "seg_device.hpp", "seg_filter.hpp"):
            assert not re.search(pat, open(os.path.join(CSRC, name)).read()), (name, pat)
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h or h == "poreseg.h"], included
    lib = open(os.path.join(CSRC, "poreseg.hip")).read()
    assert '#include "filt_plan.hpp"' in lib
    # the halo rule is written once: neither entry restates it
    assert "60.0 * std::log(2.0)" not in lib and lib.count("filt_route1(") == 2
