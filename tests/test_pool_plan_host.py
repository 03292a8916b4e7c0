"""ps_pool_plan and the parsing of GPU_MAX_HW_QUEUES (pypore_amd/csrc/pool_plan.hpp, include/poreseg.h) -- no GPU.

The table's properties are checked by a stand-alone C++ program, tests/native/pool_plan_check.cpp, which includes the header the
library is built from: n x queues over {0, 1, 2, 3, 4, 5, 15, 16, 17, 64} x {1, 4, 16, 32}; the lone row and the row of sixteen
calls and more as include/poreseg.h states them; the plan a function of min(n, queues) alone; monotone in n_eff.  The program
is built twice -- plain, and with -fsanitize=address,undefined -- and both builds run.  The same expectations are then asked of
the library's export through ctypes, so that what the program checked is what libporeseg.so applies."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pool_plan_check.cpp")
NS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 64)
QS = (1, 4, 16, 32)
ENV_CASES = ((None, 4), ("4", 4), ("16", 16), ("0", 1), ("abc", 4), ("99", 32))


def compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no C++ compiler found for tests/native/pool_plan_check.cpp")


def build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pypore_amd", "csrc"), SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pool_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


def clean_env(value):
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if value is not None:
        env["GPU_MAX_HW_QUEUES"] = value
    return env


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_table_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True, env=clean_env(None))
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "pool plan ok" in r.stdout


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_queues_from_the_environment(programs, which):
    for value, want in ENV_CASES:
        r = subprocess.run([programs[which], "env"], capture_output=True, text=True, env=clean_env(value))
        assert r.returncode == 0 and int(r.stdout) == want, (value, r.stdout, r.stderr)


def share(v):
    return v if v else 1 << 30           # k0_waves 0: every slot; k0_admit 0: no limit


def test_library_export():
    from pypore_amd import _lib
    plans = {}
    for n in NS:
        for q in QS:
            p = _lib.pool_plan(n, q)
            assert p["n_eff"] == min(n, q)
            plans.setdefault(p["n_eff"], p)
            assert plans[p["n_eff"]] == p, "the plan depends on min(n, queues) only: %r" % ((n, q),)
            if p["n_eff"] <= 1:
                assert (p["k0_waves"], p["k0_admit"], p["lat_help"]) == (0, 0, 1)
            if p["n_eff"] >= 16:
                assert (p["k0_waves"], p["k0_admit"], p["lat_help"]) == (1, 3, 0)
    rows = [_lib.pool_plan(n, 32) for n in range(0, 33)]
    for a, b in zip(rows, rows[1:]):
        assert share(b["k0_waves"]) <= share(a["k0_waves"]) and share(b["k0_admit"]) <= share(a["k0_admit"]) and b["lat_help"] <= a["lat_help"], (a, b)
    assert _lib.pool_plan(16, 0) == _lib.pool_plan(16, 4)
    with pytest.raises(ValueError):
        _lib.pool_plan(-1, 4)
    # the library read this process's variable the way the program does
    want = dict(ENV_CASES).get(os.environ.get("GPU_MAX_HW_QUEUES"))
    if want is not None:
        assert _lib.hw_queues() == want
    assert 1 <= _lib.hw_queues() <= 32
    # the gate's bookkeeping answers without a GPU
    g = _lib.gate_stats(0)
    assert g["open"] == 0 and g["gave_up"] == 0
