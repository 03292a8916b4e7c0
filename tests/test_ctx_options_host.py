"""The context's options (pypore_amd/csrc/ctx_options.hpp: one struct of values, one table of rules) -- no GPU.

A stand-alone C++ program, tests/native/ctx_options_check.cpp, includes the header the library is built from and checks, on the
CPU: every default against a literal list copied from the library before the table; for every row the lowest and the highest
value it takes, set and read back, one below and one above refused with the value left as it was; every member of the two
sets and its neighbours; the switches with 0, 1, -1 and 2^40; `timing` clamping; names the table does not have, the diagnostic
library's names in the product build; no name and no variable twice; short_chain <-> its bits; noise_k_ppm -> the float the
kernels see, 0.1f bit for bit; the environment function on a getenv that has every variable, with values it takes and with
values it refuses, PORESEG_NOISE_K=0.25, absent and empty variables, exactly the bad ones named.  The program is built four
times -- plain and with -fsanitize=address,undefined, each for the product and with -DPS_DIAG -- and all four run; nothing is
loaded into Python.  Its `table` mode prints the rows, which are compared here with the two lists Python keeps."""
import os
import re
import subprocess

import pytest

import launch_geometry
import pairwise_geometry
from pypore_amd import engine
from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "ctx_options_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")
ROW = ("name", "env", "lo", "hi", "default", "diag", "norm")


def build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, SRC, "-o", exe])
    return exe


def table_rows(exe):
    """The rows `exe table` prints, as dicts of ROW's keys (numbers as int; env None where the option has no variable)."""
    rows = []
    for line in subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.splitlines():
        r = dict(zip(ROW, line.split()))
        assert len(r) == len(ROW), line
        r.update({k: int(r[k]) for k in ("lo", "hi", "default", "diag")}, env=None if r["env"] == "-" else r["env"])
        rows.append(r)
    return rows


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ctx_options")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + (["-static-libasan", "-static-libubsan"] if gcc else [])
    return {"plain": build(tmp, "check", []), "sanitized": build(tmp, "check_san", san),
            "plain-diag": build(tmp, "check_diag", ["-DPS_DIAG"]), "sanitized-diag": build(tmp, "check_diag_san", ["-DPS_DIAG"] + san)}


@pytest.mark.parametrize("which", ["plain", "sanitized", "plain-diag", "sanitized-diag"])
def test_table_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ctx options ok (%s)" % ("diagnostic" if "diag" in which else "product") in r.stdout and not r.stderr


def test_python_keeps_the_same_lists(programs):
    """engine._ENV_OPTIONS is the table's variables (same variables, same options; the one fraction apart), and the defaults the
    test helpers restate are the table's."""
    rows = table_rows(programs["plain"])
    assert rows == table_rows(programs["plain-diag"])                       # (the product build prints the diagnostic rows too, flagged)
    by_name = {r["name"]: r for r in rows}
    assert len(by_name) == len(rows) >= 50
    with_var = {r["env"]: r["name"] for r in rows if r["env"]}
    assert with_var.pop("PORESEG_NOISE_K") == "noise_k_ppm"
    assert with_var == engine._ENV_OPTIONS
    assert engine.options_from_env({"PORESEG_NOISE_K": "0.25"})[0] == {"noise_k_ppm": 250000}
    for restated in (launch_geometry.LIBRARY_DEFAULTS, pairwise_geometry.LIBRARY_DEFAULTS):
        assert restated == {name: by_name[name]["default"] for name in restated}
    diag = {r["name"] for r in rows if r["diag"]}
    assert diag == {"dbg_phase", "dbg_k0_nogrp", "k0_sets", "scan_lds_pad", "rep_eval", "rep_stage", "rep_sum", "cu_mask"}


def test_the_library_defines_none_of_it():
    """The header stands on the standard library, poreseg.h and the plan headers; the library names no option, reads no PORESEG_*
    variable and indexes nothing ps_get_timings returns by a bare number: it goes through the table, once each."""
    header = open(os.path.join(CSRC, "ctx_options.hpp")).read()
    hip = open(os.path.join(CSRC, "poreseg.hip")).read()
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h], included
    assert set(h for h in included if h.endswith(".hpp")) == {"seg_types.hpp", "pool_plan.hpp", "range_plan.hpp", "filt_plan.hpp"}
    assert not re.search(r"__global__|__device__|hipLaunch|hipError_t|hipStream_t", header)
    assert '#include "ctx_options.hpp"' in hip
    assert 'n == "' not in hip and 'getenv("PORESEG_' not in hip and "strcmp" not in hip
    assert not re.search(r"counters\[\s*\d", hip) and not re.search(r"\bms\[\s*\d", hip)
    for call in ("opt_set(", "opt_get(", "opt_apply_env("):
        assert hip.count(call) == 1, call
    for text in ("struct CtxOptions", "OPT_ROWS[]", "SC_NO_UPLOAD = "):
        assert text in header and text not in hip, text
    # the product library reads one variable, the runtime's
    product = re.sub(r"(?ms)^#ifdef PS_DIAG$.*?^#endif$", "", hip)
    assert re.findall(r"getenv\(([^)]*)\)", product) == ['"GPU_MAX_HW_QUEUES"']
