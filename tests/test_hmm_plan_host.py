"""The host's planning of the ps_hmm_* entry points (pypore_amd/csrc/hmm_plan.hpp) -- no GPU.

A stand-alone C++ program, tests/native/hmm_plan_check.cpp, includes the header the library is built from and checks, on the
CPU, with every model in exactly sized heap arrays: the round trip check -> layout -> pack -> resolve against the host blob for a
plain model, models with kernel-density states, vector models at D = 1, 3 and 16, mixture states beside a kernel-density state,
S = 1 with NE = 0, a model without edges and one of HMM_S_MAX states -- every table read through the kernels' structs equals the
caller's array, absent tables are null, (start, end, finite) sit behind out_dst --; the layout's invariants and its equality with
the sums the library used to spell out twice; that a changed parameter, edge probability, weight, component kind, kde point,
finite, start, end or n_dim is a changed blob; every refusal of hmm_model_check and hmm_sample_check with its exact text and the
index it names, on models of four states; hostile counts, refused on a model that has no arrays at all; a struct cut off before
the kde_* fields; the sampling upload staged and read back through its pointers; the derived sizes and decisions at their edges
(2^26 accumulators, HMM_EXPECT_LDS and 8 bytes above, 255 against 256 in-edges, the int32 path bound at `largest` and
`largest + 1`, the 8 and 16 GiB caps); hmm_short_slots.  The program is built twice -- plain, and with
-fsanitize=address,undefined -- and both builds run; nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

from test_pool_plan_host import ROOT, compiler

SRC = os.path.join(ROOT, "tests", "native", "hmm_plan_check.cpp")
CSRC = os.path.join(ROOT, "pypore_amd", "csrc")


def build(tmp, name, flags):
    # (include/ for poreseg.h, plain C: the two structs; no HIP include path)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hmm_plan")
    # (the sanitizers' runtimes linked into the program itself: clang's default; gcc needs to be told)
    gcc = "clang" not in subprocess.run([compiler(), "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if gcc else []
    return {"plain": build(tmp, "check", []),
            "sanitized": build(tmp, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_properties(programs, which):
    r = subprocess.run([programs[which]], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "hmm plan ok" in r.stdout and not r.stderr


def test_the_library_defines_none_of_it():
    """What the header holds is defined there alone, the header stands on the standard library, poreseg.h and batch_plan.hpp,
    and the entry points check, lay out, pack and resolve through it, each from one place."""
    header = open(os.path.join(CSRC, "hmm_plan.hpp")).read()
    others = {name: open(os.path.join(CSRC, name)).read() for name in ("poreseg.hip", "seg_hmm.hpp")}
    moved = [r"constexpr\s+\w+\s+(\w+\s*=[^,;]*,\s*)*%s\b" % c for c in
             ("HMM_S_MAX", "HMM_D_MAX", "HMM_KDE_POINTS_MAX", "HMM_MIX_COMPONENTS_MAX", "HMM_VITERBI", "HMM_FORWARD", "HMM_BACKWARD", "HMM_SILENT",
              "HMM_NORMAL", "HMM_UNIFORM", "HMM_KDE", "HMM_VECTOR", "HMM_LOGNORMAL", "HMM_EXPONENTIAL", "HMM_MIXTURE")] + \
            [r"struct\s+%s\b[^;{]*\{" % t for t in ("HmmDev", "HmmDevK", "HmmDevV", "HmmDevM", "HmmSampleDev", "HmmModelInfo", "HmmBlobLayout",
                                                   "HmmSampleLayout")] + \
            [r"(?m)^[\w:\s]*[\w:]\s+\*?%s\s*\([^;{]*\)\s*\{" % f for f in
             ("hmm_model_check", "hmm_blob_layout", "hmm_blob_pack", "hmm_blob_resolve", "hmm_sample_check", "hmm_sample_layout", "hmm_sample_resolve",
              "hmm_short_slots", "hmm_cdf_row", "hmm_lds_bytes", "hmm_expect_in_lds", "hmm_posterior_cnt", "hmm_bp_wide", "hmm_acc_check",
              "hmm_launch_check")]
    for pat in moved:
        assert re.search(pat, header), pat
        for name, text in others.items():
            assert not re.search(pat, text), (name, pat)
    included = re.findall(r"#include\s*[<\"]([^>\"]+)", header)
    assert included and not [h for h in included if "hip" in h], included
    assert not re.search(r"__global__|__device__|hipLaunch|hipMemcpy", header)
    assert '#include "hmm_plan.hpp"' in others["seg_hmm.hpp"] and '#include "seg_hmm.hpp"' in others["poreseg.hip"]
    hip = others["poreseg.hip"]
    for call in ("hmm_model_check(", "hmm_blob_layout(", "hmm_blob_pack(", "hmm_blob_resolve(", "hmm_sample_check(", "hmm_sample_layout(",
                 "hmm_sample_resolve(", "hmm_short_slots("):
        assert hip.count(call) == 1, call
    # the texts moved with the checks: the entry points carry them out as they are
    for text in ("null model array", "kde_ptr must start at 0", "null sampling table", "a path could exceed int32", "2^26 accumulators", "GiB at most"):
        assert text in header and text not in hip, text
