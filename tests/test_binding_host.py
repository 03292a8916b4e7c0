"""The Python binding's marshalling (pypore_amd/_lib.py, the helpers at the top of pypore_amd/engine.py) -- no GPU.

The nine ctypes structures against the C compiler's layout of include/poreseg.h (a stand-alone C program, tests/native/abi_layout.c,
prints sizeof and every offsetof; nothing is loaded into Python), the two repeat-on-PS_ERR_CAPACITY rules driven with fake
calls, Context.near_tie_sites growing its buffer on a fake library, and the one sample format.  The functions' signatures
against the header are in tests/test_host_logic.py."""
import ctypes
import os
import shutil
import subprocess
import threading

import pytest
import torch

from pypore_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = _lib.PS_ERR_CAPACITY
STRUCTS = {"ps_split_params": (_lib.SplitParams, 56), "ps_sample_format": (_lib.SampleFormat, 16), "ps_pool_plan_t": (_lib.PoolPlan, 16),
           "ps_statsplit_params": (_lib.StatSplitParams, 32), "ps_grid_report": (_lib.GridReport, 48), "ps_hmm_model": (_lib.HmmModel, 200),
           "ps_hmm_sample_tables": (_lib.HmmSampleTables, 48), "ps_near_tie": (_lib.NearTie, 16),
           "ps_filter_derivative_params": (_lib.FilterDerivativeParams, 40)}


@pytest.fixture(scope="module")
def abi_lines(tmp_path_factory):
    """What tests/native/abi_layout.c prints, split into words: the struct lines, then the enum lines."""
    tmp_path = tmp_path_factory.mktemp("abi")
    cc = next((p for p in map(shutil.which, ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang", "/opt/rocm/llvm/bin/clang")) if p), None)
    assert cc, "no C compiler found for tests/native/abi_layout.c"
    exe = str(tmp_path / "abi_layout")
    subprocess.check_call([cc, "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "abi_layout.c"), "-o", exe])
    return [line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_struct_layouts_match_the_compilers(abi_lines):
    printed = [words for words in abi_lines if words[1] != "enum"]
    expected = []
    for name, (struct, size) in STRUCTS.items():
        assert ctypes.sizeof(struct) == size, name
        expected.append([name, "sizeof", str(size)])
        expected += [["%s.%s" % (name, f[0]), str(getattr(struct, f[0]).offset)] for f in struct._fields_]
    assert printed == expected


def test_timing_indices_match_the_headers(abi_lines):
    """PS_MS_* and PS_CNT_* of include/poreseg.h are _lib.MS_NAMES and _lib.COUNTER_NAMES: same names, same order, same counts."""
    printed = [(words[0], int(words[2])) for words in abi_lines if words[1] == "enum"]
    expected = [("PS_MS_" + name.upper(), i) for i, name in enumerate(_lib.MS_NAMES)] + [("PS_MS_COUNT", len(_lib.MS_NAMES))] + \
               [("PS_CNT_" + name.upper(), i) for i, name in enumerate(_lib.COUNTER_NAMES) if name] + [("PS_CNT_COUNT", len(_lib.COUNTER_NAMES))]
    assert printed == expected
    assert (len(_lib.MS_NAMES), len(_lib.COUNTER_NAMES)) == (8, 20) and _lib.COUNTER_NAMES.index(None) == 19      # the last one is reserved
    keys = ["spine_ms", "tree_ms", "gather_ms", "total_ms", "stitch_ms", "bridge_ms", "blocksum_ms", "seq_ms", "windows", "candidates", "tiles",
            "tree_jobs", "repairs", "exact_rescans", "full_exact_scans", "wide_redo", "windows_spine", "windows_bridge", "windows_tree", "near_ties",
            "helper_chunks_published", "helper_chunks_taken", "tree_deferred", "windows_screen", "lookahead_skipped", "upload_skipped", "seams_resumed"]
    assert [n + "_ms" for n in _lib.MS_NAMES] + [n for n in _lib.COUNTER_NAMES if n] == keys           # the keys of Context.timings() as they were


# ---- the scalar-capacity rule ----------------------------------------------------------------------------------------------
def scripted(script):
    """attempt(cap) that answers the k-th call with script[k] = (status, reported size) and records the capacities it was given."""
    calls = []

    def attempt(cap):
        rc, need = script[len(calls)]
        calls.append(cap)
        return rc, need, "result of call %d" % len(calls)
    return attempt, calls


def test_retry_capacity_fits_at_once():
    attempt, calls = scripted([(0, 5)])
    assert engine._retry_capacity(None, attempt, 8) == "result of call 1" and calls == [8]


def test_retry_capacity_repeats_once_with_the_reported_size():
    attempt, calls = scripted([(CAPACITY, 20), (0, 20)])
    assert engine._retry_capacity(None, attempt, 8) == "result of call 2" and calls == [8, 20]


def test_retry_capacity_twice_is_an_error_of_check():
    attempt, calls = scripted([(CAPACITY, 20), (CAPACITY, 30)])
    with pytest.raises(RuntimeError, match=r"status -5") as e:
        engine._retry_capacity(None, attempt, 8)
    assert not isinstance(e.value, engine.CapacityError) and calls == [8, 20]


def test_retry_capacity_with_a_fixed_cap_names_the_size_required():
    attempt, calls = scripted([(CAPACITY, 20)])
    with pytest.raises(engine.CapacityError) as e:
        engine._retry_capacity(None, attempt, 8, fixed=True)
    assert (e.value.required, e.value.cap) == (20, 8) and calls == [8]


@pytest.mark.parametrize("reported", [8, 3, -1])
def test_retry_capacity_does_not_repeat_unless_the_report_exceeds_the_capacity(reported):
    attempt, calls = scripted([(CAPACITY, reported)])
    with pytest.raises(RuntimeError, match=r"status -5"):
        engine._retry_capacity(None, attempt, 8)
    assert calls == [8]


def test_retry_capacity_passes_other_errors_to_check():
    attempt, calls = scripted([(_lib.PS_ERR_ARG, 0)])
    with pytest.raises(ValueError):
        engine._retry_capacity(None, attempt, 8)
    assert calls == [8]


# ---- the per-sequence-slot rule --------------------------------------------------------------------------------------------
def scripted_slots(script, exact):
    calls, reads = [], []

    def attempt(*slots):
        calls.append(slots)
        return script[len(calls) - 1], "result of call %d" % len(calls)

    def reported():
        reads.append(len(calls))
        return exact
    return attempt, reported, calls, reads


def test_retry_slots_fits_at_once():
    attempt, reported, calls, reads = scripted_slots([0], ([3, 4],))
    assert engine._retry_slots(None, attempt, reported, ([9, 9],)) == (0, "result of call 1")
    assert calls == [([9, 9],)] and reads == []


def test_retry_slots_repeats_once_with_exactly_the_reported_sizes():
    exact = ([3, 4], [1, 2])
    attempt, reported, calls, reads = scripted_slots([CAPACITY, 0], exact)
    assert engine._retry_slots(None, attempt, reported, ([1, 1], [1, 1])) == (0, "result of call 2")
    assert calls == [([1, 1], [1, 1]), exact] and calls[1][0] is exact[0] and calls[1][1] is exact[1] and reads == [1]


def test_retry_slots_twice_is_an_error_of_check():
    attempt, reported, calls, reads = scripted_slots([CAPACITY, CAPACITY], ([3],))
    with pytest.raises(RuntimeError, match=r"status -5"):
        engine._retry_slots(None, attempt, reported, ([1],))
    assert len(calls) == 2 and reads == [1]


def test_retry_slots_without_retry_returns_the_status():
    attempt, reported, calls, reads = scripted_slots([CAPACITY], ([3],))
    assert engine._retry_slots(None, attempt, reported, ([1],), retry=False) == (CAPACITY, "result of call 1")
    assert len(calls) == 1 and reads == []
    attempt, reported, calls, reads = scripted_slots([_lib.PS_ERR_ARG], ([3],))
    with pytest.raises(ValueError):                                           # (any other status raises, retry or not)
        engine._retry_slots(None, attempt, reported, ([1],), retry=False)


# ---- Context.near_tie_sites on a fake library ------------------------------------------------------------------------------
class FakeLibrary(object):
    """ps_get_near_ties of a call that logged `n` sites: site k is (k, 10 k, 10 k + 7, -1 or 10 k + 3)."""

    def __init__(self, n, rc_when_fits=0):
        self.n, self.rc_when_fits, self.caps = n, rc_when_fits, []

    def ps_get_near_ties(self, handle, buf, cap, n_out):
        self.caps.append((cap, len(buf)))
        n_out._obj.value = self.n
        if self.n > cap:
            return CAPACITY
        for k in range(max(self.n, 0)):
            buf[k].event, buf[k].window_start, buf[k].window_end, buf[k].split = k, 10 * k, 10 * k + 7, (-1 if k % 2 else 10 * k + 3)
        return self.rc_when_fits


def fake_context(L):
    ctx = engine.Context.__new__(engine.Context)
    ctx.L, ctx.handle, ctx.lock = L, None, threading.RLock()
    return ctx


def test_near_tie_sites_grows_to_the_reported_count():
    L = FakeLibrary(65)
    sites = fake_context(L).near_tie_sites()
    assert L.caps == [(64, 64), (65, 65)]
    assert sites.dtype == engine.NEAR_TIE_DTYPE and len(sites) == 65
    assert sites["event"].tolist() == list(range(65)) and sites["window_start"].tolist() == [10 * k for k in range(65)]
    assert sites["window_end"].tolist() == [10 * k + 7 for k in range(65)]
    assert sites["split"].tolist() == [(-1 if k % 2 else 10 * k + 3) for k in range(65)]


def test_near_tie_sites_that_fit_or_are_not_counted_take_one_call():
    L = FakeLibrary(64)
    assert len(fake_context(L).near_tie_sites()) == 64 and L.caps == [(64, 64)]
    for n in (_lib.PS_NT_NOT_COUNTED, _lib.PS_NT_INCOMPLETE):
        L = FakeLibrary(n)
        assert fake_context(L).near_tie_sites() is None and L.caps == [(64, 64)]
    L = FakeLibrary(0)
    assert len(fake_context(L).near_tie_sites()) == 0


# ---- the sample format -----------------------------------------------------------------------------------------------------
def fields(fmt):
    return fmt.dtype, fmt.offset_counts, fmt.quantum


@pytest.mark.parametrize("f64", [False, True])
def test_fmt_float32_and_int16(f64):
    assert fields(engine._fmt(torch.empty(0, dtype=torch.float32), 0.03125, 7, f64=f64)) == (_lib.PS_DTYPE_F32, 7, 0.03125)
    assert fields(engine._fmt(torch.empty(0, dtype=torch.int16), 0.5, -3, f64=f64)) == (_lib.PS_DTYPE_I16, -3, 0.5)


def test_fmt_float64_only_where_the_caller_allows_it():
    x = torch.empty(0, dtype=torch.float64)
    assert fields(engine._fmt(x, 0.03125, 7, f64=True)) == (_lib.PS_DTYPE_F64, 0, 1.0)
    with pytest.raises(ValueError, match="samples must be float32 or int16, got torch.float64"):
        engine._fmt(x, 0.03125, 7)
    assert fields(engine.Context._fmt(torch.empty(0, dtype=torch.int16), 0.5, 0)) == (_lib.PS_DTYPE_I16, 0, 0.5)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.float16, torch.int64])
def test_fmt_refuses_every_other_dtype(dtype, f64):
    with pytest.raises(ValueError, match="samples must be float32 or int16, got %s" % dtype):
        engine._fmt(torch.empty(0, dtype=dtype), 1.0, 0, f64=f64)


def test_host_arrays_for_the_three_element_types():
    import numpy as np
    a, p = engine._host([3, 1, 2])
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"] and [p[k] for k in range(3)] == [3, 1, 2] and isinstance(p, ctypes.POINTER(ctypes.c_int64))
    a, p = engine._host(np.arange(6, dtype=np.int64)[::2], np.int32)
    assert a.dtype == np.int32 and [p[k] for k in range(3)] == [0, 2, 4] and isinstance(p, ctypes.POINTER(ctypes.c_int32))
    a, p = engine._host([0.5, 1.5], np.float64)
    assert a.dtype == np.float64 and [p[0], p[1]] == [0.5, 1.5] and isinstance(p, ctypes.POINTER(ctypes.c_double))
    b = np.zeros(4, dtype=np.int64)
    assert engine._host(b)[0] is b                                              # (an array that fits is taken as it is: outputs land in it)
    off, p = engine._slot_offsets([2, 0, 5])
    assert off.tolist() == [0, 2, 2, 7] and off.dtype == np.int64 and p[3] == 7
