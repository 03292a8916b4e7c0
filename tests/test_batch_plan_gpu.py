"""The batch entry points launch what pypore_amd/csrc/batch_plan.hpp plans: the launches the library prints under option `debug`
are the ones the stand-alone program of tests/test_batch_plan_host.py plans for the same items, the same budget and the slot
counts the library printed, and the results are still those of the uncut calls and the oracles.

The repeat splitter: the eight sequences of the host test's pinned case under budgets of 40 000 bytes and 1 byte.  The pairwise
aligner: ten square pairs, global and repeated, under a budget of two of the 200 x 200 matrices, under slots_pct 1, and both.
Posterior decoding: five sequences of 3, 3, 3, 10 and 1 observations under a budget of 100 bytes per state."""
import re

import numpy as np
import pytest

import launch_geometry as LG
import pairwise_geometry as PG
import pairwise_oracle as PWO
import hmm_oracle as HO
import test_pairwise_gpu as TP
import test_posterior_gpu as TPOST
import test_trf_gpu as TT
import trf_cases as C
from test_batch_plan_host import CHUNK_PINNED, TRF_PINNED, build, planned_chunks, planned_launches

pytestmark = pytest.mark.gpu

_TRF_LAUNCH = re.compile(r"\[poreseg\] trf launch: sequences (\d+)\.\.(\d+), grid (\d+), (\d+) bytes of scratch per workgroup, dynamic LDS (\d+)")
_SLOTS = re.compile(r"\[poreseg\] resident slots: (\d+) \(64 threads, dynamic LDS (\d+), slots_pct \d+\)")
_POSTERIOR = re.compile(r"posterior launch: sequences (\d+)\.\.(\d+), (\d+) bytes of forward matrix")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("batch_plan_gpu"), "check", [])


def printed_slots(err):
    """{dynamic LDS: slots} of the 64-thread lookups printed in `err`; one kernel and one slots_pct per capture, so a size has
    one count."""
    table = {}
    for m in _SLOTS.finditer(err):
        assert table.setdefault(int(m.group(2)), int(m.group(1))) == int(m.group(1)), m.group(0)
    return table


@pytest.mark.parametrize("budget", [40000, 1])
def test_trf_launches_are_the_planned_ones(program, capfd, budget):
    names = ["grid_seam_n65", "off_seam_n65", "grid_seam_n129", "grid_seam_n3", "off_seam_n129", "grid_seam_n65", "grid_seam_n2"]
    by_name = {c["name"]: c for c in TT.CASES}
    seqs = [TT.pair(by_name[n]) for n in names] + [C.planted(np.random.default_rng(130), 130, True, [(5, 1, False)], 10.0, 60.0)]
    assert [len(s[0]) for s in seqs] == TRF_PINNED
    last = TT.naive_splits_batch([seqs[-1]])[0]
    ctx = TT.engine.context(None)
    capfd.readouterr()
    with LG.options(ctx, debug=1):
        got = TT.with_option("trf_budget", budget, 2 << 30, lambda: TT.naive_splits_batch(seqs))
    err = capfd.readouterr().err
    # (a call whose repeat slots were too small runs the batch again: every pass over the batch prints its launches)
    passes = PG.passes([tuple(int(g) for g in m.groups()) for m in _TRF_LAUNCH.finditer(err)])
    slots = printed_slots(err)
    print(passes, slots)
    want = planned_launches(program, "trf", budget, 0, slots, TRF_PINNED)
    assert passes and all(launches == want for launches in passes)
    if min(slots.values()) >= 8:                                                  # (the pinned case: 8 slots and more)
        assert [l[:3] for l in want] == ([(0, 7, 3), (7, 8, 1)] if budget == 40000 else [(0, 2, 1), (2, 7, 1), (7, 8, 1)])
    TT.check_batch(got[:-1], names)
    assert C.same_bits(got[-1], last)


PW_SIZES = [30, 5, 64, 1, 200, 30, 90, 400, 2, 64]


@pytest.fixture(scope="module", params=[PWO.GLOBAL, PWO.REPEATED], ids=["global", "repeated"])
def pairwise_case(request):
    """(mode, pairs, the one-launch run), that run checked against the restatement; the repeated mode's values from a wide range,
    so that the restatement's arg-max per alignment stays quick."""
    mode = request.param
    rng = np.random.default_rng(31 + mode)
    hi = 400.0 if mode == PWO.REPEATED else 26.0
    pairs = [(TP.values(rng, n, True, 20.0, hi), TP.values(rng, n, True, 20.0, hi)) for n in PW_SIZES]
    whole = TP.run(pairs, mode)
    TP.assert_equals_restatement(pairs, mode, -1, 2, whole)
    return mode, pairs, whole


@pytest.mark.parametrize("opts", [{"pairwise_budget": 2 * PG.scratch_bytes(200 * 200, 200)}, {"slots_pct": 1},
                                  {"pairwise_budget": 2 * PG.scratch_bytes(200 * 200, 200), "slots_pct": 1}],
                         ids=["budget", "slots_pct_1", "budget_and_slots_pct_1"])
def test_pairwise_launches_are_the_planned_ones(program, capfd, pairwise_case, opts):
    from pypore_amd import engine
    mode, pairs, whole = pairwise_case
    budget = opts.get("pairwise_budget", PG.LIBRARY_DEFAULTS["pairwise_budget"])
    capfd.readouterr()
    with PG.options(engine.context(), debug=1, **opts):
        cut = TP.run(pairs, mode)
    err = capfd.readouterr().err
    slots = printed_slots(err)
    want = planned_launches(program, "pw", budget, 0, slots, [(n, n) for n in PW_SIZES])
    passes = PG.passes(PG.printed_launches(err))
    print(passes, slots)
    assert passes and all(launches == want for launches in passes)
    assert all(per_wg == PG.scratch_bytes(*max((n * n, n) for n in PW_SIZES[q0:q1])) and lds == PG.lds_bytes(max(PW_SIZES[q0:q1]))
               for q0, q1, _, per_wg, lds in want)
    if "pairwise_budget" in opts:
        assert len(want) > 1
    for q in range(len(pairs)):
        assert TP.same(TP.unpack(cut, q), TP.unpack(whole, q)), q


def test_posterior_launches_are_the_planned_chunks(program, capfd):
    from pypore_amd import engine
    model = HO.line_model(6)
    S = len(model.states)
    rng = np.random.default_rng(6)
    seqs = [rng.normal(0, 3, n) for n in CHUNK_PINNED]
    whole = TPOST.check_case(model, seqs)
    capfd.readouterr()
    with LG.options(engine.context(), hmm_fb_budget=100 * S, debug=1):
        cut = TPOST.Raw(model, seqs)
    got = [tuple(int(g) for g in m.groups()) for m in _POSTERIOR.finditer(capfd.readouterr().err)]
    assert got == planned_chunks(program, 100 * S, 8 * S, CHUNK_PINNED) == [(0, 3, 96 * S), (3, 4, 88 * S), (4, 5, 16 * S)]
    assert whole.same_bits(cut)
