"""NaiveTRF on the GPU (ps_trf_split_batch, csrc/seg_trf.hpp) against the goldens recorded from the reference
(tests/golden/make_golden_trf.py) and the restatement (tests/trf_oracle.py): yields with their scores and rows, bit for
bit, on every case; then the batch, the capacity path, max_repeats, the launch split by "trf_budget", "slots_pct", the cap,
an event parsed on the device, and the scratch that a second call reuses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trf_cases as C  # noqa: E402
import trf_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pypore_amd import _lib, engine, synth  # noqa: E402
from pypore_amd.alignment import NaiveTRF, naive_splits_batch, naive_splits_batch_raw, naive_trf_batch  # noqa: E402

CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
GROUPS = {}                                  # a batch call has one penalty and one min_score: the cases by those
for _c in CASES:
    GROUPS.setdefault((_c["penalty"], _c["min_score"]), []).append(_c)
DEFAULT = GROUPS[(-1.0, 2.0)]


class Seg(object):
    def __init__(self, k, mean, std):
        self.k, self.mean, self.std = k, mean, std


def pair(c):
    return (c["means"], c["stds"])


def per_sequence():
    """The device yields of every case from a call of its own, computed once."""
    if "per" not in C._cache:
        C._cache["per"] = {c["name"]: naive_splits_batch([pair(c)], c["penalty"], c["min_score"])[0] for c in CASES}
    return C._cache["per"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden(case):
    want = C.golden_yields(case["name"])
    got = naive_splits_batch([pair(case)], case["penalty"], case["min_score"])[0]
    assert C.same_bits(got, want)
    assert C.same_bits(got, C.restated(case)[0][0]) and C.same_bits(got, C.restated(case)[1][0])
    seq = [Seg(k, m, s) for k, (m, s) in enumerate(zip(case["means"], case["stds"]))]
    rows = NaiveTRF(seq, case["penalty"], case["min_score"])
    assert all(e == '-' or e is seq[e.k] for row in rows for e in row)             # the caller's own objects
    assert [[-1 if e == '-' else e.k for e in row] for row in rows] == C.golden_rows(case["name"])


def shuffled_batch(cases=DEFAULT):
    order = np.random.default_rng(7).permutation(len(cases))
    seqs, names = [], []
    for k in order:
        seqs += [pair(cases[k]), (np.zeros(0), np.zeros(0))]                        # an empty sequence between the cases
        names += [cases[k]["name"], None]
    return seqs, names


def check_batch(got, names):
    per = per_sequence()
    assert len(got) == len(names)
    for y, name in zip(got, names):
        assert y == [] if name is None else C.same_bits(y, per[name]), name


@pytest.mark.parametrize("key", sorted(GROUPS), ids=["pen%g_min%g" % k for k in sorted(GROUPS)])
def test_one_batch_equals_the_single_calls(key):
    seqs, names = shuffled_batch(GROUPS[key])
    assert sum(len(g) for g in GROUPS.values()) == len(CASES) and len(DEFAULT) > 20
    check_batch(naive_splits_batch(seqs, *key), names)
    rows = naive_trf_batch([[Seg(k, m, s) for k, (m, s) in enumerate(zip(*sq))] for sq in seqs], *key)
    for r, name in zip(rows, names):
        assert [[-1 if e == '-' else e.k for e in row] for row in r] == ([[]] if name is None else C.golden_rows(name))


def test_small_slots_report_the_true_counts():
    seqs, names = shuffled_batch()
    per = per_sequence()
    true = np.array([0 if n is None else len(per[n]) for n in names])
    slots = np.minimum(true, np.arange(len(names)) % 4)                            # 0 .. 3 entries: too small for most
    rc, score, length, i, j, slot_off, count, status = naive_splits_batch_raw(seqs, slots=slots, retry=False)
    assert rc == _lib.PS_ERR_CAPACITY
    assert np.array_equal(count, true) and not status.any()
    for q, name in enumerate(names):                                               # what fitted is the prefix
        a, k = int(slot_off[q]), int(slots[q])
        got = [(float(score[a + t]), int(length[a + t]), int(i[a + t]), int(j[a + t])) for t in range(k)]
        assert name is None or C.same_bits(got, per[name][:k])
    rc, score, length, i, j, slot_off, count, status = naive_splits_batch_raw(seqs, slots=slots, retry=True)
    assert rc == _lib.PS_OK and np.array_equal(np.diff(slot_off), true) and np.array_equal(count, true)
    check_batch([[(float(score[t]), int(length[t]), int(i[t]), int(j[t])) for t in range(int(slot_off[q]), int(slot_off[q + 1]))]
                 for q in range(len(names))], names)
    rc = naive_splits_batch_raw(seqs, slots=true, retry=False)[0]                  # slots of exactly the counts are enough
    assert rc == _lib.PS_OK


@pytest.mark.parametrize("cap", [1, 3])
def test_max_repeats_gives_the_prefix(cap):
    seqs, names = shuffled_batch()
    per = per_sequence()
    rc, score, length, i, j, slot_off, count, status = naive_splits_batch_raw(seqs, max_repeats=cap)
    got = naive_splits_batch(seqs, max_repeats=cap)
    for q, name in enumerate(names):
        full = [] if name is None else per[name]
        assert C.same_bits(got[q], full[:cap])
        assert count[q] == min(cap, len(full))
        # a sequence stopped by the cap says so (it does not look whether more would follow)
        assert status[q] == (_lib.PS_TRF_MAX_REPEATS if len(full) >= cap and len(seqs[q][0]) >= 2 else _lib.PS_TRF_DONE)


def with_option(name, value, default, f):
    ctx = engine.context(None)
    ctx.set_option(name, value)
    try:
        return f()
    finally:
        ctx.set_option(name, default)


def test_trf_budget_splits_the_batch(capfd):
    seqs, names = shuffled_batch()
    ctx = engine.context(None)
    # 40 000 bytes: one workgroup's scratch is 4 * (130 + 2 * 129) * 8 = 12 416 bytes at 129 segments and 3 * (66 + 2 * 65) * 8 =
    # 4 704 at 65, so a launch holds 3 or 8 workgroups of those sizes and the mixed batch is cut where a longer sequence
    # would push it over; 1 byte: one workgroup per launch, cut at every sequence longer than those before it
    for budget in (40000, 1):
        ctx.set_option("debug", 1)
        try:
            got = with_option("trf_budget", budget, 2 << 30, lambda: naive_splits_batch(seqs))
        finally:
            ctx.set_option("debug", 0)
        launches = [ln for ln in capfd.readouterr().err.splitlines() if "trf launch" in ln]
        assert len(launches) > 1
        check_batch(got, names)


def test_slots_pct_25():
    seqs, names = shuffled_batch()
    check_batch(with_option("slots_pct", 25, 100, lambda: naive_splits_batch(seqs * 3)), names * 3)


def test_one_above_the_cap_raises():
    ctx = engine.context(None)
    n = _lib.TRF_N_MAX + 1
    with pytest.raises(ValueError, match="2048"):                                  # the Python layer, before any call
        naive_splits_batch([(np.zeros(n), np.ones(n))])
    z = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="takes up to 2048"):                      # the library
        ctx.trf_split_batch(z, z + 1.0, np.array([0, n]), -1.0, 2.0)
    for pen, ms in ((0.0, 2.0), (-1.0, -0.5)):
        with pytest.raises(ValueError):
            ctx.trf_split_batch(z[:4], z[:4] + 1.0, np.array([0, 4]), pen, ms)


def test_event_parsed_on_the_device():
    from pypore_amd.DataTypes import Event, File
    from pypore_amd.parsers import SpeedyStatSplit
    second = 100000.
    x = synth.counts_to_pa(synth.step_counts(26000, 2000, 11), np.float64)         # 13 dwells over a cycle of 5 levels: re-reads
    f = File(current=x, timestep=1000. / second)
    ev = Event(current=x, start=0., end=len(x) / second, duration=len(x) / second, second=second, file=f)
    ev.parse(SpeedyStatSplit(prior_segments_per_second=10.))
    segs = ev.segments
    assert len(segs) == 13
    rows = NaiveTRF(segs)
    want, _ = O.splits_upper([s.mean for s in segs], [s.std for s in segs])
    assert len(want) >= 2
    place = {id(s): k for k, s in enumerate(segs)}
    assert [[-1 if isinstance(e, str) else place[id(e)] for e in row] for row in rows] == O.stitch(len(segs), want)
    assert [place[id(e)] for row in rows for e in row if not isinstance(e, str)] == list(range(13))
    assert len({len(r) for r in rows}) == 1


def test_second_call_reuses_the_scratch():
    seqs, names = shuffled_batch()
    naive_splits_batch(seqs)
    before = engine.live_bytes()
    check_batch(naive_splits_batch(seqs), names)
    naive_splits_batch(seqs[:7])
    assert engine.live_bytes() == before
