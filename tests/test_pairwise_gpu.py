"""GPU tests of the pairwise aligner (ps_pairwise_batch / ps_pairwise_scores, csrc/seg_pairwise.hpp): the device against
the recorded reference by the three rules of test_pairwise_host.py, against the restatement (tests/pairwise_oracle.py) bit
for bit, and the launch shapes -- batches, launches split by the scratch budget, scratch reuse, slots_pct."""
import numpy as np
import pytest

import pairwise_geometry as PG
import pairwise_oracle as O
import test_pairwise_host as H

pytestmark = pytest.mark.gpu

MODE_NAMES = {O.GLOBAL: "global", O.LOCAL: "local", O.REPEATED: "local_repeated"}
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1000)


def values(rng, n, grid, lo=20.0, hi=26.0):
    v = rng.uniform(lo, hi, n)
    return np.round(v * 32.0) / 32.0 if grid else v


def unpack(raw, q):
    """(status, score, [(score, ci, cj)]) of pair q from the arrays of pairwise_align_batch_raw."""
    scores, status, ci, cj, col_off, a_score, a_start, a_len, a_off, a_count = raw
    als = []
    for k in range(int(a_count[q])):
        b = int(col_off[q]) + int(a_start[a_off[q] + k])
        e = b + int(a_len[a_off[q] + k])
        als.append((a_score[a_off[q] + k], list(ci[b:e]), list(cj[b:e])))
    return int(status[q]), scores[q], als


def same(a, b):
    """Bit for bit: status, score, number and order of alignments, their scores and index columns."""
    return a[0] == b[0] and a[1] == b[1] and len(a[2]) == len(b[2]) and all(
        p[0] == q[0] and list(p[1]) == list(q[1]) and list(p[2]) == list(q[2]) for p, q in zip(a[2], b[2]))


def run(pairs, mode, penalty=-1, min_length=2):
    from pypore_amd.alignment import pairwise_align_batch_raw

    def objects(v):         # the public surface takes '-' for the marker, the restatement NaN
        return ['-' if e != e else e for e in v] if np.isnan(v).any() else v
    return pairwise_align_batch_raw([(objects(x), objects(y)) for x, y in pairs], MODE_NAMES[mode], penalty, min_length)


def assert_equals_restatement(pairs, mode, penalty, min_length, raw):
    for q, (x, y) in enumerate(pairs):
        want = O.align(x, y, mode, float(penalty), min_length)
        assert same(unpack(raw, q), want), (q, len(x), len(y), mode, penalty)


@pytest.mark.parametrize("case", H.MANIFEST, ids=[c["name"] for c in H.MANIFEST])
def test_gpu_pairwise_goldens(case):
    x, y, als_ref = H.golden_case(H.golden(), case)
    mode = H.MODES[case["mode"]]
    raw = run([(x, y)], mode, case["penalty"], case["min_length"])
    status, _, als = unpack(raw, 0)
    H.check_against_golden(case, x, y, status, als, als_ref)
    assert same((status, raw[0][0], als), O.align(x, y, mode, float(case["penalty"]), case["min_length"]))


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "offgrid"])
@pytest.mark.parametrize("mode", [O.GLOBAL, O.LOCAL, O.REPEATED], ids=["global", "local", "repeated"])
def test_gpu_pairwise_equals_restatement_on_drawn_lengths(mode, grid):
    """Lengths drawn from LENGTHS x LENGTHS, each drawn pair in both orientations, three penalties; every pair's status,
    score, alignments and their order equal the restatement bit for bit.  The repeated mode's 1000 x 1000 pair takes its
    values from a wide range, so that the restatement's one arg-max per alignment stays within seconds."""
    rng = np.random.default_rng(100 + 10 * mode + grid)
    for penalty in (-1, -0.5, 0):
        pairs = []
        for _ in range(14):
            m, n = rng.choice(LENGTHS), rng.choice(LENGTHS)
            if mode == O.REPEATED and m >= 300 and n >= 300:
                m = 129
            x, y = values(rng, m, grid), values(rng, n, grid)
            pairs += [(x, y), (y, x)]
        x = values(rng, 300, grid)
        pairs.append((x, x.copy()))
        if penalty == -1:
            w = values(rng, 1000, grid, 20.0, 400.0) if mode == O.REPEATED else values(rng, 1000, grid)
            pairs.append((w, values(rng, 1000, grid, 20.0, 400.0) if mode == O.REPEATED else values(rng, 1000, grid)))
            pairs.append((w, w.copy()))
        raw = run(pairs, mode, penalty, 2)
        assert_equals_restatement(pairs, mode, penalty, 2, raw)


@pytest.mark.parametrize("mode", [O.GLOBAL, O.LOCAL, O.REPEATED], ids=["global", "local", "repeated"])
def test_gpu_pairwise_mixed_batch_equals_one_by_one(mode):
    """2 048 pairs of mixed lengths in one call against the same pairs each in a call of its own."""
    rng = np.random.default_rng(7 + mode)
    pairs = []
    for q in range(2048):
        m = int(rng.integers(0, 140))
        n = m if rng.random() < 0.6 else int(rng.integers(0, 140))
        pairs.append((values(rng, m, q % 2 == 0), values(rng, n, q % 2 == 0)))
    raw = run(pairs, mode, -1, 2)
    for q, p in enumerate(pairs):
        assert same(unpack(raw, q), unpack(run([p], mode, -1, 2), 0)), q
    assert len(set(raw[1].tolist())) == (1 if mode == O.GLOBAL else 2)      # both statuses occur in the local modes


@pytest.mark.parametrize("mode", [O.GLOBAL, O.REPEATED], ids=["global", "repeated"])
def test_gpu_pairwise_batch_split_by_the_scratch_budget(mode, capfd):
    """Option pairwise_budget lowered so that the batch takes several launches: the same results as in one launch."""
    from pypore_amd import engine
    rng = np.random.default_rng(21 + mode)
    pairs = []
    for q in range(600):
        m = int(rng.integers(20, 120))
        pairs.append((values(rng, m, True), values(rng, m, True)))
    pairs[100] = (values(rng, 700, True), values(rng, 700, True))              # one pair far larger than the rest
    whole = run(pairs, mode)
    ctx = engine.context()
    budget = 2 * PG.scratch_bytes(700 * 700, 700)
    capfd.readouterr()
    with PG.options(ctx, pairwise_budget=budget, debug=1):
        split = run(pairs, mode)
    for launches in PG.passes(PG.printed_launches(capfd.readouterr().err)):
        assert len(launches) > 1 and launches[0][0] == 0 and launches[-1][1] == len(pairs)
        for a, b in zip(launches, launches[1:]):
            assert a[1] == b[0]
        for first, end, grid, per_wg, lds in launches:
            assert grid >= 1 and (grid * per_wg <= budget or grid == 1)
    for q in range(len(pairs)):
        assert same(unpack(split, q), unpack(whole, q)), q


@pytest.mark.parametrize("mode", [O.GLOBAL, O.LOCAL], ids=["global", "local"])
def test_gpu_pairwise_scores_equal_the_per_pair_scores_and_are_symmetric(mode):
    from pypore_amd.alignment import pairwise_scores
    rng = np.random.default_rng(31 + mode)
    seqs = [values(rng, int(n), k % 2 == 0) for k, n in enumerate(list(rng.integers(0, 200, 40)) + [0, 1, 63, 64, 65, 128, 129, 400])]
    for penalty in (-1, -0.5):
        S = pairwise_scores(seqs, mode=MODE_NAMES[mode], penalty=penalty)
        assert S.shape == (len(seqs), len(seqs)) and S.dtype == np.float64
        assert np.array_equal(S, S.T)
        idx = [(a, b) for a in range(len(seqs)) for b in range(len(seqs))]
        raw = run([(seqs[a], seqs[b]) for a, b in idx], mode, penalty)
        assert np.array_equal(raw[0].reshape(S.shape), S)
        for a, b in idx[::7]:
            assert S[a, b] == O.score_only(seqs[a], seqs[b], mode, penalty)[0]
    others = seqs[:5]
    R = pairwise_scores(seqs, others, mode=MODE_NAMES[mode])
    assert np.array_equal(R, pairwise_scores(seqs, mode=MODE_NAMES[mode])[:, :5])


def test_gpu_pairwise_local_positions():
    """ps_pairwise_scores' optional output: the row-major-first cell of the local maximum, (0, 0) when nothing is above 0."""
    import torch
    from pypore_amd import engine
    from pypore_amd.alignment import _pack
    rng = np.random.default_rng(41)
    seqs = [values(rng, n, True) for n in (0, 1, 5, 64, 65, 130, 200)] + [values(rng, 9, True, 60.0, 64.0)]
    ctx = engine.context()
    flat, off = _pack(seqs)
    t = torch.from_numpy(flat).cuda(ctx.device)
    S, pos = ctx.pairwise_scores(t, off, t, off, O.LOCAL, -1.0, want_pos=True)
    S, pos = S.cpu().numpy(), pos.cpu().numpy()
    for a in range(len(seqs)):
        for b in range(len(seqs)):
            s, ij = O.score_only(seqs[a], seqs[b], O.LOCAL, -1.0)
            assert S[a, b] == s and tuple(pos[a, b]) == ij, (a, b)


def test_gpu_pairwise_scratch_reuse_on_one_workgroup(capfd):
    """One workgroup (slots_pct 1 and a budget of one matrix) takes a long pair, short ones, pairs that end in
    PS_PW_INDEX_ERROR and short ones again: every pair gives its own result."""
    from pypore_amd import engine
    rng = np.random.default_rng(51)
    long_x = values(rng, 400, True)
    shorts = [(lambda x: (x, x.copy()))(values(rng, n, True)) for n in (30, 5, 64, 1)]
    raising = (values(rng, 50, True), values(rng, 90, True))
    pairs = [(long_x, long_x.copy())] + shorts[:2] + [raising, shorts[2], raising, shorts[3], (long_x[:200], long_x[:200].copy()), shorts[0]]
    ctx = engine.context()
    for mode in (O.GLOBAL, O.LOCAL, O.REPEATED):
        capfd.readouterr()
        with PG.options(ctx, slots_pct=1, pairwise_budget=PG.scratch_bytes(400 * 400, 400), debug=1):
            raw = run(pairs, mode)
        passes = PG.passes(PG.printed_launches(capfd.readouterr().err))
        assert passes and all(len(p) == 1 and p[0][2] == 1 and p[0][:2] == (0, len(pairs)) for p in passes)
        assert_equals_restatement(pairs, mode, -1, 2, raw)
        if mode != O.GLOBAL:
            assert raw[1][3] == O.INDEX_ERROR and raw[1][4] == O.OK


def test_gpu_pairwise_launch_honours_slots_pct(capfd):
    from pypore_amd import engine
    rng = np.random.default_rng(61)
    pairs = [(lambda x: (x, x.copy()))(values(rng, 48, True)) for _ in range(3000)]
    ctx = engine.context()
    lds = PG.lds_bytes(48)
    seen = {}
    for pct in (1, 50, 100):
        capfd.readouterr()
        with PG.options(ctx, slots_pct=pct, debug=1):
            raw = run(pairs, O.LOCAL)
        err = capfd.readouterr().err
        slots = PG.printed_slots(err, lds)
        launches = PG.printed_launches(err)
        assert slots and all(p == pct for _, p in slots)
        assert len(launches) == 1 and launches[0][2] == min(len(pairs), slots[-1][0]) and launches[0][4] == lds
        seen[pct] = slots[-1][0]
        for q in range(0, len(pairs), 100):
            assert same(unpack(raw, q), O.align(pairs[q][0], pairs[q][1], O.LOCAL, -1.0, 2)), (pct, q)
    assert seen[1] < seen[50] < seen[100] and seen[1] == max(1, seen[100] // 100)


def test_gpu_pairwise_aligner_class_returns_the_callers_objects():
    """The reference's return shapes over the caller's own objects; the repeated generator delivers what was completed and
    then raises."""
    from pypore_amd.alignment import PairwiseAligner, pairwise_align_batch
    G = H.golden()
    case = [c for c in H.MANIFEST if c["name"] == "marker_global"][0]
    x, y, als = H.golden_case(G, case)
    xo = ['-' if np.isnan(v) else float(v) for v in x]
    yo = ['-' if np.isnan(v) else float(v) for v in y]
    s, xa, ya = PairwiseAligner(xo, yo).global_alignment()
    xa, ya = list(xa), list(ya)
    assert s == als[0][0] and len(xa) == len(ya) == als[0][1].size
    assert all(e == '-' if np.isnan(r) else e == r for e, r in zip(xa, als[0][1]))
    assert any(e is o for e in xa for o in xo if not isinstance(o, str))          # the caller's own objects
    case = [c for c in H.MANIFEST if c["name"] == "grid_repeated_yields_then_raises"][0]
    x, y, als = H.golden_case(G, case)
    gen = PairwiseAligner(list(x), list(y)).local_repeated_alignment(penalty=-1, min_length=2)
    got = []
    with pytest.raises(IndexError):
        for s, xa, ya in gen:
            got.append((s, list(xa), list(ya)))
    assert len(got) == len(als) > 0 and all(g[0] == a[0] and g[1] == list(a[1]) and g[2] == list(a[2]) for g, a in zip(got, als))
    with pytest.raises(IndexError):
        PairwiseAligner([20.0] * 3, [60.0] * 3).local_alignment()
    r = pairwise_align_batch([([20.0] * 3, [60.0] * 3), ([20.0, 21.0], [20.0, 21.0])], mode="local")
    assert isinstance(r[0], IndexError) and r[1][0] == 6.0 and list(r[1][1]) == [20.0, 21.0]
    s, xa, ya = PairwiseAligner([], [1.0, 2.0]).global_alignment(penalty=-3)
    assert s == -6.0 and list(xa) == [] and list(ya) == []
    assert list(PairwiseAligner([], [1.0]).local_repeated_alignment()) == []
