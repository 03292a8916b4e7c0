"""GPU tests of the pairwise aligner where its promise -- the device equals tests/pairwise_oracle.py bit for bit, pointers
and arg-maxima included -- rests on a tie rule or a guard: integer alphabets whose candidates tie in a quarter of the
cells, maxima held by many rows, stripes and lanes at once, gap markers at the stripe seams and in the trim, the LDS
sizes up to the cap, and slots too small for what a pair writes.  tests/test_pairwise_ties_host.py certifies on the
restatement that the inputs (tests/pairwise_ties.py) do put the rules to a decision.  Every comparison is exact."""
import numpy as np
import pytest

import pairwise_geometry as PG
import pairwise_oracle as O
import pairwise_ties as T
import test_pairwise_host as H
import test_pairwise_ties_host as HT
from test_pairwise_gpu import MODE_NAMES, assert_equals_restatement, run, same, unpack, values

pytestmark = pytest.mark.gpu

MODES = [O.GLOBAL, O.LOCAL, O.REPEATED]
MODE_IDS = ["global", "local", "repeated"]
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 130)


def tie_pairs(seed, drawn):
    """`drawn` pairs of both alphabets with lengths from LENGTHS x LENGTHS, each in both orientations, and a self pair."""
    rng = np.random.default_rng(seed)
    pairs = []
    for d in range(drawn):
        k = 2 if d % 2 else 4
        x, y = T.letters(rng, rng.choice(LENGTHS), k), T.letters(rng, rng.choice(LENGTHS), k)
        pairs += [(x, y), (y, x)]
    x = T.letters(rng, rng.choice((65, 129, 130)), 2 + 2 * (seed % 2))
    return pairs + [(x, x.copy())]


@pytest.mark.parametrize("case", HT.MANIFEST, ids=[c["name"] for c in HT.MANIFEST])
def test_gpu_pairwise_tie_goldens(case):
    x, y, als_ref = H.golden_case(HT.golden(), case)
    mode = H.MODES[case["mode"]]
    raw = run([(x, y)], mode, case["penalty"], case["min_length"])
    status, _, als = unpack(raw, 0)
    H.check_against_golden(case, x, y, status, als, als_ref)
    assert same((status, raw[0][0], als), O.align(x, y, mode, float(case["penalty"]), case["min_length"]))


@pytest.mark.parametrize("penalty", T.PENALTIES)
@pytest.mark.parametrize("mode", [O.GLOBAL, O.LOCAL], ids=["global", "local"])
def test_gpu_pairwise_ties_equal_restatement(mode, penalty):
    pairs = tie_pairs(200 + 10 * mode + T.PENALTIES.index(penalty), 10)
    assert_equals_restatement(pairs, mode, penalty, 2, run(pairs, mode, penalty, 2))


@pytest.mark.parametrize("min_length", [1, 2, 5])
@pytest.mark.parametrize("penalty", T.PENALTIES)
def test_gpu_pairwise_ties_equal_restatement_repeated(penalty, min_length):
    """(A square pair of the repeated mode takes the restatement about a second: one square pair of each alphabet, the
    self pair and four drawn pairs per case.)"""
    seed = 300 + 10 * T.PENALTIES.index(penalty) + min_length
    rng = np.random.default_rng(seed)
    pairs = tie_pairs(seed, 4)
    pairs += [(T.letters(rng, n, k), T.letters(rng, n, k)) for n, k in ((130, 4), (65, 2))]
    raw = run(pairs, O.REPEATED, penalty, min_length)
    assert_equals_restatement(pairs, O.REPEATED, penalty, min_length, raw)
    assert raw[9].max() > 1


def tied_maxima_pairs():
    rng = np.random.default_rng(71)
    tied = [T.periodic(200), T.periodic(448), T.periodic_transposed(200), T.periodic_transposed(448),
            T.periodic_square(130), T.periodic_square(200)]
    pairs = [(values(rng, 448, True), values(rng, 90, True))]  # the launch's largest matrix first: one launch
    for p in tied:          # random-valued pairs between them: a workgroup that has just run one takes the other
        n = int(rng.integers(30, 140))
        pairs += [p, (values(rng, n, True), values(rng, n, False))]
    return pairs + tied[:2]


@pytest.mark.parametrize("mode", [O.LOCAL, O.REPEATED], ids=["local", "repeated"])
def test_gpu_pairwise_tied_maxima_across_stripes_and_lanes(mode, capfd):
    from pypore_amd import engine
    pairs = tied_maxima_pairs()
    want = [O.align(x, y, mode, -1.0, 2) for x, y in pairs]
    raw = run(pairs, mode)
    ctx = engine.context()
    biggest = len(pairs[0][0]) * len(pairs[0][1])
    assert biggest == max(len(x) * len(y) for x, y in pairs)
    capfd.readouterr()
    with PG.options(ctx, slots_pct=1, pairwise_budget=PG.scratch_bytes(biggest, 448), debug=1):
        one = run(pairs, mode)                                  # the whole batch on one workgroup
    passes = PG.passes(PG.printed_launches(capfd.readouterr().err))
    assert passes and all(len(p) == 1 and p[0][2] == 1 and p[0][:2] == (0, len(pairs)) for p in passes)
    for q in range(len(pairs)):
        assert same(unpack(raw, q), want[q]) and same(unpack(one, q), want[q]), q
    for q in (1, 3, 5, 7):                                      # the periodic pairs and their transposes: from (7, 7)
        status, score, als = unpack(raw, q)
        assert score == 21.0 and als[0][0] == 21.0 and (als[0][1][0], als[0][2][0]) == (6, 6)
        if mode == O.REPEATED:
            assert status == O.INDEX_ERROR and len(als) == 1   # the next maximum's mirrored cell is out of bounds


def test_gpu_pairwise_tied_maxima_positions():
    import torch
    from pypore_amd import engine
    from pypore_amd.alignment import _pack
    rng = np.random.default_rng(72)
    a = [T.periodic(200)[0], T.periodic(448)[0], T.U.copy(), T.periodic_square(130)[0], values(rng, 70, True), T.letters(rng, 130, 2)]
    b = [T.U.copy(), T.periodic(200)[0], T.periodic_square(130)[1], values(rng, 90, True), T.letters(rng, 130, 2)]
    ctx = engine.context()
    (fa, oa), (fb, ob) = _pack(a), _pack(b)
    S, pos = ctx.pairwise_scores(torch.from_numpy(fa).cuda(ctx.device), oa, torch.from_numpy(fb).cuda(ctx.device), ob,
                                 O.LOCAL, -1.0, want_pos=True)
    S, pos = S.cpu().numpy(), pos.cpu().numpy()
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            s, ij = O.score_only(x, y, O.LOCAL, -1.0)
            assert S[i, j] == s and tuple(pos[i, j]) == ij, (i, j)
    assert tuple(pos[0, 0]) == tuple(pos[1, 0]) == tuple(pos[2, 1]) == (7, 7)


@pytest.mark.parametrize("shape", [(130, 130), (130, 70)], ids=["130x130", "130x70"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_pairwise_markers_at_the_seams(mode, shape):
    pairs = T.marker_pairs(np.random.default_rng(3), *shape)
    for penalty in (-1, 1):
        raw = run(pairs, mode, penalty, 2)
        assert_equals_restatement(pairs, mode, penalty, 2, raw)
        if mode == O.REPEATED and penalty == -1 and shape == (130, 130):
            assert not raw[1].any()             # (every pair trims some start: test_marker_cases_trim_as_they_are_meant_to)


def test_gpu_pairwise_marker_trim_cases():
    for name, x, y, mode, penalty, min_length in T.trim_cases():
        raw = run([(x, y)], mode, penalty, min_length)
        assert same(unpack(raw, 0), O.align(x, y, mode, float(penalty), min_length)), name
    cases = T.trim_cases()
    for mode in (O.LOCAL, O.REPEATED):          # and as one batch per mode
        pairs = [(x, y) for _, x, y, _, _, _ in cases]
        assert_equals_restatement(pairs, mode, 1, 1, run(pairs, mode, 1, 1))


# ---- the caps --------------------------------------------------------------------------------------------------------------

def scores_with_positions(ctx, a, b, mode, penalty):
    import torch
    from pypore_amd.alignment import _pack
    (fa, oa), (fb, ob) = _pack(a), _pack(b)
    S, pos = ctx.pairwise_scores(torch.from_numpy(fa).cuda(ctx.device), oa, torch.from_numpy(fb).cuda(ctx.device), ob,
                                 mode, penalty, want_pos=True)
    return S.cpu().numpy(), pos.cpu().numpy()


@pytest.mark.parametrize("n", [4095, 4096, 8190])
def test_gpu_pairwise_long_y_up_to_the_cap(n, capfd):
    """4095: exactly 64 KiB of dynamic LDS; 4096: the first size that needs the opt-in; 8190: the cap."""
    from pypore_amd import engine
    assert PG.lds_bytes(4095) == 65536 and PG.lds_bytes(8190) == 131056
    rng = np.random.default_rng(80 + n % 7)
    y = T.letters(rng, n, 4)
    xs = [y[n - 1:].copy(), T.letters(rng, 65, 4)]
    ctx = engine.context()
    for mode in (O.GLOBAL, O.LOCAL):
        S, pos = scores_with_positions(ctx, xs, [y], mode, -1.0)
        for k, x in enumerate(xs):
            s, ij = O.score_only(x, y, mode, -1.0)
            assert S[k, 0] == s and tuple(pos[k, 0]) == ij, (mode, k)
    pairs = [(x, y) for x in xs]
    for mode in MODES:
        capfd.readouterr()
        with PG.options(ctx, debug=1):
            raw = run(pairs, mode)
        launches = PG.printed_launches(capfd.readouterr().err)
        assert launches and all(l[4] == PG.lds_bytes(n) for l in launches)
        assert_equals_restatement(pairs, mode, -1, 2, raw)


def test_gpu_pairwise_long_x_takes_313_stripes():
    from pypore_amd import engine
    rng = np.random.default_rng(81)
    x, y = T.letters(rng, 20000, 4), T.letters(rng, 3, 4)
    assert -(-x.size // T.STRIPE) == 313
    pairs = [(x, y), (x, x[19997:].copy())]
    for mode in MODES:
        assert_equals_restatement(pairs, mode, -1, 2, run(pairs, mode))
    ctx = engine.context()
    for mode in (O.GLOBAL, O.LOCAL):
        S, pos = scores_with_positions(ctx, [x], [p[1] for p in pairs], mode, -1.0)
        for k, (_, b) in enumerate(pairs):
            s, ij = O.score_only(x, b, mode, -1.0)
            assert S[0, k] == s and tuple(pos[0, k]) == ij, (mode, k)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_pairwise_cap_pair_shares_a_launch_with_short_pairs(mode, capfd):
    from pypore_amd import engine
    rng = np.random.default_rng(82)
    short = [(T.letters(rng, rng.integers(1, 6), 2), T.letters(rng, rng.integers(1, 6), 2)) for _ in range(40)]
    pairs = short[:20] + [(T.letters(rng, 5, 4), T.letters(rng, 8190, 4))] + short[20:]
    ctx = engine.context()
    capfd.readouterr()
    with PG.options(ctx, debug=1):
        raw = run(pairs, mode)
    passes = PG.passes(PG.printed_launches(capfd.readouterr().err))
    assert passes and all(len(p) == 1 and p[0][:2] == (0, len(pairs)) and p[0][4] == PG.lds_bytes(8190) for p in passes)
    assert_equals_restatement(pairs, mode, -1, 2, raw)


def test_gpu_pairwise_y_beyond_the_cap_is_refused(capfd):
    from pypore_amd import engine
    from pypore_amd.alignment import pairwise_scores
    rng = np.random.default_rng(83)
    y = T.letters(rng, 8191, 4)
    ok = (T.letters(rng, 5, 4), T.letters(rng, 5, 4))
    ctx = engine.context()
    capfd.readouterr()
    with PG.options(ctx, debug=1):
        for mode in MODES:
            with pytest.raises(ValueError, match="8190"):
                run([ok, (y[:3].copy(), y)], mode)
        for mode in ("global", "local"):
            with pytest.raises(ValueError, match="8190"):
                pairwise_scores([ok[0]], [ok[1], y], mode=mode)
    err = capfd.readouterr().err
    assert "pairwise launch" not in err and "resident slots" not in err         # nothing was launched
    assert run([(y, y[:3].copy())], O.GLOBAL)[1][0] == O.OK                       # x is not capped


# ---- slots that are too small ----------------------------------------------------------------------------------------------

def slot_pairs():
    rng = np.random.default_rng(90)
    sq = lambda n, k: (T.letters(rng, n, k), T.letters(rng, n, k))
    return [sq(64, 2), (T.letters(rng, 30, 4), T.letters(rng, 65, 4)), sq(5, 2), (np.zeros(0), T.letters(rng, 4, 2)),
            sq(65, 4), sq(130, 4), sq(1, 2), T.periodic_square(66), (T.letters(rng, 70, 2), T.letters(rng, 20, 2)),
            sq(33, 2), T.marker_all_seams(rng, 70, 70), sq(129, 2)]


VICTIMS = (5, 11)           # a pair with neighbours on both sides, and the last one: behind its slot lies the watched margin


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gpu_pairwise_short_slots_spill_nothing(mode):
    import torch
    from pypore_amd import _lib, engine
    from pypore_amd.alignment import _pack
    pairs = slot_pairs()
    n = len(pairs)
    ctx = engine.context()
    full = run(pairs, mode, -1, 2)                              # default slots (run again with the exact ones if short)
    want = [O.align(x, y, mode, -1.0, 2) for x, y in pairs]
    for q in range(n):
        assert same(unpack(full, q), want[q]), q
    aln_need = np.array([len(w[2]) for w in want], dtype=np.int64)
    col_need = np.array([sum(len(a[1]) for a in w[2]) for w in want], dtype=np.int64)
    assert np.array_equal(full[9], aln_need)
    if mode == O.REPEATED:                                      # the tie-heavy squares overflow the default slots
        assert aln_need[5] > 131 and aln_need[11] > 130
    full_cols = []                                              # per pair: (cols_i, cols_j, aln_score, aln_start, aln_len)
    for q in range(n):
        c0, a0 = int(full[4][q]), int(full[8][q])
        full_cols.append((full[2][c0:c0 + col_need[q]], full[3][c0:c0 + col_need[q]], full[5][a0:a0 + aln_need[q]],
                          full[6][a0:a0 + aln_need[q]], full[7][a0:a0 + aln_need[q]]))

    def slots(need, short):
        s = need.copy()
        for v in VICTIMS:
            s[v] = {"0": 0, "1": min(1, need[v]), "need-1": max(need[v] - 1, 0), "need": need[v]}[short]
        return s

    kinds = ("0", "1", "need-1", "need")
    for ck in kinds:
        for ak in kinds:
            cs, als = slots(col_need, ck), slots(aln_need, ak)
            rc, buf, col_off, aln_off = PG.batch_once(ctx, pairs, mode, -1.0, 2, cs, als)
            is_short = bool((cs < col_need).any() or (als < aln_need).any())
            assert rc == (_lib.PS_ERR_CAPACITY if is_short else 0), (ck, ak, rc)
            assert np.array_equal(buf["col_need"], col_need) and np.array_equal(buf["aln_count"], aln_need), (ck, ak)
            assert (buf["cols_i"][col_off[-1]:] == PG.SENTINEL).all() and (buf["cols_j"][col_off[-1]:] == PG.SENTINEL).all(), (ck, ak)
            for name in ("aln_score", "aln_start", "aln_len"):
                assert (buf[name][aln_off[-1]:] == PG.SENTINEL).all(), (ck, ak, name)
            raw = (buf["scores"], buf["status"], buf["cols_i"], buf["cols_j"], col_off, buf["aln_score"], buf["aln_start"],
                   buf["aln_len"], aln_off, buf["aln_count"])
            for q in range(n):
                assert buf["status"][q] == want[q][0] and buf["scores"][q] == want[q][1], (ck, ak, q)
                if cs[q] >= col_need[q] and als[q] >= aln_need[q]:
                    assert same(unpack(raw, q), want[q]), (ck, ak, q)
                # a short pair's own slot: the prefix of what it writes in full, nothing else
                c0, a0 = int(col_off[q]), int(aln_off[q])
                assert np.array_equal(buf["cols_i"][c0:c0 + cs[q]], full_cols[q][0][:cs[q]]), (ck, ak, q)
                assert np.array_equal(buf["cols_j"][c0:c0 + cs[q]], full_cols[q][1][:cs[q]]), (ck, ak, q)
                for k, name in ((2, "aln_score"), (3, "aln_start"), (4, "aln_len")):
                    assert np.array_equal(buf[name][a0:a0 + als[q]], full_cols[q][k][:als[q]]), (ck, ak, q, name)
            if mode == O.GLOBAL and ak == "1":
                break                                           # one alignment per pair: 1, need - 1 = 0 and need repeat
    # the engine's own call with slots too small: after its second run the same results as with the default slots
    a, a_off = _pack([['-' if e != e else e for e in p[0]] for p in pairs])
    b, b_off = _pack([['-' if e != e else e for e in p[1]] for p in pairs])
    dev = torch.device("cuda", ctx.device)
    idx = np.arange(n, dtype=np.int32)
    for ck, ak in (("0", "0"), ("need-1", "need-1"), ("need", "1")):
        again = ctx.pairwise_batch(torch.from_numpy(a).to(dev), a_off, torch.from_numpy(b).to(dev), b_off, idx, idx, mode,
                                   -1.0, 2, col_slots=slots(col_need, ck), aln_slots=slots(aln_need, ak))
        for q in range(n):
            assert same(unpack(again, q), want[q]), (ck, ak, q)
