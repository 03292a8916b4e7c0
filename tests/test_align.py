"""Segment aligner (calignment.pyx:20-100).

CPU part: the oracle restatement against golden vectors recorded from the compiled, unmodified reference
(tests/golden/make_golden_align.py).  GPU part: ps_align_batch through the C ABI against the oracle --
scores and paths bit-exact (the kernel keeps the reference's operation order), error classes the same."""
import json
import os
import sys

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "golden_align.npz"))
CASES = json.load(open(os.path.join(HERE, "golden", "manifest_align.json")))["cases"]
sys.path.insert(0, HERE)
import launch_geometry as LG  # noqa: E402

KEYS = ("model_means", "model_stds", "model_durs", "skip_penalty", "backslip_penalty", "seq_means", "seq_stds", "seq_durs")
EXC = {"IndexError": IndexError, "ValueError": ValueError, "ZeroDivisionError": ZeroDivisionError}


def case_inputs(name):
    v = [GOLD[name + "/" + k] for k in KEYS]
    return v[0], v[1], v[2], float(v[3]), float(v[4]), v[5], v[6], v[7]


def random_case(seed, m=None, s=None):
    rng = np.random.RandomState(seed)
    m = int(rng.randint(2, 90)) if m is None else m
    s = int(rng.randint(1, 120)) if s is None else s
    mm = np.cumsum(rng.uniform(-8, 10, m)) + 40
    ms = rng.uniform(0.5, 3, m)
    md = rng.uniform(0.0005, float(rng.choice([0.002, 0.01, 0.05])), m)
    j = int(rng.randint(0, m))
    idx = []
    for _ in range(s):
        idx.append(j)
        r = rng.rand()
        j = (j if r < 0.2 else min(m - 1, j + 1) if r < 0.7 else
             min(m - 1, j + int(rng.randint(2, 5))) if r < 0.85 else max(0, j - int(rng.randint(1, 4))))
    sm = mm[np.array(idx, dtype=int)] + rng.normal(0, float(rng.choice([0.02, 0.2, 1.0])), s)
    ss = rng.uniform(0.5, 3, s)
    sd = rng.uniform(0.0005, 0.02, s)
    sp, bp = float(rng.choice([0.1, 0.5, 2., 10., 100.])), float(rng.choice([0.1, 0.5, 2., 10., 100.]))
    return mm, ms, md, sp, bp, sm, ss, sd


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_matches_reference_golden(case):
    args = case_inputs(case["name"])
    if case["raises"]:
        with pytest.raises(EXC[case["raises"]]):
            oracle.align(*args)
        return
    score, path = oracle.align(*args)
    assert score == float(GOLD[case["name"] + "/score"])              # bit-exact
    assert path.dtype == np.float64 and np.array_equal(path, GOLD[case["name"] + "/path"])


def test_golden_paths_exercise_every_move():
    moves = set()
    for c in CASES:
        if c["raises"]:
            continue
        d = np.diff(GOLD[c["name"] + "/path"])
        moves |= {"stay" if x == 0 else "step" if x == 1 else "skip" if x > 1 else "back" for x in d}
    assert moves == {"stay", "step", "skip", "back"}


# ---- GPU: ps_align_batch through the C ABI -------------------------------------------------------------------

def _gpu_aligner(args):
    from pypore_amd.calignment import cSegmentAligner
    return cSegmentAligner(*args[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gpu_matches_reference_golden(case):
    args = case_inputs(case["name"])
    al = _gpu_aligner(args)
    if case["raises"]:
        with pytest.raises(EXC[case["raises"]]):
            al.align(*args[5:])
        return
    score, path = al.align(*args[5:])
    assert score == float(GOLD[case["name"] + "/score"])              # bit-exact
    assert path.dtype == np.float64 and np.array_equal(path, GOLD[case["name"] + "/path"])


@pytest.mark.gpu
def test_gpu_batch_matches_oracle_bit_exact():
    """One model, 300 random sequences (lengths 1..120, every move, several noise levels) in one launch:
    raw score, path and status of every sequence equal the oracle's."""
    mm, ms, md, sp, bp, _, _, _ = random_case(99, m=70, s=1)
    seqs = []
    for q in range(300):
        c = random_case(1000 + q, m=70)
        rng = np.random.RandomState(q)
        idx = np.clip(np.cumsum(rng.choice([0, 1, 1, 1, 2, 3, -1, -2], size=len(c[5]))) + int(rng.randint(0, 20)), 0, 69)
        seqs.append((mm[idx] + rng.normal(0, 0.2, len(idx)), c[6], c[7]))
    seqs.append((np.zeros(0), np.zeros(0), np.zeros(0)))              # ValueError in the reference
    z = random_case(5, m=70, s=9)
    z[6][4] = 0.0
    seqs.append((z[5], z[6], z[7]))                                   # ZeroDivisionError
    from pypore_amd.calignment import cSegmentAligner
    al = cSegmentAligner(mm, ms, md, sp, bp)
    scores, paths, status = al.align_batch_raw(seqs)
    seen = set()
    for q, sq in enumerate(seqs):
        rc, score, path = oracle.align_raw(mm, ms, md, sp, bp, *sq)
        seen.add(rc)
        assert status[q] == rc, (q, status[q], rc)
        if rc == 0:
            assert scores[q] == score and np.array_equal(paths[q], path), q
    assert {0, 1, 3} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(12))
def test_gpu_random_models_match_oracle(seed):
    """Model sizes 2..1024 (one LDS-resident row set), penalties 0.1..100, single align() calls and the exception class."""
    rng = np.random.RandomState(700 + seed)
    m = int(rng.choice([2, 3, 63, 64, 65, 129, 300, 1024]))
    args = random_case(800 + seed, m=m, s=int(rng.randint(1, 200)))
    al = _gpu_aligner(args)
    try:
        want = oracle.align(*args)
    except Exception as e:                                            # noqa: BLE001
        with pytest.raises(type(e)):
            al.align(*args[5:])
        return
    got = al.align(*args[5:])
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_gpu_wrapper_and_limits():
    from pypore_amd.alignment import SegmentAligner
    args = case_inputs("A2_walk_30x25")
    sa = SegmentAligner(*args[:5])
    score, order = sa.align(*args[5:])
    assert score == float(GOLD["A2_walk_30x25/score"]) and np.array_equal(order, GOLD["A2_walk_30x25/path"])
    assert sa.align(np.zeros(0), np.zeros(0), np.zeros(0)) == (None, None)         # alignment.py:43-46
    big = SegmentAligner(np.arange(1025.), np.ones(1025), np.ones(1025), 1., 1.)
    with pytest.raises(ValueError):                                    # PS_ERR_ARG: model longer than the LDS row set
        big.aligner.align(np.ones(3), np.ones(3), np.ones(3))


# ---- GPU: launch geometries of ps_align_batch ----------------------------------------------------------------------
# The host picks the grid (resident slots, capped by 2 GiB of scratch) and the traceback block B from the batch; each case
# below states the geometry it is built for, checks it against the host's formulas and the slot count the library prints
# under option `debug`, and compares every sequence -- status, raw score and path -- with the oracle bit for bit.


def _model(seed, m):
    """Levels a random walk apart, short durations and mild penalties: a sequence near the model keeps final scores above
    -1 however long it is (random_case's long models mostly end at status 4)."""
    rng = np.random.RandomState(seed)
    mm = np.cumsum(rng.uniform(-8, 10, m)) + 40
    return (mm, rng.uniform(0.5, 3, m), rng.uniform(0.0005, 0.002, m), float(rng.choice([0.1, 0.5, 2.])),
            float(rng.choice([0.1, 0.5, 2.])))


def _walk(rng, mm, s, j0=None):
    """A random walk over the model's levels (every move), s segments."""
    m = mm.size
    j0 = int(rng.randint(min(5, m - 1), max(6, m // 3))) if j0 is None else j0
    idx = np.clip(np.cumsum(rng.choice([0, 1, 1, 1, 2, 3, -1, -2], size=s)) + j0, 0, m - 1)
    return mm[idx] + rng.normal(0, 0.2, s), rng.uniform(0.5, 3, s), rng.uniform(0.0005, 0.002, s)


def _first_level_then_up(rng, mm, stay, up):
    """`stay` segments on level 0, then a walk up over `up` levels: the traceback reaches index 0 at a row >= 1 (IndexError)."""
    idx = np.concatenate([np.zeros(stay, int), np.minimum(np.arange(1, up + 1), mm.size - 1)])
    s = idx.size
    return mm[idx] + rng.normal(0, 0.01, s), rng.uniform(0.5, 1.5, s), rng.uniform(0.005, 0.02, s)


def _far(rng, mm, s):
    """Far from every level: no final score above -1 (undefined in the reference, status 4)."""
    return np.full(s, mm.max() + 1000.0) + rng.normal(0, 1, s), rng.uniform(0.5, 3, s), rng.uniform(0.005, 0.02, s)


def _zero_std(rng, mm, s):
    sm, ss, sd = _walk(rng, mm, s)
    ss[int(rng.randint(0, s))] = 0.0
    return sm, ss, sd


def _empty():
    return np.zeros(0), np.zeros(0), np.zeros(0)


def _align_debug(model, seqs, capfd, **opts):
    """One ps_align_batch under option debug (and `opts`): (scores, paths, status, grid, B).  The grid is what the host
    launches: min(n_seq, the printed slot count, the scratch cap)."""
    from pypore_amd import engine
    from pypore_amd.calignment import cSegmentAligner
    al = cSegmentAligner(*model)
    m, n = model[0].size, len(seqs)
    B, lds, cap = LG.align_geometry(m, n, max(len(s[0]) for s in seqs))
    capfd.readouterr()
    with LG.options(engine.context(), debug=1, **opts):
        scores, paths, status = al.align_batch_raw(seqs)
    slots = LG.printed_slots(capfd.readouterr().err, lds)
    assert len(slots) == 1, slots
    if "slots_pct" in opts:
        assert slots[0][1] == opts["slots_pct"]
    return scores, paths, status, min(n, slots[0][0], cap), B


def _check_against_oracle(model, seqs, scores, paths, status):
    """Every sequence: status, raw score and path (written rows included, for an IndexError too) equal the oracle's."""
    rcs = np.zeros(len(seqs), int)
    for q, sq in enumerate(seqs):
        rc, score, path = oracle.align_raw(*model, *sq)
        rcs[q] = rc
        assert status[q] == rc, (q, status[q], rc)
        assert scores[q] == score, (q, scores[q], score)
        assert np.array_equal(paths[q], path), q
    return rcs


def _index_error_row(path, m):
    """The row at which an IndexError traceback stopped: the last entry that is not a valid interior index."""
    bad = [i for i in range(path.size) if not 0 < int(path[i]) < m]
    return bad[-1]


@pytest.mark.gpu
def test_gpu_align_slots_pct_takes_effect(capfd, record_property):
    """ps_set_option("slots_pct") applies at the next launch of a kernel and shape the context has already launched, and
    the full grid comes back when the option does (the occupancy cache holds workgroups per CU, not slots)."""
    from pypore_amd import engine
    from pypore_amd.calignment import cSegmentAligner
    model = _model(3, 70)
    rng = np.random.RandomState(4)
    seqs = [_walk(rng, model[0], int(rng.randint(1, 40))) for _ in range(300)]
    al = cSegmentAligner(*model)
    first = al.align_batch_raw(seqs)                                   # this shape is now in the occupancy cache
    _, lds, _ = LG.align_geometry(70, len(seqs), 39)
    ctx = engine.context()
    pct0 = LG.default("slots_pct")
    got = []
    for pct in (1, pct0):
        capfd.readouterr()
        with LG.options(ctx, slots_pct=pct, debug=1):
            out = al.align_batch_raw(seqs)
        got.append(LG.printed_slots(capfd.readouterr().err, lds))
        assert np.array_equal(out[0], first[0]) and np.array_equal(out[2], first[2])
        assert all(np.array_equal(a, b) for a, b in zip(out[1], first[1]))
    (small, p1), = got[0]
    (full, p0), = got[1]
    record_property("slots", {"slots_pct 1": small, "slots_pct %d" % pct0: full})
    assert p1 == 1 and p0 == pct0
    if pct0 == 100:
        assert small == max(1, full // 100)
    if pct0 > 1:
        assert small < full
    _check_against_oracle(model, seqs, *first)


@pytest.mark.gpu
def test_gpu_align_reuse_many_sequences_per_workgroup(capfd, record_property):
    """Several thousand short sequences against one m = 70 model: more than any resident grid (every workgroup aligns
    several sequences in its reused scratch, LDS rows and __shared__ state), n_seq > 512 (the small traceback block)."""
    model = _model(11, 70)
    rng = np.random.RandomState(12)
    seqs = [_walk(rng, model[0], int(rng.randint(1, 30))) for _ in range(6000)]
    scores, paths, status, grid, B = _align_debug(model, seqs, capfd)
    record_property("geometry", {"n_seq": len(seqs), "grid": grid, "B": B})
    assert B == 7 and grid < len(seqs), (B, grid)
    rcs = _check_against_oracle(model, seqs, scores, paths, status)
    assert (rcs == 0).mean() > 0.9


@pytest.mark.gpu
def test_gpu_align_reuse_after_every_error_class(capfd, record_property):
    """slots_pct 1: a few hundred sequences, dozens per workgroup, good ones interleaved with every error class -- empty (1),
    IndexError in the traceback (2), zero std (3), no final score above -1 (4).  Workgroup g aligns q = g, g + grid, ...,
    so the sequence after an error in the same workgroup is q + grid: it must still equal the oracle."""
    model = _model(21, 70)
    mm = model[0]
    rng = np.random.RandomState(22)
    makers = [lambda: _empty(), lambda: _first_level_then_up(rng, mm, int(rng.randint(3, 12)), int(rng.randint(3, 20))),
              lambda: _zero_std(rng, mm, int(rng.randint(1, 30))), lambda: _far(rng, mm, int(rng.randint(1, 30)))]
    seqs, n_err = [], 0
    for q in range(400):                                              # about one in five an error, the classes in turn
        if rng.rand() < 0.2:
            seqs.append(makers[n_err % 4]())
            n_err += 1
        else:
            seqs.append(_walk(rng, mm, int(rng.randint(1, 60)), j0=int(rng.randint(5, 30))))
    scores, paths, status, grid, B = _align_debug(model, seqs, capfd, slots_pct=1)
    record_property("geometry", {"n_seq": len(seqs), "grid": grid, "B": B})
    assert len(seqs) >= 12 * grid, grid                             # dozens of sequences per workgroup
    rcs = _check_against_oracle(model, seqs, scores, paths, status)
    assert set(rcs.tolist()) == {0, 1, 2, 3, 4}
    for rc in (1, 2, 3, 4):                                           # a good sequence follows this class in its workgroup
        assert any(rcs[q] == rc and rcs[q + grid] == 0 for q in range(len(seqs) - grid)), rc


def _block_case(m, n_seq, B_want, seed, capfd, record_property):
    model = _model(seed, m)
    mm = model[0]
    rng = np.random.RandomState(seed + 1)
    B = LG.align_geometry(m, n_seq, 300)[0]
    assert B == B_want
    lengths = [B, B + 1, 63, 64, 65, 127, 128, 129, 2 * B + 1, 300]
    seqs = [_walk(rng, mm, s, j0=int(rng.randint(5, 10))) for s in lengths]
    # IndexError whose traceback reaches index 0 many blocks above row 0 (and several blocks below the last row)
    err = [_first_level_then_up(rng, mm, 80, up) for up in (70, 100)]
    seqs += err
    seqs += [_walk(rng, mm, int(rng.randint(1, 20))) for _ in range(n_seq - len(seqs))]
    scores, paths, status, grid, B_run = _align_debug(model, seqs, capfd)
    record_property("geometry", {"m": m, "n_seq": n_seq, "grid": grid, "B": B_run})
    assert B_run == B_want
    rcs = _check_against_oracle(model, seqs, scores, paths, status)
    assert (rcs[:len(lengths)] == 0).all()
    for q in range(len(lengths), len(lengths) + len(err)):
        assert rcs[q] == 2
        s, r = len(seqs[q][0]), _index_error_row(paths[q], m)
        assert r // B >= 2 and (s - 1 - r) // B >= 2, (r, s, B)


@pytest.mark.gpu
def test_gpu_align_traceback_block_1(capfd, record_property):
    """m = 600 with n_seq > 512: 24 m bytes per row exceed the 12 KiB block budget, B = 1."""
    _block_case(600, 520, 1, 31, capfd, record_property)


@pytest.mark.gpu
def test_gpu_align_traceback_block_2(capfd, record_property):
    """m = 1024 with n_seq <= 512: B = 48 KiB / (24 m) = 2."""
    _block_case(1024, 40, 2, 41, capfd, record_property)


@pytest.mark.gpu
def test_gpu_align_traceback_block_32(capfd, record_property):
    """Small m with n_seq <= 512: B = 32 (ALIGN_B_MAX)."""
    _block_case(40, 60, 32, 51, capfd, record_property)


@pytest.mark.gpu
def test_gpu_align_scratch_cap(capfd, record_property):
    """m = 1024, one sequence of 1100 segments and 200 short ones: 24 * 1100 * 1024 bytes of scratch per workgroup cap the
    grid at 2 GiB / that = 79 workgroups, so the short sequences reuse scratch slots sized for the long one."""
    model = _model(61, 1024)
    rng = np.random.RandomState(62)
    seqs = [_walk(rng, model[0], int(rng.randint(1, 40))) for _ in range(200)]
    seqs.insert(37, _walk(rng, model[0], 1100, j0=10))
    scores, paths, status, grid, B = _align_debug(model, seqs, capfd)
    record_property("geometry", {"n_seq": len(seqs), "grid": grid, "B": B})
    assert B == 2 and grid == (2 << 30) // (24 * 1100 * 1024) == 79
    rcs = _check_against_oracle(model, seqs, scores, paths, status)
    assert rcs[37] == 0 and (rcs == 0).sum() >= 180
