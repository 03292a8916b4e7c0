"""The sampling tables' row rule and the references of the edge tests, on the host (no GPU).

The row rule (pypore_amd/hmm.py, Sampling): a cdf row is exactly 1.0 from its last entry of positive probability on.  The
tables closed only their last entry before, and so did tests/sample_oracle.py: after training, a state whose last out-edge
has probability 0 and whose positive edges sum below 1.0 then gave [sum, 1) to the impossible edge.  A draw lands there with
a chance of about 1e-16, so only the table can show it: test_trained_rows_never_pick_an_impossible_edge puts u on 1 - 2^-53.

The emission reference of tests/test_hmm_sample_edges_gpu.py is mpmath at 50 digits (sample_edges.draw_mp); here the
plain-Python oracle is held to it at the project's bar, 1e-12 max(1, |ref|), on the chosen draws, before the device is."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixture_oracle as MX  # noqa: E402
import sample_edges as E  # noqa: E402
import sample_models as SM  # noqa: E402
import sample_oracle as SO  # noqa: E402

TOL = 1e-12
COUNTS = range(1, 12)

_found = []


def trained_rows():
    """Every count vector (a, b, c, 0), a, b, c in 1..11, through one M-step of a hub of four out-edges: [(counts, the
    product's row, the oracle's row, exp(out_lp) of the row)] of those whose three positive entries sum below 1.0.
    Computed once, shared, never changed."""
    if not _found:
        m = E.hub([1.0] * 4, "trained")
        lo, hi = E.hub_row(m)
        for counts in itertools.product(COUNTS, COUNTS, COUNTS):
            E.train_hub(m, counts + (0,))
            p = np.exp(m.flat["out_lp"][lo:hi])
            assert p[3] == 0.0 and np.isneginf(m.flat["out_lp"][hi - 1]) and np.all(p[:3] > 0)
            if (p[0] + p[1]) + p[2] < 1.0:
                _found.append((counts, m._sample_tables()["out_cdf"][lo:hi].tolist(), SO.tables(m)["out_cdf"][lo:hi], p.tolist()))
    return _found


def test_trained_rows_never_pick_an_impossible_edge():
    rows = trained_rows()
    print("%d of %d count triples leave a running sum below 1.0 in front of the edge of probability 0" % (len(rows), len(COUNTS) ** 3))
    assert len(rows) >= 100
    assert (1, 2, 4) in [c for c, _, _, _ in rows]              # (1/7 + 2/7) + 4/7 = 0.9999999999999999 through exp(log())
    for counts, got, want, p in rows:
        old = E.rows_closed_in_the_last_entry(p, [0, 4]).tolist()
        assert old[2] < 1.0 and p[SO.pick(old, 0, 4, E.TOP)] == 0.0, counts       # what the row rule is for
        for row in (got, want):
            assert p[SO.pick(row, 0, 4, E.TOP)] > 0, (counts, row)
            assert row == old[:2] + [1.0, 1.0], (counts, row, old)


def every_model():
    for name in sorted(SM.MODELS):
        yield name, SM.MODELS[name][0]()
    for name, m in (("loop", SM.loop()), ("dead", SM.dead_end()), ("mixsilent", MX.silent_model(True)[0]),
                    ("mixsilent-infinite", MX.silent_model(False)[0]), ("mixtiny", MX.tiny_model(True)),
                    ("mixline", MX.line_model(70)[0]), ("bimodal", MX.bimodal_model()), ("mixtrain", MX.training_model())):
        yield name, m


def test_existing_models_keep_the_bits_of_their_tables():
    """Rows whose last entry is positive are what they were: against rows built the old way, and against the oracle."""
    n = 0
    for name, m in every_model():
        f, got, want = m.flat, m._sample_tables(), E.oracle_tables(m)
        for key, lw, ptr in (("out_cdf", "out_lp", "out_ptr"), ("kde_cdf", "kde_lw", "kde_ptr")):
            old = E.rows_closed_in_the_last_entry(np.exp(f[lw]), f[ptr])
            assert got[key].dtype == np.float64 and got[key].tolist() == old.tolist() == want[key], (name, key)
            n += got[key].size
    assert n > 500


def test_the_table_invariant():
    rows = 0
    for name, m in every_model():
        f, t = m.flat, m._sample_tables()
        rows += E.check_rows(t["out_cdf"], np.exp(f["out_lp"]), f["out_ptr"], name + " out_cdf")
        rows += E.check_rows(t["kde_cdf"], np.exp(f["kde_lw"]), f["kde_ptr"], name + " kde_cdf")
        if m._mix["mix_cdf"].size:
            rows += E.check_rows(m._mix["mix_cdf"], np.exp(m._mix["mix_lw"]), m._mix["mix_ptr"], name + " mix_cdf")
            assert MX.tables(m)["mix_cdf"] == m._mix["mix_cdf"].tolist()
    assert rows > 150
    # trained rows: the found ones, and zero edges in front, in the middle, at the end and all but one
    for counts, got, want, p in trained_rows():
        assert E.check_rows(got, p, [0, 4], counts) == E.check_rows(want, p, [0, 4], counts) == 1
    for counts in ((0, 0, 3, 0, 0, 2, 0, 0), (0, 5, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 1, 0, 1, 0), (3, 3, 3, 3, 3, 3, 3, 3),
                   (0, 0, 0, 0, 0, 0, 0, 9), (7, 0, 0, 0, 0, 0, 0, 0)):
        m = E.trained_hub(counts)
        f, t = m.flat, m._sample_tables()
        assert E.check_rows(t["out_cdf"], np.exp(f["out_lp"]), f["out_ptr"], counts) == len(counts) + 2
        assert t["out_cdf"].tolist() == SO.tables(m)["out_cdf"]
        lo, hi = E.hub_row(m)
        taken = {SO.pick(t["out_cdf"], lo, hi, u) - lo for u in (0.0, 2.0 ** -53, 0.25, 0.5, 0.75, E.TOP)}
        assert taken <= {i for i, c in enumerate(counts) if c > 0}, (counts, taken)
    # a kernel density and a mixture with weights of 0: the density's flat form leaves such points out, the mixture keeps
    # the slots and closes its row the same way
    k = E.kde_model(5, "equal")
    assert k.flat["kde_lw"].size == 5 and E.check_rows(k._sample_tables()["kde_cdf"], np.exp(k.flat["kde_lw"]), k.flat["kde_ptr"], "kde") == 1
    x = E.mixture_model([0, 1, 0, 2, 4, 0])
    assert x._mix["mix_cdf"].tolist() == [0.0, 1 / 7, 1 / 7, 3 / 7, 1.0, 1.0]
    assert E.check_rows(x._mix["mix_cdf"], np.exp(x._mix["mix_lw"]), x._mix["mix_ptr"], "mixture") == 1


def test_the_helper_models_are_what_the_device_tests_take_them_for():
    m = E.hub(E.weights(9, "falling"))
    assert [s.name for s in m.states[:9]] == ["t%04d" % i for i in range(9)] and m.flat["out_dst"][slice(*E.hub_row(m))].tolist() == list(range(9))
    big = E.hub(E.weights(E.FAN_OUT[-1], "rising"))
    assert big.flat["n_states"] == 4096 and E.hub_row(big)[1] - E.hub_row(big)[0] == 4093
    row = big._sample_tables()["out_cdf"][slice(*E.hub_row(big))]
    assert np.count_nonzero(row < 2.0 ** -53) > 1000 and np.all(np.diff(row) > 0) and row[0] > 0      # many leading entries below 2^-53
    m = E.hub(E.weights(600, "falling"))
    row = m._sample_tables()["out_cdf"][slice(*E.hub_row(m))]
    steps = np.diff(row)
    assert np.count_nonzero(steps == 2.0 ** -53) >= 1 and np.count_nonzero(steps == 0) > 400          # neighbours an ulp apart, then flat
    c = E.chained()
    assert c.flat["n_levels"] >= E.CHAIN_LEVELS and c.flat["finite"] and c.flat["n_emit"] == 1
    for n, i in ((4, 0), (4, 1), (4, 2), (7, 5)):
        for v, _ in E.neighbours(0.37):
            assert E.crafted(n, i, v)[i] == v
    assert E.neighbours(0.5)[1][0] == 0.5 + 2.0 ** -53 and E.neighbours(0.5)[2][0] == 0.5 - 2.0 ** -54


def test_the_chosen_blocks_are_what_they_are_named():
    assert E.search_chosen() == E.CHOSEN                       # each the first such sequence under the seed
    for (j, which, at), Q in E.CHOSEN.items():
        u0, u1 = SO.block(E.CHOSEN_SEED, Q, j)
        u = u0 if which == "u0" else u1
        assert abs(u - at) <= 2.0 ** -12 and 0.0 < u < 1.0, (j, which, at, Q, u)
    assert len(E.CHOSEN) == 12


@pytest.mark.parametrize("name", sorted(E.DRAW_MODELS))
def test_the_oracle_against_mpmath_on_the_chosen_draws(name, record_property):
    """sample_oracle.draw (Python floats, the C library's log, cos, sqrt and exp) against the definition at 50 digits."""
    import mpmath
    build, blocks = E.DRAW_MODELS[name]
    m = build()
    T = E.oracle_tables(m)
    assert max(T["emit_param"][1::2]) <= 10.0
    worst = 0.0
    for (j, which, at), Q in sorted(E.CHOSEN.items()):
        if j not in blocks:
            continue
        w = E.oracle_walks(m, T, 1, E.CHOSEN_SEED, Q)[0]
        ref = E.first_emission_mp(m, T, E.CHOSEN_SEED, Q)
        assert len(w.obs) == 1 and len(w.obs[0]) == len(ref) == m.flat["n_dim"]
        for got, r in zip(w.obs[0], ref):
            err = E.error_mp(got, r)
            print("%s block %d %s near %g (Q = %d): oracle %.17g, mpmath %s, error %.3g" % (name, j, which, at, Q, got, mpmath.nstr(r, 20), err))
            assert err <= TOL, (name, j, which, at, got, r)
            worst = max(worst, err)
    record_property("largest_oracle_error_against_mpmath", worst)
    # the uniform draw is exact arithmetic but for its one rounding
    from pypore_amd.hmm import UniformDistribution
    d = UniformDistribution(-3.0, 4.5)
    for u0 in (0.0, 2.0 ** -53, 0.3, E.TOP):
        assert E.error_mp(SO.draw(d, -3.0, 7.5, u0, 0.0), E.draw_mp(d, -3.0, 7.5, u0, 0.0)) <= 2.0 ** -52
