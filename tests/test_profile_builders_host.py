"""The reference's profile HMM builders (pypore_amd.hmm: HMMBoard, the three board modules, ModularProfileModel,
Phi29ProfileHMM, Hel308ProfileHMM) and bake(merge=...), on the CPU: the sizes the issue's table lists, state names, edge
probabilities, the errors, and decoding and merging judged by the numpy oracle (tests/hmm_oracle.py).

Bounds.  A merged model's log probability equals the unmerged one's to 1e-12 relative to max(1, |value|): the two sum the
same path weights, grouped differently, so only roundings differ (the largest difference seen is 2e-16).  Viterbi paths are
compared where the oracle's winning margin is at least 1e-9 on both models, which the walking and backslip sequences
here are chosen to have (asserted); the uniform-noise sequence ties exactly between insert states of equal density and is
compared by log probability alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_oracle as O  # noqa: E402
import modular_models as MM  # noqa: E402

from pypore_amd.hmm import *  # noqa: E402,F401,F403  (the issue: `import *` provides every builder)
from pypore_amd import hmm as H  # noqa: E402

# states / emitting states / silent levels / edges / largest in-degree after bake()
SIZES = {
    ("modular", "phi29"): {3: (50, 14, 11, 95, 4), 8: (140, 39, 26, 265, 4), 54: (968, 269, 164, 1829, 4)},
    ("modular", "nanopore"): {3: (31, 7, 11, 62, 4), 8: (81, 17, 26, 162, 4), 54: (541, 109, 164, 1082, 4)},
    ("modular", "global"): {3: (24, 7, 11, 45, 3), 8: (59, 17, 26, 110, 3), 54: (381, 109, 164, 708, 3)},
    ("linear", "phi29"): {3: (27, 14, 5, 68, 6), 12: (108, 59, 14, 293, 6), 54: (486, 269, 56, 1343, 6)},
    ("linear", "hel308"): {3: (27, 14, 5, 68, 6), 12: (111, 59, 14, 301, 7), 54: (531, 269, 56, 1477, 7)},
}


def build(family, kind, n):
    if family == "modular":
        return MM.modular(n, kind)
    return MM.linear(kind, n, merge=None) if kind == "phi29" else MM.linear(kind, n)


def out_probabilities(model, state):
    i = model.states.index(state)
    return {model.states[j].name: p for a, j, p in model.edges if a == i}


def by_name(model, name, k=0):
    return [s for s in model.states if s.name == name][k]


def approx(got, want):
    assert set(got) == set(want), (got, want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-15, (k, got[k], want[k])


# ---- names exported ----------------------------------------------------------------------------------------------------
def test_import_star_provides_every_name():
    for name in ("HMMBoard", "ModularProfileModel", "GlobalAlignmentModule", "NanoporeGlobalAlignmentModule",
                 "Phi29GlobalAlignmentModule", "Phi29ProfileHMM", "Hel308ProfileHMM"):
        assert globals()[name] is getattr(H, name)
    assert not hasattr(H, "Phi29ProfileHMMU")


def test_board():
    b = HMMBoard(3, "x")  # noqa: F405
    assert isinstance(b, Model) and b.name == "Board x" and b.n == 3 and b.directions == ['>'] * 3  # noqa: F405
    assert [getattr(b, "%s%d" % (side, i)).name for i in (1, 2, 3) for side in "se"] == ["bxs1", "bxe1", "bxs2", "bxe2", "bxs3", "bxe3"]
    assert all(getattr(b, "%s%d" % (side, i)).is_silent() for i in (1, 2, 3) for side in "se")
    assert [m(NormalDistribution(1, 1), 0, MM.insert()).n for m in  # noqa: F405
            (GlobalAlignmentModule, NanoporeGlobalAlignmentModule, Phi29GlobalAlignmentModule)] == [2, 3, 5]  # noqa: F405
    phi = Phi29GlobalAlignmentModule(NormalDistribution(1, 1), 7)  # noqa: F405
    assert phi.directions == ['>', '>', '<', '>', '<'] and phi._flat is None
    assert {s.name for s in phi._added} >= {"M:7", "MO:7", "MS:7", "ME:7", "D:7", "I:7", "7-start", "7-end"}
    ins = [s for s in phi._added if s.name == "I:7"][0].distribution
    assert type(ins).__name__ == "UniformDistribution" and ins.parameters == [0.0, 90.0]


# ---- sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,kind,n", [(f, k, n) for (f, k), row in SIZES.items() for n in row])
def test_sizes(family, kind, n):
    assert MM.size(build(family, kind, n)) == SIZES[(family, kind)][n]


def test_sizes_fork_and_merged():
    assert MM.size(MM.fork_model())[:4] == (104, 29, 14, 202)
    assert MM.size(MM.modular(54, merge="partial"))[:4] == (593, 269, 56, 1451)
    assert MM.size(MM.modular(54, merge="all"))[:4] == (487, 269, 56, 1345)
    assert MM.size(MM.modular(3, merge="partial"))[:4] == (32, 14, 5, 74)
    assert MM.size(MM.modular(3, merge="All"))[:4] == (28, 14, 5, 70)


def test_accumulator_row_crosses_the_lds_limit_between_96_and_97_positions():
    """16 S + 8 (E + 3 NE + 1): the E-step's two score rows and its accumulator row (csrc HMM_EXPECT_LDS = 64 KiB)."""
    def row(m):
        S, NE, _, E, _ = MM.size(m)
        return 16 * S + 8 * (E + 3 * NE + 1)
    m96, m97 = MM.modular(96), MM.modular(97)
    assert row(m96) == 65144 <= 65536 < row(m97) == 65824
    assert MM.size(m97)[0] == 1742 and MM.size(m97)[2] == 293


# ---- names and numbers ---------------------------------------------------------------------------------------------------
def test_state_names_of_three_positions():
    m = MM.modular(3)
    ne = m.flat["n_emit"]
    # MS: needs lane 4 from the board before, ME: lane 3 from the board after: the ends of the profile have neither
    assert [s.name for s in m.states[:ne]] == ["I:0", "I:0", "I:1", "I:2", "M:0", "M:1", "M:2", "ME:0", "ME:1", "MO:0", "MO:1",
                                                "MO:2", "MS:1", "MS:2"]
    ports = {"b%d%s%d" % (b, side, j) for b in range(3) for side in "se" for j in range(1, 6)}
    ports -= {"b0s3", "b0s4", "b2e3", "b2e4", "b2e5"}         # nothing reaches them
    inner = {"%d-%s" % (b, w) for b in range(3) for w in ("start", "end")} | {"D:0", "D:1", "D:2"}
    assert {s.name for s in m.states[ne:]} == ports | inner | {"modular-start", "modular-end"}
    assert m.states[ne] is m.start and m.states[-1] is m.end and m.finite
    assert len({id(s.distribution) for s in m.states[:4]}) == 1          # one insert object for all


def test_state_names_of_the_fork_model():
    m = MM.fork_model()
    ne = m.flat["n_emit"]
    boards = ["0", "a:2", "b:2", "a:3", "b:3", "3"]
    want = ["I:0"] + ["%s:%s" % (k, b) for k in ("I", "M", "MO") for b in boards] \
        + ["ME:%s" % b for b in boards[:-1]] + ["MS:%s" % b for b in boards[1:]]
    assert sorted(s.name for s in m.states[:ne]) == sorted(want)
    assert {"ba:2s1", "bb:2s1", "ba:3e5", "bb:3e5", "a:2-start", "b:3-end", "D:a:2"} <= {s.name for s in m.states[ne:]}


def test_out_probabilities():
    m = MM.modular(3)
    approx(out_probabilities(m, m.start), {"I:0": 0.02, "b0s1": 0.08, "b0s2": 0.90})
    head = [s for s in m.states if s.name == "I:0" and "b0s1" in out_probabilities(m, s)][0]
    approx(out_probabilities(m, head), {"I:0": 0.70, "b0s1": 0.1, "b0s2": 0.2})
    approx(out_probabilities(m, by_name(m, "D:1")), {"b1e1": 0.1, "I:1": 0.1, "b1e2": 0.8})
    approx(out_probabilities(m, by_name(m, "1-end")), {"I:1": 0.01, "b1e1": 0.01, "b1e2": 0.97, "b1s5": 0.01})
    approx(out_probabilities(m, by_name(m, "b1e5")), {"1-start": 0.90, "ME:1": 0.05, "b1s5": 0.05})
    approx(out_probabilities(m, by_name(m, "1-start")), {"M:1": 0.95, "MO:1": 0.05})
    approx(out_probabilities(m, by_name(m, "b2e1")), {"modular-end": 1.0})
    approx(out_probabilities(m, by_name(m, "b2e2")), {"modular-end": 1.0})
    approx(out_probabilities(m, by_name(m, "b2s5")), {"b1e5": 1.0})      # a '<' lane: s of this board -> e of the one before
    approx(out_probabilities(m, by_name(m, "b0e4")), {"b1s4": 1.0})
    assert out_probabilities(m, by_name(m, "b0s5")) == {}                # a dead end: no board before the first
    n = MM.modular(3, "nanopore")
    approx(out_probabilities(n, by_name(n, "M:1")), {k: v / 1.306 for k, v in
                                                     {"b1s3": 0.033, "M:1": 0.4, "b1e2": 0.5, "I:1": 0.033, "b1e1": 0.34}.items()})
    g = MM.modular(3, "global")
    approx(out_probabilities(g, by_name(g, "M:1")), {"b1e2": 0.9, "b1e1": 0.05, "I:1": 0.05})


def test_fork_entry_and_exit_edges():
    m = MM.fork_model()
    for j, d in zip(range(1, 6), ['>', '>', '<', '>', '<']):
        if d == '>':        # into the fork 1/2 each, between the forks and out of them 1
            approx(out_probabilities(m, by_name(m, "b0e%d" % j)), {"ba:2s%d" % j: 0.5, "bb:2s%d" % j: 0.5})
            for k in "ab":
                approx(out_probabilities(m, by_name(m, "b%s:2e%d" % (k, j))), {"b%s:3s%d" % (k, j): 1.0})
                if j != 4:  # (lane 4 of the last board is never entered: MS:3 needs it, and is there; e4 of the forks is)
                    approx(out_probabilities(m, by_name(m, "b%s:3e%d" % (k, j))), {"b3s%d" % j: 1.0})
        else:               # backwards: out of the last board 1/2 each, between the forks and into the first board 1
            approx(out_probabilities(m, by_name(m, "b3s%d" % j)), {"ba:3e%d" % j: 0.5, "bb:3e%d" % j: 0.5})
            for k in "ab":
                approx(out_probabilities(m, by_name(m, "b%s:3s%d" % (k, j))), {"b%s:2e%d" % (k, j): 1.0})
                approx(out_probabilities(m, by_name(m, "b%s:2s%d" % (k, j))), {"b0e%d" % j: 1.0})
    for k in "ab":
        approx(out_probabilities(m, by_name(m, "b%s:3e4" % k)), {"b3s4": 1.0})


def test_errors():
    ins, d = MM.insert(), NormalDistribution(30, 1.5)  # noqa: F405
    fork, other = {"a": d, "b": d}, {"a": d, "c": d}
    for bad in ([], [fork, d], [d, fork], [d, fork, other, d], [d, fork, {"b": d, "a": d}, d]):
        with pytest.raises(ValueError):
            ModularProfileModel(Phi29GlobalAlignmentModule, bad, "bad", ins)  # noqa: F405
    for kw in (dict(sb_length=0), dict(sb_length=-1)):
        with pytest.raises(ValueError):
            Phi29ProfileHMM(MM.profile(3), verbose=False, **kw)  # noqa: F405
        with pytest.raises(ValueError):
            Hel308ProfileHMM(MM.profile(3), **kw)  # noqa: F405
    with pytest.raises(ValueError):
        Hel308ProfileHMM(MM.profile(3), lb_length=0)  # noqa: F405
    with pytest.raises(ValueError):
        Phi29ProfileHMM([], verbose=False)  # noqa: F405
    with pytest.raises(ValueError):
        Hel308ProfileHMM([])  # noqa: F405
    m = MM.modular(3)
    for bad in ("bogus", "", 1):
        with pytest.raises(ValueError):
            m.bake(merge=bad)


def same_flat(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("make", [lambda: MM.modular(8), lambda: MM.fork_model(), lambda: MM.modular(8, "nanopore", merge="all"),
                                  lambda: MM.linear("phi29", 12), lambda: MM.linear("hel308", 12)])
def test_building_twice_gives_equal_arrays(make):
    a, b = make(), make()
    assert same_flat(a.flat, b.flat) and [s.name for s in a.states] == [s.name for s in b.states] and a.edges == b.edges


def test_linear_builders_keep_the_reference_names_and_defaults(capsys):
    m = Phi29ProfileHMM(MM.profile(3))  # noqa: F405     (verbose=True, merge='all')
    assert "Phi29 Profile HMM-3" in capsys.readouterr().out and m.name == "Phi29 Profile HMM-3"
    plain = MM.linear("phi29", 3, merge=None)
    assert MM.size(m) == MM.size(plain)           # (every silent state of the linear profile has two ways out or more)
    ne = plain.flat["n_emit"]
    # match, oversegmented match and the repeat states all carry the match's name
    assert [s.name for s in plain.states[:ne]] == ["I0", "I1", "I2", "I3"] + ["M1"] * 3 + ["M2"] * 4 + ["M3"] * 3
    assert {"D1", "D2", "D3", "S2", "S3", "M1-start", "M3-end"} <= {s.name for s in plain.states[ne:]}
    h = MM.linear("hel308", 12)
    assert h.name == "Hel308 Profile HMM-12" and {"L10", "L11", "L12"} <= {s.name for s in h.states}
    assert "L9" not in {s.name for s in h.states}
    approx(out_probabilities(h, by_name(h, "L11")), {"M2-start": 0.75, "L10": 0.25})
    approx(out_probabilities(h, by_name(h, "L10")), {"M1-start": 1.0})
    approx(out_probabilities(plain, by_name(plain, "S3")), {"M2-start": 0.75, "M2": 0.10, "S2": 0.15})


# ---- decoding sanity (the oracle) ------------------------------------------------------------------------------------------
def test_a_walk_decodes_along_the_match_lane():
    m = MM.modular(3)
    lp, path, margin = O.viterbi(O.Compiled(m), MM.walk(MM.means(3)))
    assert MM.emitting_names(m, path) == ["M:0", "M:1", "M:2"] and margin > 1e-9


def test_a_backslip_decodes_through_the_backslip_lane():
    m = MM.modular(3)
    lp, path, margin = O.viterbi(O.Compiled(m), [20, 35, 20, 35, 50])
    assert MM.emitting_names(m, path) == ["M:0", "M:1", "M:0", "M:1", "M:2"] and margin > 1e-9
    names = [m.states[i].name for i in path]
    assert names[names.index("1-end") + 1:][:3] == ["b1s5", "b0e5", "0-start"]


def test_fork_sequences_take_their_branch_with_equal_scores():
    m = MM.fork_model()
    c = O.Compiled(m)
    got = {k: O.viterbi(c, s) for k, s in MM.FORK_SEQS.items()}
    for k in "ab":
        assert MM.emitting_names(m, got[k][1]) == ["M:0", "M:%s:2" % k, "M:%s:3" % k, "M:3"] and got[k][2] > 1e-9
    assert got["a"][0] == got["b"][0]


# ---- merge -----------------------------------------------------------------------------------------------------------------
MERGE_CASES = {"phi29-3": (lambda mg: MM.modular(3, merge=mg), 3), "phi29-8-fork": (lambda mg: MM.fork8_model(merge=mg), 8),
               "nanopore-8": (lambda mg: MM.modular(8, "nanopore", merge=mg), 8)}


@pytest.fixture(scope="module", params=sorted(MERGE_CASES))
def merge_case(request):
    make, n = MERGE_CASES[request.param]
    mu = MM.means(n)
    walks = [MM.walk(mu), MM.walk(mu, -0.4), MM.walk_with_backslip(mu, n // 2)]
    noise = np.random.default_rng(5).uniform(0, 90, n)
    base = make(None)
    c = O.Compiled(base)
    return make, base, walks, noise, [O.viterbi(c, s) for s in walks], [O.log_probability(c, s) for s in walks + [noise]]


@pytest.mark.parametrize("mode", ["partial", "all"])
def test_merge_keeps_log_probabilities_and_paths(merge_case, mode):
    make, base, walks, noise, base_vit, base_logp = merge_case
    merged = make(mode)
    assert len(merged.states) < len(base.states) and merged.flat["n_emit"] == base.flat["n_emit"]
    assert merged.states[merged.flat["start"]] is merged.start and merged.states[merged.flat["end"]] is merged.end
    c = O.Compiled(merged)
    for s, want in zip(walks + [noise], base_logp):
        got = O.log_probability(c, s)
        print("logp %.17g merged %.17g" % (want, got))
        assert np.isfinite(want) and abs(got - want) <= 1e-12 * max(1.0, abs(want))
    kept = {s.name for s in merged.states}
    for s, (_, path, margin) in zip(walks, base_vit):
        _, mpath, mmargin = O.viterbi(c, s)
        assert margin >= 1e-9 and mmargin >= 1e-9
        assert [n for n in (base.states[i].name for i in path) if n in kept] == [merged.states[i].name for i in mpath]
    removed = {s.name for s in base.states} - kept
    assert removed and all(next(x for x in base.states if x.name == n).is_silent() for n in removed)
    again = dict(merged.flat)
    merged.bake(merge="all" if mode == "all" else "partial")
    assert same_flat(again, merged.flat)


def test_merge_none_is_the_default_bit_for_bit():
    a, b, c = MM.modular(8), MM.modular(8, merge="none"), MM.modular(8, merge="None")
    assert same_flat(a.flat, b.flat) and same_flat(a.flat, c.flat)
    a.bake()
    assert same_flat(a.flat, b.flat)


def small_model():
    """start -> a (silent) -> b and start -> b directly; c (silent) in front of the emitting x; `end` behind a silent z."""
    m = Model("small")  # noqa: F405
    a, b, c, z = (State(None, n) for n in "abcz")  # noqa: F405
    x = State(NormalDistribution(0, 1), "x")  # noqa: F405
    m.add_transition(m.start, a, 0.3, pseudocount=2.0)
    m.add_transition(m.start, b, 0.7, pseudocount=5.0)
    m.add_transition(a, b, 1.0, pseudocount=11.0)
    m.add_transition(b, c, 0.6)
    m.add_transition(b, x, 0.4)
    m.add_transition(c, x, 0.5)                     # (one out-edge: normalised to 1)
    m.add_transition(x, x, 0.5)
    m.add_transition(x, z, 0.5)
    m.add_transition(z, m.end, 1.0)
    return m, (a, b, c, x, z)


def test_merge_sums_probabilities_and_pseudocounts_and_rewrites_the_graph():
    m, (a, b, c, x, z) = small_model()
    m.bake(merge="partial")
    # a -> b folds start's two edges into one (b keeps its two ways out), z -> end folds into x -> end, and c stays
    # under 'partial' since x emits; `end` now follows an emitting state alone: level 0
    assert [s.name for s in m.states] == ["x", "small-start", "small-end", "b", "c"]
    assert m._edges[(m.start, b)] == 1.0 and m._pseudo[(m.start, b)] == 7.0
    assert (m.start, a) not in m._edges and (a, b) not in m._edges and a not in m._added
    assert m._edges[(x, m.end)] == 0.5 and (x, z) not in m._edges
    m.bake(merge="all")
    # c -> x folds into b -> x: 0.6 + 0.4; then b has one way out and folds too: start -> x
    assert [s.name for s in m.states] == ["x", "small-start", "small-end"]
    assert m._edges[(m.start, x)] == 1.0 and m._pseudo[(m.start, x)] == 7.0
    assert m.edges == [(0, 0, 0.5), (0, 2, 0.5), (1, 0, 1.0)]
    m.bake()                                         # a later bake starts from the merged graph
    assert [s.name for s in m.states] == ["x", "small-start", "small-end"]


def test_start_and_end_survive_a_merge():
    m = Model("line")  # noqa: F405
    x = State(NormalDistribution(0, 1), "x")  # noqa: F405
    s = State(None, "s")  # noqa: F405
    m.add_transition(m.start, s, 1.0)                # start: silent, one way out -- and kept
    m.add_transition(s, x, 1.0)
    m.add_transition(x, m.end, 1.0)
    m.bake(merge="all")
    assert [t.name for t in m.states] == ["x", "line-start", "line-end"] and m.finite
    assert m.edges == [(0, 2, 1.0), (1, 0, 1.0)]
    loop = Model("loop")  # noqa: F405
    t = State(None, "t")  # noqa: F405
    loop.add_transition(loop.start, t, 1.0)
    loop.add_transition(t, t, 0.5)                   # two ways out, one to itself: not merged (and a silent cycle)
    loop.add_transition(t, loop.end, 0.5)
    with pytest.raises(ValueError):
        loop.bake(merge="all")
