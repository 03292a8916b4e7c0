"""Models whose Viterbi decisions tie exactly, for tests/test_viterbi_exact_host.py and tests/test_viterbi_exact_gpu.py.

A tie here is structural: the two candidates are formed from bit-identical operands by the same operations (twin states
that share one distribution object and carry mirrored edge weights), so they are equal in every IEEE arithmetic and the
tie rule alone decides -- in-edges in ascending source index, a strictly greater score replaces the best, the lowest
source wins; an infinite model ends in the lowest best state of the last row.  Every builder returns
(model, sequences, ties): ties[q] = the least number of tied decisions on sequence q's winning path, counted from the
construction (written out per builder), which hmm_oracle.viterbi_exact must report at least."""
import numpy as np

import hmm_oracle as O
from pypore_amd.hmm import Model, NormalDistribution, State

LADDER_LENGTHS = (0, 1, 2, 17, 70)


def twin_ladder(L, strided, finite=True, seed=0):
    """L levels.  Level i holds twins A_i, B_i that share one NormalDistribution(3 i, 1) and carry mirrored dyadic edges:
    self 0.25, to the twin 0.125, on to the next hub 0.5 (bake divides all three by the same 0.875).  hub_0 = start; hub_i
    enters A_i and B_i with 0.25 each and skips to hub_(i+1) with 0.5; the hub after the last level is `end` (finite) or
    missing (infinite: the last twins keep self and twin edges only, the last hub its two entries).  By symmetry A_i and
    B_i hold the same bits in every row, so every visited level ties where it is left (hub_(i+1) or `end` scans A_i, B_i,
    hub_i), and in an infinite model the last row ties between the twins of the level the path ends in.

    strided False: names t000a, t000b, t001a, ...: twins at adjacent indices, adjacent lanes of the wave.
    strided True (L = 64): names a000.., b000..: twin i at indices i and i + 64, the same lane two strides apart.

    Sequences of LADDER_LENGTHS: observation j sits near level lv[j], lv ascending, so the winning path visits exactly the
    levels in lv.  Finite: one tie per visited level.  Infinite: one per visited level but the last, plus the last row's.
    Either way ties[q] = the number of distinct levels of sequence q (0 for the empty one)."""
    m = Model("ladder")
    twins = []
    name = (lambda i, ab: "%s%03d" % (ab, i)) if strided else (lambda i, ab: "t%03d%s" % (i, ab))
    hubs = [m.start] + [State(None, "hub%03d" % i) for i in range(1, L)] + ([m.end] if finite else [None])
    for i in range(L):
        d = NormalDistribution(3.0 * i, 1.0)
        a, b = State(d, name(i, "a")), State(d, name(i, "b"))
        twins.append((a, b))
        m.add_transition(hubs[i], a, 0.25)
        m.add_transition(hubs[i], b, 0.25)
        if hubs[i + 1] is not None:
            m.add_transition(hubs[i], hubs[i + 1], 0.5)
        for x, y in ((a, b), (b, a)):
            m.add_transition(x, x, 0.25)
            m.add_transition(x, y, 0.125)
            if hubs[i + 1] is not None:
                m.add_transition(x, hubs[i + 1], 0.5)
    m.bake()
    assert bool(m.finite) == finite
    for i, (a, b) in enumerate(twins):                  # the lanes the docstring names: bake orders emitting states by name
        ia, ib = m.states.index(a), m.states.index(b)
        assert (ia, ib) == ((i, i + 64) if strided else (2 * i, 2 * i + 1)), (i, ia, ib)
        assert ia % 64 == ib % 64 if strided else ib % 64 == ia % 64 + 1
    assert not strided or L == 64
    rng = np.random.default_rng(1000 * L + seed)
    seqs, ties = [], []
    for n in LADDER_LENGTHS:
        lv = np.sort(rng.integers(0, L, n))
        seqs.append(3.0 * lv + rng.normal(0, 0.3, n))
        ties.append(len(set(lv.tolist())))
    return m, seqs, ties


def silent_diamonds(depth):
    """start -> d0, then `depth` diamonds in a chain: join_(i-1) -> u_i, v_i (0.5 each) -> join_i (1.0 each), join_0 = d0.
    The last join enters the emitting states e (mean 0) and f (mean 20) with 0.5 each; each of them loops (0.25), returns
    to d0 (0.25) or ends (0.5).  u_i joined the model before v_i, so it has the lower index.  Every join scans u_i, v_i
    with identical scores: `depth` ties per passage through the chain, all decided in the silent phase on row `cur`.
    The observations alternate between e's level and f's (20 apart at std 1: staying costs 200, more than two passages
    of the chain at depth 40, 2 * 40 log 2), and the only way from e to f is through d0: a sequence of n observations
    passes the chain n times, ties[q] = depth * n.  The empty sequence is impossible (no silent way to `end`)."""
    m = Model("diamonds")
    d0 = State(None, "d0")
    m.add_transition(m.start, d0, 1.0)
    join = d0
    for i in range(1, depth + 1):
        u, v, nxt = State(None, "u%02d" % i), State(None, "v%02d" % i), State(None, "j%02d" % i)
        m.add_transition(join, u, 0.5)
        m.add_transition(join, v, 0.5)
        m.add_transition(u, nxt, 1.0)
        m.add_transition(v, nxt, 1.0)
        join = nxt
    for nm, mean in (("e", 0.0), ("f", 20.0)):
        s = State(NormalDistribution(mean, 1.0), nm)
        m.add_transition(join, s, 0.5)
        m.add_transition(s, s, 0.25)
        m.add_transition(s, d0, 0.25)
        m.add_transition(s, m.end, 0.5)
    m.bake()
    rng = np.random.default_rng(depth)
    seqs = [20.0 * (np.arange(n) % 2) + rng.normal(0, 0.2, n) for n in (0, 1, 4, 9)]
    return m, seqs, [depth * len(s) for s in seqs]


def all_tied(S=130):
    """S emitting states that share one distribution, start -> each with 1/128 and each -> each with 1/128 (bake divides
    by the same S/128 everywhere); no `end`, so the model is infinite.  Every state holds the same bits in every row: from
    step 2 on every decision ties S ways (all lanes, and three strides of the lanes below S - 128), and so does the last
    row.  State 0 must win everywhere; the opposite rule takes state S - 1.  ties[q] = (n - 1) + 1 for n >= 1 (step 1 has
    the single candidate `start`)."""
    m = Model("flat")
    d = NormalDistribution(0.0, 1.0)
    st = [State(d, "s%03d" % i) for i in range(S)]
    for a in st:
        m.add_transition(m.start, a, 1.0 / 128)
        for b in st:
            m.add_transition(a, b, 1.0 / 128)
    m.bake()
    assert not m.finite
    rng = np.random.default_rng(S)
    seqs = [rng.normal(0, 1, n) for n in (1, 2, 5)]
    return m, seqs, [len(s) for s in seqs]


def tied_hub(n_in, lo, hi):
    """hmm_oracle.hub_model(n_in) -- a hub state h with n_in in-edges, from the emitting states e0000 .. e(n_in - 2) in
    ordinal order and from itself last -- with e<lo> and e<hi> sharing ONE distribution (e<lo>'s), so after an observation
    at 3 lo the two hold the same bits and h's in-edges of ordinals lo and hi tie.  The lower ordinal wins; the opposite
    rule, or a backpointer that loses its high byte among tied candidates, names another state.  The largest in-degree of
    the model is n_in: 255 takes the 8-bit backpointers, more the 16-bit ones.  Each sequence enters h twice from the tied
    pair: ties[q] = 2."""
    m, h, es = O.hub_model(n_in, shared=(lo, hi))
    k = m.states.index(h)
    f = m.flat
    assert f["in_ptr"][k + 1] - f["in_ptr"][k] == n_in and int(np.diff(f["in_ptr"]).max()) == n_in
    assert f["in_src"][f["in_ptr"][k] + lo] == m.states.index(es[lo]) and f["in_src"][f["in_ptr"][k] + hi] == m.states.index(es[hi])
    other = 3.0 * ((lo + 7) % (n_in - 1))
    seqs = [np.array([3.0 * lo, -50.0, 3.0 * lo + 0.25, -50.5, other]),
            np.array([3.0 * lo - 0.125, -49.75, -50.0, other, -50.25, 3.0 * lo, -50.0])]
    return m, seqs, [2, 2]


# name -> builder.  The hub pairs: (3, 300) and (256, 300) at in-degree 600 (16-bit backpointers; 256 loses its high byte
# to 0 when cut to 8 bits), (3, 254) at 257 (16-bit, just over the width), (3, 253) at 255 (the 8-bit route: its e states end
# at ordinal 253, ordinal 254 being h's own loop, which no e state can tie).
TIE_CASES = {
    "ladder8_adjacent": lambda: twin_ladder(8, False),
    "ladder64_strided": lambda: twin_ladder(64, True),
    "ladder8_adjacent_infinite": lambda: twin_ladder(8, False, finite=False),
    "ladder64_strided_infinite": lambda: twin_ladder(64, True, finite=False),
    "all_tied_130_infinite": lambda: all_tied(130),
    "diamonds7": lambda: silent_diamonds(7),
    "diamonds40": lambda: silent_diamonds(40),
    "hub600_3_300": lambda: tied_hub(600, 3, 300),
    "hub600_256_300": lambda: tied_hub(600, 256, 300),
    "hub255_3_253": lambda: tied_hub(255, 3, 253),
    "hub257_3_254": lambda: tied_hub(257, 3, 254),
}

_built = {}


def tie_case(name):
    """(model, sequences, ties, expected) of TIE_CASES[name], built and solved once per process: expected[q] =
    hmm_oracle.viterbi_exact(model, sequences[q]).  Read only."""
    if name not in _built:
        model, seqs, ties = TIE_CASES[name]()
        _built[name] = (model, seqs, ties, [O.viterbi_exact(model, s) for s in seqs])
    return _built[name]


def launches(lengths, row_bytes, budget):
    """The launches hmm_viterbi cuts a batch into (csrc/poreseg.hip next_chunk): as many sequences as keep
    (len + 1) * row_bytes within the budget, at least one.  Returns [(q0, q1, bytes)]."""
    out, q0, n = [], 0, len(lengths)
    while q0 < n:
        size, q1 = (lengths[q0] + 1) * row_bytes, q0 + 1
        while q1 < n and size + (lengths[q1] + 1) * row_bytes <= budget:
            size += (lengths[q1] + 1) * row_bytes
            q1 += 1
        out.append((q0, q1, size))
        q0 = q1
    return out
