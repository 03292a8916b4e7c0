"""lambda_event_parser(threshold, rules=R, on_device=True): the caller's rules over the device's piece table (ps_detect_pieces)
against the same parser on the host route (numpy pieces).  Same pieces in the same order, the same start, duration, n and values
of `current`, min and max equal with ==.  mean and std are the device's, from exact integer sums; numpy's pairwise sums of at
most 1.1e5 values near 100 pA are within log2(n) * 2^-53 * 100 pA, about 2e-13 pA, of the exact value, so the two agree to 1e-9 pA
with three orders to spare -- and the mean / std rules below keep every piece at least 1e-3 pA from their constants (asserted
against the numpy values), so no decision can hinge on those last bits.

One trace of 160 000 samples: a baseline near 100 pA, blockades near 20 pA of 30 .. 100 500 samples -- one longer than the
default rule's 100 000 --, a quiet one and a noisy one, and single-sample spikes across the threshold."""
import numpy as np
import pytest

from pypore_amd import synth
from pypore_amd.core import raw_current
from pypore_amd.DataTypes import Experiment, File
from pypore_amd.parsers import lambda_event_parser

pytestmark = pytest.mark.gpu

Q = synth.QUANTUM
HEADER_Q = 10.0 / 0.0005 / 20.0 / 32768.0 * 1.0001        # an .abf header's scale: not a power of two
OFFSET = 1.75
T = 90
N = 160_000
EVENTS = [(2_000, 30), (4_000, 51), (6_000, 200), (9_000, 4_999), (16_000, 5_000), (24_000, 6_500), (33_000, 100_500), (140_000, 1_200),
          (150_000, 3_000)]
SPIKES = [100, 1_000, 1_002, 145_000, N - 1]             # all on the baseline


def counts():
    rng = np.random.default_rng(515)
    k = 3200 + rng.integers(-60, 61, N)
    for a, n in EVENTS:
        k[a:a + n] = 640 + rng.integers(-60, 61, n)
    k[140_000:141_200] = 700                                # a quiet blockade: std 0
    k[150_000:153_000] = 900 + rng.integers(-800, 801, 3_000)    # a noisy one
    for s in SPIKES:
        k[s] = 640 if k[s] > 2000 else 3200
    return k.astype(np.int16)


K = counts()


def default_rules(t):
    return [lambda ev: ev.duration > 100000, lambda ev: ev.min > -0.5, lambda ev: ev.max < t]


def short_rules(t):
    return [lambda ev: ev.duration > 50, lambda ev: ev.duration < 5000, lambda ev: ev.max < t]


MEAN_BELOW, STD_ABOVE = 60.0, 5.0                           # blockades (20 .. 30 pA) that are noisy (one: std near 14 pA; the rest below 1.2)


def moment_rules(t):
    return [lambda ev: ev.mean < MEAN_BELOW, lambda ev: ev.std > STD_ABOVE, lambda ev: ev.n > 10]


RULES = {"default": default_rules, "short": short_rules, "moments": moment_rules}


def inputs(kind):
    """(what the device parser gets, the float64 values the host parser gets)"""
    import torch
    from pypore_amd.grid import GridArray
    if kind == "grid_i16":
        g = GridArray.from_counts(K, HEADER_Q, OFFSET)
        return g, np.asarray(g)
    x = K.astype(np.float64) * Q
    if kind == "f64_pow2":
        return x, x
    return torch.from_numpy(x).cuda(), x


def same_pieces(got, want):
    assert [(s.start, s.duration, s.n) for s in got] == [(s.start, s.duration, s.n) for s in want]
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g.current), np.asarray(w.current))
        assert g.min == w.min and g.max == w.max
        assert abs(g.mean - w.mean) < 1e-9 and abs(g.std - w.std) < 1e-9


@pytest.mark.parametrize("kind", ["grid_i16", "f64_pow2", "f64_cuda"])
@pytest.mark.parametrize("rules", sorted(RULES))
def test_device_rules_equal_host_rules(kind, rules):
    dev_in, host_in = inputs(kind)
    want = lambda_event_parser(T, rules=RULES[rules](T)).parse(host_in)
    got = lambda_event_parser(T, rules=RULES[rules](T), on_device=True).parse(dev_in)
    assert len(want) == {"default": 1, "short": 5, "moments": 1}[rules]
    same_pieces(got, want)
    assert all("_gpu_stats" in s.__dict__ for s in got)
    if rules == "moments":                                   # the rule constants lie far from every piece's value
        below = host_in < T
        cuts = np.concatenate(([0], np.flatnonzero(below[1:] != below[:-1]) + 1, [N]))
        means = np.array([host_in[a:z].mean() for a, z in zip(cuts, cuts[1:])])
        stds = np.array([host_in[a:z].std() for a, z in zip(cuts, cuts[1:])])
        assert np.abs(means - MEAN_BELOW).min() > 1e-3 and np.abs(stds - STD_ABOVE).min() > 1e-3
    from pypore_amd.grid import grid_of
    for s in got:                                            # slices of the caller's array, not copies
        if kind == "f64_pow2":
            assert np.shares_memory(raw_current(s), dev_in)
        elif kind == "grid_i16":                             # (still the file's int16 counts)
            assert grid_of(raw_current(s)) is not None


@pytest.mark.parametrize("kind", ["grid_i16", "f64_pow2", "f64_cuda"])
def test_pieces_table(kind):
    dev_in, host_in = inputs(kind)
    t = lambda_event_parser(T, rules=[lambda ev: False]).pieces(dev_in)
    below = host_in < T
    cuts = np.concatenate(([0], np.flatnonzero(below[1:] != below[:-1]) + 1, [N]))
    assert np.array_equal(t.edges, cuts) and len(t) == len(cuts) - 1 and np.array_equal(t.duration, np.diff(cuts))
    assert np.array_equal(t.min, np.minimum.reduceat(host_in, cuts[:-1])) and np.array_equal(t.max, np.maximum.reduceat(host_in, cuts[:-1]))
    assert np.abs(t.mean - np.add.reduceat(host_in, cuts[:-1]) / np.diff(cuts)).max() < 1e-9
    keep = (t.duration > 50) & (t.duration < 5000) & (t.max < T)
    assert [s.start for s in t.segments(host_in, mask=keep)] == [4_000, 6_000, 9_000, 140_000, 150_000]


@pytest.mark.parametrize("kind", ["grid_i16", "f64_pow2"])
def test_builtin_rules_ignore_the_flag(kind):
    dev_in, _ = inputs(kind)
    a = lambda_event_parser(T, on_device=True).parse(dev_in)
    b = lambda_event_parser(T).parse(dev_in)
    assert [(s.start, s.duration) for s in a] == [(s.start, s.duration) for s in b] == [(33_000, 100_500)]


def test_file_parse_never_builds_the_current():
    from pypore_amd.grid import Deferred, GridArray
    f = File(current=Deferred.from_counts(K, HEADER_Q, OFFSET), timestep=0.01)
    f.parse(lambda_event_parser(T, rules=short_rules(T), on_device=True))
    cur = raw_current(f)
    assert isinstance(cur, Deferred) and not cur.built
    g = File(current=np.asarray(GridArray.from_counts(K, HEADER_Q, OFFSET)), timestep=0.01)
    g.parse(lambda_event_parser(T, rules=short_rules(T)))
    assert [(e.start, e.end, e.duration) for e in f.events] == [(e.start, e.end, e.duration) for e in g.events] and f.n == 5
    assert all(isinstance(raw_current(e), Deferred) for e in f.events)
    assert not raw_current(f).built
    assert np.array_equal(f.events[1].current, g.events[1].current)      # (reading an event's current is what builds it)


def test_experiment_parse_keeps_file_order():
    from pypore_amd.grid import Deferred, GridArray
    shifted = np.concatenate((K[1_000:], K[:1_000]))
    files = [File(current=Deferred.from_counts(k, HEADER_Q, OFFSET), timestep=0.01) for k in (K, shifted, K)]
    exp = Experiment(files)
    exp.parse(event_detector=lambda_event_parser(T, rules=short_rules(T), on_device=True), segmenter=None, filter_params=None, verbose=False)
    host = [File(current=np.asarray(GridArray.from_counts(k, HEADER_Q, OFFSET)), timestep=0.01) for k in (K, shifted, K)]
    for h in host:
        h.parse(lambda_event_parser(T, rules=short_rules(T)))
    assert len(exp.files) == 3 and all(a is b for a, b in zip(exp.files, files))
    assert [[e.start for e in f.events] for f in exp.files] == [[e.start for e in h.events] for h in host]
    assert [e.start for e in exp.files[0].events] != [e.start for e in exp.files[1].events]
