"""lambda_event_parser's rule evaluation over a piece table and PieceTable itself, on a hand-made table -- no GPU, no library."""
import numpy as np
import pytest

from pypore_amd import parsers
from pypore_amd.parsers import PieceTable, lambda_event_parser

# five pieces of a 20-sample trace; statistics that are NOT those of the samples (so a test can tell where a number came from)
EDGES = [0, 3, 4, 10, 15, 20]
STATS = np.array([[10.0, 1.0, 8.0, 12.0],
                  [50.0, 0.0, 50.0, 50.0],
                  [11.0, 2.0, 7.0, 13.0],
                  [52.0, 3.0, 40.0, 60.0],
                  [9.0, 0.5, 8.5, 9.5]])
X = np.arange(20, dtype=np.float64) * 100.0


def test_table_arrays():
    t = PieceTable(EDGES, STATS)
    assert len(t) == 5
    for name, want in (("start", [0, 3, 4, 10, 15]), ("end", [3, 4, 10, 15, 20]), ("duration", [3, 1, 6, 5, 5]), ("n", [3, 1, 6, 5, 5])):
        got = getattr(t, name)
        assert got.dtype == np.int64 and got.tolist() == want, name
    for j, name in enumerate(("mean", "std", "min", "max")):
        got = getattr(t, name)
        assert got.dtype == np.float64 and np.array_equal(got, STATS[:, j]), name
    empty = PieceTable([0], np.zeros((0, 4)))
    assert len(empty) == 0 and empty.segments(X[:0]) == []
    with pytest.raises(ValueError):
        PieceTable([0, 3], STATS)


def test_offset_goes_to_mean_min_max_and_not_to_std():
    t = PieceTable(EDGES, STATS, offset=-2.5)
    assert np.array_equal(t.mean, STATS[:, 0] + -2.5) and np.array_equal(t.min, STATS[:, 2] + -2.5)
    assert np.array_equal(t.max, STATS[:, 3] + -2.5) and np.array_equal(t.std, STATS[:, 1])
    assert np.array_equal(PieceTable(EDGES, STATS, offset=0.0).stats, STATS)


def test_segments_are_slices_with_the_tables_rows():
    t = PieceTable(EDGES, STATS)
    segs = t.segments(X)
    assert [(s.start, s.duration, s.n, s.end) for s in segs] == [(0, 3, 3, 3), (3, 1, 1, 4), (4, 6, 6, 10), (10, 5, 5, 15), (15, 5, 5, 20)]
    for p, s in enumerate(segs):
        assert np.shares_memory(s.current, X) and np.array_equal(s.current, X[EDGES[p]:EDGES[p + 1]])
        assert (s.mean, s.std, s.min, s.max) == tuple(STATS[p])          # the rows, not numpy over the samples
    some = t.segments(X, mask=t.duration >= 5)
    assert [s.start for s in some] == [4, 10, 15] and [s.max for s in some] == [13.0, 60.0, 9.5]
    assert all(np.shares_memory(s.current, X) for s in some)
    assert t.segments(X, mask=np.zeros(5, dtype=bool)) == []


def test_rules_keep_order_and_see_the_slice():
    t = PieceTable(EDGES, STATS)
    seen = []

    def reads_current(ev):
        seen.append((ev.start, ev.current.tolist()))
        return ev.current[0] >= 400.0

    kept = parsers._apply_rules(t.segments(X), [lambda ev: ev.duration > 1, lambda ev: ev.max < 20, reads_current])
    assert [s.start for s in kept] == [4, 15]
    # each rule is called per piece, in order, and stops at the first that refuses: the last rule saw the pieces the first two kept
    assert seen == [(0, X[0:3].tolist()), (4, X[4:10].tolist()), (15, X[15:20].tolist())]
    assert parsers._apply_rules(t.segments(X), [lambda ev: False]) == []
    assert [s.start for s in parsers._apply_rules(t.segments(X), [])] == [0, 3, 4, 10, 15]


def test_host_table_restates_the_host_route():
    x = np.array([100.0, 101.0, 20.0, 21.0, 19.0, 100.0, 20.0])
    t = parsers._host_table(x, 90)
    assert t.edges.tolist() == [0, 2, 5, 6, 7]
    for p, (a, z) in enumerate(zip(t.start, t.end)):
        assert t.min[p] == x[a:z].min() and t.max[p] == x[a:z].max()
        assert abs(t.mean[p] - x[a:z].mean()) < 1e-12 and abs(t.std[p] - x[a:z].std()) < 1e-12
    assert len(parsers._host_table(x[:0], 90)) == 0


def test_flag_stays_out_of_the_json():
    rules = [lambda ev: ev.duration > 1]
    p = lambda_event_parser(threshold=75, rules=rules, on_device=True)
    assert p._on_device is True and p._builtin is False and p._device_route
    d = p.to_dict()
    assert d == {"threshold": 75, "name": "lambda_event_parser"}
    assert "on_device" not in p.to_json() and "_on_device" not in p.to_json()
    q = lambda_event_parser.from_json(p.to_json())
    assert isinstance(q, lambda_event_parser) and q.threshold == 75 and q._on_device is False and q._builtin
    # the default: off, and a host-rule parser is not a device route
    h = lambda_event_parser(threshold=75, rules=rules)
    assert h._on_device is False and not h._device_route and lambda_event_parser()._device_route


def test_default_stays_on_the_host():
    x = np.array([100.0, 101.0, 20.0, 21.0, 19.0, 100.0, 20.0])
    got = lambda_event_parser(90, rules=[lambda ev: ev.max < 90]).parse(x)          # (no GPU is touched: this test has none)
    assert [(s.start, s.duration) for s in got] == [(2, 3), (6, 1)]
