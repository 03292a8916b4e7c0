"""ps_detect_pieces (engine.Context.detect_pieces): every piece a threshold cuts a trace into, with its statistics.

Oracles, both written out here.  Edges: below = float64(k) * q < threshold in numpy, an edge wherever it flips.  Statistics: the
integer oracle of test_range_stats_gpu.py restated -- k0 = the count of the piece's first sample, S1 = sum(k - k0) and S2 =
sum((k - k0)^2) exactly, then the library's final expressions in float64, none fused --
    my = S1 / n,  var = max(0, S2 / n - my * my),  mean = (k0 + my) q,  std = sqrt(var) q,  min / max = (k0 + min y) q, (k0 + max y) q.
Every comparison is == : on every edge and on the bits of all four columns.  The device sums integers, so there is no tolerance
anywhere in this file.  For every case range_stats on the pieces the call returned must give the call's own rows, bit for bit.

C is the kernels' chunk (4096 samples: one workgroup), a thread takes 16 samples, a wave 1024.  The one scan workgroup covers all
chunks of a call in a single launch (here up to 49)."""
import ctypes
import math

import numpy as np
import pytest

from pypore_amd import synth

pytestmark = pytest.mark.gpu

C = 4096
Q = synth.QUANTUM
HEADER_Q = 10.0 / 0.0005 / 20.0 / 32768.0 * 1.0001        # an .abf header's scale: not a power of two
HI, LO, KTHR = 3200, 640, 2880                             # 100 pA, 20 pA and the threshold 90 pA in counts of Q


def context():
    from pypore_amd import engine
    return engine.context(0)


def tensor(k, dtype, q, misalign=False):
    """The counts as a CUDA tensor: int16, or float32 on the grid q; misalign: a slice that starts one element into its
    allocation, so that its base is not 16-byte aligned."""
    import torch
    a = k.astype(np.int16) if dtype == "i16" else (k * q).astype(np.float32)
    if dtype == "f32":
        assert np.array_equal(a.astype(np.float64), k * q)              # on the grid, exactly
    if not misalign:
        t = torch.from_numpy(a).cuda()
        assert t.numel() == 0 or t.data_ptr() % 16 == 0
        return t
    whole = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
    t = whole[1:]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def oracle_edges(k, q, thr, offset_counts=0):
    below = (k + offset_counts).astype(np.float64) * q < thr
    cuts = np.flatnonzero(below[1:] != below[:-1]) + 1
    return np.concatenate(([0], cuts, [k.size])).astype(np.int64) if k.size else np.zeros(1, dtype=np.int64)


def oracle_stats_loop(k, edges, q, offset_counts=0):
    """Python integers, piece by piece."""
    out = np.empty((len(edges) - 1, 4), dtype=np.float64)
    for r, (a, z) in enumerate(zip(edges[:-1], edges[1:])):
        k0 = int(k[a]) + offset_counts
        y = [int(v) + offset_counts - k0 for v in k[a:z]]
        n, s1, s2 = int(z - a), sum(y), sum(v * v for v in y)
        assert abs(s1) < 2 ** 53 and s2 < 2 ** 63
        my = float(s1) / float(n)
        var = float(s2) / float(n) - my * my
        var = 0.0 if var < 0 else var
        out[r] = ((float(k0) + my) * q, math.sqrt(var) * q, float(k0 + min(y)) * q, float(k0 + max(y)) * q)
    return out


def oracle_stats(k, edges, q, offset_counts=0):
    """The same numbers for tables of many pieces: exact int64 sums per piece (|y| <= 65535 and n <= 200 000 here, so S2 < 2^50
    and every conversion to float64 is exact), then the same float64 expressions element by element."""
    a = edges[:-1]
    n = np.diff(edges)
    k0 = k[a] + offset_counts
    y = k + offset_counts - np.repeat(k0, n)
    assert np.abs(y).max() <= 65535 and k.size <= 200_000
    s1, s2 = np.add.reduceat(y, a), np.add.reduceat(y * y, a)
    mn, mx = np.minimum.reduceat(y, a), np.maximum.reduceat(y, a)
    dn = n.astype(np.float64)
    my = s1.astype(np.float64) / dn
    var = s2.astype(np.float64) / dn - my * my
    var = np.where(var < 0, 0.0, var)
    return np.stack([(k0.astype(np.float64) + my) * q, np.sqrt(var) * q, (k0 + mn).astype(np.float64) * q, (k0 + mx).astype(np.float64) * q], axis=1)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (bad[:5], got[bad[:5, 0]], want[bad[:5, 0]])


def check(k, thr, dtype="i16", q=Q, offset_counts=0, misalign=False, want_pieces=None):
    """One call against both oracles, and range_stats on its pieces against its rows.  Returns (edges, stats)."""
    ctx = context()
    x = tensor(k, dtype, q, misalign)
    off = offset_counts if dtype == "i16" else 0           # (float32 samples are absolute values)
    edges, stats = ctx.detect_pieces(x, q, thr, offset_counts=off)
    want_edges = oracle_edges(k, q, thr, off)
    assert edges.dtype == np.int64 and edges.shape == want_edges.shape, (edges.shape, want_edges.shape)
    bad = np.flatnonzero(edges != want_edges)
    assert bad.size == 0, (bad[:5], edges[bad[:5]], want_edges[bad[:5]])
    if want_pieces is not None:
        assert len(edges) - 1 == want_pieces
    want = oracle_stats(k, want_edges, q, off) if k.size else np.zeros((0, 4))
    same_bits(stats, want)
    if k.size:
        same_bits(ctx.range_stats(x, edges[:-1], edges[1:], q, offset_counts=off), stats)
    return edges, stats


def trace(n, edges, seed=1, noise=40):
    """HI from sample 0, the other level from every edge on, alternating; noise that stays on its side of the threshold."""
    side = np.zeros(n, dtype=np.int64)
    for e in edges:
        side[e:] ^= 1
    rng = np.random.default_rng(seed)
    return np.where(side == 0, HI, LO) + rng.integers(-noise, noise + 1, n)


THR = KTHR * Q - Q / 2                                      # between two counts


@pytest.fixture(scope="module")
def rails():
    """The shape of the range-statistics buffer: noisy dwells, a stretch alternating between the rails -32768 / 32767, a constant
    stretch with a sample of the other side before and behind it."""
    rng = np.random.default_rng(20241021)
    n = 70_000
    k = np.empty(n, dtype=np.int64)
    at = 0
    while at < n:
        m = int(rng.integers(150, 2500))
        k[at:at + m] = int(rng.integers(-20000, 20000))
        at += m
    k += np.rint(rng.normal(0.0, 300.0, n)).astype(np.int64)
    k[20_000:21_001] = np.where(np.arange(1001) % 2 == 0, -32768, 32767)
    k[30_003:30_600] = 12345
    k[30_002] = k[30_600] = -7
    return k


def test_the_two_oracles_agree():
    k = trace(3 * C + 5, [1, 17, 900, C - 1, C, 2 * C + 77, 3 * C + 4], seed=3)
    e = oracle_edges(k, Q, THR)
    assert e.tolist() == [0, 1, 17, 900, C - 1, C, 2 * C + 77, 3 * C + 4, 3 * C + 5]
    same_bits(oracle_stats(k, e, Q), oracle_stats_loop(k, e, Q))
    same_bits(oracle_stats(k, e, HEADER_Q, -1234), oracle_stats_loop(k, e, HEADER_Q, -1234))


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_shortest_traces(dtype):
    check(np.array([HI]), THR, dtype, want_pieces=1)
    check(np.array([LO]), THR, dtype, want_pieces=1)
    check(np.array([HI, HI + 3]), THR, dtype, want_pieces=1)
    check(np.array([HI, LO]), THR, dtype, want_pieces=2)
    check(np.array([LO, HI]), THR, dtype, want_pieces=2)
    ctx = context()
    edges, stats = ctx.detect_pieces(tensor(np.zeros(0, dtype=np.int64), dtype, Q), Q, THR)
    assert edges.tolist() == [0] and stats.shape == (0, 4)


CASES = {
    "one piece over every chunk": (3 * C + 5, []),
    "edges at 1 and n - 1": (3 * C + 5, [1, 3 * C + 4]),
    "edges round the chunk seam": (3 * C + 5, [C - 1, C, C + 1]),
    "edges round thread and wave seams": (3 * C + 5, [15, 16, 17, 31, 32, 1008, 1023, 1024, 1025, 2 * C - 16, 2 * C + 16]),
    "an edge exactly on every seam": (3 * C + 5, [C, 2 * C, 3 * C]),
    "mid-chunk to mid-chunk over two whole chunks": (4 * C + 100, [C // 2 + 3, 3 * C + C // 2 + 1]),
    "two seam-crossing pieces meet inside a chunk": (3 * C, [C - 100, C + 2000, 2 * C + 50]),
    "a piece from the first chunk to the last": (5 * C + 7, [5, 5 * C + 3]),
    "the trace ends on a seam": (2 * C, [C + 5]),
}


@pytest.mark.parametrize("dtype", ["i16", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_edges_at_the_seams(name, dtype):
    n, cuts = CASES[name]
    check(trace(n, cuts, seed=len(name)), THR, dtype, want_pieces=len(cuts) + 1)


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_every_sample_its_own_piece(dtype):
    n = 3 * C + 5
    k = np.where(np.arange(n) % 2 == 0, HI, LO) + np.arange(n) % 7
    check(k, THR, dtype, want_pieces=n)


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_more_pieces_than_sixteen_bits(dtype):
    """200 000 samples in pieces of 1 .. 4: the piece index passes 2^16 and the scan covers 49 chunks."""
    rng = np.random.default_rng(7)
    cuts = np.cumsum(rng.integers(1, 5, 90_000))
    cuts = cuts[cuts < 200_000]
    edges, _ = check(trace(200_000, cuts.tolist(), seed=8), THR, dtype)
    assert len(edges) - 1 > 70_000


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_rails_and_constant_stretch(rails, dtype):
    """Everything below the threshold: ONE piece that holds the alternation between the rails -- y = +-65535, the largest sum of
    squares.  Threshold 0: the alternation is a piece per sample and the constant stretch a piece of its own with std == 0."""
    check(rails, 40000 * Q, dtype, want_pieces=1)
    edges, stats = check(rails, 0.0, dtype)
    p = int(np.searchsorted(edges, 30_003))
    assert edges[p] == 30_003 and edges[p + 1] == 30_600 and stats[p, 1] == 0.0 and stats[p, 2] == stats[p, 3] == 12345 * Q
    assert np.isin(np.arange(20_001, 21_001), edges).all()


def test_offset_counts_on_a_header_scale():
    k = trace(3 * C + 5, [3, 700, C, C + 9, 2 * C + 1234], seed=11)
    off = -1234
    thr = (KTHR + off) * HEADER_Q - HEADER_Q / 2
    check(k, thr, "i16", HEADER_Q, offset_counts=off, want_pieces=6)
    check(k, thr, "i16", HEADER_Q, offset_counts=off, misalign=True, want_pieces=6)


@pytest.mark.parametrize("dtype, q", [("i16", Q), ("f32", Q), ("i16", HEADER_Q)])
def test_threshold_on_a_samples_value(dtype, q):
    """The predicate is strict: a sample whose value IS the threshold is not below it."""
    k = np.array([KTHR + 1, KTHR, KTHR, KTHR - 1, KTHR, KTHR - 1, KTHR - 2, KTHR + 5, KTHR] * 500)
    thr = float(KTHR) * q                                     # the very product the kernel forms
    edges, _ = check(k, thr, dtype, q)
    assert edges[:6].tolist() == [0, 3, 4, 5, 7, 12]


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_unaligned_base(dtype):
    n, cuts = CASES["edges round thread and wave seams"]
    a = check(trace(n, cuts + [C + 3, 2 * C - 1], seed=5), THR, dtype, misalign=True)
    b = check(trace(n, cuts + [C + 3, 2 * C - 1], seed=5), THR, dtype)
    assert np.array_equal(a[0], b[0])
    same_bits(a[1], b[1])


def test_capacity_one_too_small_and_retry(monkeypatch):
    import torch
    from pypore_amd import _lib, engine
    ctx = context()
    k = trace(3 * C + 5, [10, 20, C, C + 1, 2 * C + 100, 3 * C], seed=2)
    x = tensor(k, "i16", Q)
    want_edges = oracle_edges(k, Q, THR)
    P = len(want_edges) - 1
    fmt = engine._fmt(x, Q, 0)
    cnt = ctypes.c_int64(-1)

    def raw(cap):
        edges = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
        stats = torch.zeros((max(cap, 1), 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = ctx.L.ps_detect_pieces(ctx.handle, ctypes.c_void_p(x.data_ptr()), ctypes.byref(fmt), x.numel(), THR,
                                    ctypes.c_void_p(edges.data_ptr()), ctypes.c_void_p(stats.data_ptr()), cap, ctypes.byref(cnt))
        return rc, edges.cpu().numpy(), stats.cpu().numpy()

    rc, _, _ = raw(P - 1)
    assert rc == _lib.PS_ERR_CAPACITY and cnt.value == P
    rc, _, _ = raw(0)
    assert rc == _lib.PS_ERR_CAPACITY and cnt.value == P
    rc, edges, stats = raw(P)                                  # the context is usable, and exactly P is enough
    assert rc == _lib.PS_OK and cnt.value == P and np.array_equal(edges, want_edges)
    same_bits(stats, oracle_stats(k, want_edges, Q))
    monkeypatch.setattr(engine, "PIECE_CAP", 3)                # the binding starts too small and retries with the reported count
    edges, stats = ctx.detect_pieces(x, Q, THR)
    assert np.array_equal(edges, want_edges)
    same_bits(stats, oracle_stats(k, want_edges, Q))


def test_refusals_leave_the_context_usable():
    import torch
    from pypore_amd import _lib
    ctx = context()
    k = trace(2 * C + 3, [100, C + 1], seed=4)
    with pytest.raises(ValueError):                            # float64: not a type the detector takes
        ctx.detect_pieces(torch.from_numpy(k * Q).cuda(), Q, THR)
    x64 = torch.from_numpy(k * Q).cuda()
    fmt = _lib.SampleFormat(_lib.PS_DTYPE_F64, 0, Q)
    cnt = ctypes.c_int64(-1)
    edges = torch.zeros(11, dtype=torch.int64, device="cuda")
    stats = torch.zeros((10, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.L.ps_detect_pieces(ctx.handle, ctypes.c_void_p(x64.data_ptr()), ctypes.byref(fmt), x64.numel(), THR,
                                ctypes.c_void_p(edges.data_ptr()), ctypes.c_void_p(stats.data_ptr()), 10, ctypes.byref(cnt))
    assert rc == _lib.PS_ERR_ARG and cnt.value == 0 and b"dtype" in ctx.L.ps_last_error(ctx.handle)
    check(k, THR, "i16", want_pieces=3)
    off = (k * Q).astype(np.float32)
    off[C + 7] += np.float32(Q / 4)                            # one sample between two counts
    with pytest.raises(ValueError, match="not an integer multiple of quantum"):
        ctx.detect_pieces(torch.from_numpy(off).cuda(), Q, THR)
    check(k, THR, "f32", want_pieces=3)
    x = tensor(k, "i16", Q)                                    # a negative capacity, through the ABI
    f16 = _lib.SampleFormat(_lib.PS_DTYPE_I16, 0, Q)
    rc = ctx.L.ps_detect_pieces(ctx.handle, ctypes.c_void_p(x.data_ptr()), ctypes.byref(f16), x.numel(), THR,
                                ctypes.c_void_p(edges.data_ptr()), ctypes.c_void_p(stats.data_ptr()), -1, ctypes.byref(cnt))
    assert rc == _lib.PS_ERR_ARG
    check(k, THR, "i16", want_pieces=3)


def test_two_calls_give_the_same_bits(rails):
    ctx = context()
    x = tensor(rails, "i16", Q)
    a = ctx.detect_pieces(x, Q, 0.0)
    small = ctx.detect_pieces(tensor(trace(100, [50]), "i16", Q), Q, THR)       # (another call in between, on other scratch contents)
    assert small[0].tolist() == [0, 50, 100]
    b = ctx.detect_pieces(x, Q, 0.0)
    assert np.array_equal(a[0], b[0])
    same_bits(a[1], b[1])
