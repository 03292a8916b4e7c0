"""High-precision reference for Event.filter and the host restatement of the filter kernels' launch geometry.

filtfilt_ld(x, b, a) is scipy.signal.filtfilt(b, a, x) (method "pad", padtype "odd", padlen = 3 * max(len(a), len(b)))
in numpy.longdouble (64-bit mantissa on x86: eleven bits more than every float64 route under test): odd extension,
zi from (I - A) zi = B by Gaussian elimination in long double, direct form II transposed forward, the same over the
reversed intermediate, the extension dropped.  A Python loop per sample: keep n <= MAX_LD.  No scipy.

The geometry functions restate the host formulas of csrc/poreseg.hip (ps_filter_bessel, filter_order_n) and the constants
of csrc/seg_filter.hpp, so that a test can assert that its case sits on the seam it names without a GPU:

    order 1:  wo = 4 tan(pi wn / 2), alpha = (4 - wo) / (4 + wo).  Fused route when option filter_fused is set, 0 < alpha < 1
              and h_req = ceil(60 ln 2 / -ln alpha) <= 1024: H = max(64, h_req rounded up to 64), T = 4096 - 2 H,
              tiles = ceil((n + 12) / T).  Otherwise the three-pass scan: n_chunks = ceil((n + 12) / 4096),
              lead = 4096 n_chunks - (n + 12), per = ceil(n_chunks / 1024) chunks per thread of the carry kernel, loaded
              eight per trip.
    order N:  state matrix A of the direct form (first column -a[1:], ones above the diagonal); H = the first multiple of
              64 (<= 8192) with ||A^H||_inf <= 8.47e-22, none: the library refuses; S = max(1024, 4 H) outputs per thread,
              m = n + 6 (N + 1) elements, nseg = ceil(m / S) threads in workgroups of 64.

The case lists of tests/test_filter_edges.py and tests/golden/make_golden_filter_edges.py are built here from those
functions, every case with the input it is generated from (make_input())."""
import math

import numpy as np

import oracle
from pypore_amd import synth

LD = np.longdouble
MAX_LD = 200_000                     # longest input the long-double loop is asked for
CHUNK = 4096                         # FILT_CHUNK = FILT_NT * FILT_PER
PAD1 = 6                             # FILT_PAD: padlen of a first-order section
TOL = 1e-11                          # the suite's bound on a filtered current, relative to max |y| (tests/test_filter.py)
ROUTE_TOL = 2e-14                    # fused against three-pass on the same input (tests/test_filter.py)
ORACLE_TOL = 1e-10                   # the large order-1 traces against the fp64 oracle (tests/test_filter.py)


# ---- the reference ------------------------------------------------------------------------------------------------
def lfilter_zi_ld(b, a):
    """scipy.signal.lfilter_zi in long double: the state of the delays for a unit step, (I - A) zi = B."""
    order = len(a) - 1
    M = [[LD(0)] * (order + 1) for _ in range(order)]
    for r in range(order):
        for c in range(order):
            A_rc = (-a[r + 1] if c == 0 else LD(0)) + (LD(1) if c == r + 1 else LD(0))
            M[r][c] = (LD(1) if r == c else LD(0)) - A_rc
        M[r][order] = b[r + 1] - a[r + 1] * b[0]
    for c in range(order):
        piv = max(range(c, order), key=lambda r: abs(M[r][c]))
        M[c], M[piv] = M[piv], M[c]
        for r in range(order):
            if r != c:
                g = M[r][c] / M[c][c]
                for k in range(c, order + 1):
                    M[r][k] = M[r][k] - g * M[c][k]
    return [M[r][order] / M[r][r] for r in range(order)]


def _lfilter_ld(b, a, x, z):
    """Direct form II transposed over the list x from the state z (lists of long doubles); returns the output list."""
    order = len(a) - 1
    b0 = b[0]
    y = [None] * len(x)
    if order == 1:
        z0, b1, a1 = z[0], b[1], a[1]
        for i, xi in enumerate(x):
            yi = z0 + b0 * xi
            z0 = b1 * xi - a1 * yi
            y[i] = yi
        return y
    z = list(z)
    last = order - 1
    bl, al = b[order], a[order]
    mid = [(k, b[k + 1], a[k + 1]) for k in range(last)]
    for i, xi in enumerate(x):
        yi = z[0] + b0 * xi
        for k, bk, ak in mid:
            z[k] = z[k + 1] + bk * xi - ak * yi
        z[last] = bl * xi - al * yi
        y[i] = yi
    return y


def filtfilt_ld(x, b, a):
    """scipy.signal.filtfilt(b, a, x) in numpy.longdouble; returns a long-double array of len(x)."""
    a = np.asarray(a, dtype=LD)
    b = np.asarray(b, dtype=LD) / a[0]
    a = a / a[0]
    order = max(len(a), len(b)) - 1
    a = [LD(v) for v in a] + [LD(0)] * (order + 1 - len(a))
    b = [LD(v) for v in b] + [LD(0)] * (order + 1 - len(b))
    padlen = 3 * (order + 1)
    x = np.asarray(x, dtype=LD)
    if x.ndim != 1 or x.size <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    ext = np.concatenate((2 * x[0] - x[padlen:0:-1], x, 2 * x[-1] - x[-2:-padlen - 2:-1]))
    zi = lfilter_zi_ld(b, a)
    ext = list(ext)
    fwd = _lfilter_ld(b, a, ext, [v * ext[0] for v in zi])
    fwd.reverse()
    bwd = _lfilter_ld(b, a, fwd, [v * fwd[0] for v in zi])
    bwd.reverse()
    return np.array(bwd[padlen:len(bwd) - padlen], dtype=LD)


def bessel_filtfilt_ld(x, cutoff, second, order):
    """Event.filter in long double, with the oracle's (b, a) (pinned to scipy's by tests/test_filter.py)."""
    b, a = oracle.bessel_ba(int(order), cutoff / (second / 2.0))
    return filtfilt_ld(x, b, a)


def rel_err(got, ref):
    """max |got - ref| / max |ref| in long double, as a float."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / np.max(np.abs(ref)))


def bound_from(err_ref):
    """What a device result may differ from the long-double reference by, given the fp64 oracle's own distance from it."""
    return max(TOL, 4.0 * err_ref)


# ---- host restatement of the launch geometry -------------------------------------------------------------------------
def order1_geometry(n, cutoff, second, fused=1):
    """ps_filter_bessel, order 1: dict(route, alpha, h_req, H, T, tiles, last_owns, total, n_chunks, lead, per, trips)."""
    wn = cutoff / (second / 2.0)
    wo = 4.0 * math.tan(math.pi * wn / 2.0)
    alpha = -((wo - 4.0) / (wo + 4.0))
    total = n + 2 * PAD1
    g = dict(route="scan", alpha=alpha, h_req=None, H=0, T=0, tiles=0, last_owns=0, total=total)
    if 0.0 < alpha < 1.0:
        g["h_req"] = math.ceil(60.0 * math.log(2.0) / -math.log(alpha))
        if fused and g["h_req"] <= 1024.0:
            g["H"] = max(64, (int(g["h_req"]) + 63) // 64 * 64)
    if g["H"]:
        g["route"] = "fused"
        g["T"] = CHUNK - 2 * g["H"]
        g["tiles"] = (total + g["T"] - 1) // g["T"]
        g["last_owns"] = total - (g["tiles"] - 1) * g["T"]           # elements of the extended sequence the last tile writes
    g["n_chunks"] = (total + CHUNK - 1) // CHUNK
    g["lead"] = g["n_chunks"] * CHUNK - total
    g["per"] = (g["n_chunks"] + 1023) // 1024
    g["trips"] = (g["per"] + 7) // 8
    return g


_HALOS = {}


def state_matrix(a):
    order = len(a) - 1
    A = np.zeros((order, order))
    for r in range(order):
        A[r, 0] = -a[r + 1]
        if r + 1 < order:
            A[r, r + 1] += 1.0
    return A


def halo_of(order, cutoff, second):
    """filter_order_n's halo: the first multiple of 64 up to 8192 with ||A^h||_inf <= 8.47e-22; 0: the library refuses."""
    key = (int(order), float(cutoff), float(second))
    if key not in _HALOS:
        _, a = oracle.bessel_ba(int(order), cutoff / (second / 2.0))
        r = range(int(order))

        def mul(X, Y):                       # the library's loop, in its order: no BLAS blocking, no fused multiply-add
            Z = [[0.0] * len(r) for _ in r]
            for i in r:
                for j in r:
                    for k in r:
                        Z[i][j] += X[i][k] * Y[k][j]
            return Z

        A64 = state_matrix(a).tolist()
        for _ in range(6):
            A64 = mul(A64, A64)
        P, H = A64, 0
        for h in range(64, 8192 + 1, 64):
            if max(sum(abs(v) for v in row) for row in P) <= 8.47e-22:
                H = h
                break
            P = mul(P, A64)
        _HALOS[key] = H
    return _HALOS[key]


def halo_geometry(n, order, cutoff, second):
    """filter_order_n: dict(H, S, pad, m, nseg, groups); H == 0: refused."""
    H = halo_of(order, cutoff, second)
    pad = 3 * (order + 1)
    S = max(1024, 4 * H)
    m = n + 2 * pad
    nseg = (m + S - 1) // S
    return dict(H=H, S=S, pad=pad, m=m, nseg=nseg, groups=(nseg + 63) // 64)


def search_cutoff(order, second, want):
    """The first cutoff of a fixed descending ladder (1000 Hz down in steps of 2 %) whose halo satisfies want(H)."""
    c = 1000.0
    while c > 1.0:
        if want(halo_of(order, round(c, 1), second)):
            return round(c, 1)
        c *= 0.98
    raise AssertionError("no cutoff found")


# ---- inputs -----------------------------------------------------------------------------------------------------------
def make_input(gen):
    """(float64 pA, integer counts or None) of a generator spec: kind grid | offgrid, n, seed, optional slice
    [start, length] of the generated trace, optional offset (counts added to a grid trace)."""
    n = gen["n"]
    lo, hi = (2, 4) if n < 100 else (300, 5000)
    if gen["kind"] == "grid":
        k = synth.random_dwell_counts(n, gen["seed"], lo, hi).astype(np.int64)
        x = None
    else:
        k = None
        x = synth.offgrid_trace(n, gen["seed"], sigma=1.0, lo=lo, hi=hi)
    if "slice" in gen:
        s, ln = gen["slice"]
        k = None if k is None else k[s:s + ln]
        x = None if x is None else x[s:s + ln]
    if k is not None:
        x = (k + gen.get("offset", 0)).astype(np.float64) * synth.QUANTUM
    return x, k


def kind_of(dtype):
    return "offgrid" if dtype == "f64" else "grid"


def key_of(order, cutoff, second, gen):
    """The manifest key of a (filter, input) pair; int16 and float32 share a grid input."""
    k = "O%d_%gHz_%gHz_%s_n%d_s%d" % (order, cutoff, second, gen["kind"], gen["n"], gen["seed"])
    if "slice" in gen:
        k += "_at%d+%d" % tuple(gen["slice"])
    if gen.get("offset"):
        k += "_off%d" % gen["offset"]
    return k


def gen_for(dtype, n, seed=17):
    return dict(kind=kind_of(dtype), n=int(n), seed=seed)


# ---- the cases --------------------------------------------------------------------------------------------------------
SECOND = 1.0e5
DTYPES = ("i16", "f32", "f64")
FUSED_HALOS = {650.0: 1024, 700.0: 960, 1200.0: 576, 2000.0: 384, 5000.0: 192, 24000.0: 64}      # at 100 kHz
NEG_POLE = [(25000.0, 1.0e5), (26000.0, 1.0e5), (30000.0, 1.0e5), (45000.0, 1.0e5), (49000.0, 1.0e5), (15000.0, 5.0e4)]
NEG_POLE_N = (7, CHUNK - 12, 3 * CHUNK + 5)                  # the shortest input, exactly one chunk, several chunks
SCAN_CUTOFFS = [(2000.0, 0), (600.0, 1), (100.0, 1), (5.0, 1)]      # (cutoff, option filter_fused): the scan runs in each
SCAN_CHUNKS = (1, 2, 1023, 1024, 1025, 2049)
BIG_N = 34_000_000                                           # 8 301 chunks: 9 per thread of the carry kernel, two trips
HALO_FILTERS = [(2, 5000.0), (3, 2000.0), (5, 2000.0), (8, 10000.0)]


def fused_lengths(H, T):
    """(n, what) of the fused seams: n + 12 at k T - 1, k T, k T + 1 (the last tile owns T - 1, T, 1 elements) for
    k = 1, 2, 5, and inputs shorter than a halo / a tile."""
    out = []
    for k in (1, 2, 5):
        for d in (-1, 0, 1):
            out.append((k * T + d - 12, "%dT%+d" % (k, d)))
    out += [(7, "n7"), (8, "n8"), (H - 1, "H-1"), (H, "H"), (H + 1, "H+1"), (T - 13, "T-13"), (T - 12, "T-12")]
    seen, uniq = set(), []
    for n, what in out:
        if n not in seen:
            seen.add(n)
            uniq.append((n, what))
    return uniq


def fused_cases():
    cases = []
    for cutoff, H in FUSED_HALOS.items():
        T = CHUNK - 2 * H
        for n, what in fused_lengths(H, T):
            for dt in DTYPES:
                cases.append(dict(id="%gHz-%s-%s" % (cutoff, what, dt), order=1, cutoff=cutoff, second=SECOND, n=n, what=what,
                                  dtype=dt, H=H, T=T, gen=gen_for(dt, n)))
    return cases


def straddle_cases():
    """640 Hz (h_req > 1024: the scan) and 650 Hz (H = 1024) on the same input."""
    return [dict(id="640-650Hz-%s" % dt, order=1, cutoffs=(640.0, 650.0), second=SECOND, n=3 * 2048 + 77, dtype=dt,
                 gen=gen_for(dt, 3 * 2048 + 77)) for dt in DTYPES]


def negpole_cases():
    return [dict(id="%gHz@%gHz-n%d-%s" % (cutoff, second, n, dt), order=1, cutoff=cutoff, second=second, n=n, dtype=dt,
                 gen=gen_for(dt, n))
            for cutoff, second in NEG_POLE for n in NEG_POLE_N for dt in DTYPES]


def scan_lead_cases():
    """n + 12 = 4096 k - 1, 4096 k, 4096 k + 1: lead 1, 0, 4095."""
    cases = []
    for cutoff, fused in SCAN_CUTOFFS:
        for k in (1, 2, 3):
            for d, lead in ((-1, 1), (0, 0), (1, CHUNK - 1)):
                n = CHUNK * k + d - 12
                for dt in DTYPES:
                    cases.append(dict(id="%gHz-%dC%+d-%s" % (cutoff, k, d, dt), order=1, cutoff=cutoff, second=SECOND, n=n,
                                      fused=fused, lead=lead, n_chunks=k + (d == 1), dtype=dt, gen=gen_for(dt, n)))
    return cases


def scan_chunk_cases():
    """n_chunks across the carry kernel's 1 -> 2 chunks per thread; beyond MAX_LD the fp64 oracle is the reference, at the
    bound of a MAX_LD prefix of the same input."""
    cases = []
    for cutoff, fused in ((2000.0, 0), (100.0, 1)):
        for nc in SCAN_CHUNKS:
            n = CHUNK * nc - 12 - 7
            for dt in ("i16", "f64"):
                cases.append(dict(id="%gHz-%dchunks-%s" % (cutoff, nc, dt), order=1, cutoff=cutoff, second=SECOND, n=n, fused=fused,
                                  n_chunks=nc, per=(nc + 1023) // 1024, lead=7, dtype=dt, gen=gen_for(dt, n, seed=23)))
    return cases


_SEARCHED = {}


def halo_filters():
    """HALO_FILTERS and one slow filter of order 5 whose halo exceeds 4096 (found by search_cutoff)."""
    if "slow" not in _SEARCHED:
        _SEARCHED["slow"] = search_cutoff(5, SECOND, lambda H: 4096 < H <= 8192)
    return HALO_FILTERS + [(5, _SEARCHED["slow"])]


def refused_filter():
    """An order-3 filter so slow that no halo up to 8192 forgets its state: the library refuses it.  (Order 3: the powers of
    the state matrix are still computed cleanly there; at order 8 the norm stalls in rounding noise from about 1 kHz down,
    and the library refuses earlier than the poles alone would make it.)"""
    if "refused" not in _SEARCHED:
        _SEARCHED["refused"] = search_cutoff(3, SECOND, lambda H: H == 0)
    return 3, _SEARCHED["refused"]


def halo_lengths(S, H):
    """(m, what): segment seams, workgroup seams, and the tail case hi < m <= hi + H of the last-but-one segment (its
    backward pass starts exactly at the end of the sequence): m = 2 S + H is its last length, 2 S + H + 1 the first beyond."""
    return [(S - 1, "S-1"), (S, "S"), (S + 1, "S+1"), (2 * S + 1, "2S+1"), (2 * S + H, "2S+H"), (2 * S + H + 1, "2S+H+1"),
            (64 * S - 1, "64S-1"), (64 * S, "64S"), (64 * S + 1, "64S+1"), (65 * S + 3, "65S+3")]


def halo_cases():
    cases = []
    for order, cutoff in halo_filters():
        g = halo_geometry(1000, order, cutoff, SECOND)
        for m, what in halo_lengths(g["S"], g["H"]):
            n = m - 2 * g["pad"]
            for dt in DTYPES:
                cases.append(dict(id="O%d-%gHz-%s-%s" % (order, cutoff, what, dt), order=order, cutoff=cutoff, second=SECOND, n=n,
                                  what=what, dtype=dt, H=g["H"], S=g["S"], m=m, gen=gen_for(dt, n, seed=29)))
    return cases


# the batch entry: (name, order, cutoff, route)
BATCH_ROUTES = [("fused2k", 1, 2000.0, "fused"), ("scan100", 1, 100.0, "scan"), ("scan30k", 1, 30000.0, "scan"),
                ("haloO3", 3, 2000.0, "halo"), ("haloO8", 8, 10000.0, "halo")]
BATCH_TRACE_N = 1_200_000
BATCH_OFFSET = 37                        # offset_counts of the int16 batches
BATCH_CHECKED = (100_001, 50_001)        # (odd start, length) of the event that is also compared with the long-double reference


def batch_gen(dtype, sliced=True):
    g = dict(kind=kind_of(dtype), n=BATCH_TRACE_N, seed=31)
    if sliced:
        g["slice"] = list(BATCH_CHECKED)
    if dtype == "i16":
        g["offset"] = BATCH_OFFSET
    return g


def batch_events(order, n_ev, arrangement):
    """(starts, lengths) of a batch on the BATCH_TRACE_N trace: lengths from padlen + 1 to 3e5, odd starts, two events of a
    batch of 40 overlapping; arrangement ascending | descending | shuffled by length."""
    padlen = 3 * (order + 1)
    if n_ev == 1:
        return np.array([BATCH_CHECKED[0]]), np.array([BATCH_CHECKED[1]])
    if n_ev == 2:
        st, ln = np.array([BATCH_CHECKED[0], 7]), np.array([BATCH_CHECKED[1], padlen + 1])
    else:
        rng = np.random.default_rng(41)
        ln = np.exp(rng.uniform(np.log(padlen + 2), np.log(60_000), n_ev)).astype(np.int64)
        ln[:5] = BATCH_CHECKED[1], 300_000, padlen + 1, CHUNK - 12, 4 * CHUNK + 1 - 12
        st = rng.integers(0, (BATCH_TRACE_N - ln) // 2) * 2 + 1
        st[0], st[1] = BATCH_CHECKED[0], BATCH_CHECKED[0] + 20_000       # overlapping
    by = np.argsort(ln, kind="stable")
    if arrangement == "descending":
        by = by[::-1]
    elif arrangement == "shuffled":
        by = np.random.default_rng(43).permutation(len(ln))
    return st[by], ln[by]


def manifest_inputs():
    """{key: dict(order, cutoff, second, gen)} of every (filter, input) pair whose fp64 oracle is measured against the
    long-double reference (on the first MAX_LD samples of an input longer than that)."""
    out = {}

    def add(order, cutoff, second, gen):
        out.setdefault(key_of(order, cutoff, second, gen), dict(order=order, cutoff=cutoff, second=second, gen=gen))

    for c in fused_cases() + negpole_cases() + scan_lead_cases() + scan_chunk_cases() + halo_cases():
        add(c["order"], c["cutoff"], c["second"], c["gen"])
    for c in straddle_cases():
        for cutoff in c["cutoffs"]:
            add(1, cutoff, c["second"], c["gen"])
    for _, order, cutoff, _ in BATCH_ROUTES:
        for dt in DTYPES:
            add(order, cutoff, SECOND, batch_gen(dt))
    return out


def measure(entry):
    """err_ref of a manifest entry: max |oracle_fp64 - long double| / max |long double| (on the MAX_LD prefix of a longer
    input)."""
    x, _ = make_input(entry["gen"])
    x = x[:MAX_LD]
    ld = bessel_filtfilt_ld(x, entry["cutoff"], entry["second"], entry["order"])
    return rel_err(oracle.bessel_filtfilt(x, entry["cutoff"], entry["second"], entry["order"]), ld)
