"""numpy restatement of the reference's two state parsers (parsers.py:572-679) in our own words: what their parse()
returns, as (start, end) spans.  tests/test_state_parsers_host.py holds it against goldens recorded from the reference."""
import numpy as np

EMPTY = np.zeros((0, 2), dtype=np.int32)


def snakebase_spans(x, threshold=1.5):
    """Spans between the places where neighbouring samples differ by less than 1e-3: the first such place to the second,
    the third to the fourth, ...; an odd one out reaches to the last difference.  `threshold` takes no part (the
    reference computes with it and discards the result)."""
    x = np.asarray(x, dtype=np.float64)
    if x.size < 2:
        return EMPTY
    with np.errstate(invalid="ignore"):
        low = np.flatnonzero(np.abs(x[1:] - x[:-1]) < 1e-3)
    if low.size % 2:
        low = np.append(low, x.size - 1)
    return low.reshape(-1, 2).astype(np.int32)


def bessel_filtfilt(x, cutoff_freq, sampling_freq):
    """y of FilterDerivativeSegmenter: scipy's first-order Bessel low-pass, forward and backward (ValueError for n <= 6)."""
    from scipy import signal
    b, a = signal.bessel(1, cutoff_freq / (sampling_freq / 2.), btype='low', analog=0, output='ba')
    return signal.filtfilt(b, a, np.array(x, dtype=np.float64))


def _pairs(y, low_threshold):
    """(deriv, pairs): the absolute derivative and the edges of its blocks above low_threshold, paired in order."""
    d = np.abs(y[1:] - y[:-1])
    above = d > low_threshold
    tics = np.flatnonzero(above[1:] != above[:-1]) + 1
    return d, tics[:tics.size // 2 * 2].reshape(-1, 2)


def _first_counted(high_threshold):
    """The least index an argmax must have to exceed high_threshold."""
    if high_threshold < 0:
        return 0
    return int(min(np.floor(high_threshold), 2.0 ** 31)) + 1


def filter_derivative_spans_from_y(y, low_threshold=1, high_threshold=2):
    """Spans from the filtered current: the stretches outside the kept pairs.  A pair is kept when the first maximum of the
    derivative inside it lies at an index above high_threshold, i.e. when the part from index floor(high_threshold) + 1 on
    holds a value strictly above everything before it."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    if n == 0:
        return EMPTY
    if n < 3:
        return np.array([[0, n]], dtype=np.int32)
    d, pairs = _pairs(y, low_threshold)
    h1 = _first_counted(high_threshold)
    edges = [0]
    for s, t in pairs.tolist():
        left, right = d[s:s + h1], d[min(s + h1, t):t]
        if right.size and (not left.size or right.max() > left.max()):
            edges += [s, t]
    return np.array(edges + [n], dtype=np.int32).reshape(-1, 2)


def filter_derivative_spans(x, low_threshold=1, high_threshold=2, cutoff_freq=1000., sampling_freq=1.e5):
    return filter_derivative_spans_from_y(bessel_filtfilt(x, cutoff_freq, sampling_freq), low_threshold, high_threshold)


def filter_derivative_margin(y, low_threshold, high_threshold):
    """The smallest absolute decision margin of a filtered current: how far a derivative lies from low_threshold, and how
    far apart the two maxima of a pair are (pairs that are decided without comparing maxima have none)."""
    y = np.asarray(y, dtype=np.float64)
    if y.size < 2:
        return float("inf")
    d, pairs = _pairs(y, low_threshold)
    m = float(np.min(np.abs(d - low_threshold)))
    h1 = _first_counted(high_threshold)
    for s, t in pairs.tolist():
        left, right = d[s:s + h1], d[min(s + h1, t):t]
        if left.size and right.size:
            m = min(m, float(abs(right.max() - left.max())))
    return m
