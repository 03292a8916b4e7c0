"""Records the goldens of the state parsers: golden_state_parsers.npz + manifest_state_parsers.json.

    python tests/golden/make_golden_state_parsers.py /path/to/reference

The reference's parsers.py is compiled IN MEMORY into a module whose imports find the stand-ins of
make_golden_statsplit.py (load_reference there); its text is Python 2, so the module also gets xrange = range and a `map`
that returns a list (FilterDerivativeSegmenter.parse takes len() of one), and `it` = itertools, which the reference's text
gets through `from core import *` (izip = zip, as load_reference leaves it).  Nothing of the reference is written anywhere.

Stored per case of tests/state_parser_cases.py: the spans (start, end = start + len(current)) of the Segments parse()
returns -- the inputs come from the seeds.  Three families:
  snake/<name>  snakebase_parser().parse(current)
  fd/<name>     FilterDerivativeSegmenter(**par).parse(current), with the smallest absolute decision margin of the case
                (state_parser_oracle.filter_derivative_margin on scipy's own y) and max|current|
  fdy/<name>    the reference's decisions on a GIVEN y: the same parse(), run while scipy.signal.filtfilt hands its input
                back -- so that exact ties and pairs of chosen lengths, which no filter output holds, have goldens too
The GPU test compares the full route of an fd case when its margin is at least MARGIN_REL * max|current| (the device filter
agrees with scipy to 1e-11 of max|y|); this script asserts that at most 1 fd case in 10 falls below that.
"""
import builtins
import itertools
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import state_parser_cases as PC  # noqa: E402
import state_parser_oracle as PO  # noqa: E402
from make_golden_statsplit import load_reference  # noqa: E402

MARGIN_REL = 1e-9


def spans_of(segs):
    return np.array([[int(s.start), int(s.start) + len(s.current)] for s in segs], dtype=np.int32).reshape(-1, 2)


def main(root):
    from scipy import signal
    module = load_reference(root)
    module.map = lambda f, xs: list(builtins.map(f, xs))
    module.it = itertools
    arrays, rows = {}, []
    for case in PC.SNAKE_CASES:
        x = PC.snake_build(case)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            sp = spans_of(module.snakebase_parser().parse(x))
        arrays["snake/" + case["name"]] = sp
        rows.append(dict(key="snake/" + case["name"], n=int(x.size), n_spans=int(sp.shape[0])))
        print(rows[-1])
    for case in PC.FD_CASES:
        x, par = PC.fd_build(case), case["par"]
        sp = spans_of(module.FilterDerivativeSegmenter(**par).parse(x))
        y = PO.bessel_filtfilt(x, par["cutoff_freq"], par["sampling_freq"])
        d, pairs = PO._pairs(y, par["low_threshold"])
        arrays["fd/" + case["name"]] = sp
        rows.append(dict(key="fd/" + case["name"], n=int(x.size), n_spans=int(sp.shape[0]), pairs=int(pairs.shape[0]),
                         blocks0=bool(d[0] > par["low_threshold"]),
                         margin=PO.filter_derivative_margin(y, par["low_threshold"], par["high_threshold"]),
                         max_abs_current=float(np.max(np.abs(x)))))
        print(rows[-1])
    filtfilt = signal.filtfilt
    signal.filtfilt = lambda b, a, x: np.array(x, dtype=np.float64)
    try:
        for case in PC.FDY_CASES:
            y, par = PC.fdy_build(case), case["par"]
            if y.size == 0:
                continue                       # (np.diff of nothing has no first block: the reference raises)
            sp = spans_of(module.FilterDerivativeSegmenter(**par).parse(y))
            arrays["fdy/" + case["name"]] = sp
            rows.append(dict(key="fdy/" + case["name"], n=int(y.size), n_spans=int(sp.shape[0]),
                             pairs=int(PO._pairs(y, par["low_threshold"])[1].shape[0])))
            print(rows[-1])
    finally:
        signal.filtfilt = filtfilt
    fd = [r for r in rows if r["key"].startswith("fd/")]
    below = [r["key"] for r in fd if r["margin"] < MARGIN_REL * r["max_abs_current"]]
    assert 10 * len(below) <= len(fd), below
    np.savez_compressed(os.path.join(HERE, "golden_state_parsers.npz"), **arrays)
    with open(os.path.join(HERE, "manifest_state_parsers.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_state_parsers.py", "margin_rel": MARGIN_REL, "below_margin": below,
                   "cases": rows}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
