"""Records the goldens of StatSplit: golden_statsplit.npz + manifest_statsplit.json.

    python tests/golden/make_golden_statsplit.py /path/to/reference

The reference's parsers.py is Python 2 in its imports only.  Its text is compiled IN MEMORY into a module whose imports
find stand-ins: `core` (a Segment that keeps its keywords), `pyximport` (install() does nothing), `PyPore` and
`PyPore.cparsers` (an empty FastStatSplit), itertools.izip = zip; the module then gets xrange = range and, for the one
mode that needs it (splitter="slanted" with use_log=True calls an undefined `log`), log = numpy.log.  Nothing of the
reference is written anywhere.

Stored per (case, splitter, use_log) of tests/statsplit_cases.py: the boundaries StatSplit.parse returns (the starts of
its segments but the first), and for use_log=True the smallest relative decision margin over the windows it scanned --
the winner's gain against the best other candidate or the threshold, whichever is closer; with no winner, the threshold
against the best gain.  The GPU test compares use_log=True runs whose margin is at least 1e-9 (a device logarithm differs
from the host's in the last bit, ~1e-14 of a gain at these sizes); this script asserts that at most 1 run in 10 falls
below that.  A parser is built afresh for every run: the reference's parse() replaces `splitter` by a bound method.
"""
import itertools
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import statsplit_cases as SC  # noqa: E402

MARGIN_MIN = 1e-9


def load_reference(root):
    class Segment(object):
        def __init__(self, current, **kw):
            self.current = current
            self.__dict__.update(kw)

    core = types.ModuleType("core")
    core.Segment = Segment
    core.__all__ = ["Segment"]
    pyx = types.ModuleType("pyximport")
    pyx.install = lambda **kw: None
    pkg = types.ModuleType("PyPore")
    cp = types.ModuleType("PyPore.cparsers")
    cp.FastStatSplit = type("FastStatSplit", (object,), {})
    pkg.cparsers = cp
    stubs = {"core": core, "pyximport": pyx, "PyPore": pkg, "PyPore.cparsers": cp}
    saved = {k: sys.modules.get(k) for k in stubs}
    itertools.izip = zip
    sys.modules.update(stubs)
    try:
        module = types.ModuleType("reference_parsers")
        with open(os.path.join(root, "PyPore", "parsers.py")) as f:
            code = compile(f.read(), "<reference parsers.py>", "exec")
        exec(code, module.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    module.xrange = range
    module.log = np.log
    return module


def make_recorder(module):
    """StatSplit whose two splitters note, per window scanned, the relative decision margin (from the reference's own
    _var_c / _lr, candidate by candidate)."""
    base = module.StatSplit

    class Recorder(base):
        def _note(self, var, start, end, result):
            f = np.log if self.use_log else (lambda v: v)
            thr = self.min_gain_per_sample * self.window_width
            tot = (end - start) * f(var(start, end))
            g = np.array([tot - ((i - start) * f(var(start, i)) + (end - i) * f(var(i, end)))
                          for i in range(start + self.min_width, end + 1 - self.min_width)], dtype=np.float64)
            g = g[~np.isnan(g)]
            if result is None:
                m = np.inf if g.size == 0 else (thr - g.max()) / max(abs(thr), 1e-300)
            else:
                win = result[1]
                others = np.sort(g)[:-1]
                rival = max(thr, others[-1]) if others.size else thr
                m = (win - rival) / max(abs(win), 1e-300)
            self.margins.append(0.0 if np.isnan(m) else float(m))

        def _best_split_stepwise(self, start, end):
            r = base._best_split_stepwise(self, start, end)
            if end - start >= 2 * self.min_width:
                self._note(self._var_c, start, end, r)
            return r

        def _best_split_slanted(self, start, end):
            r = base._best_split_slanted(self, start, end)
            if end - start >= 2 * self.min_width:
                self._note(lambda a, b: self._lr(a, b)[2], start, end, r)
            return r

    return Recorder


def main(root):
    module = load_reference(root)
    Recorder = make_recorder(module)
    arrays, rows = {}, []
    for case, splitter, use_log in SC.runs(SC.CASES_ALL):
        x = np.array(SC.build(case))
        p = Recorder(use_log=use_log, splitter=splitter, **case["par"])
        p.margins = []
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            segs = p.parse(x, case.get("start", 0), case.get("end", -1))
        b = np.array([s.start for s in segs[1:]], dtype=np.int32)
        k = SC.key(case, splitter, use_log)
        arrays[k] = b
        margin = min(min(p.margins), 1e300) if p.margins else 1e300
        rows.append(dict(key=k, n=int(x.size), n_bounds=int(b.size), windows=len(p.margins), margin=margin if use_log else None))
        print(k, b.size, len(p.margins), margin)
    logs = [r for r in rows if r["margin"] is not None]
    dropped = [r["key"] for r in logs if r["margin"] < MARGIN_MIN]
    assert 10 * len(dropped) <= len(logs), dropped
    np.savez_compressed(os.path.join(HERE, "golden_statsplit.npz"), **arrays)
    with open(os.path.join(HERE, "manifest_statsplit.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_statsplit.py", "margin_min": MARGIN_MIN, "below_margin": dropped,
                   "runs": rows}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
