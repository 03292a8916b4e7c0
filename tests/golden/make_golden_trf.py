"""Records the goldens of the repeat splitter: golden_trf.npz + manifest_trf.json.

    python tests/golden/make_golden_trf.py /path/to/reference

The reference's `NaiveTRF` (PyPore/alignment.py) is Python 2.  Its text, and the text of its nested generator
`NaiveSplitter` dedented by one tab, are sliced out of the file IN MEMORY, passed through lib2to3, the true division
`argmax/(n+1)` is made a floor division (what Python 2 computed), and the result is exec'ed; nothing of it is written
anywhere.  Only inputs and outputs are stored.

A case is tests/trf_cases.py's (means, stds, penalty, min_score).  Stored per case: the inner generator's yields
(score, length, i, j) and NaiveTRF's rows as indices into the sequence, -1 for '-'.

The square.  The reference writes `abs(x.mean - y.mean) ** 2`; on np.float64 (and on float) operands that is libm's
pow(d, 2.0), which glibc does not round correctly for every d: 141 of 200 000 uniform d in (0, 6) gave a square one ulp
off d * d here, so the unmodified text's scores depend on the host's libm.  The device and tests/trf_oracle.py take the
square as the product, the correctly rounded value.  Every case is therefore run twice through the SAME unmodified text:
  exact   the means are floats of a subclass whose `** 2` is the product (class Sq below) -- recorded as the golden, and
          asserted to equal the restatement BIT FOR BIT, yields with their scores and rows, in both of its forms;
  libm    the means are plain np.float64, as core.Segment gives them -- recorded beside it (`*_libm`), and the manifest
          names the cases in which it differs from `exact` and how (DESIGN.md 7n explains them).
The script fails on the first case whose `exact` run differs from the restatement; no case is left out of either run."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trf_cases as C  # noqa: E402
import trf_oracle as O  # noqa: E402


class Seg(object):
    """What NaiveTRF reads of a segment (the mean as given, an np.float64 std), and its place in the sequence."""

    def __init__(self, k, mean, std):
        self.k, self.mean, self.std = k, mean, np.float64(std)


class Sq(float):
    """A float whose difference and absolute value stay of this class and whose `** 2` is the product."""

    def __sub__(self, other):
        return Sq(float(self) - float(other))

    def __abs__(self):
        return Sq(abs(float(self)))

    def __pow__(self, e):
        assert e == 2
        return float(self) * float(self)


def load_reference(root):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
    text = open(os.path.join(root, "PyPore", "alignment.py")).read()
    start = text.index("def NaiveTRF")
    nxt = [text.find(k, start + 1) for k in ("\ndef ", "\nclass ")]
    end = min([e for e in nxt if e >= 0] or [len(text)])
    outer = text[start:end]
    a = outer.index("\tdef NaiveSplitter")
    b = outer.index("\tsplits = NaiveSplitter")
    inner = "\n".join(line[1:] if line.startswith("\t") else line for line in outer[a:b].split("\n"))
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    ns = {"np": np}
    for name, src in (("NaiveTRF", outer), ("NaiveSplitter", inner)):
        src = str(tool.refactor_string(src + "\n", name))
        assert src.count("argmax/(n+1)") == 1
        src = src.replace("argmax/(n+1)", "argmax//(n+1)")
        exec(compile(src, "<%s>" % name, "exec"), ns)
    return ns["NaiveTRF"], ns["NaiveSplitter"]


def main(root):
    trf, splitter = load_reference(root)
    arrays, manifest = {}, []
    for c in C.all_cases():
        def run(mean_type):
            seq = [Seg(k, mean_type(m), s) for k, (m, s) in enumerate(zip(c["means"], c["stds"]))]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                y = [(float(s), int(L), int(i), int(j)) for s, L, i, j in splitter(seq, c["penalty"], c["min_score"])]
                rows = [[-1 if isinstance(e, str) else e.k for e in row] for row in trf(seq, c["penalty"], c["min_score"])]
            return y, rows
        ref_y, ref_rows = run(Sq)
        libm_y, libm_rows = run(np.float64)
        for form in (O.splits_full, O.splits_upper):
            got, _ = form(c["means"], c["stds"], c["penalty"], c["min_score"])
            assert len(got) == len(ref_y), (c["name"], form.__name__, len(got), len(ref_y))
            for g, r in zip(got, ref_y):
                assert g[1:] == r[1:] and np.float64(g[0]).tobytes() == np.float64(r[0]).tobytes(), (c["name"], form.__name__, g, r)
        assert O.stitch(len(c["means"]), ref_y) == ref_rows, c["name"]
        n = c["name"]
        arrays[n + "/means"], arrays[n + "/stds"] = c["means"], c["stds"]
        same_structure = [v[1:] for v in libm_y] == [v[1:] for v in ref_y] and libm_rows == ref_rows
        differing = [k for k, (a, b) in enumerate(zip(libm_y, ref_y)) if a[0] != b[0]] if same_structure else None
        for tag, y, rows in (("", ref_y, ref_rows), ("_libm", libm_y, libm_rows)):
            if tag and differing == []:
                continue                # the libm run is stored only where it differs
            arrays[n + "/score" + tag] = np.array([v[0] for v in y], dtype=np.float64)
            arrays[n + "/lij" + tag] = np.array([v[1:] for v in y], dtype=np.int16).reshape(-1, 3)
            arrays[n + "/rows" + tag] = np.array(rows, dtype=np.int16)
        manifest.append({"name": n, "n": len(c["means"]), "penalty": c["penalty"], "min_score": c["min_score"], "grid": c["grid"],
                         "yields": len(ref_y), "rows": len(ref_rows), "row0_end": any(y[2] == 0 for y in ref_y),
                         "libm_same_structure": same_structure, "libm_scores_differing": differing})
        print("%-28s n %3d  yields %3d  rows %3d  libm pow: %s" % (n, len(c["means"]), len(ref_y), len(ref_rows),
              "identical" if differing == [] else "same structure, scores differ at %s" % differing if same_structure else "STRUCTURE DIFFERS"))
    np.savez_compressed(os.path.join(HERE, "golden_trf.npz"), **arrays)
    with open(os.path.join(HERE, "manifest_trf.json"), "w") as f:
        json.dump({"reference": "PyPore/alignment.py NaiveTRF, NaiveSplitter (lib2to3, argmax // (n+1))", "cases": manifest}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
