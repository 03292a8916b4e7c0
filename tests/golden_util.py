"""Loader for the golden vectors recorded from the compiled reference (tests/golden/make_golden.py)."""
import json
import os

import numpy as np

from pypore_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
_npz = None
_manifest = None


def npz():
    global _npz
    if _npz is None:
        _npz = np.load(os.path.join(HERE, "golden", "golden.npz"))
    return _npz


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(HERE, "golden", "manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def cases(op):
    return [c for c in manifest()["cases"] if c["op"] == op]


def case_ids(op):
    return [c["name"] for c in cases(op)]


def input_counts(case):
    gen = case["gen"]
    kind = gen["kind"]
    if kind == "step":
        c = synth.step_counts(gen["n"], gen["dwell"], gen["seed"], gen.get("level_offset", 0))
    elif kind == "random_dwell":
        c = synth.random_dwell_counts(gen["n"], gen["seed"], gen.get("lo", 1000), gen.get("hi", 20000))
    elif kind == "stored":
        c = npz()[gen["key"]]
    else:
        raise ValueError(kind)
    return np.asarray(c[case.get("offset", 0):], dtype=np.int32)


def input_pa(case, dtype=np.float64):
    return synth.counts_to_pa(input_counts(case), dtype)


_npz_off = None
_manifest_off = None


def offgrid_npz():
    global _npz_off
    if _npz_off is None:
        _npz_off = np.load(os.path.join(HERE, "golden", "golden_offgrid.npz"))
    return _npz_off


def offgrid_cases(op):
    """Cases of tests/golden/manifest_offgrid.json (make_golden_offgrid.py): op 'parse_offgrid' or 'score_samples'."""
    global _manifest_off
    if _manifest_off is None:
        with open(os.path.join(HERE, "golden", "manifest_offgrid.json")) as f:
            _manifest_off = json.load(f)
    return [c for c in _manifest_off["cases"] if c["op"] == op]


# ---- event detector edges (tests/golden/make_golden_detect.py) --------------------------------------------------------

def detect_npz():
    return np.load(os.path.join(HERE, "golden", "golden_detect.npz"))


def detect_cases():
    with open(os.path.join(HERE, "golden", "manifest_detect.json")) as f:
        return json.load(f)["cases"]


def detect_input(gen):
    """float64 pA of a detector case from its generator parameters: `chatter` -- counts on the 2^-5 pA grid, noise straddling
    90 pA where the blockades begin and end; `decimal` -- float64 rounded to 1 / per_pA (no power-of-two grid); `abf_grid`
    -- int16 counts * an .abf header scale + offset, computed as abf.read_abf does (a GridArray that keeps its counts)."""
    from pypore_amd.grid import GridArray
    rng = np.random.default_rng(gen["seed"])
    n, kind = gen["n"], gen["kind"]
    if kind == "chatter":
        k = 3520 + rng.integers(-40, 41, n)
        for a, b in gen["blockades"]:
            k[a:b] = 1440 + rng.integers(-40, 41, b - a)
        for a in gen["chatter_at"]:
            k[a:a + gen["chatter_len"]] = 2880 + rng.integers(-3, 3, gen["chatter_len"])
        for i, v in gen.get("plant_counts", []):
            k[i] = v
        return k.astype(np.float64) * synth.QUANTUM
    if kind == "decimal":
        x = 110 + rng.normal(0, 1.5, n)
        for a, b in gen["blockades"]:
            x[a:b] = 45 + rng.normal(0, 1.5, b - a)
        x = np.round(x * gen["per_pA"]) / gen["per_pA"]
        for i, v in gen.get("plant", []):
            x[i] = v
        return x
    if kind == "abf_grid":
        q = float(gen["scale"])
        k = np.rint((110 + rng.normal(0, 1.5, n)) / q)
        for a, b in gen["blockades"]:
            k[a:b] = np.rint((45 + rng.normal(0, 1.5, b - a)) / q)
        for i, v in gen.get("plant_counts", []):
            k[i] = v
        return GridArray.from_counts(k.astype(np.int16), q, gen["offset"])
    raise ValueError(kind)
