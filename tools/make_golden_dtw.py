#!/usr/bin/env python3
"""Generate tests/golden/g15_dtw.npz by running the REFERENCE's utils/dtw.py on the seeded cases of tests/dtw_shapes.py, and scipy's
moments on their tracks.  TEST INFRASTRUCTURE; needs the reference checkout (DICT_TTS_REFERENCE) and scipy, runs on the CPU.

Nothing of the reference is copied: utils/dtw.py is loaded from the checkout by path (its package's __init__ pulls the training stack in)
and the fixture stores what its functions return.  F = 1 cases go through ``dtw(x, y, lambda a, b: np.abs(a - b), w=w, s=s)`` exactly as
scripts/pitch_dtw.py calls it (float32 tracks are then subtracted in float32), feature cases through ``accelerated_dtw(x, y, 'cityblock')``.

Stored per case: the distance, the path, the inputs (a fingerprint instead when a side has more than GOLDEN_INPUT_MAX values; the tests
regenerate the inputs from the seed either way and compare), the accumulated-cost matrix D1 for cases up to 70 x 70, and for 1-D cases
np.mean / np.std / scipy.stats.skew / kurtosis (bias=True) of both tracks, widened to float64 first (numpy would
reduce a float32 track in float32).  The case whose band is narrower than |N - M| is stored as the
AssertionError the reference raises.
"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle.make_golden import REF  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g15_dtw.npz")


def main():
    sys.dont_write_bytecode = True
    from scipy.stats import kurtosis, skew
    import dtw_shapes as ds
    spec = importlib.util.spec_from_file_location("ref_dtw", os.path.join(REF, "utils", "dtw.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    manhattan = lambda a, b: np.abs(a - b)

    out = {"names": np.array([c["name"] for c in ds.CASES])}
    for c in ds.CASES:
        x, y = ds.inputs(c)
        k = c["name"]
        if c["F"] == 1:
            dist, _, D1, path = ref.dtw(x, y, manhattan, w=np.inf if c["w"] is None else c["w"], s=c["s"])
            with np.errstate(all="ignore"):
                out[k + ".moments"] = np.array([[np.mean(t), np.std(t), skew(t, axis=0, bias=True), kurtosis(t, axis=0, bias=True)]
                                                for t in (x.astype(np.float64), y.astype(np.float64))], np.float64)
        else:
            dist, _, D1, path = ref.accelerated_dtw(x, y, "cityblock")
        out[k + ".dist"] = np.float64(dist)
        out[k + ".path"] = np.stack([np.asarray(path[0]), np.asarray(path[1])]).astype(np.int32)
        if max(x.size, y.size) <= ds.GOLDEN_INPUT_MAX:
            out[k + ".x"], out[k + ".y"] = x, y
        else:
            out[k + ".fp"] = ds.fingerprint(x, y)
        if max(c["N"], c["M"]) <= ds.GOLDEN_D1_MAX:
            out[k + ".D1"] = np.asarray(D1, np.float64)
        print(f"{k}: distance {dist!r}, path of {len(path[0])}")
    c = ds.REFUSED
    x, y = ds.inputs(c)
    try:
        ref.dtw(x, y, manhattan, w=c["w"], s=c["s"])
        out["refused"] = np.array("accepted")
    except AssertionError:
        out["refused"] = np.array("AssertionError")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
