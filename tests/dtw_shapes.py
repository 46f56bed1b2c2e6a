"""The case list of the DTW tests (test infrastructure): seeded pairs for dtts_text2mel_fetch(DTTS_OUT_DTW), shared by
tools/make_golden_dtw.py (which feeds them to the reference's utils/dtw.py), tests/test_dtw_cpu.py and tests/test_dtw_gpu.py.

The shapes derive from the schedule: a lane owns R = abi.DTW_LANE_ROWS rows, 64 lanes make a strip of S = abi.DTW_STRIP_ROWS rows, and
lane t is t columns behind lane 0.  So: degenerate lengths; N around R k and around the wave (63 / 64 / 65 lanes' worth would be 16 times
that: here 63 / 64 / 65 ROWS, i.e. a partly filled fourth lane, and R k +- 1); the strip seam (S - 1, S, S + 1, and three strips); a y
shorter than the pipeline's skew (M = 1, 3 against S + 1 rows); tracks full of exact ties; every kind of band; slopes on either side
of 1; both dtypes; feature rows.

F0-like tracks: a smooth voiced contour between 80 and 400 Hz with unvoiced runs of exact zeros, the two tracks of a pair warped against
each other.  float32 tracks carry full 24-bit significands, so that the float32 subtract of a pair such as (311.7, 93.2) ROUNDS and a
kernel that subtracted in float64 would differ (test_dtw_cpu checks that the two costs differ in every float32 f0 case).
"""
import zlib

import numpy as np

from dict_tts_amd import abi

SEED = 20240915
S = abi.DTW_STRIP_ROWS
R = abi.DTW_LANE_ROWS


def _rng(name):
    return np.random.Generator(np.random.Philox(key=[SEED, zlib.crc32(name.encode())]))


def _case(N, M, kind="f0", F=1, dtype="f64", w=None, s=1.0, tag=""):
    name = f"{kind}_{N}x{M}" + (f"_F{F}" if F > 1 else "") + f"_{dtype}" + (f"_w{w}" if w is not None else "") + (f"_s{s}" if s != 1.0 else "") + tag
    return {"name": name, "N": N, "M": M, "kind": kind, "F": F, "dtype": dtype, "w": w, "s": s}


CASES = []
CASES += [_case(1, 1), _case(1, 5), _case(5, 1), _case(1, 1, dtype="f32")]                                    # degenerate lengths
CASES += [_case(n, 67, dtype=dt) for n in (63, 64, 65) for dt in ("f64", "f32")]                              # around the wave
CASES += [_case(n, 20) for n in (R - 1, R, R + 1, 2 * R - 1, 2 * R + 1)]                                      # around a lane's rows
CASES += [_case(n, 70, dtype=dt) for n, dt in ((S - 1, "f64"), (S, "f32"), (S + 1, "f64"), (S + 1, "f32"))]   # the strip seam
CASES += [_case(70, S + 1), _case(2 * S + 1, S + 3, dtype="f32")]
CASES += [_case(S + 1, 1), _case(S + 1, 3)]                                                                   # the pipeline is shorter than its skew
CASES += [_case(37, 41, kind="zeros"), _case(50, 50, kind="same"), _case(40, 44, kind="const"), _case(37, 41), _case(37, 41, dtype="f32")]   # ties
CASES += [_case(40, 44, w=4), _case(40, 40, w=0), _case(40, 44, w=50), _case(44, 40, w=4, dtype="f32"), _case(S + 1, S - 2, w=3)]   # the band
CASES += [_case(40, 44, s=0.7), _case(40, 44, s=1.3), _case(65, 67, s=1.3, dtype="f32"), _case(33, 30, w=3, s=0.7), _case(S + 1, 70, s=0.7)]   # the slope
CASES += [_case(n, m, kind="feat", F=F, dtype="f32") for (n, m) in ((65, 67), (S + 1, 40)) for F in (2, 80, 128)]                # feature rows
CASES += [_case(65, 67, kind="feat", F=2, dtype="f64")]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
REFUSED = _case(40, 44, w=3, tag="_refused")      # w < |N - M|: the reference asserts; the device marks the pair (dist NaN, path_len 0)
# one batch of five pairs at leading dimensions above every length, the padding NaN
BATCH_X_LENS, BATCH_Y_LENS = (1, 64, S + 1, 37, 300), (3, 67, 70, 41, 320)
BATCH_X_LD, BATCH_Y_LD = S + 5, 330
GOLDEN_D1_MAX = 70        # the fixture stores the accumulated-cost matrix of cases up to 70 x 70
GOLDEN_INPUT_MAX = 1 << 12   # ... and the inputs of cases up to this many values per side (a fingerprint beyond)


def f0_track(rng, n, base, dtype):
    """a voiced contour over `base` (a smooth curve on [0, 1]) sampled at n warped positions, with unvoiced runs of exact zeros"""
    pos = np.sort(rng.uniform(0.0, 1.0, n))
    v = 80.0 + 320.0 * np.interp(pos, np.linspace(0.0, 1.0, len(base)), base) * rng.uniform(0.97, 1.03, n)
    voiced = np.ones(n, bool)
    for _ in range(max(1, n // 24)):
        a = int(rng.integers(0, n))
        voiced[a:a + int(rng.integers(1, 9))] = False
    if n > 2:
        voiced[0] = False                       # a track usually starts in silence: column 0 / row 0 are then full of ties
    return np.where(voiced, v, 0.0).astype(dtype)


def inputs(case):
    """-> x [N] or [N, F], y [M] or [M, F] in the case's dtype"""
    rng = _rng(case["name"].replace("_refused", ""))
    N, M, F, kind = case["N"], case["M"], case["F"], case["kind"]
    dt = np.float32 if case["dtype"] == "f32" else np.float64
    if kind == "zeros":
        return np.zeros(N, dt), np.zeros(M, dt)
    if kind == "feat":
        # mel-like rows: a smooth random walk along time, the two sequences sampled at different rates
        base = np.cumsum(rng.standard_normal((96, F)), axis=0) * 0.3 - 3.0
        t = np.linspace(0.0, 1.0, 96)
        pick = lambda n: np.stack([np.interp(np.sort(rng.uniform(0, 1, n)), t, base[:, f]) for f in range(F)], 1)
        return (pick(N) + 0.05 * rng.standard_normal((N, F))).astype(dt), (pick(M) + 0.05 * rng.standard_normal((M, F))).astype(dt)
    # the contour spans 0.05 .. 0.95 of the range (96 .. 384 Hz), so that a pair's values differ by more than a factor 2 somewhere
    t48 = np.linspace(0.0, 1.0, 48)
    base = np.clip(0.5 + 0.45 * np.sin(2 * np.pi * (rng.uniform(1.0, 2.0) * t48 + rng.uniform())) + np.cumsum(rng.standard_normal(48)) * 0.01, 0.0, 1.0)
    x = f0_track(rng, N, base, dt)
    if kind == "same":
        return x, x.copy()
    if kind == "const":
        y = f0_track(rng, M, base, dt)
        return (np.round(y[np.minimum(np.arange(N), M - 1)]) + 7.0).astype(dt), np.round(y).astype(dt)   # integers 7 apart: every cost ties
    return x, f0_track(rng, M, base, dt)


def batch_inputs(dtype="f64"):
    """-> x [5, BATCH_X_LD], y [5, BATCH_Y_LD] with NaN behind each pair's length, x_lens, y_lens (int32), and the five unpadded pairs"""
    dt = np.float32 if dtype == "f32" else np.float64
    x = np.full((5, BATCH_X_LD), np.nan, dt)
    y = np.full((5, BATCH_Y_LD), np.nan, dt)
    pairs = []
    for b, (n, m) in enumerate(zip(BATCH_X_LENS, BATCH_Y_LENS)):
        xb, yb = inputs(_case(n, m, dtype=dtype, tag=f"_batch{b}"))
        x[b, :n], y[b, :m] = xb, yb
        pairs.append((xb, yb))
    return x, y, np.asarray(BATCH_X_LENS, np.int32), np.asarray(BATCH_Y_LENS, np.int32), pairs


def fingerprint(*arrays):
    """a few float64 numbers that pin seeded arrays down (the fixture stores them for inputs too large to store)"""
    out = []
    for a in arrays:
        a = np.asarray(a, np.float64).reshape(-1)
        out += [a.sum(), np.abs(a).sum(), (a * np.cos(np.arange(a.size))).sum(), float(a.size)]
    return np.array(out, np.float64)
