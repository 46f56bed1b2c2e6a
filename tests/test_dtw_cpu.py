"""Dynamic time warping, the parts that need no GPU: the float64 restatement (tests/dtw_ref.py) against the reference's own outputs
(tests/golden/g15_dtw.npz, written by tools/make_golden_dtw.py from utils/dtw.py and scipy), the ABI surface of
dtts_text2mel_fetch(DTTS_OUT_DTW) with every refusal of its argument block (the block is checked before the handle, so a NULL handle
reaches them all and reports through dtts_last_error(NULL)), and the Python layer's pairing and argument checks.

Distance, accumulated cost and path are compared bit for bit: the recurrence is one add of an exact minimum per cell.  The moments are held
to 1e-12 relative of scipy's (both sum about 2000 terms in fp64: 2000 x 1.1e-16 of the sum of magnitudes, which for these tracks is within
a factor 10 of the result).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dtw_ref as dr
import dtw_shapes as ds
from dict_tts_amd import abi
from dict_tts_amd import dtw as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R = abi.DTW_STRIP_ROWS, abi.DTW_LANE_ROWS
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_dtw.npz"))


def test_argument_block_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert int(re.search(r"#define DTTS_OUT_DTW (\d+)", hdr).group(1)) == abi.OUT_DTW == 15
    assert int(re.search(r"#define DTTS_DTW_STRIP_ROWS (\d+)", hdr).group(1)) == abi.DTW_STRIP_ROWS == 64 * abi.DTW_LANE_ROWS
    assert int(re.search(r"#define DTTS_DTW_MAX_LEN (\d+)", hdr).group(1)) == abi.DTW_MAX_LEN >= 8192
    src = open(os.path.join(ROOT, "dict_tts_amd", "csrc", "dtw.h")).read()
    assert int(re.search(r"DTW_LANE_ROWS = (\d+);", src).group(1)) == abi.DTW_LANE_ROWS
    body = re.search(r"typedef struct dtts_dtw_args \{(.*?)\} dtts_dtw_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.search(r"([A-Za-z_0-9]+)$", part.strip()).group(1) for part in decl.split(",")]
    assert names == [f[0] for f in abi.DtwArgs._fields_], names
    assert C.sizeof(abi.DtwArgs) == 8 * 4 + 8 + 9 * C.sizeof(C.c_void_p)
    assert abi.DtwArgs.slope.offset == 32 and abi.DtwArgs.x_dev.offset == 40 and abi.DtwArgs.moments_dev.offset == 104
    # the ABI keeps its entry points: the unit is an item of dtts_text2mel_fetch
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "dtw" in s]
    assert "dtw" not in open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()


def test_every_refusal_names_its_value():
    lib = abi.load_library()
    good = dict(B=2, x=0x1000, y=0x2000, x_ld=40, y_ld=44, dist=0x3000, path=0x4000, path_ld=83, path_len=0x5000, acc=0x6000, moments=0x7000)

    def refused(match, **kw):
        a = abi.dtw_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_DTW, C.byref(a), None) == -22   # DTTS_E_INVAL
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"B = 0", B=0)
    refused(r"B = -3", B=-3)
    refused(r"F = 0 ", F=0)
    refused(r"F = 129", F=129, moments=None)
    refused(r"dtype = 2", dtype=2)
    refused(r"dtype = -1", dtype=-1)
    for s, shown in ((0.0, "0"), (-1.5, "-1.5"), (float("inf"), "inf"), (float("nan"), "nan")):
        refused(rf"slope = -?{re.escape(shown)}", slope=s)
    refused(r"x_ld = 0 ", x_ld=0)
    refused(rf"x_ld = {abi.DTW_MAX_LEN + 1}", x_ld=abi.DTW_MAX_LEN + 1, path=None)
    refused(r"y_ld = -4", y_ld=-4)
    refused(rf"y_ld = {abi.DTW_MAX_LEN + 1}", y_ld=abi.DTW_MAX_LEN + 1, path=None)
    refused(r"path_ld = 82 entries for x_ld \+ y_ld - 1 = 83", path_ld=82)
    refused(r"moments_dev with F = 2", F=2)
    refused(r"null x_dev", x=None)
    refused(r"null x_dev / y_dev", y=None)
    refused(r"dist_dev", dist=None)
    refused(r"path_dev without path_len_dev", path_len=None)
    refused(r"x_dev = 0x1002 is not aligned to 4", x=0x1002)
    refused(r"y_dev = 0x2004 is not aligned to 8", y=0x2004, dtype=1)
    refused(r"x_lens_dev = 0x[0-9a-f]+ is not aligned to 4", x_lens=0x8001)
    refused(r"y_lens_dev = 0x[0-9a-f]+ is not aligned to 4", y_lens=0x8002)
    refused(r"dist_dev = 0x3004 is not aligned to 8", dist=0x3004)
    refused(r"path_dev = 0x4002 is not aligned to 4", path=0x4002)
    refused(r"path_len_dev = 0x5001 is not aligned to 4", path_len=0x5001)
    refused(r"acc_dev = 0x6004 is not aligned to 8", acc=0x6004)
    refused(r"moments_dev = 0x7004 is not aligned to 8", moments=0x7004)
    a = abi.dtw_args(**good)
    a.size -= 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_DTW, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.DtwArgs) - 8}" in lib.dtts_last_error(None).decode()
    refused(r"null handle")                                      # a good block: only then is the handle looked at
    assert lib.dtts_text2mel_fetch(None, abi.OUT_DTW, None, None) == -22


def test_case_list_covers_the_schedule():
    shapes = {(c["N"], c["M"]) for c in ds.CASES if c["F"] == 1}
    assert {(1, 1), (1, 5), (5, 1), (63, 67), (64, 67), (65, 67), (S - 1, 70), (S, 70), (S + 1, 70), (70, S + 1), (2 * S + 1, S + 3),
            (S + 1, 1), (S + 1, 3), (R - 1, 20), (R + 1, 20)} <= shapes
    assert {c["s"] for c in ds.CASES} == {0.7, 1.0, 1.3} and {c["dtype"] for c in ds.CASES} == {"f32", "f64"}
    assert {(c["N"], c["M"], c["F"]) for c in ds.CASES if c["F"] > 1} >= {(n, m, F) for (n, m) in ((65, 67), (S + 1, 40)) for F in (2, 80, 128)}
    banded = [c for c in ds.CASES if c["w"] is not None]
    assert any(c["w"] == abs(c["N"] - c["M"]) > 0 for c in banded) and any(c["w"] == 0 and c["N"] == c["M"] for c in banded)
    assert any(c["w"] >= max(c["N"], c["M"]) for c in banded) and ds.REFUSED["w"] < abs(ds.REFUSED["N"] - ds.REFUSED["M"])
    for c in ds.CASES:   # float32 tracks: the float32 subtract rounds somewhere, so a float64 subtract would be caught
        if c["dtype"] == "f32" and c["kind"] == "f0" and c["N"] * c["M"] > 1:
            x, y = ds.inputs(c)
            assert (dr.cost_abs(x, y) != dr.cost_abs(x.astype(np.float64), y.astype(np.float64))).any(), c["name"]
    x, y, xl, yl, pairs = ds.batch_inputs()
    assert x.shape[1] > xl.max() and y.shape[1] > yl.max() and sorted(xl) == sorted([1, 64, S + 1, 37, 300])
    assert all(np.isnan(x[b, xl[b]:]).all() and np.isnan(y[b, yl[b]:]).all() and not np.isnan(x[b, :xl[b]]).any() for b in range(5))


@pytest.mark.parametrize("case", ds.CASES, ids=lambda c: c["name"])
def test_float64_restatement_equals_reference_golden_g15(g15, case):
    x, y = ds.inputs(case)
    k = case["name"]
    if k + ".x" in g15:
        assert x.dtype == g15[k + ".x"].dtype and np.array_equal(x, g15[k + ".x"]) and np.array_equal(y, g15[k + ".y"])
    else:
        assert np.array_equal(ds.fingerprint(x, y), g15[k + ".fp"])
    dist, D1, (p, q) = dr.dtw(x, y, case["w"], case["s"])
    assert bits(dist) == bits(g15[k + ".dist"]), (dist, float(g15[k + ".dist"]))
    want = g15[k + ".path"]
    assert len(p) == want.shape[1] and np.array_equal(p, want[0]) and np.array_equal(q, want[1])
    assert len(p) <= case["N"] + case["M"] - 1 and (p[0], q[0]) == (0, 0) and (p[-1], q[-1]) == (case["N"] - 1, case["M"] - 1)
    if max(case["N"], case["M"]) <= ds.GOLDEN_D1_MAX:
        assert np.array_equal(bits(D1), bits(g15[k + ".D1"]))
    if case["kind"] in ("zeros", "same", "const") or case["s"] != 1.0:
        # ties everywhere (or a slope): the path is the unscaled, diagonal-first argmin's; a forward-order argmin (diagonal, j - 1, i - 1)
        # or a scaled one gives another path on at least one of these cases (checked below on the case list as a whole)
        assert (np.diff(p) >= 0).all() and (np.diff(q) >= 0).all()


def test_the_tie_order_and_the_unscaled_argmin_matter(g15):
    """the fixture can tell the traceback's argmin from the two mistakes the design warns of"""
    def other_path(D0, s, order):
        i, j = D0.shape[0] - 2, D0.shape[1] - 2
        out = [(i, j)]
        while i > 0 or j > 0:
            cand = {"d": D0[i, j], "i": s * D0[i, j + 1], "j": s * D0[i + 1, j]}
            tb = min(order, key=lambda n: (cand[n], order.index(n)))
            i, j = (i - 1, j - 1) if tb == "d" else (i - 1, j) if tb == "i" else (i, j - 1)
            out.append((i, j))
        return out[::-1]

    swapped = scaled = 0
    for c in ds.CASES:
        if c["F"] > 1 or max(c["N"], c["M"]) > 70:
            continue
        x, y = ds.inputs(c)
        want = list(zip(*g15[c["name"] + ".path"].tolist()))
        D0 = dr.accumulate(dr.cost_abs(x, y), c["w"], c["s"])
        assert other_path(D0, 1.0, "dij") == want
        swapped += other_path(D0, 1.0, "dji") != want
        scaled += other_path(D0, c["s"], "dij") != want
    assert swapped >= 1 and scaled >= 1, (swapped, scaled)


def test_moments_match_scipy(g15):
    n = 0
    for c in ds.CASES:
        if c["F"] > 1:
            continue
        x, y = ds.inputs(c)
        want = g15[c["name"] + ".moments"]
        for t, w in ((x, want[0]), (y, want[1])):
            got = dr.moments(t)
            if len(t) == 1 or not np.asarray(t).any() or np.ptp(t) == 0:
                assert np.isnan(got[2:]).all() and np.isnan(w[2:]).all() and got[1] == 0.0
                continue
            assert np.allclose(got, w, rtol=1e-12, atol=0), (c["name"], got, w)
            assert np.abs((np.asarray(t, np.float64) - got[0]) / got[1]).max() <= 4.0      # |z| <= 4: the GPU test's bound leans on it
            n += 1
    assert n >= 40


def test_pairing_by_name():
    names = ["f0/b_gt.npy", "f0/a.npy", "f0/b.npy", "f0/a_gt.npy", "f0/notes.txt"]
    assert D.pair_f0_files(names) == [("a.npy", "a_gt.npy"), ("b.npy", "b_gt.npy")]
    with pytest.raises(FileNotFoundError, match="b_gt.npy has no prediction b.npy"):
        D.pair_f0_files(["a.npy", "a_gt.npy", "b_gt.npy"])
    with pytest.raises(FileNotFoundError, match="c.npy has no recording c_gt.npy"):
        D.pair_f0_files(["a.npy", "a_gt.npy", "c.npy"])
    with pytest.raises(FileNotFoundError, match="no \\*_gt.npy"):
        D.pair_f0_files(["readme.txt"])


def test_argument_errors_surface_without_a_gpu():
    d = D.DTW()
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        d(z(5), z(5))
    with pytest.raises(ValueError, match="agree in B and F"):
        d(z(2, 5), z(3, 5))
    with pytest.raises(ValueError, match="agree in B and F"):
        d(z(2, 5, 3), z(2, 5, 4))
    with pytest.raises(ValueError, match="F = 129"):
        d(z(1, 5, 129), z(1, 5, 129))
    with pytest.raises(ValueError, match=rf"N = {abi.DTW_MAX_LEN + 1}"):
        d(z(1, abi.DTW_MAX_LEN + 1), z(1, 5))
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="slope"):
            d(z(1, 5), z(1, 5), slope=s)
    for w in (-1, 2.5):
        with pytest.raises(ValueError, match="window"):
            d(z(1, 5), z(1, 5), window=w)
    with pytest.raises(ValueError, match="x_lens has 3 entries"):
        d(z(2, 5), z(2, 5), x_lens=[1, 2, 3])
    with pytest.raises(ValueError, match="moments"):
        d(z(1, 5, 2), z(1, 5, 2), moments=True)
    with pytest.raises(ValueError, match="pair by pair"):
        D.pitch_dtw([z(5)], [z(5), z(6)])
    with pytest.raises(ValueError, match=r"f0_gt\[0\] must be a non-empty 1-D track"):
        D.pitch_dtw([z(5)], [z(5, 2)])
    with pytest.raises(ValueError, match=r"\[B, T, n_mel\]"):
        D.mel_dtw(z(5, 80), z(5, 80))
