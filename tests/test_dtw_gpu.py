"""Dynamic time warping on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_DTW) and ``dict_tts_amd.dtw`` against
the float64 restatement (tests/dtw_ref.py, itself bit-identical to the reference's utils/dtw.py on every case: tests/test_dtw_cpu.py)
over the cases of tests/dtw_shapes.py.

Bounds.  Distance, accumulated cost, path and path_len: BIT-IDENTICAL (one add of an exact minimum per cell; no schedule can change it).
Moments: 1e-9 relative on mean and sigma, 1e-9 absolute on skewness and kurtosis, against the math.fsum restatement — a sequential fp64
sum of n <= 8192 terms carries at most n x 1.1e-16 ~ 1e-12 of the sum of magnitudes, the cases keep |z| <= 4 (checked in
test_dtw_cpu.py), so the standardised moments stay O(10): roughly 100 x margin.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import dtw_ref as dr
import dtw_shapes as ds
from dict_tts_amd import abi
from dict_tts_amd import dtw as D

pytestmark = pytest.mark.gpu
T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
S, R = abi.DTW_STRIP_ROWS, abi.DTW_LANE_ROWS
SENT = -7.0   # the fill of every output buffer (guard bands, and the cells a call must leave untouched)
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
ibits = lambda t: t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    return abi.Context()


_REFS = {}


def _ref(key, x, y, w, s):
    """the restatement of one pair, computed once per key"""
    if key not in _REFS:
        _REFS[key] = dr.dtw(x, y, w, s)
    return _REFS[key]


def _run(ctx, x, y, x_lens=None, y_lens=None, w=None, s=1.0, path=True, acc=True, moments=False):
    """raw ABI call on host arrays x [B, x_ld(, F)], y [B, y_ld(, F)] -> dict of numpy outputs; checks guard bands and that the inputs stay"""
    B, x_ld, y_ld = x.shape[0], x.shape[1], y.shape[1]
    F = x.shape[2] if x.ndim == 3 else 1
    xd, yd = T_(x).cuda(), T_(y).cuda()
    xl = None if x_lens is None else T_(np.asarray(x_lens, np.int32)).cuda()
    yl = None if y_lens is None else T_(np.asarray(y_lens, np.int32)).cuda()
    pl = x_ld + y_ld - 1
    dist = torch.full((B + 8,), SENT, dtype=torch.float64, device="cuda")
    pth = torch.full((B * 2 * pl + 64,), -7, dtype=torch.int32, device="cuda") if path else None
    plen = torch.full((B + 8,), -7, dtype=torch.int32, device="cuda") if path else None
    accb = torch.full((B * x_ld * y_ld + 64,), SENT, dtype=torch.float64, device="cuda") if acc else None
    mom = torch.full((B * 8 + 8,), SENT, dtype=torch.float64, device="cuda") if moments else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.dtw(B, _stream(), x=xd.data_ptr(), y=yd.data_ptr(), x_ld=x_ld, y_ld=y_ld, F=F, dtype=1 if x.dtype == np.float64 else 0,
            window=-1 if w is None else w, slope=s, x_lens=ptr(xl), y_lens=ptr(yl), dist=dist.data_ptr(), path=ptr(pth), path_ld=pl,
            path_len=ptr(plen), acc=ptr(accb), moments=ptr(mom))
    torch.cuda.synchronize()
    assert torch.equal(ibits(xd.cpu()), ibits(T_(x))) and torch.equal(ibits(yd.cpu()), ibits(T_(y)))
    assert (dist[B:] == SENT).all()
    out = {"dist": dist[:B].cpu().numpy()}
    if path:
        assert (pth[B * 2 * pl:] == -7).all() and (plen[B:] == -7).all()
        out["path"], out["path_len"] = pth[:B * 2 * pl].reshape(B, 2, pl).cpu().numpy(), plen[:B].cpu().numpy()
    if acc:
        assert (accb[B * x_ld * y_ld:] == SENT).all()
        out["acc"] = accb[:B * x_ld * y_ld].reshape(B, x_ld, y_ld).cpu().numpy()
    if moments:
        assert (mom[B * 8:] == SENT).all()
        out["moments"] = mom[:B * 8].reshape(B, 2, 4).cpu().numpy()
    return out


def _check_pair(out, b, ref, N, M):
    dist, D1, (p, q) = ref
    assert bits(out["dist"][b]) == bits(dist), (out["dist"][b], dist)
    if "acc" in out:
        a = out["acc"][b]
        assert np.array_equal(bits(a[:N, :M]), bits(D1))
        assert (a[N:] == SENT).all() and (a[:, M:] == SENT).all()          # cells outside [0, N) x [0, M) are left untouched
    if "path" in out:
        n = int(out["path_len"][b])
        assert n == len(p), (n, len(p))
        assert np.array_equal(out["path"][b, 0, :n], p) and np.array_equal(out["path"][b, 1, :n], q)
        assert (out["path"][b, :, n:] == -1).all()


def _check_moments(got, track):
    want = dr.moments(track)
    if np.isnan(want[2]):
        assert np.isnan(got[2:]).all() and got[1] == 0.0 and got[0] == want[0]
        return
    print(f"moments dev: mean rel {abs(got[0] - want[0]) / abs(want[0]):.2e}, sigma rel {abs(got[1] - want[1]) / want[1]:.2e}, "
          f"skew abs {abs(got[2] - want[2]):.2e}, kurtosis abs {abs(got[3] - want[3]):.2e}")
    assert abs(got[0] - want[0]) <= 1e-9 * abs(want[0]) and abs(got[1] - want[1]) <= 1e-9 * want[1]
    assert abs(got[2] - want[2]) <= 1e-9 and abs(got[3] - want[3]) <= 1e-9


@pytest.mark.parametrize("case", ds.CASES, ids=lambda c: c["name"])
def test_single_pair_is_bit_identical(ctx, case):
    x, y = ds.inputs(case)
    N, M = case["N"], case["M"]
    out = _run(ctx, x[None], y[None], w=case["w"], s=case["s"], moments=case["F"] == 1)
    assert np.isfinite(out["dist"]).all()
    _check_pair(out, 0, _ref(case["name"], x, y, case["w"], case["s"]), N, M)
    if case["F"] == 1:
        _check_moments(out["moments"][0, 0], x)
        _check_moments(out["moments"][0, 1], y)
    again = _run(ctx, x[None], y[None], w=case["w"], s=case["s"], acc=False)       # without the debug output: the other instantiation
    assert bits(again["dist"][0]) == bits(out["dist"][0]) and np.array_equal(again["path"], out["path"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_batch_with_poisoned_padding(ctx, dtype):
    x, y, xl, yl, pairs = ds.batch_inputs(dtype)
    out = _run(ctx, x, y, xl, yl, moments=True)
    assert np.isfinite(out["dist"]).all() and np.isfinite(out["moments"][1:]).all()          # the NaN padding reached no output
    for b, (xb, yb) in enumerate(pairs):
        ref = _ref(f"batch{b}_{dtype}", xb, yb, None, 1.0)
        _check_pair(out, b, ref, len(xb), len(yb))
        _check_moments(out["moments"][b, 0], xb)
        _check_moments(out["moments"][b, 1], yb)
        # alone, at its own leading dimensions: the same bits, moments included
        one = _run(ctx, xb[None], yb[None], moments=True)
        _check_pair(one, 0, ref, len(xb), len(yb))
        assert np.array_equal(one["moments"][0].view(np.int64), out["moments"][b].view(np.int64)), b
    # ... and at another batch position, between other neighbours, at other leading dimensions, without lens for the pair that fills them
    perm = [3, 1, 3]
    ldx, ldy = 70, 75
    xp, yp = np.full((3, ldx), np.nan, x.dtype), np.full((3, ldy), np.nan, y.dtype)
    for i, b in enumerate(perm):
        xp[i, :xl[b]], yp[i, :yl[b]] = pairs[b][0], pairs[b][1]
    o2 = _run(ctx, xp, yp, xl[perm], yl[perm], moments=True)
    for i, b in enumerate(perm):
        _check_pair(o2, i, _ref(f"batch{b}_{dtype}", *pairs[b], None, 1.0), xl[b], yl[b])
        assert np.array_equal(o2["moments"][i].view(np.int64), out["moments"][b].view(np.int64))


def test_bad_pairs_are_marked_and_their_neighbours_are_right(ctx):
    c = ds.BY_NAME["f0_40x44_f64_w4"]
    x1, y1 = ds.inputs(c)
    xr, yr = ds.inputs(ds.REFUSED)
    x = np.full((6, 48), np.nan)
    y = np.full((6, 50), np.nan)
    for b in range(6):
        x[b, :40], y[b, :44] = (xr, yr) if b == 2 else (x1, y1)
    #        good      N = 0     good      N > ld    M < 0     good
    xl = np.array([40, 0, 40, 49, 40, 40], np.int32)
    yl = np.array([44, 44, 44, 44, -1, 44], np.int32)
    ref = _ref(c["name"], x1, y1, 4, 1.0)
    out = _run(ctx, x, y, xl, yl, w=4, moments=True)
    for b in (0, 2, 5):
        _check_pair(out, b, ref if b != 2 else _ref("refused_w4", xr, yr, 4, 1.0), 40, 44)
    for b in (1, 3, 4):
        assert np.isnan(out["dist"][b]) and out["path_len"][b] == 0 and (out["path"][b] == -1).all() and (out["acc"][b] == SENT).all()
        assert np.isnan(out["moments"][b]).all()
    # the band narrower than |N - M|: refused per pair (the reference asserts), the pair next to it is not
    xl2, yl2 = np.array([40, 40, 40], np.int32), np.array([44, 43, 41], np.int32)
    out = _run(ctx, x[:3], y[:3], xl2, yl2, w=3)
    assert np.isnan(out["dist"][0]) and out["path_len"][0] == 0 and (out["path"][0] == -1).all() and (out["acc"][0] == SENT).all()
    _check_pair(out, 1, _ref("w3_40x43", x1, y1[:43], 3, 1.0), 40, 43)
    _check_pair(out, 2, _ref("w3_40x41", xr, yr[:41], 3, 1.0), 40, 41)


def test_invalid_arguments_are_refused_by_name(ctx):
    x, y = ds.inputs(ds.BY_NAME["f0_37x41_f64"])
    xd, yd = T_(x).cuda(), T_(y).cuda()
    dist = torch.zeros(4, dtype=torch.float64, device="cuda")
    good = dict(x=xd.data_ptr(), y=yd.data_ptr(), x_ld=37, y_ld=41, dtype=1, dist=dist.data_ptr())

    def refused(match, B=1, **kw):
        with pytest.raises(abi.DttsError, match=match):
            ctx.dtw(B, _stream(), **{**good, **kw})

    refused(r"\(-22\).*B = 0", B=0)
    refused(r"\(-22\).*F = 200", F=200)
    refused(r"\(-22\).*dtype = 3", dtype=3)
    refused(r"\(-22\).*slope = -1", slope=-1.0)
    refused(rf"\(-22\).*x_ld = {abi.DTW_MAX_LEN + 1}", x_ld=abi.DTW_MAX_LEN + 1)
    refused(r"\(-22\).*path_dev without path_len_dev", path=dist.data_ptr(), path_ld=77)
    refused(r"\(-22\).*path_ld = 76", path=dist.data_ptr(), path_len=dist.data_ptr(), path_ld=76)
    refused(r"\(-22\).*x_dev = 0x[0-9a-f]+ is not aligned to 8", x=xd.data_ptr() + 4)
    a = abi.dtw_args(1, **good)
    a.size += 8
    assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_DTW, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.DtwArgs) + 8}" in ctx.last_error()
    torch.cuda.synchronize()
    assert not dist.any()                      # nothing was written by a refused call
    ctx.dtw(1, _stream(), **good)              # distance alone: no path, no workspace
    torch.cuda.synchronize()
    assert bits(dist[0].item()) == bits(_ref("f0_37x41_f64", x, y, None, 1.0)[0])


def test_memory_safety_dtw(ctx):
    """debug_redzone = 1: the direction and cost workspaces sit between red zones and start out as 0xFF; no launch damages a zone, no
    stale word reaches an output, and the results are the plain context's, bit for bit"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg = abi.Context(cfg)
    for name in ("f0_1x1_f64", f"f0_{S + 1}x70_f32", f"f0_{S + 1}x3_f64", f"f0_{2 * S + 1}x{S + 3}_f32", f"f0_{S + 1}x{S - 2}_f64_w3",
                 "feat_65x67_F80_f32", f"feat_{S + 1}x40_F128_f32"):
        c = ds.BY_NAME[name]
        x, y = ds.inputs(c)
        got = _run(dbg, x[None], y[None], w=c["w"], s=c["s"], acc=False)
        assert dbg.debug_check(_stream()) == 0, dbg.last_error()
        _check_pair(got, 0, _ref(name, x, y, c["w"], c["s"]), c["N"], c["M"])
    x, y, xl, yl, pairs = ds.batch_inputs("f64")
    got = _run(dbg, x, y, xl, yl, moments=True)
    assert dbg.debug_check(_stream()) == 0, dbg.last_error()
    want = _run(ctx, x, y, xl, yl, moments=True)
    for k in ("dist", "acc", "moments"):
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
    assert np.array_equal(got["path"], want["path"]) and np.array_equal(got["path_len"], want["path_len"])
    dbg.close()


def test_python_layer():
    d = D.DTW()
    x, y, xl, yl, pairs = ds.batch_inputs("f32")
    out = d(np.nan_to_num(x), np.nan_to_num(y), xl, yl, acc=True, moments=True)
    assert out["dist"].dtype == torch.float64 and out["path"].shape == (5, 2, x.shape[1] + y.shape[1] - 1) and out["path"].dtype == torch.int32
    for b, (xb, yb) in enumerate(pairs):
        dist, D1, (p, q) = _ref(f"batch{b}_f32", xb, yb, None, 1.0)
        n = int(out["path_len"][b])
        assert bits(out["dist"][b].item()) == bits(dist) and n == len(p)
        assert np.array_equal(out["path"][b, 0, :n].cpu().numpy(), p) and np.array_equal(out["path"][b, 1, :n].cpu().numpy(), q)
        a = out["acc"][b].cpu().numpy()
        assert np.array_equal(bits(a[:len(xb), :len(yb)]), bits(D1)) and np.isnan(a[len(xb):]).all() and np.isnan(a[:, len(yb):]).all()
    # float64 when either side is; window and slope; feature rows with both
    c = ds.BY_NAME["f0_33x30_f64_w3_s0.7"]
    xc, yc = ds.inputs(c)
    o = d(T_(xc[None]), yc[None], window=3, slope=0.7)
    assert bits(o["dist"][0].item()) == bits(_ref(c["name"], xc, yc, 3, 0.7)[0])
    assert bits(d(xc[None], yc[None], window=float("inf"), path=False)["dist"][0].item()) == bits(dr.dtw(xc, yc)[0])
    c = ds.BY_NAME["feat_65x67_F2_f32"]
    xf, yf = ds.inputs(c)
    o = d(xf[None], yf[None], window=4, slope=1.3)
    dist, _, (p, q) = dr.dtw(xf, yf, 4, 1.3)
    assert bits(o["dist"][0].item()) == bits(dist) and int(o["path_len"][0]) == len(p)
    assert np.array_equal(o["path"][0, 0, :len(p)].cpu().numpy(), p) and np.array_equal(o["path"][0, 1, :len(p)].cpu().numpy(), q)

    # pitch_dtw: what scripts/pitch_dtw.py prints
    res = D.pitch_dtw([p[0] for p in pairs], [p[1] for p in pairs])
    want = [_ref(f"batch{b}_f32", *pairs[b], None, 1.0)[0] / len(pairs[b][1]) for b in range(5)]
    assert res["dtw_list"] == want and res["dtw"] == float(np.mean(want))
    moms = np.array([dr.moments(p[0]) for p in pairs[1:]])
    assert np.allclose(res["std_list"][1:], moms[:, 1], rtol=1e-9, atol=0) and np.allclose(res["skew_list"][1:], moms[:, 2], rtol=0, atol=1e-9)
    assert np.allclose(res["kurtosis_list"][1:], moms[:, 3], rtol=0, atol=1e-9) and np.isnan(res["skew"])     # the one-frame track has no skewness
    # a float64 recording makes the pair float64, as np.abs(x - y) does
    r64 = D.pitch_dtw([pairs[3][0]], [pairs[3][1].astype(np.float64)])
    assert bits(r64["dtw_list"][0]) == bits(dr.dtw(pairs[3][0].astype(np.float64), pairs[3][1].astype(np.float64))[0] / len(pairs[3][1]))

    # mel_dtw: accelerated_dtw(x, y, 'cityblock') per pair of a padded batch
    c = ds.BY_NAME["feat_65x67_F80_f32"]
    xm, ym = ds.inputs(c)
    mp, mg = np.zeros((2, 70, 80), np.float32), np.zeros((2, 67, 80), np.float32)
    mp[0, :65], mg[0] = xm, ym
    mp[1, :40], mg[1, :50] = xm[:40], ym[:50]
    o = D.mel_dtw(mp, mg, [65, 40], [67, 50])
    r0, r1 = _ref(c["name"], xm, ym, None, 1.0), dr.dtw(xm[:40], ym[:50])
    assert bits(o["dist"][0].item()) == bits(r0[0]) and bits(o["dist"][1].item()) == bits(r1[0])
    assert o["dtw"].cpu().tolist() == [r0[0] / 67, r1[0] / 50]
    assert int(o["path_len"][1]) == len(r1[2][0]) and np.array_equal(o["path"][1, 0, :len(r1[2][0])].cpu().numpy(), r1[2][0])


def test_pitch_dtw_tool_reads_an_f0_directory(tmp_path, monkeypatch, capsys):
    """tools/pitch_dtw.py DIR: NAME.npy against NAME_gt.npy by name, the four lines scripts/pitch_dtw.py prints"""
    _, _, _, _, pairs = ds.batch_inputs("f64")
    os.makedirs(tmp_path / "f0")
    names = {"zz_utt": 1, "a_utt": 3, "m_utt": 4}                      # written so that directory order is not name order
    for name, b in names.items():
        np.save(tmp_path / "f0" / f"{name}_gt.npy", pairs[b][1])
        np.save(tmp_path / "f0" / f"{name}.npy", pairs[b][0])
    spec = importlib.util.spec_from_file_location("pitch_dtw_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pitch_dtw.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["pitch_dtw.py", str(tmp_path)])
    tool.main()
    got = [float(line) for line in capsys.readouterr().out.split()]
    order = [names[n] for n in sorted(names)]
    dists = [_ref(f"batch{b}_f64", *pairs[b], None, 1.0)[0] / len(pairs[b][1]) for b in order]
    moms = np.array([dr.moments(pairs[b][0]) for b in order])
    assert got[0] == float(np.mean(dists))
    assert np.allclose(got[1:], moms[:, 1:].mean(0), rtol=1e-9, atol=1e-9)
