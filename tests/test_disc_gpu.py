"""HifiGAN's discriminators on the GPU (dict_tts_amd/discriminators.py, csrc/disc.hip, csrc/gconv.hip) against the float64 restatement
tests/disc_ref.py, which tests/test_disc_cpu.py holds against the reference.

Gates.
  * D per discriminator: max |D - D64| / max |D64| (over both signals of a pair) <= 8 x e_ref[d], e_ref[d] being the reference's own
    float32 error against its float64 in tests/golden/g16_disc.npz, normalised the same way.  The kernels and the reference's float32 form
    the same exact products and differ in summation order only (here one fp32 chain over up to K C_in = 5120 terms, there blocked), which
    changes the rounding error by a single-digit factor: hence 8, not a number chosen from these results.  The measured ratios are printed.
  * the fp64 sums: 1e-12 relative of the same sums formed in float64 from the GPU's own D (at most 1e3 terms of equal sign).
  * feature sums of map l: every element of a map is off by at most 8 x e_fm[d][l] x max |fmap| (e_fm: the reference's float32 error of
    that map, as e_ref), so the sum |a - b| over n elements by at most 2 n times that.
  * an utterance alone and inside a batch, and a second call after the workspace grew: bit-identical.
"""
import os

import numpy as np
import pytest
import torch

import disc_ref as dr
import disc_shapes as ds
from dict_tts_amd import abi, synth
from dict_tts_amd import discriminators as D

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_disc.npz")
MARGIN = 8.0


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def state():
    return synth.hifigan_disc_state_dict(ds.SEED)


@pytest.fixture(scope="module")
def w64(state):
    return D.fold_state_dict(state, np.float64)


@pytest.fixture(scope="module")
def disc(state):
    return D.Discriminators.from_checkpoint({"state_dict": {"model_disc": state}})


_REF = {}


def ref(w64, case, b):
    key = (case["name"], b)
    if key not in _REF:
        _REF[key] = dr.score_pair(w64, *ds.utterance(case, b))
    return _REF[key]


def run(disc, case, pad=3, **kw):
    y, yh, lens = ds.batch(case, pad)
    out = disc.scores(torch.from_numpy(y), torch.from_numpy(yh), lens, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def check_pair(got, b, r, golden, label):
    e_ref, e_fm = golden["e_ref"], golden["e_fm"]
    assert got["status"][b] == 0
    assert list(got["counts"][b]) == list(r["counts"])
    for d in range(8):
        n = int(r["counts"][d])
        dr_, dg_ = got["d"][d, 0, b, :n].astype(np.float64), got["d"][d, 1, b, :n].astype(np.float64)
        assert np.all(np.isnan(got["d"][d, :, b, n:]))                       # nothing written behind the outputs
        scale = max(np.abs(r["d_real"][d]).max(), np.abs(r["d_gen"][d]).max())
        err = max(np.abs(dr_ - r["d_real"][d]).max(), np.abs(dg_ - r["d_gen"][d]).max()) / scale
        print(f"{label} d{d}: n {n}, D error {err:.3e} = {err / e_ref[d]:.2f} x e_ref")
        assert err <= MARGIN * e_ref[d], (label, d, err, e_ref[d])
        own = np.array([((1 - dr_) ** 2).sum(), (dr_ ** 2).sum(), ((1 - dg_) ** 2).sum(), (dg_ ** 2).sum()])
        assert np.all(np.abs(got["sums"][b, d] - own) <= 1e-12 * own), (label, d, got["sums"][b, d], own)
        for l in range(6 if d < 5 else 8):
            cnt = int(r["fm_counts"][d, l])
            assert got["fm_counts"][b, d, l] == cnt
            bound = 2.0 * cnt * MARGIN * e_fm[d, l] * r["fmax"][d, l]
            diff = abs(got["fm"][b, d, l] - r["fm"][d, l])
            print(f"{label} d{d} map {l}: sum |delta| {got['fm'][b, d, l]:.6e} (ref {r['fm'][d, l]:.6e}), off by {diff:.2e}, bound {bound:.2e}")
            assert diff <= bound, (label, d, l, diff, bound)
        last = 5 if d < 5 else 7
        assert abs(got["fm"][b, d, last] - np.abs(dr_ - dg_).sum()) <= 1e-12 * max(np.abs(dr_ - dg_).sum(), 1e-300)


@pytest.mark.parametrize("name", [c["name"] for c in ds.CASES])
def test_case_against_restatement(disc, w64, golden, name):
    case = ds.CASE_BY_NAME[name]
    got = run(disc, case, feature_matching=True, return_d=True)
    fig_ref = []
    for b in range(len(case["lens"])):
        r = ref(w64, case, b)
        check_pair(got, b, r, golden, f"{name}.{b}")
        fig_ref.append(r)
    if case.get("kind") == "same":
        assert np.all(got["fm"][0, :5, :6] == 0) and np.all(got["fm"][0, 5:, :] == 0)
        assert np.array_equal(bits(got["sums"][0, :, 0]), bits(got["sums"][0, :, 2]))   # r and a from the same D
        assert np.array_equal(bits(got["d"][:, 0]), bits(got["d"][:, 1]))
    # the figures, per utterance and pooled: a mean of (1 - D)^2 or D^2 moves by at most 2 (1 + max |D|) dD + dD^2 per element
    want = dr.figures(np.stack([r["sums"] for r in fig_ref]), np.stack([r["counts"] for r in fig_ref]),
                      np.stack([r["fm"] for r in fig_ref]), np.stack([r["fm_counts"] for r in fig_ref]))
    dD = MARGIN * golden["e_ref"] * golden["d_max"] * 2      # (d_max: over the fixture's cases; twice it covers every case's own scale)
    tol = {"p": (2 * (1 + 2 * golden["d_max"][:5]) * dD[:5] + dD[:5] ** 2).mean(), "s": (2 * (1 + 2 * golden["d_max"][5:]) * dD[5:] + dD[5:] ** 2).mean()}
    for n in ("a_p", "r_p", "f_p", "a_s", "r_s", "f_s"):
        assert np.all(np.abs(got[n] - want[n]) <= tol[n[-1]]), (n, got[n], want[n])
        assert abs(got[n + "_batch"] - want[n + "_batch"]) <= tol[n[-1]], n


def test_mpd_alone_msd_alone(disc):
    case = ds.CASE_BY_NAME["L12_13"]
    both = run(disc, case, feature_matching=True, return_d=True)
    for which, sl, other in ((("mpd",), slice(0, 5), slice(5, 8)), (("msd",), slice(5, 8), slice(0, 5))):
        got = run(disc, case, feature_matching=True, return_d=True, which=which)
        for k in ("sums", "counts", "fm", "fm_counts"):
            assert np.array_equal(bits(got[k][:, sl]), bits(both[k][:, sl])), (which, k)
        assert np.array_equal(bits(got["d"][sl]), bits(both["d"][sl]))
        assert np.all(got["counts"][:, other] == 0) and np.all(np.isnan(got["sums"][:, other])) and np.all(np.isnan(got["d"][other]))
    plain = run(disc, case)                                   # no feature sums, no D
    assert "fm" not in plain and np.array_equal(bits(plain["sums"]), bits(both["sums"]))


def test_alone_equals_in_batch(disc):
    case = ds.CASE_BY_NAME["mixed"]
    inb = run(disc, case, pad=5, feature_matching=True, return_d=True)
    for b, L in enumerate(case["lens"]):
        y, yh = ds.utterance(case, b)
        out = disc.scores(torch.from_numpy(y)[None], torch.from_numpy(yh)[None], feature_matching=True, return_d=True)
        torch.cuda.synchronize()
        one = {k: v.cpu().numpy() for k, v in out.items()}
        for k in ("sums", "counts", "fm", "fm_counts"):
            assert np.array_equal(bits(one[k][0]), bits(inb[k][b])), (b, k)
        n = one["d"].shape[3]
        assert np.array_equal(bits(one["d"][:, :, 0, :]), bits(inb["d"][:, :, b, :n])), b


def test_device_lengths_mark_a_short_pair(disc):
    case = ds.CASE_BY_NAME["L12_13"]
    y, yh, lens = ds.batch(case)
    bad = torch.tensor([5, int(lens[1])], dtype=torch.int32, device="cuda")
    out = disc.scores(torch.from_numpy(y), torch.from_numpy(yh), bad)
    good = disc.scores(torch.from_numpy(y), torch.from_numpy(yh), lens)
    torch.cuda.synchronize()
    assert out["status"].tolist() == [abi.DISC_TOO_SHORT, 0]
    assert out["counts"][0].tolist() == [0] * 8 and np.all(out["sums"][0].cpu().numpy() == 0)
    assert np.array_equal(bits(out["sums"][1].cpu().numpy()), bits(good["sums"][1].cpu().numpy()))


def test_memory_safety_and_grown_workspace(state, disc):
    """debug_redzone = 1: every workspace buffer sits between red zones and starts out as 0xFF; no launch damages a zone, no stale word
    reaches an output; and a call after the workspace grew equals the call before"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg_ctx = abi.Context(cfg)
    dbg = D.Discriminators.from_checkpoint(state, ctx=dbg_ctx)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    small, large = ds.CASE_BY_NAME["L12_13"], ds.CASE_BY_NAME["mixed"]
    first = run(dbg, small, feature_matching=True, return_d=True)
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    big = run(dbg, large, feature_matching=True, return_d=True)          # the workspace grows
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    second = run(dbg, small, feature_matching=True, return_d=True)
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    plain_small = run(disc, small, feature_matching=True, return_d=True)
    plain_big = run(disc, large, feature_matching=True, return_d=True)
    for k in ("sums", "counts", "fm", "fm_counts", "d"):
        assert np.array_equal(bits(first[k]), bits(second[k])), k
        assert np.array_equal(bits(first[k]), bits(plain_small[k])), k
        assert np.array_equal(bits(big[k]), bits(plain_big[k])), k
    dbg_ctx.close()


def test_finalize_names_what_is_wrong(state):
    """DTTS_E_NOENT names the first missing tensor, DTTS_E_INVAL the layer whose shape is not the reference architecture's"""
    w = D.fold_state_dict(state)
    ctx = abi.Context()
    ctx.load_state_dict("disc", {k: v for k, v in w.items() if k != "msd.1.convs.3.bias"})
    with pytest.raises(abi.DttsError, match=r"\(-2\).*missing tensor disc\.msd\.1\.convs\.3\.bias"):
        ctx.finalize(abi.PART_DISC)
    ctx.close()
    ctx = abi.Context()
    ctx.load_state_dict("disc", {**w, "msd.2.convs.2.weight": np.zeros((256, 16, 41), np.float32)})   # groups = 8 instead of 16
    with pytest.raises(abi.DttsError, match=r"\(-22\).*disc\.msd\.2\.convs\.2\.weight is \[256, 16, 41\].*\[256, 8, 41\]"):
        ctx.finalize(abi.PART_DISC)
    y = torch.zeros(1, 64, device="cuda")
    sums, counts, status = torch.zeros(1, 8, 4, dtype=torch.float64, device="cuda"), torch.zeros(1, 8, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(abi.DttsError, match=r"before dtts_finalize_weights\(DTTS_PART_DISC\)"):
        ctx.disc(1, torch.cuda.current_stream().cuda_stream, y=y.data_ptr(), y_hat=y.data_ptr(), wav_ld=64, sums=sums.data_ptr(), counts=counts.data_ptr(),
                 status=status.data_ptr())
    ctx.close()
