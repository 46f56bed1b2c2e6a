"""The validation losses, the parts that need no GPU: the ABI surface of dtts_text2mel_fetch(DTTS_OUT_LOSSES), the Python-side rules
(parse_mel_loss, ssim_window) and the float64 restatement (tests/losses_ref.py) against the reference's own float32 outputs
(tests/golden/g13_losses.npz, written by tools/make_golden_losses.py).

The tolerance between the float64 restatement and the reference's float32 figures was MEASURED on the fixture (the reference's float32
conv2d result moves with thread count and BLAS path; LABNOTES.md "Validation losses").  Largest relative deviation per figure over the
cases: l1 1.1e-7, mse 1.4e-7, ssim 1.3e-5; wdur 4.9e-7, sdur 2.8e-4 (a difference of two float32 sums of about 300 that nearly cancel),
wdur_train 1.1e-7; the two stored SSIM maps deviate by up to 2.0e-3 absolute (|ssim| <= 1).  The gates are 4 x those.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import losses_ref as lr
import losses_shapes as ls
from dict_tts_amd import abi
from dict_tts_amd import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEL_REL = 4 * np.array([1.1e-7, 1.4e-7, 1.3e-5])    # l1, mse, ssim
DUR_REL = 4 * np.array([4.9e-7, 2.8e-4, 1.1e-7])    # wdur, sdur, wdur_train
MAP_ABS = 4 * 2.0e-3


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_losses.npz"))


def test_argument_block_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert int(re.search(r"#define DTTS_OUT_LOSSES (\d+)", hdr).group(1)) == abi.OUT_LOSSES == 14
    assert int(re.search(r"#define DTTS_LOSS_TILE_ROWS (\d+)", hdr).group(1)) == abi.LOSS_TILE_ROWS
    assert int(re.search(r"#define DTTS_LOSS_MAX_WORDS (\d+)", hdr).group(1)) == abi.LOSS_MAX_WORDS
    body = re.search(r"typedef struct dtts_loss_args \{(.*?)\} dtts_loss_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.search(r"([A-Za-z_0-9]+)$", part.strip()).group(1) for part in decl.split(",")]
    assert names == [f[0] for f in abi.LossArgs._fields_], names
    assert C.sizeof(abi.LossArgs) == 12 * 4 + 10 * C.sizeof(C.c_void_p)
    assert abi.LossArgs.pred_dev.offset == 48 and abi.LossArgs.bias.offset == 24
    # the ABI keeps its entry points: the unit is an item of dtts_text2mel_fetch
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "loss" in s]
    exports = open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()
    assert "loss" not in exports


def test_losses_on_a_null_handle_is_invalid():
    lib = abi.load_library()
    args = abi.LossArgs(C.sizeof(abi.LossArgs))
    assert lib.dtts_text2mel_fetch(None, abi.OUT_LOSSES, C.byref(args), None) == -22   # DTTS_E_INVAL


def test_ssim_window_is_the_references(g13):
    w = L.ssim_window()
    assert w.dtype == np.float32 and w.shape == (11, 11)
    assert np.array_equal(w, g13["window"])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(w, w.T)


def test_parse_mel_loss(g13):
    got = L.parse_mel_loss(str(g13["mel_loss_spec"]))
    assert list(got.keys()) == [str(n) for n in g13["mel_loss_names"]]
    assert list(got.values()) == [float(v) for v in g13["mel_loss_lambdas"]]
    assert L.parse_mel_loss("ssim:0.5|l1:0.5") == {"ssim": 0.5, "l1": 0.5}
    assert L.parse_mel_loss("l1") == {"l1": 1.0} and L.parse_mel_loss("l1||mse:2") == {"l1": 1.0, "mse": 2.0}
    with pytest.raises(NotImplementedError, match="gdl"):
        L.parse_mel_loss("l1:0.5|gdl:0.5")
    with pytest.raises(ValueError, match="huber"):
        L.parse_mel_loss("huber")


def test_argument_errors_surface_without_a_gpu():
    v = L.ValidationLosses(hparams={})
    assert v.loss_and_lambda == {"ssim": 0.5, "l1": 0.5} and v.lambda_kl == 1.0 and v.dur_scale == "log"
    with pytest.raises(ValueError, match="n_mel"):
        v.mel(np.zeros((1, 4, 129), np.float32), np.zeros((1, 4, 129), np.float32))
    with pytest.raises(ValueError, match=r"\[B, T, n_mel\]"):
        v.mel(np.zeros((1, 4, 80), np.float32), np.zeros((1, 5, 80), np.float32))
    with pytest.raises(ValueError, match="dur_scale"):
        v.dur(np.zeros((1, 4), np.float32), np.zeros((1, 9), np.int64), [4], dur_scale="sqrt")
    with pytest.raises(ValueError, match="word_lengths"):
        v.dur(np.zeros((2, 4), np.float32), np.zeros((2, 9), np.int64), [4])
    with pytest.raises(NotImplementedError, match="gdl"):
        L.ValidationLosses(hparams={"mel_loss": "gdl"})
    with pytest.raises(NotImplementedError, match="dur_level"):
        L.ValidationLosses(hparams={"dur_level": "ph"})
    with pytest.raises(ValueError, match="lambda_sent_dur"):
        L.ValidationLosses(hparams={"lambda_sent_dur": 1.0})


def test_case_list_covers_the_window_and_the_tile():
    R = abi.LOSS_TILE_ROWS
    Ts = {c["T"] for c in ls.MEL_CASES if c["n_mel"] == 80}
    assert {1, 5, 6, 10, 11, R - 1, R, R + 1, 2 * R + 3} <= Ts
    assert {c["n_mel"] for c in ls.MEL_CASES if c["T"] == R + 1} >= {1, 11, 20, 80, 128}
    assert {c["T_w"] for c in ls.DUR_CASES} == {1, 7, 64, 300} and {c["scale"] for c in ls.DUR_CASES} == {"log", "linear"}
    pred, tgt, _ = ls.mel_inputs(ls.MEL_BY_NAME["ld_poisoned"])
    assert pred.shape[1] == R + 4 and tgt.shape[1] == R + 6 and np.isnan(pred[:, R + 1:]).all() and np.isnan(tgt[:, R + 1:]).all()
    _, tgt, _ = ls.mel_inputs(ls.MEL_BY_NAME["zero_row_seam"])
    assert not tgt[2, R - 1].any() and not tgt[2, R].any() and not tgt[0, 2 * R].any() and tgt[2, R + 1].any()


@pytest.mark.parametrize("case", ls.MEL_CASES, ids=lambda c: c["name"])
def test_float64_restatement_matches_reference_golden_g13_mel(g13, case):
    pred, tgt, _ = ls.mel_inputs(case)
    k = "mel." + case["name"]
    assert np.allclose(ls.fingerprint(pred, tgt), g13[k + ".fp"], rtol=1e-12, atol=0)
    T = case["T"]
    sums, count, m = lr.mel_sums64(pred[:, :T], tgt[:, :T])
    got, want = lr.batch_figures(sums, count), g13[k + ".losses"].astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"{k}: l1 / mse / ssim relative deviation from the reference's float32 {rel}")
    assert np.isfinite(got).all() and (rel <= MEL_REL).all(), (got, want, rel)
    if k + ".ssim_map" in g13:
        dev = np.abs(m - g13[k + ".ssim_map"]).max()
        print(f"{k}: SSIM map max deviation {dev:.3e}")
        assert dev <= MAP_ABS, dev
    if case["all_zero"] is not None:
        b = case["all_zero"]
        assert count[b] == 0 and not sums[b].any()


@pytest.mark.parametrize("case", ls.DUR_CASES, ids=lambda c: c["name"])
def test_float64_restatement_matches_reference_golden_g13_dur(g13, case):
    dp, m2w, wl = ls.dur_inputs(case)
    k = "dur." + case["name"]
    assert np.allclose(ls.fingerprint(dp, m2w, wl), g13[k + ".fp"], rtol=1e-12, atol=0)
    sums, d = lr.dur_sums64(dp, m2w, wl, case["scale"])
    assert np.array_equal(d, g13[k + ".dur_gt"])                      # exact
    if case["T_w"] > 2:
        assert wl[0] == case["T_w"] and (d[0] == 0).any() and wl[1] < case["T_w"] and (d[1, wl[1]:] > 0).any()
        assert (m2w[:, :5] == 0).any() and not m2w[:, -3:].any()
    got, want = np.array(lr.dur_figures(sums)), g13[k + ".losses"].astype(np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"{k}: wdur / sdur / wdur_train relative deviation from the reference's float32 {rel}")
    assert (rel <= DUR_REL).all(), (got, want, rel)

