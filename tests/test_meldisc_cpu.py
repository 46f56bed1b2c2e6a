"""The multi-window mel discriminator without a GPU: the float64 restatement (tests/meldisc_ref.py) against the reference's own float64
and float32 runs (tests/golden/g17_meldisc.npz, written by tools/make_golden_meldisc.py), forward's None and x_len rules, BatchNorm's eps,
the loader on every norm layout and its refusals, the argument block through the library without a handle, and the ABI constants.

Bounds.  Restatement against the reference's float64: 1e-12 of max |.| — both are float64 over at most 9 x 128 = 1152 terms per output and
three layers and differ in summation order only.  Against the reference's float32: its own float32 error (e_ref / e_h) plus that.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meldisc_ref as mr
import meldisc_shapes as ms
from dict_tts_amd import abi, synth
from dict_tts_amd import mel_discriminator as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_meldisc.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_W64 = {}


def w64(run):
    rid = ms.run_id(run)
    if rid not in _W64:
        _W64[rid] = M.fold_state_dict(synth.mel_disc_state_dict(ms.SEED, run[0], run[1], run[3], run[2]), np.float64)
    return _W64[rid]


@pytest.mark.parametrize("run,name", ms.RUN_CASES, ids=[f"{ms.run_id(r)}-{n}" for r, n in ms.RUN_CASES])
def test_restatement_against_reference(golden, run, name):
    case, rid, W = ms.CASE_BY_NAME[name], ms.run_id(run), w64(run)
    for b in range(len(case["lens"])):
        g, p = ms.utterance(case, b)
        starts = [ms.starts_of(case, b, win) for win in ms.WINS[:run[3]]]
        r = mr.score_utterance(W, g, p, starts)
        for w in range(run[3]):
            assert r["counts"][0, w] == r["counts"][1, w] == len(starts[w]) * (ms.WINS[w] // 8 if run[2] == "none" else 1)
            if not starts[w]:
                assert name in ("short", "w32_edge", "w64_edge", "w128_edge", "mixed", "same", "zeros")
                continue
            scale = max(np.abs(golden[f"{rid}.{name}.{b}.{s}.{w}.f64"]).max() for s in "gp")
            for sig, mine in (("g", r["d_g"][w]), ("p", r["d_p"][w])):
                g64, g32 = golden[f"{rid}.{name}.{b}.{sig}.{w}.f64"], golden[f"{rid}.{name}.{b}.{sig}.{w}.f32"].astype(np.float64)
                assert mine.shape == g64.shape
                e64, e32 = np.abs(mine - g64).max() / scale, np.abs(mine - g32).max() / scale
                print(f"{rid} {name}.{b} {sig} w{w}: vs f64 {e64:.2e}, vs f32 {e32:.2e} (e_ref {golden['e_ref.' + rid][w]:.2e})")
                assert e64 <= 1e-12
                assert e32 <= golden["e_ref." + rid][w] + 1e-12
        if name == "short":
            assert np.all(r["counts"] == 0) and np.all(r["sums"] == 0)
        if case.get("kind") == "same":
            assert np.array_equal(r["sums"][0], r["sums"][1])


@pytest.mark.parametrize("norm", ["in", "bn", "sn"])
def test_hidden_maps_against_reference(golden, norm):
    run = (norm, 128, "stack", 3, None)
    rid = ms.run_id(run)
    g, _ = ms.utterance(ms.CASE_BY_NAME[ms.HIDDEN_CASE], ms.HIDDEN_B)
    _, h = mr.window_forward(w64(run), 0, g[ms.HIDDEN_START:ms.HIDDEN_START + 32])
    for l in range(3):
        g64, g32 = golden[f"h.{rid}.{l}.f64"], golden[f"h.{rid}.{l}.f32"].astype(np.float64)
        mine = h[l][ms.HIDDEN_CH]
        assert mine.shape == g64.shape == (8, 16 >> l, 40 >> l)
        assert np.abs(mine - g64).max() <= 1e-12 * np.abs(g64).max()
        assert np.abs(mine - g32).max() <= (golden["e_h." + rid][l] + 1e-12) * np.abs(h[l]).max()


@pytest.mark.parametrize("run", [r for r in ms.RUNS if r[1] == 128 and r[3] == 3], ids=ms.run_id)
def test_forward_against_reference(golden, run):
    rid, W = ms.run_id(run), w64(run)
    for fw in ms.FORWARD:
        x = ms.batch(ms.CASE_BY_NAME[fw["case"]], fill=0.0)[0]
        y, h = mr.forward(W, run[2], x, fw["starts"])
        k = f"{rid}.{fw['name']}"
        assert (y is None) == bool(golden[k + ".y_none"]) and len(h) == int(golden[k + ".n_h"])
        if y is None:
            assert fw["name"] == "fw_none" and len(h) == 6
            continue
        g64 = golden[k + ".y.f64"]
        assert y.shape == g64.shape
        assert np.abs(y - g64).max() <= 1e-12 * np.abs(g64).max() * (3 if run[2] == "sum" else 1)


def test_x_len_counts_the_frames_that_do_not_sum_to_zero():
    x = np.ones((2, 40, 80))
    x[0, 35:] = 0
    x[1, 10] = 0                               # a silent frame inside an utterance is not counted either
    x[1, 11, :40], x[1, 11, 40:] = 1.0, -1.0   # nor is one whose bins cancel
    assert list(mr.x_len_of(x)) == [35, 38]
    W = w64(ms.RUNS[0])
    x = np.zeros((1, 40, 80))
    x[0, :31] = -2.0
    assert mr.forward(W, "stack", x, [0, 0, 0])[0] is None     # 31 frames: not even the 32-frame window runs
    x[0, 31] = -2.0
    y, h = mr.forward(W, "stack", x, [0, 0, 0])
    assert y is None and len(h) == 3


def test_batchnorm_eps_is_0_8():
    sd = synth.mel_disc_state_dict(3, "bn", 32, 1)
    w = M.fold_state_dict(sd, np.float64)
    n = "discriminator.conv_layers.0.model.1.3"
    want = sd[n + ".weight"].astype(np.float64) / np.sqrt(sd[n + ".running_var"].astype(np.float64) + 0.8)
    assert np.allclose(w["0.affine.1.scale"], want, rtol=1e-15)
    assert np.allclose(w["0.affine.1.shift"], sd[n + ".bias"] - sd[n + ".running_mean"].astype(np.float64) * want, rtol=1e-15, atol=1e-18)
    wrong = sd[n + ".weight"].astype(np.float64) / np.sqrt(sd[n + ".running_var"].astype(np.float64) + 1e-5)
    assert np.abs(w["0.affine.1.scale"] - wrong).max() > 0.05
    assert M.BN_EPS == 0.8 and "0.norm.1.weight" not in w


def test_loader_layouts_and_refusals(tmp_path):
    import torch
    sd = synth.mel_disc_state_dict(5, "in", 64, 2, "none")
    plain = M.fold_state_dict(sd)
    assert M.describe(plain) == (2, 64, "in", True)
    assert M.check_hparams(None, plain) == (2, 64, "in", "none")
    hp = {"disc_win_num": 2, "mel_disc_hidden_size": 64, "disc_norm": "in", "disc_reduction": "none", "audio_num_mel_bins": 80}
    assert M.check_hparams(hp, plain) == (2, 64, "in", "none")
    assert M.mel_disc_of({"state_dict": {"model": {}, "mel_disc": sd}}) is sd
    assert set(M.mel_disc_of({"mel_disc." + k: v for k, v in sd.items()})) == set(sd)
    assert M.mel_disc_of(sd) is sd
    torch.save({"state_dict": {"model": {}, "mel_disc": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}}, tmp_path / "model_ckpt_steps_7.ckpt")
    torch.save({"state_dict": {"model": {}}}, tmp_path / "model_ckpt_steps_3.ckpt")
    assert set(M.mel_disc_of(str(tmp_path))) == set(sd)
    assert set(M.mel_disc_of(str(tmp_path / "model_ckpt_steps_7.ckpt"))) == set(sd)
    md = M.MelDiscriminator.from_checkpoint(str(tmp_path), hparams=hp)
    assert (md.win_num, md.hidden, md.norm, md.reduction) == (2, 64, "in", "none")
    with pytest.raises(KeyError, match="no mel_disc"):
        M.mel_disc_of(str(tmp_path / "model_ckpt_steps_3.ckpt"))
    for key, val, match in (("disc_win_num", 3, r"disc_win_num = 3 but the checkpoint's mel_disc has 2"),
                            ("mel_disc_hidden_size", 128, r"mel_disc_hidden_size = 128 but the checkpoint's mel_disc has 64"),
                            ("disc_norm", "bn", r"disc_norm = 'bn' but the checkpoint's mel_disc holds the tensors of 'in'"),
                            ("disc_norm", "ln", r"disc_norm = 'ln'"),
                            ("disc_reduction", "stack", r"disc_reduction = 'stack' but the checkpoint's adv_layer is per time row"),
                            ("disc_reduction", "mean", r"disc_reduction = 'mean'"),
                            ("audio_num_mel_bins", 100, r"audio_num_mel_bins = 100")):
        with pytest.raises(ValueError, match=match):
            M.MelDiscriminator.from_checkpoint(sd, hparams={**hp, key: val})
    with pytest.raises(ValueError, match=r"cond_disc\.conv_layers\.0"):
        M.fold_state_dict({**sd, "cond_disc.conv_layers.0.adv_layer.weight": np.zeros((1, 640), np.float32)})
    broken = dict(synth.mel_disc_state_dict(5, "sn", 32, 1))
    del broken["discriminator.conv_layers.0.model.1.0.weight_u"]
    with pytest.raises(KeyError, match=r"model\.1\.0\.weight_u"):
        M.fold_state_dict(broken)
    with pytest.raises(ValueError, match=r"mel_disc_hidden_size = 48"):
        M.MelDiscriminator(M.fold_state_dict(synth.mel_disc_state_dict(5, "in", 48, 1)))
    with pytest.raises(ValueError, match=r"mel_disc_hidden_size = 288"):
        M.MelDiscriminator(M.fold_state_dict(synth.mel_disc_state_dict(5, "in", 288, 1)))
    bad = dict(plain)
    bad["1.adv.weight"] = np.zeros((1, 64 * 10 * 4), np.float32)
    with pytest.raises(ValueError, match=r"conv_layers\.1\.adv_layer\.weight has 2560 inputs; the 64-frame window's head has 640"):
        M.MelDiscriminator(bad)
    # the spectral layer really is normalised (u, v from power iterations, not random)
    sn = M.fold_state_dict(synth.mel_disc_state_dict(5, "sn", 64, 1), np.float64)
    assert 1.0 - 1e-6 <= np.linalg.norm(sn["0.conv.1.weight"].reshape(64, -1), 2) < 1.1
    # refusals of the inputs, without a GPU
    md = M.MelDiscriminator(plain)
    with pytest.raises(ValueError, match="audio_num_mel_bins = 100"):
        md.scores(np.zeros((1, 40, 100), np.float32), np.zeros((1, 40, 100), np.float32))
    with pytest.raises(ValueError, match=r"lens\[1\] = 41"):
        md.scores(np.zeros((2, 40, 80), np.float32), np.zeros((2, 40, 80), np.float32), lens=[40, 41])
    with pytest.raises(ValueError, match=r"start_frames_wins\[0\] = 20"):
        md.forward(np.ones((1, 40, 80), np.float32), [[20], [0]])
    out = md.forward(np.ones((1, 31, 80), np.float32))          # nothing fits: no device needed
    assert out["y"] is None and out["h"] == [] and out["start_frames_wins"] == [None, None]
    assert M.hop_starts(200, 128) == [0, 64] and M.hop_starts(33, 32, 1) == [0, 1] and M.hop_starts(31, 32) == []


def test_fixture_is_sane(golden):
    for run in ms.RUNS:
        rid = ms.run_id(run)
        assert np.all(golden["e_ref." + rid] > 0) and np.all(golden["e_ref." + rid] < 1e-4)
        assert np.all(golden["e_h." + rid] > 0) and np.all(golden["e_h." + rid] < 1e-4)
        assert np.all((golden["d_max." + rid] >= 1e-3) & (golden["d_max." + rid] <= 1e3))
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    # data only: arrays of numbers
    assert all(golden[k].dtype.kind in "fi" for k in golden.files)


def test_abi_constants_struct_and_exports():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    val = lambda n: int(re.search(rf"#define {n} (\d+)", hdr).group(1))
    assert val("DTTS_PART_MELDISC") == abi.PART_MELDISC == 512
    assert val("DTTS_OUT_MELDISC") == abi.OUT_MELDISC == 21
    assert (val("DTTS_MELDISC_STACK"), val("DTTS_MELDISC_SUM"), val("DTTS_MELDISC_NONE")) == (abi.MELDISC_STACK, abi.MELDISC_SUM, abi.MELDISC_NONE)
    assert val("DTTS_MELDISC_WITHIN_LEN") == abi.MELDISC_WITHIN_LEN and val("DTTS_MELDISC_BAD_LEN") == abi.MELDISC_BAD_LEN
    assert (val("DTTS_MELDISC_MELS"), val("DTTS_MELDISC_MAX_WIN"), val("DTTS_MELDISC_D_LD"), val("DTTS_MELDISC_MAX_HIDDEN")) == (
        abi.MELDISC_MELS, abi.MELDISC_MAX_WIN, abi.MELDISC_D_LD, abi.MELDISC_MAX_HIDDEN) == (80, 3, 16, 256)
    A = abi.MeldiscArgs
    assert C.sizeof(A) == 176
    assert [getattr(A, f).offset for f in ("size", "n_sig", "T_ld", "n_win", "reduction", "flags", "clips_ld", "hop", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 40]
    assert [getattr(A, f).offset for f in ("mel_dev", "lens_dev", "starts_dev", "d_dev", "sums_dev", "counts_dev", "status_dev", "h_dev")] == [
        48, 56, 64, 72, 80, 88, 96, 104]
    # the unit is an item of dtts_text2mel_fetch: no new entry point
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "meldisc" in s]
    assert "meldisc" not in open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()


def test_argument_block_refusals_without_a_handle():
    lib = abi.load_library()
    good = dict(n_sig=2, mel=4096, T_ld=200, n_win=3, clips_ld=4, sums=4096, counts=4096, status=4096, hop=(16, 32, 64))

    def refused(match, **kw):
        a = abi.meldisc_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_MELDISC, C.byref(a), None) == -22   # DTTS_E_INVAL
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"n_sig = 0", n_sig=0)
    refused(r"n_sig = 65536", n_sig=65536)
    refused(r"T_ld = 0", T_ld=0)
    refused(r"T_ld = 1048577", T_ld=(1 << 20) + 1)
    refused(r"n_win = 0", n_win=0)
    refused(r"n_win = 4", n_win=4)
    refused(r"reduction = 3", reduction=3)
    refused(r"flags = 2", flags=2)
    refused(r"clips_ld = 0", clips_ld=0)
    refused(r"clips_ld = 65536 for n_sig = 512", clips_ld=65536, n_sig=512)
    refused(r"hop\[1\] = 0 frames without starts_dev", hop=(16, 0, 64))
    refused(r"null mel_dev", mel=0)
    refused(r"null mel_dev", sums=0)
    refused(r"null mel_dev", status=0)
    refused(r"mel_dev = .* is not aligned to 4 bytes", mel=4098)
    refused(r"starts_dev = .* is not aligned to 4 bytes", starts=4098)
    refused(r"sums_dev = .* is not aligned to 8 bytes", sums=4100)
    refused(r"h_dev\[4\] = .* is not aligned to 4 bytes", h=(None,) * 4 + (4097,) + (None,) * 4)
    a = abi.meldisc_args(**good)
    a.size -= 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_MELDISC, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.MeldiscArgs) - 8}" in lib.dtts_last_error(None).decode()
    a = abi.meldisc_args(**good)
    a.reserved[1] = 1
    assert lib.dtts_text2mel_fetch(None, abi.OUT_MELDISC, C.byref(a), None) == -22
    assert "reserved" in lib.dtts_last_error(None).decode()
    refused(r"null handle")                                      # a good block: only then is the handle looked at
    refused(r"null handle", hop=(0, 0, 0), starts=4096)
    assert lib.dtts_text2mel_fetch(None, abi.OUT_MELDISC, None, None) == -22
