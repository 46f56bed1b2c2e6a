"""HifiGAN's discriminators without a GPU: the float64 restatement (tests/disc_ref.py) against the reference's own float64 and float32 runs
(tests/golden/g16_disc.npz, written by tools/make_golden_disc.py), the weight folding against what the reference's modules hold after a
load, the loader on every norm layout, the refusals of the argument block through the library without a handle, and the ABI constants.

Bounds.  Restatement against the reference's float64: 1e-10 of max |D| — both are float64 over at most K C_in = 5120 terms per output and
eight layers and differ only in summation order (5120 x 1.1e-16 x 8 layers is 5e-12 before cancellation).  Against the reference's
float32: ``e_ref[d]``, the reference's own float32 error, plus the 1e-10 above.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import disc_ref as dr
import disc_shapes as ds
from dict_tts_amd import abi, synth
from dict_tts_amd import discriminators as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_disc.npz")
NAMES = ["a_p", "r_p", "f_p", "fm_f", "a_s", "r_s", "f_s", "fm_s"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def state():
    return synth.hifigan_disc_state_dict(ds.SEED)


@pytest.fixture(scope="module")
def w64(state):
    return D.fold_state_dict(state, np.float64)


_SCORED = {}


def scored(w64, case, b):
    key = (case["name"], b)
    if key not in _SCORED:
        y, yh = ds.utterance(case, b)
        _SCORED[key] = dr.score_pair(w64, y, yh)
    return _SCORED[key]


PAIRS = [(c["name"], b) for c in ds.CASES for b in range(len(c["lens"]))]


@pytest.mark.parametrize("name,b", PAIRS)
def test_restatement_against_reference(golden, w64, name, b):
    case = ds.CASE_BY_NAME[name]
    r = scored(w64, case, b)
    k = f"{name}.{b}"
    counts = golden[k + ".d_counts"]
    assert list(r["counts"]) == list(counts)
    assert [ds.d_count(d, case["lens"][b]) for d in range(8)] == list(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    for d in range(8):
        # normalised as e_ref is: by max |D64| over both signals of the pair
        scale = max(np.abs(golden[f"{k}.{sig}.f64"][off[d]:off[d + 1]]).max() for sig in ("d_real", "d_gen"))
        for sig, mine in (("d_real", r["d_real"][d]), ("d_gen", r["d_gen"][d])):
            g64 = golden[f"{k}.{sig}.f64"][off[d]:off[d + 1]]
            g32 = golden[f"{k}.{sig}.f32"][off[d]:off[d + 1]].astype(np.float64)
            e64 = np.abs(mine - g64).max() / scale
            e32 = np.abs(mine - g32).max() / scale
            print(f"{k} d{d} {sig}: vs f64 {e64:.2e}, vs f32 {e32:.2e} (e_ref {golden['e_ref'][d]:.2e})")
            assert e64 <= 1e-10
            assert e32 <= golden["e_ref"][d] + 1e-10
    fig = dr.figures(r["sums"][None], r["counts"][None], r["fm"][None], r["fm_counts"][None])
    want = dict(zip(NAMES, golden[k + ".figures.f64"]))
    for n in NAMES:
        assert abs(fig[n][0] - want[n]) <= 1e-10 * max(1.0, abs(want[n])), (n, fig[n][0], want[n])
        assert abs(fig[n + "_batch"] - want[n]) <= 1e-10 * max(1.0, abs(want[n]))   # one utterance: pooled = per utterance
    gfm = golden[k + ".fm.f64"]
    for d in range(8):
        for l in range(6 if d < 5 else 8):
            assert abs(r["fm"][d, l] - gfm[d, l]) <= 1e-10 * max(gfm[d, l], r["fm_counts"][d, l] * r["fmax"][d, l]), (d, l)
    if case.get("kind") == "same":
        assert np.all(r["fm"][:5, :6] == 0) and np.all(r["fm"][5:] == 0)
        assert np.array_equal(r["sums"][:, 0], r["sums"][:, 2])


def test_fixture_is_sane(golden):
    assert int(golden["min_len"]) == abi.DISC_MIN_LEN == dr.MIN_LEN == 6
    assert np.all((golden["d_max"] >= 1e-3) & (golden["d_max"] <= 1e3))
    assert np.all(golden["e_ref"] > 0) and np.all(golden["e_ref"] < 1e-4)
    assert os.path.getsize(GOLDEN) < 600 * 1024


def test_shortest_length_is_refused_by_the_restatement(w64):
    with pytest.raises(ValueError):
        dr.mpd_forward(w64, 4, np.zeros(5))


def test_weight_folding_against_the_reference_modules(golden, state):
    w = D.fold_state_dict(state)
    assert len(w) == 2 * (5 * 6 + 3 * 8)
    for k in [k for k in golden.files if k.startswith("fold.")]:
        mine = w[k[len("fold."):] + ".weight"].astype(np.float64)
        s, a, first, last = golden[k]
        assert abs(np.abs(mine).sum() - a) <= 1e-6 * a, k
        assert abs(mine.sum() - s) <= 1e-6 * a, k
        # float32 folds differ in the norm's summation order (1 ulp of the norm) and by the roundings of g / n and v * (g / n): 4 x 2^-23
        assert abs(mine.flat[0] - first) <= 4.8e-7 * abs(first) + 1e-12 and abs(mine.flat[-1] - last) <= 4.8e-7 * abs(last) + 1e-12, k
    # the spectral layer really is normalised: u . (W v) of a few power iterations bounds the spectral norm from below, so the folded
    # layer's gain is 1 or slightly above (not the 1e25 of random u, v)
    m = w["msd.0.convs.3.weight"].reshape(512, -1).astype(np.float64)
    assert 1.0 - 1e-6 <= np.linalg.norm(m, 2) < 1.1


def test_loader_layouts_and_refusals(state):
    plain = D.fold_state_dict(state)
    # already-plain weights under the checkpoint's names, nested as a checkpoint is
    as_ckpt = {"state_dict": {"model_gen": {}, "model_disc": {}}}
    for src, dst in D._layer_names():
        as_ckpt["state_dict"]["model_disc"][src + ".weight"] = plain[dst + ".weight"]
        as_ckpt["state_dict"]["model_disc"][src + ".bias"] = plain[dst + ".bias"]
    again = D.fold_state_dict(D.model_disc_of(as_ckpt))
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    flat = {"model_disc." + k: v for k, v in state.items()}
    assert set(D.model_disc_of(flat)) == set(state)
    assert D.model_disc_of(state) is state
    with pytest.raises(KeyError, match="no model_disc"):
        D.model_disc_of({"state_dict": {"model_gen": {"conv_pre.bias": np.zeros(1)}}})
    with pytest.raises(ValueError, match="use_cond_disc"):
        D.fold_state_dict({**state, "mpd.discriminators.0.cond_net.weight": np.zeros((80, 1, 512), np.float32)})
    with pytest.raises(ValueError, match="use_spec_disc"):
        D.fold_state_dict({**state, "specd.layers.0.weight": np.zeros(1, np.float32)})
    with pytest.raises(ValueError, match="use_cond_disc"):
        D.Discriminators.from_checkpoint(state, hparams={"use_cond_disc": True})
    with pytest.raises(ValueError, match="use_spec_disc"):
        D.Discriminators.from_checkpoint(state, hparams={"use_spec_disc": True})
    broken = dict(state)
    del broken["msd.discriminators.0.convs.2.weight_u"]
    with pytest.raises(KeyError, match=r"msd\.discriminators\.0\.convs\.2\.weight_u"):
        D.fold_state_dict(broken)
    # weight norm and spectral norm in float64 from the float32 parameters
    g, v = state["mpd.discriminators.1.convs.1.weight_g"], state["mpd.discriminators.1.convs.1.weight_v"]
    w = D.fold_weight_norm(g, v, np.float64)
    assert np.allclose(np.sqrt((w.reshape(128, -1) ** 2).sum(1)), g.reshape(-1).astype(np.float64), rtol=1e-12)


def test_python_refuses_short_lengths_without_a_gpu(state):
    disc = D.Discriminators(D.fold_state_dict({k: v for k, v in state.items()}))
    y = np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match=r"lens\[1\] = 5 samples is below DISC_MIN_LEN = 6"):
        disc.scores(y, y, lens=[64, 5])
    with pytest.raises(ValueError, match="DISC_MIN_LEN"):
        disc.scores(y[:, :5], y[:, :5])
    with pytest.raises(ValueError, match="which"):
        disc.scores(y, y, which=("specd",))
    with pytest.raises(ValueError, match=r"lens\[0\] = 65"):
        disc.scores(y, y, lens=[65, 64])


def test_abi_constants_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    val = lambda n: int(re.search(rf"#define {n} (\d+)", hdr).group(1))
    assert val("DTTS_PART_DISC") == abi.PART_DISC == 128
    assert val("DTTS_OUT_DISC") == abi.OUT_DISC == 19
    assert (val("DTTS_DISC_MPD"), val("DTTS_DISC_MSD"), val("DTTS_DISC_FM")) == (abi.DISC_MPD, abi.DISC_MSD, abi.DISC_FM)
    assert val("DTTS_DISC_DENSE_GROUPED") == abi.DISC_DENSE_GROUPED
    assert val("DTTS_DISC_N") == abi.DISC_N and val("DTTS_DISC_MAX_FMAPS") == abi.DISC_MAX_FMAPS
    assert val("DTTS_DISC_MIN_LEN") == abi.DISC_MIN_LEN and val("DTTS_DISC_TOO_SHORT") == abi.DISC_TOO_SHORT
    assert (val("DTTS_DISC_DENSE_TILE"), val("DTTS_DISC_GROUP_TILE"), val("DTTS_DISC_GROUP_TILE_WIDE")) == (
        abi.DISC_DENSE_TILE, abi.DISC_GROUP_TILE, abi.DISC_GROUP_TILE_WIDE)
    # the unit is an item of dtts_text2mel_fetch: no new entry point
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "disc" in s]
    assert "disc" not in open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()
    # every D count fits the row the block asks for
    for L in (6, 7, 11, 12, 13, 63, 64, 65, 891, 892, 4099, 179200):
        assert max(ds.d_count(d, L) for d in range(8)) <= abi.disc_d_ld(L)


def test_argument_block_refusals_without_a_handle():
    lib = abi.load_library()
    good = dict(B=2, y=4096, y_hat=8192, wav_ld=64, sums=4096, counts=4096, status=4096)

    def refused(match, **kw):
        a = abi.disc_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_DISC, C.byref(a), None) == -22   # DTTS_E_INVAL
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"B = 0", B=0)
    refused(r"B = 65536", B=65536)
    refused(r"wav_ld = 5 samples is below DTTS_DISC_MIN_LEN = 6", wav_ld=5)
    refused(r"wav_ld = 16777217", wav_ld=(1 << 24) + 1)
    refused(r"which = 0", which=0)
    refused(r"which = 4", which=abi.DISC_FM)
    refused(r"which = 8", which=abi.DISC_DENSE_GROUPED)
    refused(r"which = 17", which=17)
    refused(r"null y_dev", y=0)
    refused(r"null y_dev", sums=0)
    refused(r"null y_dev", status=0)
    refused(r"DTTS_DISC_FM without fm_dev", which=abi.DISC_MPD | abi.DISC_FM)
    refused(r"DTTS_DISC_FM without fm_dev", which=abi.DISC_MPD | abi.DISC_FM, fm=4096)
    refused(r"d_ld = 16 entries for wav_ld = 64 \(needs 17\)", d=4096, d_ld=16)
    refused(r"y_hat_dev = .* is not aligned to 4 bytes", y_hat=8194)
    refused(r"sums_dev = .* is not aligned to 8 bytes", sums=4100)
    refused(r"fm_counts_dev = .* is not aligned to 8 bytes", which=7, fm=4096, fm_counts=4100)
    a = abi.disc_args(**good)
    a.size -= 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_DISC, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.DiscArgs) - 8}" in lib.dtts_last_error(None).decode()
    a = abi.disc_args(**good)
    a.reserved = 1
    assert lib.dtts_text2mel_fetch(None, abi.OUT_DISC, C.byref(a), None) == -22
    refused(r"null handle")                                      # a good block: only then is the handle looked at
    refused(r"null handle", d=4096, d_ld=17)
    assert lib.dtts_text2mel_fetch(None, abi.OUT_DISC, None, None) == -22


def test_checkpoint_discovery(tmp_path, state):
    """the newest model_ckpt_steps_*.ckpt's model_disc, or None when that checkpoint carries none"""
    import torch
    from dict_tts_amd import vocoder
    (tmp_path / "config.yaml").write_text("resblock: '1'\nupsample_rates: [8, 8, 2, 2]\nuse_cond_disc: false\n")
    few = {k: torch.from_numpy(v) for k, v in list(state.items())[:4]}
    torch.save({"state_dict": {"model_gen": {}, "model_disc": few}}, tmp_path / "model_ckpt_steps_20.ckpt")
    torch.save({"state_dict": {"model_gen": {}}}, tmp_path / "model_ckpt_steps_3.ckpt")
    cfg, md = vocoder.find_vocoder_discriminators(str(tmp_path))
    assert set(md) == set(few) and cfg["use_cond_disc"] is False
    torch.save({"state_dict": {"model_gen": {}}}, tmp_path / "model_ckpt_steps_100.ckpt")
    assert vocoder.find_vocoder_discriminators(str(tmp_path))[1] is None
    assert vocoder.find_vocoder_discriminators(str(tmp_path / "nothing")) == (None, None)
