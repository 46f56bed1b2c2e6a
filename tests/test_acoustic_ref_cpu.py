"""The text-to-mel references that need no GPU: the shape-parameterised synthetic state dict (the default arrays pinned bit for bit),
the config-driven restatement (tests/acoustic_ref.py) against the oracle at the default shape and against itself in float64 at every
non-default shape, and planted seam defects that the old end-to-end gates let through and the per-row bounds catch."""
import hashlib

import numpy as np
import pytest
import torch

import acoustic_ref as ar
import posterior_ref as pr
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref

# sha256 over (key, dtype, shape, bytes) of every array, in key order, as dict_tts_state_dict returned them before it took a shape
PINNED = {
    (1234, None): "ed5d504830820d64bd18874d878aba612d872d546ab3657a5a101e400d39723d",
    (1234, "id"): "3dda038c1710e6505fa63840ed1b5116427f6c899d9535c3ddca6945d7be2e8d",
    (1234, "embed"): "82d98ab02c3b2455c4c42bb2569171bf58ffc2bf9dd2b5b57a970e575f71bde8",
    (77, None): "4d0d4013363bd983d491ff0d7e6c59af745a9e9699e1003e5efea81e47ea5acf",
}


@pytest.fixture(autouse=True)
def eight_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        a = np.ascontiguousarray(sd[k])
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("seed,speaker", sorted(PINNED, key=str))
def test_default_state_dict_is_pinned(seed, speaker):
    kw = {} if speaker is None else {"speaker": speaker, "num_spk": 8 if speaker == "id" else 4}
    assert _digest(synth.dict_tts_state_dict(seed, **kw)) == PINNED[(seed, speaker)]
    assert _digest(synth.dict_tts_state_dict(seed, acoustic={}, **kw)) == PINNED[(seed, speaker)]
    assert _digest(synth.dict_tts_state_dict(seed, acoustic=dict(synth.ACOUSTIC_SHAPE), **kw)) == PINNED[(seed, speaker)]


@pytest.mark.parametrize("name", sorted(ar.CONFIGS))
def test_state_dict_shapes_follow_the_hparams(name):
    hp = ar.CONFIGS[name]
    sh = synth.acoustic_shape(hp)
    sd = synth.dict_tts_state_dict(ar.SEED, acoustic=hp)
    H, Hd, Z, Hf = sh["hidden_size"], sh["fvae_enc_dec_hidden"], sh["latent_size"], sh["prior_glow_hidden"]
    p = "dict_encoder.S2PA_module"
    assert sd[p + ".word_emb.weight"].shape == (synth.WORD_SIZE, H)
    assert sd[p + ".semantic_encoder.ffn_layers.3.conv_1.weight"].shape == (4 * H, H, sh["enc_ffn_kernel_size"])
    assert sd[f"dur_predictor.conv.{sh['dur_predictor_layers'] - 1}.1.weight"].shape == (128, 128 if sh["dur_predictor_layers"] > 1 else H,
                                                                                        sh["dur_predictor_kernel"])
    assert f"dur_predictor.conv.{sh['dur_predictor_layers']}.1.weight" not in sd
    assert sd["fvae.decoder.pre_net.0.weight"].shape == (Z, Hd, 4)
    assert sd["fvae.encoder.out_proj.weight"].shape == (2 * Z, Hd, 1)
    assert sd[f"fvae.decoder.wn.in_layers.{sh['fvae_dec_n_layers'] - 1}.weight_v"].shape == (2 * Hd, Hd, sh["fvae_kernel_size"])
    last = 2 * (sh["prior_glow_n_blocks"] - 1)
    assert sd[f"fvae.prior_flow.flows.{last}.enc.in_layers.0.weight_v"].shape == (2 * Hf, Hf, sh["glow_kernel_size"])
    assert sd[f"fvae.prior_flow.flows.{last}.pre.weight"].shape == (Hf, Z // 2, 1)
    assert f"fvae.prior_flow.flows.{last + 2}.pre.weight" not in sd


def test_restatement_is_the_oracle_at_the_default_shape():
    """fp32 at ps_flow.yaml's shape, predicted durations: every output bit-identical to oracle.dict_tts_ref.forward_infer"""
    batch = synth.make_batch(synth.biaobei_struct()["sentences"][:3], 77)
    sd = ar.state(synth.dict_tts_state_dict(77))
    z = lambda B, T4: torch.from_numpy(synth.noise(77, B, T4))
    want = ref.forward_infer(sd, *ar.inputs(batch), z_p=z)
    got = ar.forward(sd, {}, *ar.inputs(batch), z_p=z)
    assert torch.equal(got["mel2word"], want["mel2word"])
    for k in ("word_encoder_out", "context", "dur", "dict_attn", "pron_attn", "x_mask", "mel_out"):
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
    assert torch.equal(got["z"], want["z_p"])


def _small_case(hp, frames=(4 * 21, 4 * 13)):
    batch = ar.batch_of([9, 6], offset=40)
    m2w = torch.from_numpy(ar.spread_mel2word(batch["word_tokens"], frames))
    Z = synth.acoustic_shape(hp)["latent_size"]
    z = torch.from_numpy(synth.randn(ar.SEED, "cpu.z", (2, Z, max(frames) // 4)))
    return batch, m2w, z


@pytest.mark.parametrize("name", sorted(ar.CONFIGS))
def test_nondefault_shapes_fp32_and_float64_agree(name):
    """every non-default shape runs end to end in both dtypes (float64 inputs everywhere: no fp32 tensor leaks into the float64 run) and
    the two agree to fp32 rounding noise, relative to each output's scale"""
    hp = ar.CONFIGS[name]
    sd_np = synth.dict_tts_state_dict(ar.SEED, acoustic=hp)
    batch, m2w, z = _small_case(hp)
    a = ar.forward(ar.state(sd_np), hp, *ar.inputs(batch), mel2word=m2w, z_p=z)
    b = ar.forward(ar.state(sd_np, torch.float64), hp, *ar.inputs(batch, torch.float64), mel2word=m2w, z_p=z)
    assert torch.equal(a["mel2word"], b["mel2word"])
    for k in ("word_encoder_out", "context", "dur", "dict_attn", "pron_attn", "z", "mel_out"):
        assert a[k].dtype == torch.float32 and b[k].dtype == torch.float64, k
        scale = float(b[k].abs().max())
        err = float((a[k].double() - b[k]).abs().max())
        assert torch.isfinite(b[k]).all() and scale > 0, k
        assert err <= 2e-5 * max(1.0, scale), (k, err, scale)
    # the posterior pass at the same shape (latent 16 only: the library refuses the pass otherwise)
    if synth.acoustic_shape(hp)["latent_size"] == 16:
        mels = pr.tgt_mels_for(m2w.numpy(), name="cpu.mel")
        eps = synth.randn(ar.SEED, "cpu.eps", (2, 16, mels.shape[1] // 4))
        T = torch.from_numpy
        pa = pr.forward_posterior(ar.state(sd_np), *ar.inputs(batch), T(mels), m2w, T(eps), hp=hp)
        pb = pr.forward_posterior(ar.state(sd_np, torch.float64), *ar.inputs(batch, torch.float64), T(mels).double(), m2w, T(eps).double(),
                                  hp=hp)
        for k in ("mel_out", "z_p", "m_q", "logs_q", "kl"):
            assert pb[k].dtype == torch.float64, k
            scale = float(pb[k].abs().max())
            assert float((pa[k].double() - pb[k]).abs().max()) <= 2e-5 * max(1.0, scale), k


# A flow chunk seam and a decoder tile edge of the default shape, with one halo row rounded to bf16 (the low half of a split-bf16
# operand dropped there).  T_mel/4 = 2 RC + 1: two seams; the decoder's 64-row tiles start at frames 64, 128, ...
RC = ar.flow_rc()
DEFECTS = {
    "flow_seam_halo_row": ("fvae.prior_flow.flows.0.enc", 0, RC, [RC - 1]),
    "flow_seam_halo_row_first_block": ("fvae.prior_flow.flows.6.enc", 0, 2 * RC, [2 * RC - 1]),
    "decoder_tile_edge_halo_row": ("fvae.decoder.wn", 0, 128, [127]),
}


@pytest.fixture(scope="module")
def seam_case():
    batch = ar.batch_of([20, 30])
    m2w = torch.from_numpy(ar.spread_mel2word(batch["word_tokens"], [4 * (2 * RC + 1), 4 * 100]))
    z = torch.from_numpy(synth.noise(ar.SEED, 2, 2 * RC + 1, "cpu.seam.z"))
    sd_np = synth.dict_tts_state_dict(ar.SEED)
    want = ar.forward(ar.state(sd_np, torch.float64), {}, *ar.inputs(batch, torch.float64), mel2word=m2w, z_p=z)
    return batch, m2w, z, ar.state(sd_np), want


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_seam_defects_pass_the_old_gates_and_fail_the_row_bounds(seam_case, defect):
    batch, m2w, z, sd, want = seam_case
    clean = ar.forward(sd, {}, *ar.inputs(batch), mel2word=m2w, z_p=z)
    assert not ar.check("cpu clean", "mel", clean["mel_out"], want["mel_out"], ar.BOUNDS["mel"])
    site, layer, row, halo = DEFECTS[defect]
    bad = ar.forward(sd, {}, *ar.inputs(batch), mel2word=m2w, z_p=z, hook=ar.bf16_halo(sd, site, layer, row, halo))
    # the old gates: mel max-abs 1e-3 against the fp32 oracle; the encoder is untouched (word_encoder_out 1e-4)
    assert float((bad["mel_out"] - clean["mel_out"]).abs().max()) <= 1e-3
    assert torch.equal(bad["word_encoder_out"], clean["word_encoder_out"])
    fails = ar.check(f"cpu planted {defect}", "mel", bad["mel_out"], want["mel_out"], ar.BOUNDS["mel"])
    assert fails, "the per-row bounds let a seam defect through"
    # and they point at the seam: the worst window starts within a window of the defective row's frames
    v = ar.rowcmp(bad["mel_out"], want["mel_out"])
    first = row * (4 if "flow" in site else 1)
    assert first - 2 * ar.WIN <= v["win_at"][1] <= first + 4 + ar.WIN, (v, first)


def test_rowcmp_reports_max_window_and_rms():
    want = np.zeros((2, 40, 3))
    got = want.copy()
    got[1, 17, 2] = -4e-3
    got[0, 30:38, :] = 1e-3
    v = ar.rowcmp(torch.from_numpy(got), want)
    assert v["max"] == pytest.approx(4e-3) and v["at"] == [1, 17]
    assert v["win"] == pytest.approx(1e-3) and v["win_at"] == [0, 30]
    assert v["rms"] == pytest.approx(np.sqrt((16e-6 + 24e-6) / 240))
    assert ar.check("unit", "x", got, want, {"max": 1e-2, "win": 1e-2, "rms": 1e-2}) == []
    assert len(ar.check("unit", "x", got, want, {"max": 1e-3, "win": 1e-2, "rms": 1e-2})) == 1
