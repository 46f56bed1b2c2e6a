"""The teacher-forced FVAE posterior pass on the GPU (run with `-m gpu` on an MI355X): PortaSpeech_dict.forward(infer=False) with
tgt_mels under torch.no_grad() -> dtts_text2mel_fetch(DTTS_OUT_POSTERIOR), against the reference's own outputs (tests/golden/g12_posterior.npz, both
cases) and the CPU restatement (tests/posterior_ref.py).  The infer path on the same handle must not move."""
import os

import numpy as np
import pytest
import torch

import posterior_ref as pr
from dict_tts_amd import abi, synth

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
KEYS = ("mel_out", "z_p", "m_q", "logs_q")


def _model(case="plain", sd=None, **hp_extra):
    from dict_tts_amd import model
    import speaker_ref as sr
    form = pr.CASES[case]["form"]
    hp = dict(sr.FORMS[form]["hparams"]) if form else {}
    hp.update(hp_extra)
    m = model.PortaSpeech_dict(hparams=hp)
    sd = sd if sd is not None else pr.g12_state_dict(case)
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m


@pytest.fixture(scope="module")
def models():
    return {case: _model(case) for case in pr.CASES}


@pytest.fixture(scope="module")
def g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_posterior.npz"))


def _mels(g12):
    """the G12 inputs (regenerated: the fixture stores their fingerprint)"""
    mels = pr.tgt_mels_for(g12["mel2word_in"])
    assert np.allclose(pr.mels_fingerprint(mels), g12["tgt_mels_fingerprint"], rtol=1e-12, atol=0)
    return mels


def _dm(b):
    return (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"])


def _post(m, batch, mels, mel2word, eps=None, spk=None):
    b = {k: T(v) for k, v in batch.items()}
    with torch.no_grad():
        return m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None, _dm(b), infer=False, tgt_mels=T(mels),
                 mel2word=None if mel2word is None else T(mel2word), eps=None if eps is None else T(eps),
                 spk_embed=None if spk is None else T(spk))


def _infer(m, batch, z, mel2word=None):
    b = {k: T(v) for k, v in batch.items()}
    return m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None, _dm(b), infer=True, z_p=z,
             mel2word=None if mel2word is None else T(mel2word))


def _errs(got, want):
    """max-abs errors; z_p's bound scales with its magnitude (the synthetic flow reaches |57|)"""
    out = {}
    for k in KEYS:
        g, w = got[k].cpu().numpy(), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        out[k] = float(np.abs(g - w).max()) / max(1.0, float(np.abs(w).max()) if k == "z_p" else 1.0)
    kl, wkl = float(got["kl"]), float(want["kl"])
    out["kl_rel"] = abs(kl - wkl) / abs(wkl)
    return out


def _gates(e, what):
    assert e["mel_out"] <= 1e-3, (what, e)
    assert max(e["m_q"], e["logs_q"], e["z_p"]) <= 1e-4, (what, e)
    assert e["kl_rel"] <= 1e-4, (what, e)


@pytest.mark.parametrize("case", ["plain", "id"])
def test_posterior_matches_reference_golden_g12(models, g12, case):
    batch = pr.g12_batch()
    m2w = g12["mel2word_in"]
    spk = g12[case + ".spk"] if case == "id" else None
    got = _post(models[case], batch, _mels(g12), m2w, g12[case + ".eps"], spk)
    want = {k: g12[f"{case}.{k}"] for k in KEYS + ("kl",)}
    e = _errs(got, want)
    print(f"G12 {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    _gates(e, case)
    # the padded frames inside T_mel (the ragged tails, the interior hole of utterance 2) are compared too: that is where the mask acts
    x_mask = g12[case + ".x_mask"][..., 0]
    pad = x_mask == 0
    assert pad[pr.G12_HOLE[0], pr.G12_HOLE[1]:pr.G12_HOLE[2]].all() and pad.sum() > 100
    assert np.abs(got["mel_out"].cpu().numpy()[pad] - g12[case + ".mel_out"][pad]).max() <= 1e-3
    assert np.array_equal(got["x_mask"].cpu().numpy(), g12[case + ".x_mask"])
    assert np.abs(got["dur"].cpu().numpy() - g12[case + ".dur"]).max() <= 1e-4
    assert got["kl"].shape == () and got["mel_out_fvae"] is got["mel_out"]
    for k in ("pron_attn", "dict_attn", "word_encoder_out", "mel2word"):
        assert k in got


def test_posterior_b60_biaobei_teacher_forced_vs_restatement(models):
    from oracle import hifigan_ref as href
    batch = synth.biaobei_batch(0, 60, pr.SEED)
    m2w = synth.teacher_mel2word(batch["word_tokens"])
    mels = pr.tgt_mels_for(m2w, name="b60.mel")
    B, T_mel = mels.shape[:2]
    eps = synth.randn(pr.SEED, "b60.eps", (B, 16, T_mel // 4))
    got = _post(models["plain"], batch, mels, m2w, eps)
    torch.set_num_threads(8)
    sd = href.fold_weight_norm({k: T(v) for k, v in pr.g12_state_dict("plain").items()})
    b = {k: T(v) for k, v in batch.items()}
    want = pr.forward_posterior(sd, b["word_tokens"], _dm(b), b["pron_modified"], T(mels), T(m2w), T(eps))
    e = _errs(got, want)
    per_utt = (got["mel_out"].cpu() - want["mel_out"]).abs().amax(dim=(1, 2))
    worst = int(per_utt.argmax())
    print(f"B=60 posterior: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; worst utterance {worst}: mel {float(per_utt[worst]):.2e}")
    _gates(e, "B=60")


def test_posterior_device_noise_is_seeded_and_the_kl_reduction_deterministic(models, g12):
    m = models["plain"]
    batch, m2w, mels = pr.g12_batch(), g12["mel2word_in"], _mels(g12)
    given = _post(m, batch, mels, m2w, g12["plain.eps"])
    again = _post(m, batch, mels, m2w, g12["plain.eps"])
    for k in KEYS + ("kl",):
        assert torch.equal(given[k], again[k]), k   # same inputs -> same bits (the KL's fixed-order reduction included)
    m.ctx.set_noise_seed(77)
    a = _post(m, batch, mels, m2w)
    m.ctx.set_noise_seed(77)
    b = _post(m, batch, mels, m2w)
    c = _post(m, batch, mels, m2w)
    for k in KEYS + ("kl",):
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["z_p"], c["z_p"])   # the next call draws new noise
    for k in ("m_q", "logs_q"):   # independent of the noise
        assert torch.equal(a[k], given[k]), k


def test_posterior_leaves_the_infer_path_bit_identical(models, g12):
    m = models["plain"]
    batch, m2w = pr.g12_batch(), g12["mel2word_in"]
    z = T(synth.noise(pr.SEED, 5, _mels(g12).shape[1] // 4, "g12.iso"))
    before = _infer(m, batch, z, m2w)
    _post(m, batch, _mels(g12), m2w, g12["plain.eps"])
    after = _infer(m, batch, z, m2w)
    for k in ("mel_out", "dur", "x_mask", "mel2word", "word_encoder_out"):
        assert torch.equal(before[k], after[k]), k


def test_posterior_errors(models, g12):
    m = models["plain"]
    batch, m2w, mels = pr.g12_batch(), g12["mel2word_in"], _mels(g12)
    with pytest.raises(ValueError, match=rf"{mels.shape[1] - 4}.*{mels.shape[1]}"):
        _post(m, batch, mels[:, :-4], m2w)
    b = {k: T(v) for k, v in batch.items()}
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="gradients"):
        m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None, _dm(b), infer=False, tgt_mels=T(mels),
          mel2word=T(m2w))
    fresh = _model("plain")
    buf = torch.zeros(1 << 16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(abi.DttsError, match=r"DTTS_OUT_POSTERIOR\) failed \(-1\).*before encode"):
        fresh.ctx.text2mel_posterior(buf.data_ptr(), 0, None, 0, buf.data_ptr(), 0, None, None, None, None, s)
    sd = {k: v for k, v in pr.g12_state_dict("plain").items() if not k.startswith("fvae.encoder.")}
    lacking = _model("plain", sd=sd)
    infer_ok = _infer(lacking, batch, T(synth.noise(pr.SEED, 5, mels.shape[1] // 4, "g12.iso")), m2w)   # loading and inference unchanged
    assert torch.isfinite(infer_ok["mel_out"]).all()
    with pytest.raises(abi.DttsError, match=r"\(-1\).*fvae\.encoder\.pre_net\.0\.weight"):
        _post(lacking, batch, mels, m2w, g12["plain.eps"])


def test_posterior_predicted_durations_vs_restatement(models):
    """mel2word=None: the predicted durations fix T_mel (known after the encode), as in the reference"""
    from oracle import hifigan_ref as href
    batch = pr.g12_batch()
    m = models["plain"]
    r = _infer(m, batch, None)
    T_mel = r["mel_out"].shape[1]
    m2w_pred = r["mel2word"].cpu().numpy()
    mels = pr.tgt_mels_for(m2w_pred, name="g12.pred.mel")
    assert mels.shape[1] == T_mel
    eps = synth.randn(pr.SEED, "g12.pred.eps", (5, 16, T_mel // 4))
    got = _post(m, batch, mels, None, eps)
    sd = href.fold_weight_norm({k: T(v) for k, v in pr.g12_state_dict("plain").items()})
    b = {k: T(v) for k, v in batch.items()}
    want = pr.forward_posterior(sd, b["word_tokens"], _dm(b), b["pron_modified"], T(mels), None, T(eps))
    _gates(_errs(got, want), "predicted durations")
    with pytest.raises(ValueError, match=rf"{T_mel + 4}.*{T_mel}"):
        _post(m, batch, np.concatenate([mels, mels[:, :4]], 1), None, eps)


def test_memory_safety_posterior(g12):
    """debug_redzone = 1: the posterior workspace sits between red zones; the pass damages none, and its outputs are finite"""
    m = _model("plain", dtts_debug_redzone=1)
    batch = pr.g12_batch()
    got = _post(m, batch, _mels(g12), g12["mel2word_in"], g12["plain.eps"])
    assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()
    for k in KEYS + ("kl",):
        assert torch.isfinite(got[k]).all(), k
    one = _post(m, {k: v[:1] for k, v in batch.items()}, _mels(g12)[:1], g12["mel2word_in"][:1])   # a smaller batch, device noise
    assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()
    assert torch.isfinite(one["mel_out"]).all()


@pytest.mark.parametrize("variant", ["launch_by_launch_flow", "decoder_fp32"])
def test_posterior_other_engines_match_g12(g12, variant):
    """DTTS_TUNE bit 8: the masked forward flow launch by launch (conv1d row masks) instead of flowstack_kernel<., MASK>;
    decoder_fp32 = 1: every WaveNet of the pass on the fp32-grade conv1d kernels (their row-mask epilogue) and the fused flow on fp32 MFMA"""
    from dict_tts_amd import hparams, model
    cfg = hparams.fill_abi_config(abi.default_config(), {"dtts_tune_flags": 256} if variant == "launch_by_launch_flow" else {}, None)
    if variant == "decoder_fp32":
        cfg.decoder_fp32 = 1
    m = model.PortaSpeech_dict(hparams={}, ctx=abi.Context(cfg))
    m.load_state_dict({k: T(v) for k, v in pr.g12_state_dict("plain").items()}, strict=True)
    got = _post(m, pr.g12_batch(), _mels(g12), g12["mel2word_in"], g12["plain.eps"])
    e = _errs(got, {k: g12[f"plain.{k}"] for k in KEYS + ("kl",)})
    print(f"G12 plain, {variant}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    _gates(e, variant)
