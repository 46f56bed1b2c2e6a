"""Speaker conditioning on the GPU (run with `-m gpu` on an MI355X), through the C ABI via the model shim: dtts_text2mel_speakers
(spk_embed_proj on the device) + the speaker epilogue of the linguistic encoder's last LayerNorm, against the reference's own outputs
(tests/golden/g11_speaker.npz, both forms) and the CPU restatement (tests/speaker_ref.py).  The unconditioned path must not move."""
import os

import numpy as np
import pytest
import torch

import speaker_ref as sr
from dict_tts_amd import abi, synth

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
OUT_KEYS = ("mel_out", "dur", "mel2word", "x_mask", "word_encoder_out", "pron_attn", "dict_attn", "mel_lens")


def _model(form=None, sd=None, **hp_extra):
    from dict_tts_amd import model
    hp = dict(sr.FORMS[form]["hparams"]) if form else {}
    hp.update(hp_extra)
    m = model.PortaSpeech_dict(hparams=hp)
    sd = sd if sd is not None else (sr.g11_state_dict(form) if form else synth.dict_tts_state_dict(sr.SEED, n_phone=6))
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m


@pytest.fixture(scope="module")
def plain():
    return _model()


@pytest.fixture(scope="module")
def spk_models():
    return {form: _model(form) for form in sr.FORMS}


@pytest.fixture(scope="module")
def g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_speaker.npz"))


def _dm(b):
    return (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"])


def _run(m, batch, spk=None, z=None, mel2word=None):
    b = {k: T(v) for k, v in batch.items()}
    return m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None, _dm(b), infer=True, z_p=z,
             mel2word=mel2word, spk_embed=None if spk is None else T(spk))


def _run_unarmed(m, batch, z):
    """encode + decode + fetches through the C ABI with NOTHING armed (whatever the model's hparams say)"""
    b = {k: T(v).cuda() for k, v in batch.items()}
    B, T_w = b["word_tokens"].shape
    L_k, P = b["keys"].shape[2], b["pinyin"].shape[2]
    s = torch.cuda.current_stream().cuda_stream
    T_mel = m.ctx.text2mel_encode(*(b[k].data_ptr() for k in ("word_tokens", "keys", "values", "key_map", "pinyin", "pinyin_map",
                                                              "pron_modified")), None, B, T_w, L_k, P, s)
    return m._finish(T_mel, z, B, T_w, L_k, P)


def _z_unconditioned(plain, batch, name):
    """a fixed prior sample sized for the unconditioned durations of `batch` (a first, probing pass)"""
    T_mel = _run(plain, batch)["mel_out"].shape[1]
    return T(synth.noise(sr.SEED, batch["word_tokens"].shape[0], T_mel // 4, name))


def _same(a, b, what, keys=OUT_KEYS):
    for k in keys:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.shape == y.shape and torch.equal(x, y), (what, k, float((x.float() - y.float()).abs().max()) if x.shape == y.shape else x.shape)


@pytest.mark.parametrize("form", ["embed", "id"])
def test_g11_speaker_parity_vs_reference_golden(spk_models, g11, form):
    m = spk_models[form]
    r = _run(m, sr.g11_batch(), g11[form + ".spk"], z=T(g11[form + ".z_p"]))
    assert np.array_equal(r["mel2word"].cpu().numpy(), g11[form + ".mel2word"]), "integer durations differ from the reference"
    assert np.array_equal(r["x_mask"].cpu().numpy(), g11[form + ".x_mask"])
    errs = {k: float(np.abs(r[k].cpu().numpy() - g11[f"{form}.{k}"]).max()) for k in ("dur", "word_encoder_out", "mel_out")}
    print(f"\n[G11 {form}] worst |gpu - reference|: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["dur"] <= 1e-4 and errs["word_encoder_out"] <= 1e-4 and errs["mel_out"] <= 1e-3, errs


@pytest.mark.parametrize("form", ["embed", "id"])
def test_speakers_on_the_resident_table_id_path(spk_models, g11, form):
    """forward_ids (resident table + ids) with speakers = the tensor path with speakers, to the tolerances the two dictionary paths keep
    without speakers (test_resident_dictionary_ids_equal_collated_tensors: the table holds projected rows); the speaker rows themselves
    (padded rows of word_encoder_out) are bit-identical, and so are two id-path runs"""
    m = spk_models[form]
    st = synth.biaobei_struct()
    table = synth.dict_table(sr.SEED)
    m.upload_dict_table(table)
    sents = [st["sentences"][i] for i in sr.G11_SENTENCES]
    ib = synth.make_id_batch(sents, table, pron_every=2)
    tb = sr.g11_batch()
    assert np.array_equal(tb["word_tokens"], ib["word_tokens"])
    spk = g11[form + ".spk"]
    ra = _run(m, tb, spk)
    args = (T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"])
    rb = m.forward_ids(*args, z_p=ra["z_p_in"], spk_embed=T(spk))
    rc = m.forward_ids(*args, z_p=ra["z_p_in"], spk_embed=T(spk))
    _same(rb, rc, "id path twice")
    assert torch.equal(ra["mel2word"], rb["mel2word"])
    for k, tol in (("dur", 1e-5), ("pron_attn", 1e-5), ("word_encoder_out", 1e-4), ("mel_out", 1e-3)):
        assert (ra[k] - rb[k]).abs().max() <= tol, (k, float((ra[k] - rb[k]).abs().max()))
    pad = T(ib["word_tokens"]).cuda() == 0
    assert torch.equal(ra["word_encoder_out"][pad], rb["word_encoder_out"][pad])
    assert np.array_equal(rb["mel2word"].cpu().numpy(), g11[form + ".mel2word"])


@pytest.mark.parametrize("form", ["embed", "id"])
def test_mixed_speaker_batch_equals_each_utterance_alone(spk_models, g11, form):
    """each utterance of the mixed-speaker batch gets BIT-identical log-durations, encoder output and mel2word when it runs alone with
    its own speaker (the same padded row: both runs far below the 128-word attention threshold, as in
    test_results_do_not_depend_on_batch_composition)"""
    m = spk_models[form]
    full = sr.g11_batch()
    assert full["word_tokens"].shape[1] <= 128
    spk = g11[form + ".spk"]
    rB = _run(m, full, spk)
    lens = (full["word_tokens"] > 0).sum(1)
    for u in range(full["word_tokens"].shape[0]):
        r1 = _run(m, {k: v[u:u + 1] for k, v in full.items()}, spk[u:u + 1])
        n = int(lens[u])
        for k in ("dur", "word_encoder_out"):
            a, b = r1[k][0, :n].cpu(), rB[k][u, :n].cpu()
            assert torch.equal(a, b), (u, k, float((a - b).abs().max()))
        mB = rB["mel2word"][u].cpu()
        kf = int((mB > 0).sum())
        assert kf > 0 and torch.equal(r1["mel2word"][0].cpu()[:kf], mB[:kf]) and r1["mel2word"].shape[1] - kf <= 3, u


@pytest.mark.parametrize("form", ["embed", "id"])
def test_unarmed_and_zero_projection_leave_the_default_path_bit_identical(plain, spk_models, form):
    """(a) speaker weights loaded but nothing armed: every output bit-identical to a handle without speaker weights, the same number of
    timed stage launches; (b) an all-zero projection (weight and bias zero) armed: bit-identical to the unconditioned run"""
    batch = sr.g11_batch()
    z = _z_unconditioned(plain, batch, "spk.zero")
    m2w = T(synth.teacher_mel2word(batch["word_tokens"], 8, 4))
    z_tf = T(synth.noise(sr.SEED, 5, (m2w.shape[1] + 3) // 4, "spk.zero.tf"))
    m = spk_models[form]
    counts = []
    for ctx_model in (plain, m):
        ctx = ctx_model.ctx
        for w in (abi.TIMER_STAGE_ENCODER, abi.TIMER_STAGE_DICT_ENCODER, abi.TIMER_STAGE_FVAE, abi.TIMER_S2PA):
            ctx.timer_enable(w)
        ctx.timer_reset()
    want = _run_unarmed(plain, batch, z)
    got = _run_unarmed(m, batch, z)
    _same(got, want, "loaded, not armed")
    for ctx_model in (plain, m):
        counts.append([ctx_model.ctx.timer_read(w)[1] for w in (abi.TIMER_STAGE_ENCODER, abi.TIMER_STAGE_DICT_ENCODER,
                                                                abi.TIMER_STAGE_FVAE, abi.TIMER_S2PA)])
    assert counts[0] == counts[1] and counts[0][0] == 1, counts
    # teacher-forced durations too (no synchronisation in the encode)
    b = {k: T(v) for k, v in batch.items()}
    want_tf = plain((b["word_tokens"], None), b["pron_modified"], (None,) * 3, None, None, _dm(b), infer=True, z_p=z_tf, mel2word=m2w)
    # (b) zero projection
    sd = sr.g11_state_dict(form)
    sd["spk_embed_proj.weight"] = np.zeros_like(sd["spk_embed_proj.weight"])
    if "spk_embed_proj.bias" in sd:
        sd["spk_embed_proj.bias"] = np.zeros_like(sd["spk_embed_proj.bias"])
    mz = _model(form, sd=sd)
    spk = sr.g11_speakers(form)
    _same(_run(mz, batch, spk, z=z), want, "zero projection")
    _same(_run(mz, batch, spk, z=z_tf, mel2word=m2w), want_tf, "zero projection, teacher-forced")


def test_speaker_errors_fail_loudly_and_leave_the_handle_usable(plain, spk_models, g11):
    batch = sr.g11_batch()
    m_id, m_emb = spk_models["id"], spk_models["embed"]
    z = T(g11["id.z_p"])
    good = _run(m_id, batch, g11["id.spk"], z=z)
    s = torch.cuda.current_stream().cuda_stream
    # an out-of-range id: reported at the T_mel synchronisation, naming the utterance and the id (nn.Embedding raises there)
    bad = g11["id.spk"].copy()
    bad[2] = 8
    with pytest.raises(abi.DttsError, match=r"speaker id 8 of utterance 2 .*8 rows"):
        _run(m_id, batch, bad, z=z)
    bad[2], bad[4] = -3, 1 << 40
    with pytest.raises(abi.DttsError, match=r"speaker id -3 of utterance 2"):
        _run(m_id, batch, bad, z=z)
    _same(_run(m_id, batch, g11["id.spk"], z=z), good, "after an out-of-range id")
    # armed B != encode B: refused, and the speakers are dropped (the next unarmed encode is unconditioned)
    ids3 = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    m_id.ctx.text2mel_speakers(abi.SPK_ID, ids3.data_ptr(), 3, s)
    z0 = _z_unconditioned(plain, batch, "spk.err")
    with pytest.raises(abi.DttsError, match=r"armed 3 utterances but this encode has B=5"):
        _run_unarmed(m_id, batch, z0)
    _same(_run_unarmed(m_id, batch, z0), _run_unarmed(plain, batch, z0), "after a B mismatch")
    # the wrong kind for the loaded weights, a bad B
    e = torch.zeros(5, 256, device="cuda")
    with pytest.raises(abi.DttsError, match="does not match the loaded spk_embed_proj"):
        m_id.ctx.text2mel_speakers(abi.SPK_EMBED, e.data_ptr(), 5, s)
    with pytest.raises(abi.DttsError, match="does not match the loaded spk_embed_proj"):
        m_emb.ctx.text2mel_speakers(abi.SPK_ID, ids3.data_ptr(), 3, s)
    with pytest.raises(abi.DttsError, match="bad argument"):
        m_id.ctx.text2mel_speakers(abi.SPK_ID, ids3.data_ptr(), abi_max_batch() + 1, s)
    # a handle without speaker weights
    with pytest.raises(abi.DttsError, match="no speaker weights"):
        plain.ctx.text2mel_speakers(abi.SPK_ID, ids3.data_ptr(), 3, s)
    # use_spk_* without spk_embed (the reference crashes in spk_embed_proj(None))
    with pytest.raises(abi.DttsError, match="needs spk_embed"):
        _run(m_emb, batch, None)
    with pytest.raises(abi.DttsError, match="needs spk_embed"):
        _run(m_id, batch, None)
    # a checkpoint without spk_embed_proj for speaker hparams, and a malformed projection
    with pytest.raises(RuntimeError, match="spk_embed_proj"):
        _model("embed", sd=synth.dict_tts_state_dict(sr.SEED, n_phone=6))
    sd = sr.g11_state_dict("embed")
    sd["spk_embed_proj.weight"] = sd["spk_embed_proj.weight"][:, :128].copy()
    with pytest.raises(RuntimeError, match=r"nn.Linear\(256, 192\)"):
        _model("embed", sd=sd)
    _same(_run(m_id, batch, g11["id.spk"], z=z), good, "after the errors")
    _same(_run(m_emb, batch, g11["embed.spk"], z=T(g11["embed.z_p"])), _run(m_emb, batch, g11["embed.spk"], z=T(g11["embed.z_p"])),
          "embed handle after the errors")


def abi_max_batch():
    return 4096   # DTTS_MAX_SPEAKER_BATCH


@pytest.mark.parametrize("form", ["embed", "id"])
def test_speakers_under_memory_safety_mode(spk_models, g11, form):
    """debug_redzone = 1: the speaker workspace sits between red zones too; nothing is damaged by the projection, the conditioned
    encode / decode, or the word_encoder_out fetch, and every output is bit-identical to the release context's"""
    m = _model(form, dtts_debug_redzone=1)
    batch = sr.g11_batch()
    z = T(g11[form + ".z_p"])
    got = _run(m, batch, g11[form + ".spk"], z=z)
    n = m.ctx.debug_check(torch.cuda.current_stream().cuda_stream)
    assert n == 0, m.ctx.last_error()
    _same(got, _run(spk_models[form], batch, g11[form + ".spk"], z=z), "debug_redzone")
    one = _run(m, {k: v[:1] for k, v in batch.items()}, g11[form + ".spk"][:1])   # a smaller armed batch in the same workspace
    assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()
    assert torch.isfinite(one["mel_out"]).all()


def test_end_to_end_speaker_batch_through_the_default_vocoder(spk_models, g11):
    """infer.infer_batch on a batch carrying spk_embed (use_spk_embed: the field tasks/tts/dict_tts.py:182 passes), vocoded in the
    default DTTS_VOC_F16 mode: every utterance passes the waveform gate against the restatement + oracle.hifigan_ref"""
    from dict_tts_amd import infer, vocoder
    from oracle import hifigan_ref as href
    voc_sd = {k: T(v) for k, v in synth.hifigan_state_dict(sr.SEED).items()}
    voc = vocoder.HifiGAN(state_dict=voc_sd, config=synth.hifigan_config(), precision="f16")
    assert voc.precision == abi.VOC_F16
    batch = {k: T(v) for k, v in sr.g11_batch().items()}
    batch["spk_embed"] = T(g11["embed.spk"])
    batch["spk_ids"] = T(g11["id.spk"])   # present too: use_spk_embed picks spk_embed
    out, wavs = infer.infer_batch(spk_models["embed"], voc, batch, z_p=T(g11["embed.z_p"]))
    sd = href.fold_weight_norm({k: T(v) for k, v in sr.g11_state_dict("embed").items()})
    want = sr.forward_infer_spk(sd, "embed", batch["spk_embed"], batch["word_tokens"], _dm(batch), batch["pron_modified"],
                                z_p=T(g11["embed.z_p"]))
    assert torch.equal(out["mel2word"].cpu(), want["mel2word"])
    assert (out["mel_out"].cpu() - want["mel_out"]).abs().max() <= 1e-3
    hsd = href.fold_weight_norm(voc_sd)
    lens = out["mel_lens"].cpu().tolist()
    worst = 0.0
    for u, w in enumerate(wavs):
        ref = href.spec2wav(hsd, synth.hifigan_config(), want["mel_out"][u, :lens[u]].numpy()).numpy()
        assert w.shape == ref.shape
        worst = max(worst, rms(w - ref))
        assert rms(w - ref) <= 1e-4 and abs(rms(w) - rms(ref)) <= 1e-4, (u, rms(w - ref), rms(w), rms(ref))
    print(f"\n[speaker end to end] worst RMS(gpu - ref) {worst:.2e}")
