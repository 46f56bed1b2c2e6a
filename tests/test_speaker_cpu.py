"""Speaker conditioning, the parts that need no GPU: the CPU restatement (tests/speaker_ref.py) against the reference's own outputs
(tests/golden/g11_speaker.npz, both forms), the hparams rule (use_spk_* needs num_spk > 1), and the C ABI surface of
dtts_text2mel_speakers."""
import os
import re

import numpy as np
import pytest
import torch

import speaker_ref as sr
from dict_tts_amd import abi, synth
from dict_tts_amd import hparams as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("form", ["embed", "id"])
def test_restatement_matches_reference_golden_g11(golden_dir, form):
    from oracle import hifigan_ref as href
    g = np.load(os.path.join(golden_dir, "g11_speaker.npz"))
    b = {k: T(v) for k, v in sr.g11_batch().items()}
    assert np.array_equal(b["word_tokens"].numpy(), g["word_tokens"])
    assert np.array_equal(sr.g11_speakers(form), g[form + ".spk"])
    sd = href.fold_weight_norm({k: T(v) for k, v in sr.g11_state_dict(form).items()})
    r = sr.forward_infer_spk(sd, form, T(g[form + ".spk"]), b["word_tokens"],
                             (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), b["pron_modified"],
                             z_p=T(g[form + ".z_p"]))
    assert np.array_equal(r["mel2word"].numpy(), g[form + ".mel2word"])
    assert np.array_equal(r["x_mask"].numpy(), g[form + ".x_mask"])
    assert np.abs(r["word_encoder_out"].numpy() - g[form + ".word_encoder_out"]).max() <= 1e-5
    assert np.abs(r["dur"].numpy() - g[form + ".dur"]).max() <= 1e-5
    assert np.abs(r["mel_out"].numpy() - g[form + ".mel_out"]).max() <= 1e-4
    # the speakers matter: padded rows of word_encoder_out hold the speaker row, and the durations differ from the unconditioned model's
    pad = b["word_tokens"].numpy() == 0
    proj = sr.project(sd, form, T(g[form + ".spk"])).numpy()
    u, t = np.argwhere(pad)[0]
    assert np.abs(g[form + ".word_encoder_out"][u, t] - proj[u]).max() <= 1e-6
    plain = synth.dict_tts_state_dict(sr.SEED, n_phone=6)
    from oracle import dict_tts_ref as ref
    r0 = ref.forward_infer(href.fold_weight_norm({k: T(v) for k, v in plain.items()}), b["word_tokens"],
                           (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), b["pron_modified"],
                           z_p=lambda B, T4: T(sr.g11_noise(form, B, T4)))
    assert r0["dur"].shape != r["dur"].shape or not torch.equal(r0["dur"], r["dur"])


@pytest.mark.parametrize("hp,kind", [({"use_spk_embed": True, "num_spk": 4}, "embed"), ({"use_spk_id": True, "num_spk": 8}, "id"),
                                     ({"use_spk_id": True, "use_spk_embed": True, "num_spk": 2}, "id")])
def test_fill_abi_config_accepts_speakers_with_num_spk_above_one(hp, kind):
    cfg = H.fill_abi_config(abi.DttsConfig(), hp)
    assert cfg.hidden_size == 192
    assert H.speaker_kind(hp) == kind
    assert H.speaker_kind({}) is None and H.speaker_kind({"num_spk": 8}) is None


@pytest.mark.parametrize("hp", [{"use_spk_embed": True}, {"use_spk_embed": True, "num_spk": 1}, {"use_spk_id": True, "num_spk": 0}])
def test_fill_abi_config_rejects_speakers_with_num_spk_one(hp):
    with pytest.raises(ValueError, match=r"num_spk.*num_spk=N"):
        H.fill_abi_config(abi.DttsConfig(), hp)


def test_wenetspeech_shaped_yaml_chain_resolves_to_the_embed_form(tmp_path):
    """base.yaml (num_spk: 1) <- dict_tts base <- base_text2mel.yaml (use_spk_embed: true) <- dict_tts.yaml: the reference's layering of
    egs/datasets/audio/wenetspeech/; num_spk must come from the checkpoint / the command line"""
    (tmp_path / "base.yaml").write_text("num_spk: 1\nuse_spk_id: false\nuse_spk_embed: false\nhidden_size: 192\n")
    (tmp_path / "tts_dict.yaml").write_text("base_config: ./base.yaml\nuse_dict: true\n")
    (tmp_path / "base_text2mel.yaml").write_text("base_config: ./base.yaml\nuse_spk_id: false\nuse_spk_embed: true\n")
    (tmp_path / "dict_tts.yaml").write_text("base_config:\n  - ./tts_dict.yaml\n  - ./base_text2mel.yaml\nword_size: 8000\n")
    cfg = str(tmp_path / "dict_tts.yaml")
    hp = H.set_hparams(cfg, global_hparams=False)
    assert hp["use_spk_embed"] is True and hp["num_spk"] == 1 and hp["use_dict"] is True
    with pytest.raises(ValueError, match="num_spk"):
        H.fill_abi_config(abi.DttsConfig(), hp)
    hp = H.set_hparams(cfg, hparams_str="num_spk=4", global_hparams=False)
    assert hp["num_spk"] == 4 and H.speaker_kind(hp) == "embed"
    H.fill_abi_config(abi.DttsConfig(), hp)


def test_synth_speaker_weights_are_opt_in():
    a = synth.dict_tts_state_dict(1234)
    for form, keys in (("embed", {"spk_embed_proj.weight", "spk_embed_proj.bias"}), ("id", {"spk_embed_proj.weight"})):
        b = synth.dict_tts_state_dict(1234, speaker=form, num_spk=8)
        assert set(b) - set(a) == keys and all(np.array_equal(a[k], b[k]) for k in a)
    assert synth.dict_tts_state_dict(1234, speaker="embed")["spk_embed_proj.weight"].shape == (192, 256)
    assert synth.dict_tts_state_dict(1234, speaker="id", num_spk=8)["spk_embed_proj.weight"].shape == (8, 192)
    ids = synth.speaker_inputs(5, "id", 40, num_spk=8)
    assert ids.dtype == np.int64 and ids.min() >= 0 and ids.max() < 8
    e = synth.speaker_inputs(5, "embed", 3)
    assert e.shape == (3, 256) and np.allclose(np.linalg.norm(e, axis=1), 1, atol=1e-5)


def test_header_library_and_binding_agree_on_the_speaker_entry_point():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert re.search(r"DTTS_API int dtts_text2mel_speakers\(dtts_handle h, int kind, const void\* spk_dev, int B, dtts_stream stream\);", hdr)
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (DTTS_SPK_\w+)\s+(\d+)", hdr))
    assert consts == {"DTTS_SPK_EMBED": abi.SPK_EMBED, "DTTS_SPK_ID": abi.SPK_ID} == {"DTTS_SPK_EMBED": 1, "DTTS_SPK_ID": 2}
    assert "dtts_text2mel_speakers" in abi.EXPORTS and len(set(abi.EXPORTS)) == 32
    lib = abi.load_library()
    assert hasattr(lib, "dtts_text2mel_speakers") and len(lib.dtts_text2mel_speakers.argtypes) == 5
