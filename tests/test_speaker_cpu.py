"""Speaker conditioning, the parts that need no GPU: the CPU restatement (tests/speaker_ref.py) against the reference's own outputs
(tests/golden/g11_speaker.npz, both forms), the hparams rule (use_spk_* needs num_spk > 1), the C ABI surface of
dtts_text2mel_speakers, and the float64 side of tests/test_speaker_kernels_gpu.py: the conditioned restatement at any shape
(tests/acoustic_ref.forward(form=, spk=)) pinned on speaker_ref and on the reference's goldens, the tie cap of every case of
tests/speaker_shapes.py, and three planted defects of the speaker epilogue that the per-row bounds report (one of which the G11 gates
let through)."""
import os
import re

import numpy as np
import pytest
import torch

import acoustic_ref as ar
import posterior_ref as pr
import speaker_ref as sr
import speaker_shapes as sh
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# The float64 restatement of the conditioned forward (tests/acoustic_ref.forward(form=, spk=)), the cases of
# tests/test_speaker_kernels_gpu.py (tests/speaker_shapes.py), and planted defects of the speaker epilogue
INFER_KEYS = ("word_encoder_out", "context", "dur", "dict_attn", "pron_attn", "mel_out")


@pytest.fixture
def eight_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _g11_inputs(g, form, dtype):
    spk = T(g[form + ".spk"])
    return ar.inputs(sr.g11_batch(), dtype), spk if form == "id" else spk.to(dtype), T(g[form + ".z_p"])


@pytest.mark.parametrize("form", ["embed", "id"])
def test_extended_restatement_is_speaker_ref_bit_for_bit_at_g11(golden_dir, eight_threads, form):
    """fp32, the G11 shapes, predicted durations: acoustic_ref.forward(form=, spk=) IS speaker_ref.forward_infer_spk"""
    g = np.load(os.path.join(golden_dir, "g11_speaker.npz"))
    (wt, dm, pm), spk, z = _g11_inputs(g, form, torch.float32)
    sd = ar.state(sr.g11_state_dict(form))
    want = sr.forward_infer_spk(sd, form, spk, wt, dm, pm, z_p=z)
    got = ar.forward(sd, {}, wt, dm, pm, z_p=z, form=form, spk=spk)
    assert torch.equal(got["mel2word"], want["mel2word"])
    for k in INFER_KEYS + ("x_mask",):
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("form", ["embed", "id"])
def test_float64_restatement_lies_within_the_g11_gates_of_the_reference(golden_dir, eight_threads, form):
    g = np.load(os.path.join(golden_dir, "g11_speaker.npz"))
    (wt, dm, pm), spk, z = _g11_inputs(g, form, torch.float64)
    r = ar.forward(ar.state(sr.g11_state_dict(form), torch.float64), {}, wt, dm, pm, z_p=z, form=form, spk=spk)
    assert r["mel_out"].dtype == torch.float64 and r["word_encoder_out"].dtype == torch.float64
    assert np.array_equal(r["mel2word"].numpy(), g[form + ".mel2word"]) and np.array_equal(r["x_mask"].numpy(), g[form + ".x_mask"])
    errs = {k: float(np.abs(r[k].numpy() - g[f"{form}.{k}"]).max()) for k in ("dur", "word_encoder_out", "mel_out")}
    assert errs["dur"] <= 1e-4 and errs["word_encoder_out"] <= 1e-4 and errs["mel_out"] <= 1e-3, errs


def test_float64_posterior_restatement_lies_within_the_g12_gates_of_the_reference(golden_dir, eight_threads):
    g = np.load(os.path.join(golden_dir, "g12_posterior.npz"))
    m2w = g["mel2word_in"]
    wt, dm, pm = ar.inputs(pr.g12_batch(), torch.float64)
    r = pr.forward_posterior(ar.state(pr.g12_state_dict("id"), torch.float64), wt, dm, pm, T(pr.tgt_mels_for(m2w)).double(), T(m2w),
                             T(g["id.eps"]).double(), form="id", spk=T(g["id.spk"]))
    assert r["mel_out"].dtype == torch.float64 and np.array_equal(r["x_mask"].numpy(), g["id.x_mask"])
    e = {k: float(np.abs(r[k].numpy() - g["id." + k]).max()) / max(1.0, float(np.abs(g["id." + k]).max()) if k == "z_p" else 1.0)
         for k in ("mel_out", "z_p", "m_q", "logs_q", "dur")}
    assert e["mel_out"] <= 1e-3 and max(e["m_q"], e["logs_q"], e["z_p"], e["dur"]) <= 1e-4, e
    assert abs(float(r["kl"]) - float(g["id.kl"])) <= 1e-4 * abs(float(g["id.kl"]))


@pytest.mark.parametrize("form", ["embed", "id"])
def test_posterior_restatement_with_speakers_runs_in_float64_at_a_nondefault_shape(eight_threads, form):
    """hidden 256, both dtypes: no fp32 tensor leaks into the float64 run (speaker_ref.project follows the state dict's dtype), and the
    two agree to fp32 rounding noise relative to each output's scale"""
    hp = ar.CONFIGS[sh.H256]
    batch = ar.batch_of([9, 6], offset=40)
    m2w = T(ar.spread_mel2word(batch["word_tokens"], (4 * 21, 4 * 13)))
    mels = pr.tgt_mels_for(m2w.numpy(), name="spk.cpu.mel")
    eps = synth.randn(ar.SEED, "spk.cpu.eps", (2, 16, mels.shape[1] // 4))
    spk = synth.speaker_inputs(ar.SEED, form, 2, num_spk=8, name="spk.cpu")
    sd = ar.sd_np(hp, form, 8)
    assert sd["spk_embed_proj.weight"].shape == ((256, 256) if form == "embed" else (8, 256))
    out = {}
    for dt in (torch.float32, torch.float64):
        s = T(spk) if form == "id" else T(spk).to(dt)
        out[dt] = pr.forward_posterior(ar.state(sd, dt), *ar.inputs(batch, dt), T(mels).to(dt), m2w, T(eps).to(dt), form=form, spk=s, hp=hp)
    a, b = out[torch.float32], out[torch.float64]
    for k in ("word_encoder_out", "dur", "mel_out", "z_p", "m_q", "logs_q", "kl"):
        assert a[k].dtype == torch.float32 and b[k].dtype == torch.float64, k
        scale = float(b[k].abs().max())
        assert float((a[k].double() - b[k]).abs().max()) <= 2e-5 * max(1.0, scale), k
    plain = pr.forward_posterior(ar.state(sd, torch.float64), *ar.inputs(batch, torch.float64), T(mels).double(), m2w, T(eps).double(), hp=hp)
    assert float((plain["dur"] - b["dur"]).abs().max()) > 1e-3   # the speakers matter


def test_unconditioned_state_dict_and_forward_ignore_the_speaker_arguments():
    a, b = ar.sd_np({}), ar.sd_np({}, "id", 8)
    assert set(b) - set(a) == {"spk_embed_proj.weight"} and all(np.array_equal(a[k], b[k]) for k in a)
    assert ar.sd_np(ar.CONFIGS[sh.H384], "embed")["spk_embed_proj.weight"].shape == (384, 256)


@pytest.mark.parametrize("name", [c["name"] for c in sh.INFER])
def test_case_keeps_the_tie_cap_in_float64(eight_threads, name):
    """the float64 restatement alone: at most MAX_TIES utterances of a case have a duration so near a rounding tie that the GPU test
    leaves their mel2word uncompared; the case's shapes are what its name says; every padded row holds its utterance's speaker row"""
    c = sh.BY_NAME[name]
    want = sh.reference(name)
    b = sh.batch(name)
    B, T_w = b["word_tokens"].shape
    assert len(want["ties"]) <= sh.MAX_TIES, want["ties"]
    print(f"{name}: B={B} T_w={T_w} near-tie utterances {want['ties']}")
    assert want["word_encoder_out"].shape == (B, T_w, sh.hidden_of(c["shape"])) and len(c["spk"]) == B
    m2w = T(sh.mel2word(name))
    assert torch.equal(want["mel2word"][:, :m2w.shape[1]], m2w) and want["pred_mel2word"].shape[1] % 4 == 0
    rows64, _ = sh.speaker_rows(c)
    pad = b["word_tokens"] == 0
    weo = want["word_encoder_out"].numpy()
    for u, t in np.argwhere(pad):
        assert np.abs(weo[u, t] - rows64[u]).max() <= 1e-12
    if c["kind"] == "rowmap":
        n = sh.word_counts(name)
        assert n[0] == T_w and n[1] == 1 and len(set(np.asarray(c["spk"]).reshape(B, -1).sum(1).tolist())) == B
    if c["kind"] == "wide" and c["form"] == "id":
        assert B > 256 and c["spk"].min() == 0 and c["spk"].max() == c["num_spk"] - 1 and c["spk"][255] == c["spk"][256]
    if c["kind"] == "exact":
        assert np.array_equal(sh.exact_rows(c), rows64.astype(np.float32))   # one exact product and the bias: a single rounding


# planted on the G11 batch with its unit-norm embeddings (the case the old gates were written for)
@pytest.fixture(scope="module")
def planted_case():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    name = sh.G11["name"]
    want = sh.reference(name)
    clean = sh.forward(name, torch.float32)
    torch.set_num_threads(n)
    return name, want, clean


def _bounds_report(case, got, want, batch):
    fails = []
    ar.compare(case, got, want, INFER_KEYS, fails, batch)
    return fails


def test_undamaged_fp32_restatement_stays_inside_every_bound(planted_case):
    name, want, clean = planted_case
    assert _bounds_report("cpu clean", clean, want, sh.batch(name)) == []


def test_planted_neighbour_speaker_row_passes_the_old_gates_and_fails_the_row_bounds(planted_case, golden_dir, eight_threads):
    """(a) the first valid row of every utterance b > 0 moved by 5e-5 towards utterance b - 1's speaker row: invisible to G11's gates
    (1e-4 / 1e-4 / 1e-3 max-abs and equal integer durations, against the reference's own goldens), reported per row"""
    name, want, clean = planted_case
    bad = sh.forward(name, torch.float32, sh.defect_neighbour_row(5e-5))
    moved = (bad["word_encoder_out"] - clean["word_encoder_out"]).abs().amax(-1)
    assert moved[1:, 0].min() > 4.9e-5 and moved[:, 1:].max() == 0 and moved[0].max() == 0
    fails = _bounds_report("cpu planted (a)", bad, want, sh.batch(name))
    assert any("word_encoder_out max" in f for f in fails), fails
    assert ar.rowcmp(bad["word_encoder_out"], want["word_encoder_out"])["at"][1] == 0
    # the old gates, as tests/test_speaker_gpu.py applies them: predicted durations, the golden's prior sample
    g = np.load(os.path.join(golden_dir, "g11_speaker.npz"))
    (wt, dm, pm), spk, z = _g11_inputs(g, "embed", torch.float32)
    r = ar.forward(ar.state(sr.g11_state_dict("embed")), {}, wt, dm, pm, z_p=z, form="embed", spk=spk, spk_hook=sh.defect_neighbour_row(5e-5))
    assert np.array_equal(r["mel2word"].numpy(), g["embed.mel2word"]) and np.array_equal(r["x_mask"].numpy(), g["embed.x_mask"])
    errs = {k: float(np.abs(r[k].numpy() - g[f"embed.{k}"]).max()) for k in ("dur", "word_encoder_out", "mel_out")}
    assert errs["dur"] <= 1e-4 and errs["word_encoder_out"] <= 1e-4 and errs["mel_out"] <= 1e-3, errs
    assert errs["word_encoder_out"] > 4e-5   # the defect is in there


def test_planted_untransposed_projection_pair_fails_the_row_bounds(planted_case, eight_threads):
    """(b) one (o, k) pair of W^T read as (k mod C, o mod 256): one channel of every speaker row is off"""
    name, want, clean = planted_case
    c = sh.BY_NAME[name]
    sd = ar.state(sh.state_np(c))
    bad = sh.forward(name, torch.float32, sh.defect_untransposed_pair(sd, T(c["spk"]), o=5, k=200))
    off = (bad["word_encoder_out"] - clean["word_encoder_out"]).abs().amax((0, 1))
    assert off[5] > 0 and off[:5].max() == 0 and off[6:].max() == 0
    fails = _bounds_report("cpu planted (b)", bad, want, sh.batch(name))
    assert any("word_encoder_out" in f for f in fails), fails
    # and the element-wise bound of the projected rows (the GPU test's) reports it on the padded rows
    rows64, bound = sh.speaker_rows(c)
    u, t = np.argwhere(sh.batch(name)["word_tokens"] == 0)[0]
    ratio = np.abs(bad["word_encoder_out"][u, t].double().numpy() - rows64[u]) / bound[u]
    ok = np.abs(clean["word_encoder_out"][u, t].double().numpy() - rows64[u]) / bound[u]
    assert ratio[5] > 1 and np.delete(ratio, 5).max() <= 1 and ok.max() <= 1, (ratio[5], ok.max())


def test_planted_unmasked_duration_input_fails_the_row_bounds(planted_case, eight_threads):
    """(c) the nonpadding mask in front of the duration predictor dropped: the padded rows carry the speaker into its convolutions"""
    name, want, clean = planted_case
    bad = sh.forward(name, torch.float32, sh.defect_unmasked_duration_input())
    assert torch.equal(bad["word_encoder_out"], clean["word_encoder_out"])
    fails = _bounds_report("cpu planted (c)", bad, want, sh.batch(name))
    assert any(f.split(": ")[1].startswith("dur ") for f in fails), fails
