"""The PortaSpeech baseline without a GPU: the float64 restatement (tests/portaspeech_ref.py) against the reference's own run
(tests/golden/g19_portaspeech.npz, tools/make_golden_portaspeech.py), the conditions the GPU gate relies on, and the ABI's refusals.

  * per output, max |f64 - golden| <= 8 x max |f32 - f64| of the restatement itself; integer mel2word equal exactly;
  * condition, not measurement: every exp(dur) - 1 the length regulator reads, of the golden and of every seeded shape with predicted
    durations, lies >= 1e-3 from a half-integer in float64 (and the float32 restatement rounds it the same way);
  * the band formula of the relative attention against a literal pad / flatten / reshape restatement of the reference's
    relative <-> absolute conversion at T = 1 .. 12 (5 = window + 1 is where the reference stops slicing the table and starts padding it);
  * positions for non-contiguous and empty words;
  * planted defects (portaspeech_ref.DEFECTS): each exceeds the GPU gate at its least sensitive shape;
  * the argument block's wording, the numbering of the header, the refusals of fill_abi_config and the class picked from task_cls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import portaspeech_ref as pr
import portaspeech_shapes as ps
from dict_tts_amd import abi
from dict_tts_amd import hparams as H
from dict_tts_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,pre", [("golden", ""), ("golden_tf", "tf.")])
def test_float64_restatement_against_the_golden(golden_dir, name, pre):
    g = np.load(os.path.join(golden_dir, "g19_portaspeech.npz"))
    f64, f32 = ps.reference(name), ps.reference(name, torch.float32)
    assert np.array_equal(f64["mel2word"].numpy(), g[pre + "mel2word"]) and np.array_equal(f32["mel2word"].numpy(), g[pre + "mel2word"])
    if not pre:
        i = ps.inputs(name)
        assert np.array_equal(i["txt_tokens"], g["txt_tokens"]) and np.array_equal(i["ph2word"], g["ph2word"])
    live = g[pre + "mel2word"] > 0
    for k in ("ph_encoder_out", "word_encoder_out", "dur", "decoder_inp", "attn", "mel_out"):
        a64, a32, gg = f64[k].numpy(), f32[k].numpy().astype(np.float64), g[pre + k].astype(np.float64)
        if k == "attn":
            a64, a32, gg = a64[live], a32[live], gg[live]
        err, base = np.abs(a64 - gg).max(), np.abs(a32 - a64).max()
        print(f"{name} {k}: |f64 - golden| = {err:.3g}, |f32 - f64| = {base:.3g}")
        assert err <= pr.GATE * base, (k, err, base)
    assert np.array_equal(f64["x_mask"].numpy(), g[pre + "x_mask"])


@pytest.mark.parametrize("name", ["golden"] + ps.PREDICTED)
def test_durations_stay_clear_of_half_integers(name):
    f64, f32 = ps.reference(name, decode=name == "golden"), ps.reference(name, torch.float32, decode=name == "golden")
    gap = pr.min_half_distance(f64["dur"].numpy(), ps.live_words(name))
    print(f"{name}: min |exp(dur) - 1 - half-integer| = {gap:.4g}")
    assert gap >= 1e-3, f"{name}: pick another seed (a rounding flip could not be told from an error)"
    assert torch.equal(f32["mel2word"], f64["mel2word"])
    assert (f64["mel2word"] > 0).sum() <= 400                      # every case totals at most a few hundred frames


def test_golden_file_durations(golden_dir):
    g = np.load(os.path.join(golden_dir, "g19_portaspeech.npz"))
    assert pr.min_half_distance(g["dur"], ps.live_words("golden")) >= 1e-3
    assert g["tf.mel2word_in"].shape[1] % 4 != 0 and g["tf.mel2word"].shape[1] % 4 == 0
    assert os.path.getsize(os.path.join(golden_dir, "g19_portaspeech.npz")) < 700 * 1024


# ---------------------------------------------------------------------------------------------------------------------------------------
def _literal_rel_attention(q, k, v, ek, ev, w):
    """one head, no mask: the reference's route — cut or zero-pad the table to 2 T - 1 rows, logits against all of them, then the
    pad / flatten / reshape moves between relative and absolute indexing (rel_transformer_encoder.py:178-222), written out in numpy"""
    T, dk = q.shape

    def used(table):
        pad = max(T - (w + 1), 0)
        t = np.pad(table, ((pad, pad), (0, 0)))
        s = max((w + 1) - T, 0)
        return t[s:s + 2 * T - 1]

    def rel_to_abs(x):                                   # [T, 2T-1] -> [T, T]
        x = np.pad(x, ((0, 0), (0, 1))).reshape(-1)      # a column of padding, flattened: T * 2T
        x = np.pad(x, (0, T - 1))                        # up to (T + 1) * (2T - 1)
        return x.reshape(T + 1, 2 * T - 1)[:T, T - 1:]

    def abs_to_rel(x):                                   # [T, T] -> [T, 2T-1]
        x = np.pad(x, ((0, 0), (0, T - 1))).reshape(-1)  # T * (2T - 1)
        x = np.pad(x, (T, 0))                            # T zeros in front skew the rows
        return x.reshape(T, 2 * T)[:, 1:]

    s = q @ k.T / math.sqrt(dk) + rel_to_abs(q @ used(ek).T) / math.sqrt(dk)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p @ v + abs_to_rel(p) @ used(ev)


@pytest.mark.parametrize("T", range(1, 13))
def test_band_formula_equals_the_pad_and_reshape_route(T):
    w, dk = pr.WINDOW, 8
    rng = np.random.default_rng(T)
    q, k, v = (rng.standard_normal((T, dk)) for _ in range(3))
    ek, ev = rng.standard_normal((2 * w + 1, dk)), rng.standard_normal((2 * w + 1, dk))
    t = lambda a: torch.from_numpy(a)[None, None]
    got = pr.rel_attention(t(q), t(k), t(v), torch.from_numpy(ek), torch.from_numpy(ev), [T], w)[0, 0].numpy()
    assert np.abs(got - _literal_rel_attention(q, k, v, ek, ev, w)).max() <= 1e-12


def test_positions_of_non_contiguous_and_empty_words():
    x2w = torch.tensor([[1, 3, 1, 0, 3, 3, 5, 0], [2, 2, 2, 2, 0, 0, 0, 0]])
    got = pr.positions(x2w, 5, torch.float64).numpy()
    want = np.zeros(x2w.shape)
    for b in range(2):
        for t in range(8):
            wd = int(x2w[b, t])
            if wd:
                want[b, t] = sum(int(x2w[b, u]) == wd for u in range(t + 1)) / sum(int(x2w[b, u]) == wd for u in range(8))
    assert np.array_equal(got, want)
    assert want[0].tolist() == [0.5, 1 / 3, 1.0, 0.0, 2 / 3, 1.0, 1.0, 0.0]
    e = pr.sin_pos(torch.from_numpy(want), 8).numpy()
    f = np.exp(-np.arange(4) * math.log(10000) / 3)
    assert np.allclose(e[0, 1], np.concatenate([np.sin(f / 3), np.cos(f / 3)]), atol=1e-15)
    hid = torch.arange(16, dtype=torch.float64).reshape(1, 8, 2)
    m = pr.segment_mean(hid, x2w[:1], 5).numpy()[0]
    assert np.array_equal(m[0], [2.0, 3.0]) and np.array_equal(m[1], [0.0, 0.0]) and np.array_equal(m[3], [0.0, 0.0]) and np.array_equal(m[4], [12.0, 13.0])


# ---------------------------------------------------------------------------------------------------------------------------------------
DEFECT_CASES = ["tph1", "tph4", "tph5", "tph6", "tph10", "tph33", "ragged3", "words_of_1", "one_word", "word70", "h128_heads2"]


@pytest.mark.parametrize("defect", pr.DEFECTS)
def test_planted_defects_exceed_the_gate(defect):
    """the GPU gate can see each defect: at every shape where the defect changes anything, some output moves by more than
    8 x |f32 - f64|; the smallest such excess over the shapes is printed"""
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    worst = None
    for name in DEFECT_CASES:
        i = ps.inputs(name)
        if defect == "mean_is_sum" and max(max(w) for w in i["words"]) == 1:
            continue                                              # every word has one phoneme: sum = mean
        f64, f32 = ps.reference(name, decode=False), ps.reference(name, torch.float32, decode=False)
        bad = pr.forward(pr.state(ps.sd_np(i["hp"]), torch.float64), i["hp"], T(i["txt_tokens"]), T(i["ph2word"]), i["T_w"],
                         f64["mel2word"] if i["mel2word"] is None else T(i["mel2word"]), defect=defect, decode=False)
        best = 0.0
        for k in pr.KEYS:
            kk = "attn_live" if k == "attn" else k
            base = pr.row_err(f32[kk], f64[kk])
            e = pr.row_err(bad[kk], f64[kk])
            best = max(best, e / (pr.GATE * base) if base > 0 else (float("inf") if e > 0 else 0.0))
        print(f"{defect} at {name}: {best:.3g} x the gate")
        worst = best if worst is None else min(worst, best)
        assert best > 1.0, f"{defect} stays within the gate at {name}"
    assert worst is not None


# ---------------------------------------------------------------------------------------------------------------------------------------
def _block():
    return abi.ps_args(B=2, T_ph=9, T_w=4, txt_tokens=0x1000, ph2word=0x2000, status=0x3000, T_mel=C.c_int32(0))


def test_argument_block_wording():
    lib = abi.load_library()
    fetch = lambda a: (lib.dtts_text2mel_fetch(None, abi.PS_ENCODE, C.byref(a), None), lib.dtts_last_error(None).decode())
    a = _block()
    a.size -= 8
    rc, msg = fetch(a)
    assert rc == -22 and "DTTS_PS_ENCODE" in msg and f"size = {C.sizeof(a) - 8}" in msg, (rc, msg)
    rc, msg = fetch(_block())
    assert rc == -22 and msg == "dtts_text2mel_fetch(DTTS_PS_ENCODE): null handle", (rc, msg)
    for field, value, text in (("B", 0, "B = 0"), ("T_m2w", 5, "T_m2w = 5"), ("txt_tokens_dev", None, "null txt_tokens_dev"),
                               ("ph2word_dev", 0x2004, "not aligned")):
        a = _block()
        setattr(a, field, value)
        rc, msg = fetch(a)
        assert rc == -22 and text in msg, (field, rc, msg)


def test_header_numbers_and_names():
    with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as f:
        text = f.read()
    defs = {n: int(v) for n, v in re.findall(r"^#define (DTTS_\w+) (\d+)\b", text, re.M)}
    assert defs["DTTS_PART_PORTASPEECH"] == abi.PART_PORTASPEECH == 2048
    assert (defs["DTTS_PS_ENCODE"], defs["DTTS_PS_PH_ENCODER_OUT"], defs["DTTS_PS_ATTN"], defs["DTTS_PS_DECODER_INP"]) == \
        (abi.PS_ENCODE, abi.PS_PH_ENCODER_OUT, abi.PS_ATTN, abi.PS_DECODER_INP) == (65, 66, 67, 68)
    for n in ("BAD_TOKEN", "ZERO_TOKEN", "BAD_PH2WORD", "EMPTY_WORD", "BAD_MEL2WORD"):
        assert defs["DTTS_PS_" + n] == getattr(abi, "PS_" + n) and ("DTTS_PS_" + n) in abi.PS_STATUS_NAMES[getattr(abi, "PS_" + n)]
    assert not any(v >= 22 for v in abi.OUT_NAMES)            # the new items are no DTTS_OUT_* outputs
    assert abi.ps_status_error([0, 0, 0, 0]) is None and "utterance 2, position 7, value 99: DTTS_PS_BAD_TOKEN" in abi.ps_status_error([3, 1, 99, 7])


def _chain(tmp_path, extra):
    (tmp_path / "base.yaml").write_text("hidden_size: 192\nnum_heads: 2\nenc_layers: 4\nenc_ffn_kernel_size: 5\nword_enc_layers: 4\n"
                                        "dur_level: word\nuse_post_glow: false\nnum_spk: 1\nuse_spk_id: false\nuse_spk_embed: false\n")
    (tmp_path / "ps_adv.yaml").write_text("base_config: ./base.yaml\ntask_cls: tasks.tts.ps_adv.PortaSpeechAdvTask\n")
    (tmp_path / "leaf.yaml").write_text("base_config:\n  - ./ps_adv.yaml\n" + extra)
    return H.load_config_chain(str(tmp_path / "leaf.yaml"))


def test_fill_abi_config_on_the_two_ps_adv_chains(tmp_path):
    """the keys the two chains of the reference resolve to: biaobei (single speaker) fills; wenetspeech (use_spk_embed: true) is refused by name"""
    abi.load_library()
    hp = _chain(tmp_path, "ds_name: biaobei\n")
    assert H.is_baseline(hp) and M.model_cls(hp) is M.PortaSpeech and M.model_cls({"task_cls": "tasks.tts.dict_tts.DictTTSTask"}) is M.PortaSpeech_dict
    cfg = H.fill_abi_config(abi.default_config(), hp, n_phone=64, baseline=True)
    assert (cfg.hidden_size, cfg.num_heads, cfg.enc_layers, cfg.enc_ffn_kernel_size, cfg.n_phone) == (192, 2, 4, 5, 64)
    with pytest.raises(NotImplementedError, match="use_spk_embed"):
        H.fill_abi_config(abi.default_config(), _chain(tmp_path, "ds_name: wenetspeech\nuse_spk_embed: true\n"), n_phone=64, baseline=True)
    with pytest.raises(NotImplementedError, match="use_spk_id"):
        H.fill_abi_config(abi.default_config(), {**hp, "use_spk_id": True, "num_spk": 4}, baseline=True)
    with pytest.raises(NotImplementedError, match="dur_level"):
        H.fill_abi_config(abi.default_config(), {**hp, "dur_level": "ph"}, baseline=True)
    with pytest.raises(NotImplementedError, match="use_post_glow"):
        H.fill_abi_config(abi.default_config(), {**hp, "use_post_glow": True}, baseline=True)
    if not torch.cuda.is_available():
        with pytest.raises(abi.DttsError, match="needs a ROCm GPU"):
            M.PortaSpeech(hparams=hp)


def test_infer_takes_the_baselines_batches(tmp_path):
    """infer._model_forward / run_inference with a baseline batch (txt_tokens, ph2word, word_lengths): PortaSpeech.forward's arguments,
    a teacher-forced mel2word passed on, an empty pinyin_tokens column; a Dict-TTS batch is still told apart"""
    from dict_tts_amd import infer
    seen = {}

    class Model:
        def __call__(self, txt_tokens, ph2word, word_len, mel2word=None, infer=False, z_p=None):
            seen.update(txt=txt_tokens, p2w=ph2word, word_len=int(word_len), m2w=mel2word, infer=infer, z_p=z_p)
            B = txt_tokens.shape[0]
            return {"mel_out": torch.zeros(B, 8, 80), "mel_lens": torch.tensor([8, 5][:B], dtype=torch.int32)}

    class Vocoder:
        hop = 4

        def forward_batch(self, mel, lens):
            return torch.full((mel.shape[0], mel.shape[1] * self.hop), 0.25)

    b = ps.inputs("raw_not_mult4")
    batch = {"txt_tokens": torch.from_numpy(b["txt_tokens"]), "ph2word": torch.from_numpy(b["ph2word"]),
             "word_lengths": torch.tensor([len(w) for w in b["words"]]), "item_name": ["a", "b"], "text": ["x,y", "z."]}
    assert infer.is_baseline_batch(batch) and not infer.is_baseline_batch({"word_tokens": 0, "ph2word": 0})
    out, wavs = infer.infer_batch(Model(), Vocoder(), batch, z_p="noise")
    assert seen["infer"] is True and seen["word_len"] == 4 and seen["m2w"] is None and seen["z_p"] == "noise" and seen["txt"] is batch["txt_tokens"]
    assert [len(w) for w in wavs] == [32, 20]
    m2w = torch.from_numpy(b["mel2word"])
    infer.infer_batch(Model(), Vocoder(), {**batch, "mel2word_forced": m2w}, None)
    assert seen["m2w"] is m2w
    del batch["word_lengths"]                                     # without the lengths: ph2word's own maximum
    rows = infer.run_inference(Model(), Vocoder(), [batch], str(tmp_path), pinyin_encoder=[], save_wavs=True)
    assert seen["word_len"] == 4
    assert [r["pinyin_tokens"] for r in rows] == ["", ""] and rows[0]["text"] == "x，y"
    assert len(os.listdir(tmp_path / "wavs")) == 2 and (tmp_path / "meta.csv").exists()
