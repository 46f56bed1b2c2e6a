"""The PortaSpeech baseline on the GPU (dict_tts_amd.model.PortaSpeech, csrc/portaspeech.hip) against the float64 restatement
tests/portaspeech_ref.py, which tests/test_portaspeech_cpu.py anchors on the reference's own run (tests/golden/g19_portaspeech.npz).
Seeded weights (synth.portaspeech_state_dict), never a checkpoint.

Gate, per output (ph_encoder_out, word_encoder_out, dur, decoder_inp, attn) and per case of tests/portaspeech_shapes.py:
max |gpu - float64| <= 8 x max |float32 restatement - float64|, both measured here on the same inputs; the ratios are printed as
``PSMEAS {json}`` lines.  Integer durations and mel2word equal the float64 restatement's exactly (the seeds keep every exp(dur) - 1
at least 1e-3 from a half-integer: tests/test_portaspeech_cpu.py).  mel_out against the golden within the project's mel tolerance 1e-3
(tests/test_gpu_parity.py).

Measured on an MI355X (LABNOTES.md "PortaSpeech baseline"), ratio = max|gpu - f64| / max|f32 restatement - f64| over the 22 cases and the
four alone-against-batch comparisons: ph_encoder_out 0.48 .. 1.29, word_encoder_out 0.46 .. 0.86, dur 0.10 .. 3.79, decoder_inp 0.26 ..
1.62, attn 0 .. 2.14 (spans of one phoneme are exact on both sides).  Above 3: dur at `one_word` only (3.79: one word of three phonemes,
so the yardstick is a single number, 5.0e-8 or a quarter ulp; the GPU's 1.9e-7 is under one ulp, and dur reads 0.10 .. 2.4 elsewhere).
mel_out: 3.3e-5 / 2.7e-5 against the golden; 3.49 / 4.20 x the float32 restatement's error against float64 (the decoder WaveNet runs on
split-bf16 operands, as for Dict-TTS).  An utterance alone, at the batch's padded widths and at wider ones (T_ph + 51 crosses a 64-key
tile), is bit-identical to itself in the batch."""
import numpy as np
import pytest
import torch

import fft_shapes
import portaspeech_ref as pr
import portaspeech_shapes as ps
from dict_tts_amd import abi, synth
from dict_tts_amd import model as M

pytestmark = pytest.mark.gpu
_MODELS, _RUNS = {}, {}
T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))


class _Dict:
    def __len__(self):
        return ps.N_PHONE


def model_of(hp, redzone=False):
    key = tuple(sorted(hp.items())) + (redzone,)
    if key not in _MODELS:
        m = M.PortaSpeech(_Dict(), hparams={**hp, **({"dtts_debug_redzone": 1} if redzone else {})})
        m.load_state_dict({k: T(v) for k, v in ps.sd_np(hp).items()})
        _MODELS[key] = m
    return _MODELS[key]


def run(name, redzone=False):
    """the GPU's forward of case `name`, once: every returned tensor as a CPU tensor"""
    key = (name, redzone)
    if key not in _RUNS:
        i = ps.inputs(name)
        m = model_of(i["hp"], redzone)
        f64 = ps.reference(name)
        B, T4 = f64["mel_out"].shape[0], f64["mel_out"].shape[1] // 4
        r = m(T(i["txt_tokens"]), T(i["ph2word"]), torch.tensor(i["T_w"]), mel2word=T(i["mel2word"]), infer=True, z_p=T(ps.noise(name, B, T4)))
        _RUNS[key] = {k: v.cpu() for k, v in r.items()}
    return _RUNS[key]


def gate(name, got, fails):
    f64, f32 = ps.reference(name), ps.reference(name, torch.float32)
    assert torch.equal(got["mel2word"], f64["mel2word"]), f"{name}: mel2word differs from the float64 restatement's"
    assert torch.equal(f32["mel2word"], f64["mel2word"]), f"{name}: the float32 restatement rounds a duration differently"
    d = lambda r: torch.clamp(torch.round(r["dur"].double().exp() - 1), min=0)
    live_w = ps.live_words(name)
    for b, n in enumerate(live_w):   # (a word whose frame count is beyond 2^23 has no integer resolution in float32: the 70-phoneme word, teacher-forced)
        ok = d(f64)[b, :n] < 2 ** 23
        assert torch.equal(d(got)[b, :n][ok], d(f64)[b, :n][ok]), f"{name}: integer durations of utterance {b} differ"
    ratios = {}
    for k in pr.KEYS:
        kk = "attn_live" if k == "attn" else k
        g = got[k].double().numpy()
        a32, a64 = f32[kk].double().numpy(), f64[kk].double().numpy()
        if k == "dur":
            g, a32, a64 = g[..., None], a32[..., None], a64[..., None]
        ratios[k] = pr.gate_check(name, k, g, a32, a64, fails)
        assert np.isfinite(g).all(), f"{name} {k}: non-finite values"
    return ratios


@pytest.mark.parametrize("name", ["golden", "golden_tf"] + ps.GPU_CASES)
def test_outputs_within_the_gate_of_float64(name):
    fails = []
    gate(name, run(name), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,pre", [("golden", ""), ("golden_tf", "tf.")])
def test_golden_is_reproduced(golden_dir, name, pre):
    g = np.load(f"{golden_dir}/g19_portaspeech.npz")
    got = run(name)
    assert np.array_equal(got["mel2word"].numpy(), g[pre + "mel2word"])
    err = float(np.abs(got["mel_out"].numpy() - g[pre + "mel_out"]).max())
    f64 = ps.reference(name)
    e64 = pr.row_err(got["mel_out"], f64["mel_out"])
    b64 = pr.row_err(ps.reference(name, torch.float32)["mel_out"], f64["mel_out"])
    print(f'PSMEAS {{"case": "{name}", "what": "mel_out", "err_golden": {err:.3e}, "err": {e64:.3e}, "f32_err": {b64:.3e}, "ratio": {e64 / b64:.2f}}}')
    assert err <= 1e-3, f"{name}: mel max-abs error {err} against the golden"
    live = g[pre + "mel2word"] > 0
    for k in ("ph_encoder_out", "word_encoder_out", "dur", "decoder_inp"):
        assert np.abs(got[k].numpy() - g[pre + k]).max() <= 1e-4, k
    assert np.abs(got["attn"].numpy()[live] - g[pre + "attn"][live]).max() <= 1e-5
    assert np.array_equal(got["x_mask"].numpy(), g[pre + "x_mask"])


def test_attention_rows():
    for name in ("ragged3", "zero_frame_word", "word70", "golden_tf"):
        got, i = run(name), ps.inputs(name)
        attn, m2w = got["attn"].numpy(), got["mel2word"].numpy()
        live = m2w > 0
        assert np.abs(attn[live].sum(-1) - 1).max() <= 1e-6, name
        assert (attn[~live] == 0).all(), f"{name}: attn rows of frames without a word must be zeros"
        same = m2w[:, :, None] == i["ph2word"][:, None, :]
        assert (attn[~same] == 0).all(), f"{name}: weight outside the frame's word span"
        assert (got["decoder_inp"].numpy()[~live] == 0).all()


def _kernels(B, T_ph, T_w, hidden=192, heads=2):
    enc = fft_shapes.kernels({"hidden": hidden, "heads": heads, "k": 5}, B, T_ph)
    word = fft_shapes.kernels({"hidden": hidden, "heads": heads, "k": 1}, B, T_w)
    return {"enc": {k: v for k, v in enc.items() if k != "mha"}, "word": word}


@pytest.mark.parametrize("b", [0, 1])
def test_an_utterance_alone_and_in_a_batch(b):
    """the same utterance alone, padded to the batch's T_ph / T_w: within the gate always, bit-identical whenever the convolutions and
    the word encoder's attention run the same kernels at both batch sizes (the baseline's own kernels never depend on B or the widths)"""
    name = "ragged3"
    i, batch = ps.inputs(name), run(name)
    m = model_of(i["hp"])
    n_f = int((batch["mel2word"][b] > 0).sum())
    # teacher-forced with the batch's own frames of this utterance, zeros up to a multiple of 4 (no last column to repeat)
    m2w = batch["mel2word"][b:b + 1, :(n_f + 3) // 4 * 4]
    r = m(T(i["txt_tokens"][b:b + 1]), T(i["ph2word"][b:b + 1]), torch.tensor(i["T_w"]), mel2word=m2w, infer=True,
          z_p=torch.zeros(1, 16, m2w.shape[1] // 4))
    alone = {k: v.cpu() for k, v in r.items()}
    f64, f32 = ps.reference(name), ps.reference(name, torch.float32)
    same = _kernels(1, *i["txt_tokens"].shape[1:], i["T_w"]) == _kernels(i["txt_tokens"].shape[0], i["txt_tokens"].shape[1], i["T_w"])
    fails = []
    for k in pr.KEYS:
        rows = slice(0, n_f) if k in ("decoder_inp", "attn") else slice(None)
        a, g = alone[k][0][rows].double().numpy(), batch[k][b][rows].double().numpy()
        kk = "attn_live" if k == "attn" else k
        pr.gate_check(f"{name}[{b}] alone", k, a, f32[kk][b][rows].double().numpy(), f64[kk][b][rows].double().numpy(), fails)
        if same:
            assert np.array_equal(a, g), f"{k}: utterance {b} alone differs from itself in the batch (same kernels at both shapes)"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["tph33", "tph65"])
def test_memory_safety_mode(name):
    got = run(name, redzone=True)
    m = model_of(ps.inputs(name)["hp"], True)
    assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()
    plain = run(name)
    for k in pr.KEYS + ("mel_out",):
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], plain[k]), f"{k}: the NaN-filled workspace changes the result (a stale or out-of-range read)"


def _encode(m, txt, ph2word, T_w, mel2word=None):
    dev = m.device
    txt, ph2word = T(txt).to(dev), T(ph2word).to(dev)
    m2w = None if mel2word is None else T(mel2word).to(dev)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    m.ctx.ps_encode(txt.shape[0], txt.shape[1], T_w, txt.data_ptr(), ph2word.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream,
                    mel2word=(m2w.data_ptr(), m2w.shape[1]) if m2w is not None else None)
    return status.cpu().tolist()


def test_status_codes_are_raised_by_name():
    """argument errors only: every kernel bounds-checks what it indexes by, so no launch can fault on these inputs"""
    i = ps.inputs("ragged3")
    m = model_of({})
    txt, p2w, T_w = i["txt_tokens"], i["ph2word"], i["T_w"]
    fwd = lambda t, p, **kw: m(T(t), T(p), torch.tensor(T_w), infer=True, **kw)

    def bad(t, p, code, text, utt, **kw):
        with pytest.raises(abi.DttsError) as e:
            fwd(t, p, **kw)
        assert text in str(e.value) and f"utterance {utt}," in str(e.value), str(e.value)
        # the same through the call without a synchronisation (a teacher-forced mel2word): the status word carries it
        st = _encode(m, t, p, T_w, mel2word=kw.get("mel2word", np.ones((t.shape[0], 4), np.int64)))
        assert st[0] == utt + 1 and st[1] == code, st

    t = txt.copy(); t[1, 0] = ps.N_PHONE
    bad(t, p2w, abi.PS_BAD_TOKEN, "DTTS_PS_BAD_TOKEN", 1)
    t = txt.copy(); t[0, 3] = 0
    bad(t, p2w, abi.PS_ZERO_TOKEN, "DTTS_PS_ZERO_TOKEN", 0)
    p = p2w.copy(); p[0, 4] = 1
    bad(txt, p, abi.PS_BAD_PH2WORD, "DTTS_PS_BAD_PH2WORD", 0)
    p = p2w.copy(); p[1, 3] = T_w + 1
    bad(txt, p, abi.PS_BAD_PH2WORD, "DTTS_PS_BAD_PH2WORD", 1)
    # a live frame of a word without phonemes (utterance 2 has one word; word 2 is empty), and a mel2word that is no such sequence
    m2w = np.array([[1, 1, 2, 2], [1, 2, 2, 0], [1, 2, 2, 0]], np.int64)
    bad(txt, p2w, abi.PS_EMPTY_WORD, "DTTS_PS_EMPTY_WORD", 2, mel2word=m2w)
    m2w = np.array([[1, 1, 2, 2], [2, 1, 2, 0], [1, 0, 0, 0]], np.int64)
    bad(txt, p2w, abi.PS_BAD_MEL2WORD, "DTTS_PS_BAD_MEL2WORD", 1, mel2word=m2w)
    m2w = np.array([[1, 1, 2, T_w + 1], [1, 1, 2, 0], [1, 0, 0, 0]], np.int64)
    bad(txt, p2w, abi.PS_BAD_MEL2WORD, "DTTS_PS_BAD_MEL2WORD", 0, mel2word=m2w)
    # the context still works afterwards
    assert _encode(m, txt, p2w, T_w) == [0, 0, 0, 0]


def test_dict_only_items_are_refused_after_a_baseline_encode():
    m = model_of({})
    run("one_word")
    i = ps.inputs("one_word")
    assert _encode(m, i["txt_tokens"], i["ph2word"], i["T_w"]) == [0, 0, 0, 0]
    buf = torch.zeros(1 << 16, device=m.device)
    for what in (abi.OUT_PRON_ATTN, abi.OUT_DICT_ATTN, abi.OUT_CONTEXT):
        with pytest.raises(abi.DttsError, match="PortaSpeech baseline"):
            m.ctx.fetch(what, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(abi.DttsError, match="one acoustic model"):
        m.ctx.finalize(abi.PART_ACOUSTIC)


@pytest.mark.parametrize("b,extra_ph,extra_w", [(0, 7, 3), (1, 51, 1)])
def test_an_utterance_alone_at_wider_padded_axes(b, extra_ph, extra_w):
    """the same utterance alone with T_ph and T_w padded WIDER than in the batch (51 more phonemes cross a 64-key tile): within the gate,
    and bit-identical on its own rows whenever the shared convolution / attention kernels are the same at both shapes — the baseline's own
    kernels depend neither on B nor on the padded widths"""
    name = "ragged3"
    i, batch = ps.inputs(name), run(name)
    m = model_of(i["hp"])
    B, T_ph = i["txt_tokens"].shape
    wide = synth.portaspeech_batch([i["words"][b]], ps.SEED, ps.N_PHONE, T_ph=T_ph + extra_ph, T_w=i["T_w"] + extra_w)
    n_ph, n_w = int(sum(i["words"][b])), len(i["words"][b])
    if b == 0:   # (the tokens are seeded by utterance index and length: utterance 0 alone draws the same ones)
        assert np.array_equal(wide["txt_tokens"][0, :n_ph], i["txt_tokens"][b, :n_ph])
    else:
        wide["txt_tokens"][0, :n_ph] = i["txt_tokens"][b, :n_ph]
    n_f = int((batch["mel2word"][b] > 0).sum())
    m2w = batch["mel2word"][b:b + 1, :(n_f + 3) // 4 * 4]
    r = m(T(wide["txt_tokens"]), T(wide["ph2word"]), torch.tensor(wide["T_w"]), mel2word=m2w, infer=True, z_p=torch.zeros(1, 16, m2w.shape[1] // 4))
    alone = {k: v.cpu() for k, v in r.items()}
    f64, f32 = ps.reference(name), ps.reference(name, torch.float32)
    same = _kernels(1, T_ph + extra_ph, wide["T_w"]) == _kernels(B, T_ph, i["T_w"])
    fails = []
    for k in pr.KEYS:
        kk = "attn_live" if k == "attn" else k
        rows = {"ph_encoder_out": n_ph, "word_encoder_out": n_w, "dur": n_w, "decoder_inp": n_f, "attn": n_f}[k]
        cut = lambda x: (x[:rows, :n_ph] if k == "attn" else x[:rows]).double().numpy()
        a, g = cut(alone[k][0]), cut(batch[k][b])
        pr.gate_check(f"{name}[{b}] alone, wider axes", k, a, cut(f32[kk][b]), cut(f64[kk][b]), fails)
        if same:
            assert np.array_equal(a, g), f"{k}: utterance {b} alone at wider padded axes differs from itself in the batch"
        if k == "attn":
            assert (alone[k][0][:, n_ph:] == 0).all()
        elif k != "dur":
            assert (alone[k][0][rows:] == 0).all(), f"{k}: rows past the utterance's own must be zeros"
    assert not fails, "\n".join(fails)


def test_python_refusals():
    m = model_of({})
    i = ps.inputs("one_word")
    with pytest.raises(NotImplementedError, match="infer=False"):
        m(T(i["txt_tokens"]), T(i["ph2word"]), torch.tensor(i["T_w"]), infer=False)
    with pytest.raises(NotImplementedError, match="infer=False"):
        m(T(i["txt_tokens"]), T(i["ph2word"]), torch.tensor(i["T_w"]), tgt_mels=torch.zeros(1, 8, 80))
    with pytest.raises(NotImplementedError, match="dur_level"):
        M.PortaSpeech(_Dict(), hparams={"dur_level": "ph"})
    with pytest.raises(NotImplementedError, match="use_spk_embed"):
        M.PortaSpeech(_Dict(), hparams={"use_spk_embed": True, "num_spk": 4})
    with pytest.raises(ValueError, match="ph2word must be"):
        m(T(i["txt_tokens"]), T(i["ph2word"][:, :2]), torch.tensor(i["T_w"]), infer=True)
