"""CPU tests of the spectral-subtraction filter's pieces that need no device: the float64 oracle (tests/istft_ref.py) against torch.stft /
torch.istft in float64, the envelope criterion, the argument refusals of dict_tts_amd.spectral.Spectral, and the inference harness's
denoise_c switch with stand-in model / vocoder objects."""
import os

import numpy as np
import pytest
import torch

import istft_ref as ir
from dict_tts_amd import infer, spectral, synth

CONFIGS = [(1024, 256, 1024), (512, 128, 400), (1024, 200, 800), (2048, 300, 1200)]   # (n_fft, hop, win) of tests/test_melspec_gpu.py::CONFIGS


def _torch_stft64(x, w, hop):
    N = len(w)
    S = torch.stft(torch.as_tensor(np.asarray(x, np.float64)), N, hop_length=hop, win_length=N, window=torch.as_tensor(np.asarray(w, np.float64)),
                   center=True, pad_mode="constant", return_complex=True)
    return S.numpy().T   # [T, bins]


def _torch_istft64(S, w, hop):
    N = len(w)
    return torch.istft(torch.as_tensor(np.ascontiguousarray(S.T)), N, hop_length=hop, win_length=N, window=torch.as_tensor(np.asarray(w, np.float64)),
                       center=True).numpy()


@pytest.mark.parametrize("n_fft,hop,win", CONFIGS)
def test_oracle_against_torch_float64(n_fft, hop, win):
    w = ir.window32(n_fft, win)
    rng = np.random.default_rng(n_fft + hop)
    for L in (hop * 40 + 77, hop * 9, n_fft // 2 + 1):
        x = (0.1 * rng.standard_normal(L)).astype(np.float32)
        S = ir.stft(x, w, hop)
        assert S.shape == (ir.frame_count(L, hop), n_fft // 2 + 1)
        St = _torch_stft64(x, w, hop)
        assert St.shape == S.shape and np.max(np.abs(S - St)) <= 1e-12 * max(np.abs(St).max(), 1.0)
        m = np.abs(S)
        for v in (0.0, float(np.median(m)), 2.0 * float(m.max())):
            Se = ir.edit(S, v)
            if v == 0.0:
                assert Se is S
            want_S = St * (np.maximum(np.abs(St) - v, 0.0) / np.where(np.abs(St) > 0, np.abs(St), 1.0))
            assert np.max(np.abs(Se - want_S)) <= 1e-12 * max(np.abs(St).max(), 1.0)
            y = ir.istft(Se, w, hop)
            assert y.shape == (ir.out_len(L, hop),)
            yt = _torch_istft64(want_S, w, hop)
            assert yt.shape == y.shape and np.max(np.abs(y - yt)) <= 1e-12
            if v > 1.5 * m.max():
                assert not y.any()
            assert np.array_equal(y, ir.denoise(x, w, hop, v))
    for L in (100, 0):   # shorter than n_fft / 2: one frame, no output sample
        x = np.ones(L, np.float32)
        assert ir.stft(x, w, hop).shape[0] == ir.frame_count(L, hop) == 1 + L // hop
        assert ir.denoise(x, w, hop, 0.1).shape == (ir.out_len(L, hop),) == (hop * (L // hop),)


@pytest.mark.parametrize("n_fft,hop,win", CONFIGS)
def test_identity_at_v_zero(n_fft, hop, win):
    w = ir.window32(n_fft, win)
    x = (0.1 * np.random.default_rng(5).standard_normal(hop * 40 + 77)).astype(np.float32)
    y = ir.denoise(x, w, hop, 0.0)
    assert y.shape == (hop * 40,) and np.max(np.abs(y - x[:hop * 40])) <= 1e-12


def test_imaginary_parts_of_the_real_bins_are_ignored():
    n_fft, hop, win = 512, 128, 400
    w = ir.window32(n_fft, win)
    rng = np.random.default_rng(6)
    S = rng.standard_normal((12, n_fft // 2 + 1)) + 1j * rng.standard_normal((12, n_fft // 2 + 1))   # no signal has this spectrum
    S0 = S.copy()
    S0[:, 0] = S0[:, 0].real
    S0[:, -1] = S0[:, -1].real
    assert np.array_equal(ir.istft(S, w, hop), ir.istft(S0, w, hop))
    assert np.max(np.abs(ir.istft(S, w, hop) - _torch_istft64(S0, w, hop))) <= 1e-12


def test_envelope_criterion():
    hann = ir.window32(1024, 1024)
    assert hann[0] == 0.0
    assert ir.envelope_min(hann, 1024) == 0.0 == spectral.envelope_min(hann, 1024)       # w[0] = 0 is the only cover of a kept sample
    assert ir.envelope_min(hann, 512) > 0.49 and spectral.envelope_min(hann, 512) == ir.envelope_min(hann, 512)
    with pytest.raises(ValueError, match=r"hop_size = 1024.*envelope falls to 0"):
        spectral.Spectral(dict(fft_size=1024, hop_size=1024, win_size=1024))
    sp = spectral.Spectral(dict(fft_size=1024, hop_size=512, win_size=1024))
    assert sp.envelope_min == ir.envelope_min(hann, 512)
    with pytest.raises(ValueError, match="envelope"):
        ir.istft(np.ones((3, 513), np.complex128), hann, 1024)
    # the two-frame envelope is the smallest any signal sees, and restated identically in the package
    for n_fft, hop, win in CONFIGS + [(512, 1, 512), (512, 511, 300), (1024, 700, 1024), (512, 512, 100)]:
        w = ir.window32(n_fft, win)
        lo = ir.envelope_min(w, hop)
        assert spectral.envelope_min(w, hop) == lo
        assert np.array_equal(spectral.centred_hann(n_fft, win), w)
        for T in (2, 3, 4, 5, 9, n_fft // hop + 3):
            kept = ir.envelope(w, hop, T)[n_fft // 2:n_fft // 2 + hop * (T - 1)]
            assert kept.min() >= lo and (T > 2 or kept.min() == lo), (n_fft, hop, win, T)


def test_spectral_refuses_bad_arguments_without_a_device():
    with pytest.raises(ValueError, match="fft_size = 768"):
        spectral.Spectral(dict(fft_size=768, hop_size=192, win_size=768))
    with pytest.raises(ValueError, match="hop_size = 0"):
        spectral.Spectral(dict(fft_size=1024, hop_size=0, win_size=1024))
    with pytest.raises(ValueError, match="hop_size = 1025"):
        spectral.Spectral(dict(fft_size=1024, hop_size=1025, win_size=1024))
    with pytest.raises(ValueError, match="win_size = 1200"):
        spectral.Spectral(dict(fft_size=1024, hop_size=256, win_size=1200))
    sp = spectral.Spectral()   # the Biaobei defaults; no context yet
    assert (sp.n_fft, sp.hop, sp.win, sp.n_bins, sp.ctx) == (1024, 256, 1024, 513, None) and sp.frames(1000) == 4
    with pytest.raises(ValueError, match="v = -0.1"):
        sp.denoise(torch.zeros(1, 1000), v=-0.1)
    with pytest.raises(ValueError, match="v = nan"):
        sp.denoise(torch.zeros(1, 1000), v=float("nan"))
    with pytest.raises(ValueError, match="float32 cuda tensor"):
        sp.denoise(torch.zeros(1, 1000))
    with pytest.raises(ValueError, match="float32 cuda tensor"):
        sp.stft(np.zeros((1, 1000), np.float32))
    with pytest.raises(ValueError, match="complex64 cuda tensor"):
        sp.istft(torch.zeros(1, 4, 513))


class _FakeModel:
    def __call__(self, txt_tokens, pron_modified, kvm, ph2word, word_len, dict_msg, infer=False, z_p=None):
        B, Tw = txt_tokens[0].shape
        lens = torch.tensor([8 + 4 * b for b in range(B)], dtype=torch.int32)
        return {"mel_out": torch.zeros(B, int(lens.max()), 80), "pron_attn": torch.ones(B, Tw, dict_msg[3].shape[2]), "mel_lens": lens}


class _FakeVocoder:
    hop = 256

    def __init__(self):
        self.calls = []

    def forward_batch(self, mel, lens):
        B, T, _ = mel.shape
        return (0.5 * torch.sin(torch.arange(T * self.hop, dtype=torch.float32) / 20.0)).repeat(B, 1)

    def denoise(self, wav, lens, v):
        self.calls.append((tuple(wav.shape), lens.tolist(), v))
        return 0.5 * wav, lens * self.hop


def _run(tmp, voc, **kw):
    b = synth.make_batch(synth.biaobei_struct()["sentences"][:2], 1234)
    batch = {k: torch.from_numpy(v) for k, v in b.items()}
    batch["item_name"], batch["text"] = ["a", "b"], ["x", "y"]
    os.makedirs(tmp)
    rows = infer.run_inference(_FakeModel(), voc, [batch], str(tmp), [f"p{i}" for i in range(185)], **kw)
    return [open(os.path.join(tmp, "wavs", r["wav_fn_pred"] + ".wav"), "rb").read() for r in rows]


def test_run_inference_denoise_switch(tmp_path):
    """denoise_c = 0.0 (the default) never touches vocoder.denoise and writes the same bytes as a run without the argument; a positive
    value runs it between forward_batch and the int16 conversion, with the lengths in frames"""
    voc = _FakeVocoder()
    plain = _run(tmp_path / "plain", voc)
    zero = _run(tmp_path / "zero", voc, denoise_c=0.0)
    assert voc.calls == [] and plain == zero
    filtered = _run(tmp_path / "filtered", voc, denoise_c=0.25)
    assert voc.calls == [((2, 12 * 256), [8, 12], 0.25)]
    assert [len(f) for f in filtered] == [len(f) for f in plain] and filtered != plain
    half = np.frombuffer(filtered[0][44:], np.int16)
    full = np.frombuffer(plain[0][44:], np.int16)
    assert np.max(np.abs(half.astype(np.int32) * 2 - full)) <= 2
