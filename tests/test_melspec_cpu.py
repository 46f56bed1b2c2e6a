"""The log-mel front end without a GPU: the float64 yardstick (tests/melspec_ref.py) against an independent STFT, the filterbank's
defining properties, the binding against the header, and the refusals that happen before the GPU is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import melspec_ref as mr
from dict_tts_amd import abi, melspec, vocoder

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("n_fft,hop,win,L", [(1024, 256, 1024, 1357), (512, 128, 400, 100), (1024, 200, 800, 1400)])
def test_restatement_matches_an_independent_stft(n_fft, hop, win, L):
    """librosa.stft(center=True, pad_mode='constant', window='hann') == torch.stft with the periodic Hann window, in float64"""
    wav = np.random.default_rng(L).standard_normal(L)
    want = torch.stft(torch.from_numpy(wav), n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="constant", return_complex=True).abs().numpy().T
    got = mr.stft_mag(wav, n_fft, hop, win)
    assert got.shape == want.shape == (1 + L // hop, n_fft // 2 + 1)
    assert np.max(np.abs(got - want)) <= 1e-12
    assert np.allclose(melspec.hann_window(win), torch.hann_window(win, periodic=True, dtype=torch.float64).numpy(), rtol=0, atol=1e-15)
    assert np.array_equal(melspec.hann_window(win), mr.hann(win))


def test_empty_waveform_is_one_zero_frame():
    got = mr.stft_mag(np.zeros(0), 1024, 256, 1024)
    assert got.shape == (1, 513) and not got.any()
    fb = melspec.mel_filterbank(22050, 1024, 80, 80, 7600)
    assert np.all(mr.log_mel(mr.mel_lin(np.zeros(0), 1024, 256, 1024, fb)) == -6.0)


def test_float32_path_is_close_to_the_yardstick():
    """the reference's own arithmetic (float32 FFT) sits a few 1e-7 of a frame's largest mel value from float64: the scale of the GPU bound"""
    wav = (0.1 * np.random.default_rng(5).standard_normal(40 * 256 + 77)).astype(np.float32)
    fb = melspec.mel_filterbank(22050, 1024, 80, 80, 7600).astype(np.float32)
    e = mr.lin_error(mr.mel_lin_f32(wav, 1024, 256, 1024, fb), mr.mel_lin(wav, 1024, 256, 1024, fb))
    assert 1e-8 < e < 1e-6, e


def test_filterbank_properties():
    fb = melspec.mel_filterbank(22050, 1024, 80, 80, 7600)
    assert fb.shape == (80, 513) and fb.dtype == np.float64
    assert (fb >= 0).all()
    for row in fb:   # one peak: rises, then falls
        nz = np.flatnonzero(row)
        assert len(nz) and np.all(np.diff(nz) == 1)
        k = int(np.argmax(row))
        assert np.all(np.diff(row[nz[0]:k + 1]) >= 0) and np.all(np.diff(row[k:nz[-1] + 1]) <= 0)
    # Slaney normalisation: unit area per triangle, sum w * delta f.  The sum is taken on a grid fine enough to resolve the narrowest
    # triangle (67 Hz at the low end): on the 21.5 Hz grid of n_fft = 1024 two or three samples per triangle give 0.957 .. 1.079, which says
    # nothing about the normalisation
    fine = melspec.mel_filterbank(22050, 16384, 80, 80, 7600)
    area = fine.sum(axis=1) * (22050 / 16384)
    assert np.all(np.abs(area - 1.0) <= 0.02), (area.min(), area.max())
    assert abs(fb.max() - 0.02789) < 5e-6, fb.max()
    # fmin = -1 / fmax = -1 resolve as process_utterance resolves them
    assert np.array_equal(melspec.mel_filterbank(16000, 1024, 80, -1, -1), melspec.mel_filterbank(16000, 1024, 80, 0, 8000))
    nyq = melspec.mel_filterbank(16000, 1024, 80, 0, 8000)
    assert nyq[-1, -1] == 0.0 and nyq[-1, -2] > 0.0   # the last triangle ends ON the Nyquist bin
    assert (nyq[:, 0] == 0).all()                      # ... and the first starts on bin 0


def test_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert int(re.search(r"#define DTTS_OUT_MELSPEC (\d+)", hdr).group(1)) == abi.OUT_MELSPEC == 10
    assert int(re.search(r"#define DTTS_PART_MELSPEC (\d+)", hdr).group(1)) == abi.PART_MELSPEC == 8
    body = re.search(r"typedef struct dtts_melspec_args \{(.*?)\} dtts_melspec_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?([a-z_0-9A-Z]+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [f[0] for f in abi.MelspecArgs._fields_], names
    assert names == ["size", "hop", "B", "wav_ld", "mel_cap", "eps", "wav_dev", "wav_lens_dev", "mel_dev", "mel_lens_dev", "lin_dev"]
    assert C.sizeof(abi.MelspecArgs) == 6 * 4 + 5 * C.sizeof(C.c_void_p)
    assert abi.MelspecArgs.eps.offset == 20 and abi.MelspecArgs.wav_dev.offset == 24
    assert len(set(abi.EXPORTS)) == 32 and not any("melspec" in e for e in abi.EXPORTS)
    assert hasattr(abi.Context, "melspec")


def test_melspec_on_a_null_handle_is_invalid():
    lib = abi.load_library()
    args = abi.MelspecArgs(C.sizeof(abi.MelspecArgs))
    assert lib.dtts_text2mel_fetch(None, abi.OUT_MELSPEC, C.byref(args), None) == -22   # DTTS_E_INVAL


def test_defaults_carry_the_front_end_keys():
    from dict_tts_amd.hparams import BIAOBEI_DEFAULTS as d
    assert (d["fft_size"], d["hop_size"], d["win_size"], d["audio_num_mel_bins"], d["fmin"], d["fmax"], d["audio_sample_rate"]) == \
        (1024, 256, 1024, 80, 80, 7600, 22050)   # egs/egs_bases/tts/base.yaml:48-54


def test_return_linear_is_refused_before_the_gpu_is_touched():
    with pytest.raises(NotImplementedError, match="return_linear"):
        vocoder.HifiGAN.wav2spec(np.zeros(10, np.float32), return_linear=True)


def test_a_wav_file_at_another_rate_is_refused_before_the_gpu_is_touched(tmp_path):
    from scipy.io import wavfile
    fn = str(tmp_path / "a.wav")
    wavfile.write(fn, 16000, np.zeros(800, np.int16))
    with pytest.raises(ValueError, match=r"16000.*22050"):
        vocoder.HifiGAN.wav2spec(fn)
    assert melspec.read_wav(fn, 16000).shape == (800,)
