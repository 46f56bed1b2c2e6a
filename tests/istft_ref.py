"""float64 numpy restatement of the reference's spectral-subtraction filter, vocoders/vocoder_utils.py:7-15 — librosa's STFT (periodic Hann,
center=True, constant padding), v subtracted from every magnitude and clipped at zero with the phase kept, librosa's inverse STFT — and of
its halves (utils/audio.py:35-42).  librosa is not at hand where this suite is built; tests/test_spectral_cpu.py pins this
restatement against torch.stft / torch.istft in float64.  Every function takes the window as the transforms apply it: n_fft values, the
win_length samples zero padded and centred — the float32 array the library is given, computed with here in float64.

Also here: the same pipeline in float32 (torch.stft -> edit -> torch.istft on the CPU), the reference's own working precision, which sets
the unit of the accuracy bound of tests/test_spectral_gpu.py.
"""
import numpy as np

import melspec_ref as mr

ENV_MIN = 1e-11   # torch.istft's criterion


def window32(n_fft, win):
    """the periodic Hann window of win samples, centred in n_fft, rounded to float32: what dict_tts_amd.spectral hands to the library"""
    return mr.window_of(n_fft, win).astype(np.float32)


def frame_count(n_samples, hop):
    return 1 + int(n_samples) // int(hop)


def out_len(n_samples, hop):
    return int(hop) * (int(n_samples) // int(hop))


def stft(x, window, hop):
    """-> S [T, n_fft // 2 + 1] complex128, T = 1 + len // hop: n_fft // 2 zeros on both sides, S[t, k] = sum_n w[n] x_pad[t hop + n] e^(-2 pi i k n / n_fft)"""
    w = np.asarray(window, np.float64)
    return np.fft.rfft(mr.frames_of(x, len(w), hop) * w[None, :], axis=1)


def edit(S, v):
    """S max(|S| - v, 0) / |S|, 0 where |S| = 0; v = 0 returns S itself"""
    if v == 0:
        return S
    m = np.abs(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, S * (np.maximum(m - v, 0.0) / np.where(m > 0, m, 1.0)), 0.0)


def envelope(window, hop, T):
    """sum_t w^2[n - t hop] over the padded signal of hop (T - 1) + n_fft samples"""
    w2 = np.asarray(window, np.float64) ** 2
    N = len(w2)
    env = np.zeros(hop * (T - 1) + N)
    for t in range(T):
        env[t * hop:t * hop + N] += w2
    return env


def envelope_min(window, hop):
    """the smallest envelope value at a kept sample of ANY signal: a two-frame signal's (every further frame adds non-negative terms)"""
    N = len(window)
    return float(envelope(window, hop, 2)[N // 2:N // 2 + hop].min())


def istft(S, window, hop):
    """S [T, n_fft // 2 + 1] complex -> hop (T - 1) samples: y_t = w irfft(S[t]) (the imaginary parts of bins 0 and n_fft / 2 ignored),
    overlap-add at t hop, division by the envelope of the covering frames, n_fft // 2 samples dropped at both ends"""
    w = np.asarray(window, np.float64)
    N, T = len(w), S.shape[0]
    assert S.shape[1] == N // 2 + 1
    S = np.array(S, np.complex128, copy=True)
    S[:, 0] = S[:, 0].real
    S[:, -1] = S[:, -1].real
    fr = np.fft.irfft(S, n=N, axis=1) * w[None, :]
    y = np.zeros(hop * (T - 1) + N)
    for t in range(T):
        y[t * hop:t * hop + N] += fr[t]
    keep = slice(N // 2, N // 2 + hop * (T - 1))
    env = envelope(w, hop, T)[keep]
    if env.size and not env.min() > ENV_MIN:
        raise ValueError(f"hop = {hop}: the window envelope falls to {env.min():g}")
    return y[keep] / env


def denoise(x, window, hop, v):
    return istft(edit(stft(x, window, hop), v), window, hop)


def denoise_f32(x, window, hop, v):
    """the filter in the reference's working precision: float32 torch.stft -> edit -> torch.istft on the CPU.  -> float32 [hop (len // hop)]"""
    import torch
    x = torch.as_tensor(np.asarray(x, np.float32))
    w = torch.as_tensor(np.asarray(window, np.float32))
    N = len(w)
    S = torch.stft(x, N, hop_length=hop, win_length=N, window=w, center=True, pad_mode="constant", return_complex=True)
    if v != 0:
        m = S.abs()
        S = torch.where(m > 0, S * ((m - np.float32(v)).clamp(min=0) / torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(S))
    if S.shape[1] < 2:
        return np.zeros(0, np.float32)
    return torch.istft(S, N, hop_length=hop, win_length=N, window=w, center=True).numpy()


def unit_error(y, y64):
    """max |y - y64| in units of the waveform's peak (floored at 1e-6)"""
    y64 = np.asarray(y64, np.float64)
    if y64.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(y, np.float64) - y64)) / max(np.max(np.abs(y64)), 1e-6))
