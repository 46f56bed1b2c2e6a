"""Restatement of the reference's Griffin-Lim (utils/audio.py:35-42 ``griffin_lim``, 136-158 ``griffin_lim_torch``, 91-95 ``_mel_to_linear``) on
torch.stft / torch.istft, the yardstick of tests/test_griffinlim_cpu.py and tests/test_griffinlim_gpu.py.  The reference's own functions
cannot run where this suite is built (``np.complex``, librosa).  Per utterance of T frames, with the window as the transforms apply it (n_fft
values, zero padded and centred: tests/istft_ref.py):

    S = A init;  y = istft(S);  n_iter times { X = stft(y);  S = A X / |X| (S = A where |X| = 0, as np.angle(0) = 0);  y = istft(S) }

``griffin_lim`` is the loop in float64.  ``griffin_lim_f32`` is the same loop in float32 with the projection spelled as the reference spells it,
``amp * exp(1j * angle(X))``: "the reference arithmetic", whose error against float64 is the unit of the GPU tests' bounds, as
``istft_ref.denoise_f32`` is for the filter.
"""
import numpy as np
import torch

import istft_ref as ir

CONFIGS = {   # name -> (n_fft, hop, win, T)
    "n512": (512, 128, 512, 41),
    "n1024": (1024, 256, 1024, 37),
    "n2048": (2048, 512, 1200, 20),
}
SAMPLE_RATE = 22050


def hparams(name):
    n_fft, hop, win, _ = CONFIGS[name]
    return dict(fft_size=n_fft, hop_size=hop, win_size=win, audio_sample_rate=SAMPLE_RATE, audio_num_mel_bins=80, fmin=80, fmax=7600)


def signal(n_samples, seed=0):
    """a chirp, an amplitude-modulated tone and 0.02 white noise: float32 [n_samples], RMS about 0.26"""
    t = np.arange(n_samples, dtype=np.float64) / SAMPLE_RATE
    dur = max(n_samples / SAMPLE_RATE, 1e-9)
    chirp = 0.25 * np.sin(2.0 * np.pi * (300.0 * t + 0.5 * (3000.0 - 300.0) / dur * t * t))
    tone = 0.25 * (1.0 + 0.8 * np.sin(2.0 * np.pi * 7.0 * t)) * np.sin(2.0 * np.pi * 1234.5 * t)
    noise = 0.02 * np.random.default_rng(seed).standard_normal(n_samples)
    return (chirp + tone + noise).astype(np.float32)


def _w(window, dtype):
    return torch.as_tensor(np.asarray(window, np.float64)).to(dtype)


def stft(y, window, hop, dtype=torch.float64):
    """y [L] (tensor or array) -> [T, n_fft // 2 + 1] complex tensor, T = 1 + L // hop: center=True, constant padding"""
    y = torch.as_tensor(y).to(dtype)
    N = len(window)
    return torch.stft(y, N, hop_length=hop, win_length=N, window=_w(window, dtype), center=True, pad_mode="constant", return_complex=True).T


def istft(S, window, hop, dtype=torch.float64):
    """S [T, n_fft // 2 + 1] complex -> [hop (T - 1)] real tensor (empty for one frame)"""
    N = len(window)
    S = torch.as_tensor(S).to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    if S.shape[0] < 2:
        return torch.zeros(0, dtype=dtype)
    S = S.clone()
    S[:, 0] = S[:, 0].real.to(S.dtype)     # the imaginary parts of the two real bins are not part of a c2r transform's input
    S[:, -1] = S[:, -1].real.to(S.dtype)
    return torch.istft(S.T.contiguous(), N, hop_length=hop, win_length=N, window=_w(window, dtype), center=True)


def project(A, X):
    """A X / |X|, A where |X| = 0"""
    m = X.abs()
    return torch.where(m > 0, A * X / torch.where(m > 0, m, torch.ones_like(m)), A.to(X.dtype))


def griffin_lim(A, init, window, hop, n_iter, dtype=torch.float64, return_spec=False, reference_spelling=False):
    """A [T, bins] magnitudes, init [T, bins] complex -> y [hop (T - 1)] as a numpy array of `dtype` (and the last S)"""
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    A = torch.as_tensor(np.asarray(A)).to(dtype)
    S = A * torch.as_tensor(np.asarray(init)).to(cdtype)
    y = istft(S, window, hop, dtype)
    for _ in range(n_iter):
        X = stft(y, window, hop, dtype)
        S = A * torch.exp(1j * torch.angle(X)) if reference_spelling else project(A, X)
        y = istft(S, window, hop, dtype)
    return (y.numpy(), S.numpy()) if return_spec else y.numpy()


def griffin_lim_f32(A, init, window, hop, n_iter):
    """the reference arithmetic: float32 torch.stft / torch.istft, ``amp * exp(1j * angle(X))``"""
    return griffin_lim(np.asarray(A, np.float32), np.asarray(init, np.complex64), window, hop, n_iter, torch.float32, reference_spelling=True)


def consistency(y, A, window, hop):
    """d = || |STFT(y)| - A || / || A || in float64"""
    A = np.asarray(A, np.float64)
    return float(np.linalg.norm(np.abs(stft(np.asarray(y, np.float64), window, hop).numpy()) - A) / np.linalg.norm(A))


def mel_to_linear(mel_log10, inv_basis):
    """``_mel_to_linear`` on the project's log10-mels: max(1e-10, P 10^mel), float64; mel [T, n_mels], P [bins, n_mels] -> [T, bins]"""
    return np.maximum(1e-10, (10.0 ** np.asarray(mel_log10, np.float64)) @ np.asarray(inv_basis, np.float64).T)


def case(name, start, seed=0):
    """-> dict(window, hop, x, A float32 [T, bins], init complex64 [T, bins]) of a configuration: A = |STFT| of the test signal in float64
    rounded once; start 'perturbed' = the true phase + 0.5 rad Gaussian noise, 'random' = a uniform phase"""
    n_fft, hop, win, T = CONFIGS[name]
    w = ir.window32(n_fft, win)
    x = signal(hop * (T - 1), seed)
    X = stft(x, w, hop).numpy()
    assert X.shape == (T, n_fft // 2 + 1)
    rng = np.random.default_rng(100 + seed)
    if start == "perturbed":
        phase = np.angle(X) + 0.5 * rng.standard_normal(X.shape)
    else:
        assert start == "random"
        phase = 2.0 * np.pi * rng.random(X.shape)
    return dict(window=w, hop=hop, n_fft=n_fft, T=T, x=x, A=np.abs(X).astype(np.float32), init=np.exp(1j * phase).astype(np.complex64))
