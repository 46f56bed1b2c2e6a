"""Restatement of the reference's multi-resolution STFT figures (modules/hifigan/stft_loss.py: stft(), SpectralConvergengeLoss,
LogSTFTMagnitudeLoss, MultiResolutionSTFTLoss) for the tests of dict_tts_amd/csrc/stftdist.hip.  The module itself calls torch.stft
without return_complex and no longer runs on a current torch; what it computes is

    X    = torch.stft(sig, fft_size, hop, win_length, torch.hann_window(win_length))          # center=True, pad_mode='reflect'
    m    = sqrt(clamp(re^2 + im^2, min=1e-7))                                                  # [B, frames, bins]
    sc   = norm(m_y - m_x, 'fro') / norm(m_y, 'fro')         mag = l1_loss(log m_y, log m_x)   # forward(x, y): y normalises

Three oracles:
  * the same in float64: the yardstick;
  * the same in float32: the reference's OWN arithmetic, whose distance from the float64 figures is the unit of every accuracy bound;
  * ``emulate_mag``: the kernel's summation on the CPU (fp32 sums over eight samples, joined in fp64, against the fp64 basis rounded to fp32),
    so that the bounds can be checked before the kernel ever runs.
Also the signal pairs, the lengths and the error figures that tests/test_stftdist_cpu.py and tests/test_stftdist_gpu.py share.
"""
import functools

import numpy as np
import torch

import melspec_ref as mr

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))   # (fft_size, hop, win_length): MultiResolutionSTFTLoss defaults
CLAMP = 1e-7
FACTOR = 4.0   # a direct fp32 sum against a float32 FFT: tests/test_melspec_gpu.py derives the factor
PAIRS = ("speech", "noise", "tone", "same", "dcnyq")
SR = 22050


def lengths(res):
    """two tiles and a frame count that is no multiple of 16; the last frame centred on the end (for fft_size 2048 the first multiple of the
    hop above fft_size / 2 would be 5 hops: 33 hops serves all three); the shortest signal torch.stft accepts (the mirror reaches all of it)"""
    n_fft, hop, _ = res
    return (69 * hop + 7, 33 * hop, n_fft // 2 + 1)


@functools.lru_cache(maxsize=None)
def _signals(L):
    sig = mr.signals(SR, L // 40 + 1)   # 40 * hop + 77 >= L samples
    return {k: v[:L] for k, v in sig.items()}


@functools.lru_cache(maxsize=None)
def pair(name, L):
    """(x, y) float32 [L].  dcnyq: an offset plus alternating +-1 puts the energy into bins 0 and fft_size / 2 — a kernel that drops
    either, or counts one twice, misses these figures."""
    s = _signals(L)
    if name == "speech":
        x, y = s["speech"], s["speech"] + np.float32(1e-3) * s["noise"]
    elif name == "noise":
        x, y = s["noise"], np.float32(0.5) * s["noise"]
    elif name == "tone":
        x, y = s["tone"], s["silence"]
    elif name == "same":
        x, y = s["speech"], s["speech"]
    elif name == "dcnyq":
        x = (0.5 + (1.0 - 2.0 * (np.arange(L) & 1))).astype(np.float32)
        y = np.float32(0.9) * x
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def stft_mag(sig, res, dtype=torch.float64):
    """the module's stft(): clamped magnitudes [frames, bins] (or [B, frames, bins]) in `dtype`, as a torch tensor"""
    n_fft, hop, win = res
    x = torch.as_tensor(np.asarray(sig), dtype=dtype)
    X = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=dtype), return_complex=True)
    return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=CLAMP)).transpose(-1, -2)


def sc_mag(mx, my):
    """SpectralConvergengeLoss / LogSTFTMagnitudeLoss of forward(x, y) in the dtype of the magnitudes -> (sc, mag) as Python floats"""
    mx, my = torch.as_tensor(mx), torch.as_tensor(my)
    sc = torch.norm(my - mx, p="fro") / torch.norm(my, p="fro")
    mag = torch.mean(torch.abs(torch.log(my) - torch.log(mx)))
    return float(sc), float(mag)


def sums_of(mx, my):
    """the three sums the library returns, in float64 from float64 magnitudes, and the count"""
    mx, my = np.asarray(mx, np.float64), np.asarray(my, np.float64)
    return np.array([np.sum((my - mx) ** 2), np.sum(my ** 2), np.sum(np.abs(np.log(my) - np.log(mx)))]), mx.size


def mag_error(m, m64):
    """max |m - m64| in units of each frame's largest m64 (floored at 1e-6)"""
    m64 = np.asarray(m64, np.float64)
    scale = np.maximum(m64.max(axis=-1, keepdims=True), 1e-6)
    return float(np.max(np.abs(np.asarray(m, np.float64) - m64) / scale))


def rel_dev(v, v64):
    return abs(v - v64) / abs(v64) if v64 != 0 else (0.0 if v == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def reference(name, res, L):
    """-> dict: m64 / m32 = (x, y) magnitudes as numpy, sc64 / mag64 / sc32 / mag32, e32 = (x, y) mag_error of the float32 path"""
    x, y = pair(name, L)
    m64 = tuple(stft_mag(s, res, torch.float64) for s in (x, y))
    m32 = tuple(stft_mag(s, res, torch.float32) for s in (x, y))
    sc64, mag64 = sc_mag(*m64)
    sc32, mag32 = sc_mag(*m32)
    m64n, m32n = tuple(m.numpy() for m in m64), tuple(m.numpy() for m in m32)
    return {"m64": m64n, "m32": m32n, "sc64": sc64, "mag64": mag64, "sc32": sc32, "mag32": mag32,
            "e32": tuple(mag_error(a, b) for a, b in zip(m32n, m64n))}


@functools.lru_cache(maxsize=None)
def scalar_unit():
    """the unit of the scalar bound: the largest relative deviation of the float32 path's sc / mag from the float64 figures over all pairs,
    resolutions and lengths of the set — pooled, so that a chance cancellation in one case does not set it"""
    unit = 0.0
    for res in RESOLUTIONS:
        for L in lengths(res):
            for name in PAIRS:
                r = reference(name, res, L)
                for k in ("sc", "mag"):
                    if r[k + "64"] != 0:
                        unit = max(unit, rel_dev(r[k + "32"], r[k + "64"]))
    return unit


# ---- the kernel's summation on the CPU ---------------------------------------------------------------------------------------------------
CHUNK = 8   # samples per fp32 chain (MELSPEC_CHUNK = 4 MFMA steps of two samples)


def centred_window32(n_fft, win):
    w = np.zeros(n_fft, np.float32)
    left = (n_fft - win) // 2
    w[left:left + win] = mr.hann(win).astype(np.float32)
    return w


def reflect_frames(sig, n_fft, hop):
    """torch.stft's center=True, pad_mode='reflect' by the kernel's index rule: g < 0 -> -g, g >= len -> 2 (len - 1) - g"""
    sig = np.asarray(sig, np.float32)
    n = len(sig)
    assert n > n_fft // 2
    g = hop * np.arange(1 + n // hop)[:, None] + np.arange(n_fft)[None, :] - n_fft // 2
    g = np.where(g < 0, -g, g)
    g = np.where(g >= n, 2 * (n - 1) - g, g)
    return sig[g]


@functools.lru_cache(maxsize=4)
def _basis32(n_fft, win):
    """the windowed DFT basis as the library packs it: fp32 window, fp64 cosine / sine of the exactly reduced angle, rounded once to fp32"""
    w = centred_window32(n_fft, win).astype(np.float64)
    ang = (np.arange(n_fft)[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft
    c, s = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft), np.sin(2.0 * np.pi * np.arange(n_fft) / n_fft)
    re, im = (w[:, None] * c[ang]).astype(np.float32), (-w[:, None] * s[ang]).astype(np.float32)
    im[:, 0] = 0.0
    im[:, n_fft // 2] = 0.0   # both edge bins are real: the kernel never forms their imaginary parts
    return re, im


def emulate_mag(sig, res):
    """clamped magnitudes [frames, bins] float32 by the kernel's arithmetic: fp32 products and sums over chunks of eight samples, the chunks
    joined in fp64, re / im rounded to fp32, p = max(re^2 + im^2, 1e-7) and sqrt in fp32.  (The MFMA fuses the product into the sum; here the
    product is rounded first, which can only cost accuracy.)"""
    n_fft, hop, win = res
    fr = reflect_frames(sig, n_fft, hop)
    bre, bim = _basis32(n_fft, win)
    left = (n_fft - win) // 2
    lo, hi = left // 128 * 128, min(n_fft, (left + win + 127) // 128 * 128)   # whole fours of 32-sample super-groups around the window
    T, bins = fr.shape[0], n_fft // 2 + 1
    dre, dim = np.zeros((T, bins)), np.zeros((T, bins))
    tmp = np.empty((T, bins), np.float32)
    for k0 in range(lo, hi, CHUNK):
        are, aim = np.zeros((T, bins), np.float32), np.zeros((T, bins), np.float32)
        for k in range(k0, k0 + CHUNK):
            col = fr[:, k:k + 1]
            np.multiply(col, bre[k][None, :], out=tmp)
            are += tmp
            np.multiply(col, bim[k][None, :], out=tmp)
            aim += tmp
        dre += are
        dim += aim
    re, im = dre.astype(np.float32), dim.astype(np.float32)
    p = np.maximum(re * re + im * im, np.float32(CLAMP))
    return np.sqrt(p)


def emulate_sums(mx, my):
    """the kernel's three sums from fp32 magnitudes: fp32 per element (one logarithm of the power ratio), fp64 across"""
    px, py = mx.astype(np.float32) ** 2, my.astype(np.float32) ** 2
    d = my.astype(np.float32) - mx.astype(np.float32)
    lg = np.float32(0.5) * np.abs(np.log(py / px))
    return np.array([np.sum((d * d).astype(np.float64)), np.sum(py.astype(np.float64)), np.sum(lg.astype(np.float64))]), mx.size


def sc_mag_of_sums(sums, count):
    return float(np.sqrt(sums[0] / sums[1])), float(sums[2] / count)
