"""Restatements of the validation losses (test infrastructure), for dtts_text2mel_fetch(DTTS_OUT_LOSSES):

  * float64 numpy (``mel_sums64`` / ``dur_sums64``): what the kernels are held to.  The bias is added in float64, the window is the
    float32 one of dict_tts_amd.losses.ssim_window widened; the masked sums follow tasks/tts/tts_base.py:196-222 and
    tasks/tts/ps_flow.py:99-139 (eval mode), restated.
  * float32 torch (``ssim_map32`` / ``mel_sums32``): the reference's own arithmetic (F.conv2d on float32 images that carry the bias),
    the accuracy yardstick: the kernels may deviate from float64 no more than this path does.
"""
import numpy as np
import torch
import torch.nn.functional as F

from dict_tts_amd import losses as L

C1, C2 = 0.01 ** 2, 0.03 ** 2


def frame_weights(tgt):
    """[B, T] float64: 1 where the target row is not all zero (weights_nonzero_speech: abs().sum(-1).ne(0))"""
    return (np.abs(np.asarray(tgt, np.float64)).sum(-1) != 0).astype(np.float64)


def _moments64(a, win):
    B, T, M = a.shape
    k = win.shape[0]
    pad = np.pad(a, ((0, 0), (k // 2, k // 2), (k // 2, k // 2)))
    out = np.zeros_like(a)
    for i in range(k):
        for j in range(k):
            out += win[i, j] * pad[:, i:i + T, j:j + M]
    return out


def ssim_map64(pred, tgt, bias=L.SSIM_BIAS):
    """[B, T, n_mel] float64: the SSIM map of pred + bias and tgt + bias, zero outside the image"""
    win = L.ssim_window().astype(np.float64)
    x, y = np.asarray(pred, np.float64) + bias, np.asarray(tgt, np.float64) + bias
    mx, my = _moments64(x, win), _moments64(y, win)
    sxx, syy, sxy = _moments64(x * x, win) - mx * mx, _moments64(y * y, win) - my * my, _moments64(x * y, win) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def mel_sums64(pred, tgt, bias=L.SSIM_BIAS):
    """-> sums [B, 3] float64 (sum w |p - t|, sum w (p - t)^2, sum w (1 - ssim)), count [B] int64, the map"""
    pred, tgt = np.asarray(pred, np.float32), np.asarray(tgt, np.float32)
    w = frame_weights(tgt)[:, :, None]
    d = pred.astype(np.float64) - tgt.astype(np.float64)
    m = ssim_map64(pred, tgt, bias)
    sums = np.stack([(w * np.abs(d)).sum((1, 2)), (w * d * d).sum((1, 2)), (w * (1 - m)).sum((1, 2))], 1)
    count = (w[:, :, 0].sum(1) * pred.shape[2]).astype(np.int64)
    return sums, count, m


def batch_figures(sums, count):
    """the reference's batch figures l1, mse, ssim = sum_b sums / sum_b count"""
    return np.asarray(sums, np.float64).sum(0) / float(np.asarray(count).sum())


def ssim_map32(pred, tgt, bias=L.SSIM_BIAS):
    """[B, T, n_mel] float32: the map along the reference's float32 path (the bias added in float32, five F.conv2d with the window)"""
    win = torch.from_numpy(L.ssim_window())[None, None]
    x = torch.from_numpy(np.asarray(pred, np.float32))[:, None] + bias
    y = torch.from_numpy(np.asarray(tgt, np.float32))[:, None] + bias
    conv = lambda a: F.conv2d(a, win, padding=win.shape[-1] // 2)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx.pow(2), conv(y * y) - my.pow(2), conv(x * y) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx.pow(2) + my.pow(2) + C1) * (sxx + syy + C2))
    return m[:, 0].numpy()


def mel_sums32(pred, tgt, bias=L.SSIM_BIAS):
    """the per-utterance sum w (1 - ssim) of the float32 path, [B] float64 (the map float32, summed in float64: only the map's error)"""
    m = ssim_map32(pred, tgt, bias)
    w = frame_weights(tgt)[:, :, None]
    return (w * (1.0 - m.astype(np.float64))).sum((1, 2)), m


def dur_gt64(mel2word, T_w):
    """[B, T_w] int64: frames per word 1 .. T_w (mel2ph_to_dur); index 0 and values outside 0 .. T_w are ignored"""
    m = np.asarray(mel2word, np.int64)
    out = np.zeros((m.shape[0], T_w), np.int64)
    for b in range(m.shape[0]):
        v = m[b][(m[b] >= 1) & (m[b] <= T_w)]
        out[b] = np.bincount(v, minlength=T_w + 1)[1:]
    return out


def dur_sums64(dur_pred, mel2word, word_len, scale):
    """-> sums [B, 5] float64 (sum n |dp - g|, sum n, sum [g2 > 0] |dp2 - g2|, sum [g2 > 0], sum dp2 - sum g2), dur_gt [B, T_w]"""
    dp = np.asarray(dur_pred, np.float32).astype(np.float64)
    B, T_w = dp.shape
    d = dur_gt64(mel2word, T_w)
    n = (np.arange(1, T_w + 1)[None, :] <= np.asarray(word_len, np.int64).reshape(-1, 1)).astype(np.float64)
    dp = dp * n
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (np.log(d + 1.0) if scale == "log" else d.astype(np.float64)) * n
        dp2, g2 = (np.log(dp + 1.0), np.log(g + 1.0)) if scale == "log" else (dp, g)
    m2 = (g2 > 0).astype(np.float64)
    sums = np.stack([(n * np.abs(dp - g)).sum(1), n.sum(1), (m2 * np.abs(dp2 - g2)).sum(1), m2.sum(1), (dp2 - g2).sum(1)], 1)
    return sums, d


def dur_figures(sums):
    """wdur (eval), sdur, wdur_train of a batch"""
    s = np.asarray(sums, np.float64)
    t = s.sum(0)
    return t[2] / t[3], np.abs(s[:, 4]).mean(), t[0] / t[1]
