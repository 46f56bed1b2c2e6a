"""Dynamic time warping on the device: the reference's ``utils/dtw.py`` (``dtw`` with the cost ``np.abs(x - y)``, as
``scripts/pitch_dtw.py`` drives it, and ``accelerated_dtw`` with the cityblock cost) and the F0 moments that script prints — computed by
dict_tts_amd/csrc/dtw.hip (dtts_text2mel_fetch(DTTS_OUT_DTW)).  Free-running inference predicts its own durations, so its mels and pitch
tracks do not line up with the recordings frame for frame; these are the figures the reference evaluates them by.

The recurrence is one add of an exact minimum per cell, so the device result equals the reference's in every bit — distance, accumulated
cost and path, including the tie order of ``_traceback`` (diagonal, then i - 1, then j - 1 on the unscaled values).  Tracks come in as
arrays, as the reference's ``f0/*.npy`` files do, or straight from the device's own F0 extraction (dict_tts_amd/pitch.py: Praat's
autocorrelation method; ``pitch.pitch_dtw_from_wavs`` chains the two without a host round trip).  pyworld's extractors stay outside.
"""
import math
import os

import numpy as np
import torch

from . import abi
from .unit import DeviceUnit

GT_SUFFIX = "_gt.npy"


def _as_batch(name, a):
    a = torch.as_tensor(a)
    if a.dim() == 2:
        a = a.unsqueeze(-1)
    if a.dim() != 3:
        raise ValueError(f"{name} must be [B, T] (one value per frame) or [B, T, F] (got {tuple(a.shape)})")
    if not a.dtype.is_floating_point:
        a = a.to(torch.float64)
    return a


def _lens(name, lens, B, ld):
    if lens is None:
        return None
    lens = torch.as_tensor(lens).reshape(-1)
    if lens.shape[0] != B:
        raise ValueError(f"{name} has {lens.shape[0]} entries for a batch of {B}")
    return lens


class DTW(DeviceUnit):
    """``DTW(ctx)(x, y, ...)``: a batch of pairs -> distance, path, accumulated cost, moments, as tensors on the device.

    ctx: an existing ``abi.Context`` (e.g. the model's), or None for one of its own; it is created on the first call, so that argument
    errors surface without a GPU."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def __call__(self, x, y, x_lens=None, y_lens=None, window=None, slope=1.0, path=True, acc=False, moments=False):
        """x [B, N] or [B, N, F], y [B, M] or [B, M, F] (float32, or float64 when either is), x_lens / y_lens [B] or None (= N / M),
        window: None (no band) or w >= 0, slope s > 0.  -> dict: dist f64 [B] (NaN for a bad pair: a length outside 1 .. its dimension, or
        w < |N - M|); with path=True path i32 [B, 2, N + M - 1] (rows: the x indices, the y indices; -1 behind path_len) and path_len
        i32 [B]; with acc=True acc f64 [B, N, M] (NaN outside a pair's own lengths); with moments=True (F = 1) moments f64 [B, 2, 4]:
        mean, sigma, skewness, Fisher kurtosis of x, then of y."""
        x, y = _as_batch("x", x), _as_batch("y", y)
        if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
            raise ValueError(f"x and y must agree in B and F (got {tuple(x.shape)} and {tuple(y.shape)})")
        B, N, F = x.shape
        M = y.shape[1]
        if B < 1:
            raise ValueError(f"B = {B}: an empty batch has no alignment")
        if not 1 <= F <= 128:
            raise ValueError(f"F = {F} (supported: 1 .. 128)")
        if not (1 <= N <= abi.DTW_MAX_LEN and 1 <= M <= abi.DTW_MAX_LEN):
            raise ValueError(f"N = {N}, M = {M} frames (supported: 1 .. {abi.DTW_MAX_LEN})")
        slope = float(slope)
        if not (math.isfinite(slope) and slope > 0):
            raise ValueError(f"slope = {slope} (must be finite and > 0; the reference asserts s > 0)")
        if window is None or (isinstance(window, float) and math.isinf(window) and window > 0):
            w = -1
        else:
            w = int(window)
            if w < 0 or w != window:
                raise ValueError(f"window = {window!r} (None or inf for no band, or an integer >= 0)")
            w = min(w, abi.DTW_MAX_LEN)
        if moments and F > 1:
            raise ValueError(f"moments are those of 1-D tracks (F = {F})")
        x_lens, y_lens = _lens("x_lens", x_lens, B, N), _lens("y_lens", y_lens, B, M)
        dt = torch.float64 if torch.float64 in (x.dtype, y.dtype) else torch.float32
        ctx = self._context()
        dev = self.device
        xd, yd = x.to(device=dev, dtype=dt).contiguous(), y.to(device=dev, dtype=dt).contiguous()
        xl = None if x_lens is None else x_lens.to(device=dev, dtype=torch.int32).contiguous()
        yl = None if y_lens is None else y_lens.to(device=dev, dtype=torch.int32).contiguous()
        out = {"dist": torch.empty(B, dtype=torch.float64, device=dev)}
        ptr = lambda t: None if t is None else t.data_ptr()
        if path:
            out["path"] = torch.empty(B, 2, N + M - 1, dtype=torch.int32, device=dev)
            out["path_len"] = torch.empty(B, dtype=torch.int32, device=dev)
        if acc:
            out["acc"] = torch.full((B, N, M), float("nan"), dtype=torch.float64, device=dev)
        if moments:
            out["moments"] = torch.empty(B, 2, 4, dtype=torch.float64, device=dev)
        ctx.dtw(B, torch.cuda.current_stream().cuda_stream, x=xd.data_ptr(), y=yd.data_ptr(), x_ld=N, y_ld=M, F=F, dtype=1 if dt == torch.float64 else 0,
                window=w, slope=slope, x_lens=ptr(xl), y_lens=ptr(yl), dist=out["dist"].data_ptr(), path=ptr(out.get("path")), path_ld=N + M - 1,
                path_len=ptr(out.get("path_len")), acc=ptr(out.get("acc")), moments=ptr(out.get("moments")))
        return out


def _pad_tracks(tracks, dtype):
    lens = [len(t) for t in tracks]
    out = np.zeros((len(tracks), max(lens)), dtype)
    for b, t in enumerate(tracks):
        out[b, :lens[b]] = t
    return out, np.asarray(lens, np.int32)


def _tracks(name, tracks):
    tracks = [np.asarray(t) for t in tracks]
    for b, t in enumerate(tracks):
        if t.ndim != 1 or t.shape[0] < 1:
            raise ValueError(f"{name}[{b}] must be a non-empty 1-D track (got shape {t.shape})")
        if t.shape[0] > abi.DTW_MAX_LEN:
            raise ValueError(f"{name}[{b}] has {t.shape[0]} frames (supported: 1 .. {abi.DTW_MAX_LEN})")
    return tracks


def pitch_dtw(f0_pred, f0_gt, ctx=None):
    """What ``scripts/pitch_dtw.py`` prints, for lists of 1-D F0 tracks (prediction b against recording b): -> dict of floats ``dtw`` (mean
    of distance / len(gt)), ``std``, ``skew``, ``kurtosis`` (means over the predictions of np.std, scipy.stats.skew / kurtosis with
    bias=True) and the per-utterance lists ``dtw_list``, ``std_list``, ``skew_list``, ``kurtosis_list``.  The tracks are warped in their own
    precision: float32 when every track is float32, float64 otherwise (parselmouth's are float64), as np.abs(x - y) is."""
    f0_pred, f0_gt = _tracks("f0_pred", f0_pred), _tracks("f0_gt", f0_gt)
    if len(f0_pred) != len(f0_gt) or not f0_pred:
        raise ValueError(f"{len(f0_pred)} predicted tracks for {len(f0_gt)} recordings: the tracks are compared pair by pair")
    dt = np.float32 if all(t.dtype == np.float32 for t in f0_pred + f0_gt) else np.float64
    x, xl = _pad_tracks(f0_pred, dt)
    y, yl = _pad_tracks(f0_gt, dt)
    out = DTW(ctx)(x, y, xl, yl, path=False, moments=True)
    dist = out["dist"].cpu().numpy() / yl.astype(np.float64)
    mom = out["moments"][:, 0].cpu().numpy()
    res = {"dtw": float(dist.mean()), "std": float(mom[:, 1].mean()), "skew": float(mom[:, 2].mean()), "kurtosis": float(mom[:, 3].mean())}
    res.update(dtw_list=dist.tolist(), std_list=mom[:, 1].tolist(), skew_list=mom[:, 2].tolist(), kurtosis_list=mom[:, 3].tolist())
    return res


def mel_dtw(mel_pred, mel_gt, pred_lens=None, gt_lens=None, ctx=None):
    """The cityblock DTW (``accelerated_dtw(x, y, 'cityblock')``) between predicted and recorded mels [B, T, n_mel] of their own lengths:
    -> dict of device tensors ``dtw`` f64 [B] (distance per ground-truth frame), ``dist`` f64 [B], ``path`` i32 [B, 2, T_pred + T_gt - 1]
    (the predicted frames, the recorded frames of the alignment; -1 behind ``path_len``), ``path_len`` i32 [B]."""
    mel_pred, mel_gt = torch.as_tensor(mel_pred), torch.as_tensor(mel_gt)
    if mel_pred.dim() != 3 or mel_gt.dim() != 3:
        raise ValueError(f"mel_pred and mel_gt must be [B, T, n_mel] (got {tuple(mel_pred.shape)} and {tuple(mel_gt.shape)})")
    out = DTW(ctx)(mel_pred, mel_gt, pred_lens, gt_lens, path=True)
    n = torch.full_like(out["dist"], mel_gt.shape[1]) if gt_lens is None else torch.as_tensor(gt_lens).reshape(-1).to(out["dist"])
    out["dtw"] = out["dist"] / n
    return out


def pair_f0_files(names, ext=".npy"):
    """The file names of a reference ``f0/`` directory -> [(prediction, recording)] sorted by name: ``NAME_gt.npy`` is the recording of
    ``NAME.npy``.  (scripts/pitch_dtw.py pairs the two glob lists by position, which holds only while both happen to come back in the same
    order.)  A recording without its prediction, or a prediction without its recording, is an error.  ext=".wav": the same rule for a
    directory of waveforms (``NAME.wav`` / ``NAME_gt.wav``)."""
    gt_suffix = "_gt" + ext
    names = sorted(os.path.basename(n) for n in names if n.endswith(ext))
    gts = [n for n in names if n.endswith(gt_suffix)]
    preds = set(n for n in names if not n.endswith(gt_suffix))
    pairs = []
    for g in gts:
        p = g[:-len(gt_suffix)] + ext
        if p not in preds:
            raise FileNotFoundError(f"{g} has no prediction {p}")
        preds.discard(p)
        pairs.append((p, g))
    if preds:
        raise FileNotFoundError(f"{sorted(preds)[0]} has no recording {sorted(preds)[0][:-len(ext)] + gt_suffix}")
    if not pairs:
        raise FileNotFoundError(f"no *{gt_suffix} track found")
    return pairs
