"""F0 extraction on the device: Boersma's autocorrelation method (Praat's ``Sound: To Pitch (ac)``, Hanning window), which the reference's
``data_gen/tts/data_gen_utils.py::get_pitch`` asks parselmouth for — ``Sound(wav, sr).to_pitch_ac(time_step=hop / sr,
voicing_threshold=0.6, pitch_floor=80, pitch_ceiling=750)`` — computed by dict_tts_amd/csrc/pitch.hip
(dtts_text2mel_fetch(DTTS_OUT_PITCH)) in fp64.  ``tasks/tts/dict_tts.py::after_infer`` calls it on the vocoded prediction and on the
recording; ``pitch_dtw_from_wavs`` does the same and hands the tracks to the pitch DTW (dict_tts_amd/dtw.py) without a host round trip.

The arithmetic is specified in include/dicttts_hip.h and restated in float64 by tests/pitch_ref.py.  No Praat was available to compare
against: what could not be settled is listed in INTEGRATION.md ("Known uncertainties of the F0 extraction").
"""
import math

import numpy as np
import torch

from . import abi
from . import dtw as _dtw
from .unit import DeviceUnit

PRAAT_DEFAULTS = dict(silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14)
REFERENCE_LPAD = {256: 4, 128: 8}   # get_pitch: pad_size * 2, pad_size = 2 (hop 256) / 4 (hop 128); any other hop trips its assert

# utils/pitch_utils.py
F0_BIN = 256
F0_MAX = 1100.0
F0_MIN = 50.0
F0_MEL_MIN = 1127 * np.log(1 + F0_MIN / 700)
F0_MEL_MAX = 1127 * np.log(1 + F0_MAX / 700)


def f0_to_coarse(f0):
    """utils/pitch_utils.py::f0_to_coarse for numpy input: 256 mel-spaced bins over 50 .. 1100 Hz, bin 1 = unvoiced or below, np.rint"""
    f0 = np.asarray(f0, np.float64)
    f0_mel = 1127 * np.log(1 + f0 / 700)
    pos = f0_mel > 0
    f0_mel[pos] = (f0_mel[pos] - F0_MEL_MIN) * (F0_BIN - 2) / (F0_MEL_MAX - F0_MEL_MIN) + 1
    f0_mel[f0_mel <= 1] = 1
    f0_mel[f0_mel > F0_BIN - 1] = F0_BIN - 1
    return np.rint(f0_mel).astype(np.int64)


def geometry(sample_rate, f0_min):
    """what the sample rate and the pitch floor fix (csrc/pitch.h::pitch_geometry): dict of nsw (window samples), half, nper, halfper,
    maxlag, brent (= brent_ixmax), n_lag, first (the shortest utterance with a frame)"""
    q = (3.0 * float(int(sample_rate))) / float(f0_min)      # the one real quotient
    nsw0 = int(math.floor(q))
    half = nsw0 // 2 - 1
    nsw = 2 * half
    nper = int(math.floor(float(int(sample_rate)) / float(f0_min)))
    return dict(nsw=nsw, half=half, nper=nper, halfper=nper // 2 + 1, maxlag=min(nsw // 3 + 2, nsw), brent=nsw // 2, n_lag=nsw // 2 + 1,
                first=int(math.ceil(q)))


def n_frames_of(L, first, hop):
    """frames of an L-sample utterance: floor((L / sr - 3 / floor) / (hop / sr)) + 1, from integers; 0 when too short"""
    return (int(L) - first) // hop + 1 if L >= first else 0


class PitchAC(DeviceUnit):
    """``PitchAC(...)(wavs, lens)``: a batch of waveforms -> F0 tracks, as tensors on the device.

    ctx: an existing ``abi.Context`` (e.g. the vocoder's), or None for one of its own; it is created on the first call, so that argument
    errors surface without a GPU.  The analysis parameters default to the reference's (get_pitch) and, where it leaves them alone, Praat's."""

    def __init__(self, ctx=None, sample_rate=22050, hop_size=256, f0_min=80.0, f0_max=750.0, voicing_threshold=0.6, silence_threshold=0.03,
                 octave_cost=0.01, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14):
        self.ctx = ctx
        self.sample_rate, self.hop = int(sample_rate), int(hop_size)
        if self.sample_rate != sample_rate or not 8000 <= self.sample_rate <= 48000:
            raise ValueError(f"sample_rate = {sample_rate!r} (supported: an integer in 8000 .. 48000)")
        if self.hop != hop_size or not 1 <= self.hop <= 4096:
            raise ValueError(f"hop_size = {hop_size!r} (supported: an integer in 1 .. 4096)")
        self.f0_min, self.f0_max = float(f0_min), float(f0_max)
        if not (math.isfinite(self.f0_min) and self.f0_min >= 10.0):
            raise ValueError(f"f0_min = {f0_min!r} (must be finite and >= 10 Hz)")
        self.geo = geometry(self.sample_rate, self.f0_min)
        if not 32 <= self.geo["nsw"] <= abi.PITCH_MAX_WINDOW:
            raise ValueError(f"f0_min = {f0_min!r} gives a window of {self.geo['nsw']} samples at {self.sample_rate} Hz (supported: 32 .. {abi.PITCH_MAX_WINDOW})")
        if not (math.isfinite(self.f0_max) and self.f0_max > self.f0_min):
            raise ValueError(f"f0_max = {f0_max!r} (must be finite and above f0_min = {self.f0_min})")
        self.params = dict(voicing_threshold=float(voicing_threshold), silence_threshold=float(silence_threshold), octave_cost=float(octave_cost),
                           octave_jump_cost=float(octave_jump_cost), voiced_unvoiced_cost=float(voiced_unvoiced_cost))
        for k in ("voicing_threshold", "silence_threshold"):
            if not (math.isfinite(self.params[k]) and self.params[k] > 0):
                raise ValueError(f"{k} = {self.params[k]} (must be finite and > 0)")
        for k in ("octave_cost", "octave_jump_cost", "voiced_unvoiced_cost"):
            if not (math.isfinite(self.params[k]) and self.params[k] >= 0):
                raise ValueError(f"{k} = {self.params[k]} (must be finite and >= 0)")

    @classmethod
    def from_hparams(cls, hp, ctx=None, **kw):
        """the extractor get_pitch runs for the reference's hparams: audio_sample_rate, hop_size, pitch_extractor (parselmouth)"""
        from .hparams import BIAOBEI_DEFAULTS
        hp = {**BIAOBEI_DEFAULTS, **(hp or {})}
        ext = hp.get("pitch_extractor", "parselmouth")
        if ext in ("harvest", "dio"):
            raise NotImplementedError(f"pitch_extractor = {ext!r} is pyworld's; only parselmouth's autocorrelation method runs on the device")
        if ext != "parselmouth":
            raise ValueError(f"pitch_extractor = {ext!r} (the reference knows parselmouth, harvest and dio)")
        return cls(ctx, sample_rate=hp["audio_sample_rate"], hop_size=hp["hop_size"], **kw)

    def frames(self, L):
        return n_frames_of(L, self.geo["first"], self.hop)

    def __call__(self, wavs, lens=None, stages=False):
        """wavs [B, L] float32 (anything else is converted), lens [B] or None (= L).  -> dict of device tensors: f0 f64 [B, nF] with
        nF = the frames of an L-sample utterance (0 behind n_frames, and for an utterance whose length is outside 1 .. L or too short for
        a frame), n_frames i32 [B]; with stages=True also acf f64 [B, nF, n_lag], cand f64 [B, nF, 15, 2], n_cand i32 [B, nF],
        intensity f64 [B, nF] (NaN / 0 behind n_frames) and selected i32 [B, nF] (-1 behind n_frames)."""
        wavs = torch.as_tensor(wavs)
        if wavs.dim() != 2:
            raise ValueError(f"wavs must be [B, L] (got {tuple(wavs.shape)})")
        B, L = wavs.shape
        if B < 1 or B > 65535:
            raise ValueError(f"B = {B} (supported: 1 .. 65535)")
        if not 1 <= L <= 1 << 26:
            raise ValueError(f"L = {L} samples (supported: 1 .. {1 << 26})")
        nF = self.frames(L)
        if nF > abi.PITCH_MAX_FRAMES:
            raise ValueError(f"L = {L} samples give {nF} frames (supported: up to {abi.PITCH_MAX_FRAMES})")
        if lens is not None:
            lens = torch.as_tensor(lens).reshape(-1)
            if lens.shape[0] != B:
                raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
        ctx = self._context()
        dev = self.device
        wd = wavs.to(device=dev, dtype=torch.float32).contiguous()
        ld = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
        ldf = max(nF, 1)
        out = {"f0": torch.empty(B, ldf, dtype=torch.float64, device=dev), "n_frames": torch.empty(B, dtype=torch.int32, device=dev)}
        if stages:
            nan = float("nan")
            out["acf"] = torch.full((B, ldf, self.geo["n_lag"]), nan, dtype=torch.float64, device=dev)
            out["cand"] = torch.full((B, ldf, abi.PITCH_CANDIDATES, 2), nan, dtype=torch.float64, device=dev)
            out["n_cand"] = torch.zeros(B, ldf, dtype=torch.int32, device=dev)
            out["intensity"] = torch.full((B, ldf), nan, dtype=torch.float64, device=dev)
            out["selected"] = torch.empty(B, ldf, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        ctx.pitch(B, torch.cuda.current_stream().cuda_stream, wav=wd.data_ptr(), wav_ld=L, frames_ld=ldf, f0=out["f0"].data_ptr(),
                  n_frames=out["n_frames"].data_ptr(), sample_rate=self.sample_rate, hop=self.hop, pitch_floor=self.f0_min, pitch_ceiling=self.f0_max,
                  lens=ptr(ld), acf=ptr(out.get("acf")), cand=ptr(out.get("cand")), n_cand=ptr(out.get("n_cand")), intensity=ptr(out.get("intensity")),
                  selected=ptr(out.get("selected")), **self.params)
        if ldf != nF:
            out = {k: (v if k == "n_frames" else v[:, :nF]) for k, v in out.items()}
        return out


def align_to_mel(f0, n_frames, n_mel, lpad=None, lens=None, hop=256):
    """Tracker frames -> mel frames: f0 [B, nF] (tensor or array), n_frames [B] -> [B, n_mel] of the same kind, zeros where no tracker
    frame lands.  Default (lpad=None): frame k goes to the mel frame nearest to its centre c_k = (L - n hop + hop - 1) / 2 + k hop samples,
    i.e. k + floor(c_0 / hop + 1 / 2) — a shift of 2 for an utterance of a whole number of hops, which is also what is used when
    lens is None.  lpad=4 / 8: the reference's get_pitch shift (np.pad by lpad on the left); where its right pad would be negative the track
    is truncated as its f0[:len(mel)] would, not refused."""
    is_np = not torch.is_tensor(f0)
    f = torch.as_tensor(f0)
    if f.dim() != 2:
        raise ValueError(f"f0 must be [B, nF] (got {tuple(f.shape)})")
    n = torch.as_tensor(n_frames).reshape(-1).to("cpu", torch.int64)
    B, nF = f.shape
    if n.shape[0] != B:
        raise ValueError(f"n_frames has {n.shape[0]} entries for a batch of {B}")
    n_mel = int(n_mel)
    if n_mel < 0:
        raise ValueError(f"n_mel = {n_mel}")
    if lpad is not None and (int(lpad) != lpad or lpad < 0):
        raise ValueError(f"lpad = {lpad!r} (None, or an integer >= 0)")
    if lens is not None:
        lens = torch.as_tensor(lens).reshape(-1).to("cpu", torch.int64)
        if lens.shape[0] != B:
            raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
    out = torch.zeros(B, n_mel, dtype=f.dtype, device=f.device)
    for b in range(B):
        nb = min(int(n[b]), nF)
        if lpad is not None:
            shift = int(lpad)
        elif lens is None:
            shift = 2
        else:
            shift = (int(lens[b]) - nb * hop + hop - 1 + hop) // (2 * hop)
        m = max(0, min(nb, n_mel - shift))
        if m:
            out[b, shift:shift + m] = f[b, :m]
    return out.numpy() if is_np else out


_EXTRACTORS = {}


def get_pitch(wav_data, mel, hparams, ctx=None):
    """data_gen_utils.py::get_pitch for one utterance: wav [L], mel [T, n_mel] (only its length is used), hparams -> (f0 float64 [T],
    pitch_coarse int64 [T]) as numpy arrays.  The track is shifted by the reference's lpad (4 frames at hop 256, 8 at hop 128) and cut or
    zero-padded to len(mel).  An utterance too short for one analysis frame raises ValueError, as Praat does."""
    from .hparams import BIAOBEI_DEFAULTS
    hp = {**BIAOBEI_DEFAULTS, **(hparams or {})}
    key = (int(hp["audio_sample_rate"]), int(hp["hop_size"]), hp.get("pitch_extractor", "parselmouth"), id(ctx))
    if key not in _EXTRACTORS:
        _EXTRACTORS[key] = PitchAC.from_hparams(hp, ctx)
    ex = _EXTRACTORS[key]
    if ex.hop not in REFERENCE_LPAD:
        raise ValueError(f"hop_size = {ex.hop}: the reference's get_pitch knows the padding of hop 128 and 256 only")
    wav = np.asarray(wav_data)
    if wav.ndim != 1:
        raise ValueError(f"wav_data must be one utterance [L] (got shape {wav.shape})")
    if ex.frames(wav.shape[0]) < 1:
        raise ValueError(f"{wav.shape[0]} samples are too short for one analysis frame ({ex.geo['first']} samples at f0_min = {ex.f0_min} Hz)")
    out = ex(torch.from_numpy(np.ascontiguousarray(wav, np.float32))[None])
    f0 = align_to_mel(out["f0"].cpu().numpy(), out["n_frames"].cpu().numpy(), len(mel), lpad=REFERENCE_LPAD[ex.hop])[0]
    return f0, f0_to_coarse(f0)


def pitch_dtw_from_wavs(wav_pred, pred_lens, wav_gt, gt_lens, ctx=None, **kw):
    """What ``scripts/pitch_dtw.py`` prints, from the waveforms themselves: wav_pred [B, L1] against wav_gt [B, L2] with their lengths (or
    None).  Both F0 tracks are made on the device and go to the DTW as they are (float64, with n_frames as the lengths): nothing returns to
    the host in between.  Keywords: those of ``PitchAC``.  -> what ``dtw.pitch_dtw`` returns."""
    ex = PitchAC(ctx, **kw)
    wav_pred, wav_gt = torch.as_tensor(wav_pred), torch.as_tensor(wav_gt)
    if wav_pred.dim() != 2 or wav_gt.dim() != 2 or wav_pred.shape[0] != wav_gt.shape[0]:
        raise ValueError(f"wav_pred and wav_gt must be [B, L] with one B (got {tuple(wav_pred.shape)} and {tuple(wav_gt.shape)})")
    for name, w in (("wav_pred", wav_pred), ("wav_gt", wav_gt)):
        if ex.frames(w.shape[1]) < 1:
            raise ValueError(f"{name}: {w.shape[1]} samples are too short for one analysis frame ({ex.geo['first']} samples)")
    p, g = ex(wav_pred, pred_lens), ex(wav_gt, gt_lens)
    out = _dtw.DTW(ex.ctx)(p["f0"], g["f0"], p["n_frames"], g["n_frames"], path=False, moments=True)
    dist = out["dist"].cpu().numpy() / g["n_frames"].cpu().numpy().astype(np.float64)
    mom = out["moments"][:, 0].cpu().numpy()
    res = {"dtw": float(dist.mean()), "std": float(mom[:, 1].mean()), "skew": float(mom[:, 2].mean()), "kurtosis": float(mom[:, 3].mean())}
    res.update(dtw_list=dist.tolist(), std_list=mom[:, 1].tolist(), skew_list=mom[:, 2].tolist(), kurtosis_list=mom[:, 3].tolist())
    return res
