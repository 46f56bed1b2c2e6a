"""STFT, inverse STFT and the spectral-subtraction filter between them on the device: the reference's one post-filter on the vocoder's
output, ``denoise(wav, v)`` (vocoders/vocoder_utils.py:7-15, imported by vocoders/hifigan.py:13; strength key ``vocoder_denoise_c``,
egs/egs_bases/tts/base.yaml:112), and the ``_stft`` / ``_istft`` pair Griffin-Lim is built on (utils/audio.py:35-42).  The filter takes
librosa's STFT of the waveform (fft_size, hop_size, win_size of the hparams, periodic Hann, center=True with constant padding), subtracts v
from every magnitude and clips at zero, keeps the phase, and returns librosa's inverse STFT of the result.  Here all of it is run by the
kernels of dict_tts_amd/csrc/istft.hip (``abi.PART_ISTFT`` / ``abi.OUT_SPECTRAL``) — no librosa, no ``torch.stft``, nothing leaves the
device.  The periodic Hann window is restated here, zero padded and centred to fft_size as both transforms apply it.

Griffin-Lim itself (``griffin_lim`` / ``griffin_lim_torch``, utils/audio.py:35-42, 136-158, with ``_mel_to_linear``, 91-95) is
``Spectral.griffin_lim``: the same two transforms with the projection onto the target magnitudes between them, run by
dict_tts_amd/csrc/griffinlim.hip (``abi.OUT_GRIFFIN_LIM``).
"""
import math

import numpy as np
import torch

from . import abi
from .hparams import BIAOBEI_DEFAULTS
from .unit import DeviceUnit

ENVELOPE_MIN = 1e-11   # torch.istft's criterion on the window envelope (librosa divides where it exceeds the smallest float instead)


def centred_hann(fft_size, win_length):
    """scipy.signal.get_window('hann', win_length, fftbins=True) — the PERIODIC Hann window librosa.stft / librosa.istft build — zero padded
    to fft_size with (fft_size - win_length) // 2 zeros on the left: float32 [fft_size], what "istft.window" takes"""
    if not 1 <= win_length <= fft_size:
        raise ValueError(f"win_size = {win_length} (supported: 1 .. fft_size = {fft_size})")
    w = np.zeros(fft_size, np.float32)
    left = (fft_size - win_length) // 2
    w[left:left + win_length] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)).astype(np.float32)
    return w


def envelope_min(window, hop):
    """the smallest value of the window envelope sum_t w^2[n - t hop] at any kept sample of any signal, float64: that of a two-frame signal,
    min over p in [N / 2, N / 2 + hop) of w^2[p] (p < N) + w^2[p - hop] (p >= hop) — a longer signal only adds non-negative terms.  The
    library computes the same figure and refuses the inverse where it is not above ENVELOPE_MIN."""
    w2 = np.asarray(window, np.float64) ** 2
    N, hop = len(w2), int(hop)
    p = np.arange(N // 2, N // 2 + hop)
    return float(np.min(np.where(p < N, w2[np.minimum(p, N - 1)], 0.0) + np.where(p >= hop, w2[np.maximum(p - hop, 0)], 0.0)))


def inverse_mel_basis(hp, n_fft):
    """``np.linalg.pinv(_build_mel_basis(hparams))`` of ``_mel_to_linear`` (utils/audio.py:91-101): the pseudo-inverse of the float32 mel
    filterbank (``melspec.mel_filterbank``, librosa's dtype), computed in float64 and rounded once: float32 [n_fft // 2 + 1, n_mels], what
    "istft.inv_mel_basis" takes.  hp: audio_num_mel_bins, fmin, fmax, audio_sample_rate."""
    from .melspec import mel_filterbank
    missing = [k for k in ("audio_num_mel_bins", "fmin", "fmax", "audio_sample_rate") if hp.get(k) is None]
    if missing:
        raise ValueError(f"mel input needs the hparams {', '.join(missing)}")
    sr, n_mels = int(hp["audio_sample_rate"]), int(hp["audio_num_mel_bins"])
    if not 1 <= n_mels <= 128:
        raise ValueError(f"audio_num_mel_bins = {n_mels} (supported: 1 .. 128)")
    if hp["fmax"] != -1 and hp["fmax"] > sr // 2:   # utils/audio.py:99
        raise ValueError(f"fmax = {hp['fmax']} exceeds audio_sample_rate // 2 = {sr // 2}")
    basis = mel_filterbank(sr, n_fft, n_mels, hp["fmin"], hp["fmax"]).astype(np.float32)
    return np.ascontiguousarray(np.linalg.pinv(basis.astype(np.float64)).astype(np.float32))


class Spectral(DeviceUnit):
    """``stft`` / ``istft`` / ``denoise`` / ``griffin_lim`` of batches of waveforms with one plan (fft_size, hop_size, win_size).

    hp: the reference's hparams keys fft_size, hop_size, win_size (egs/egs_bases/tts/base.yaml:48-54; Biaobei's by default), fft_size 512 /
    1024 / 2048, any hop in 1 .. fft_size whose window envelope stays above 1e-11 (``envelope_min``), any win_size <= fft_size.  ctx: an
    existing ``abi.Context`` to load the plan into (e.g. the vocoder's), or None for one of its own; it is created on the first call, so
    that argument errors surface without a GPU.  All three methods take and return cuda tensors and enqueue on the current stream."""

    def __init__(self, hp=None, ctx=None):
        hp = {**BIAOBEI_DEFAULTS, **(hp or {})}
        self.n_fft, self.hop, self.win = int(hp["fft_size"]), int(hp["hop_size"]), int(hp["win_size"] or hp["fft_size"])
        if self.n_fft not in (512, 1024, 2048):
            raise ValueError(f"fft_size = {self.n_fft} (supported: 512, 1024, 2048)")
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"hop_size = {self.hop} (supported: 1 .. fft_size = {self.n_fft})")
        self.window = centred_hann(self.n_fft, self.win)
        self.envelope_min = envelope_min(self.window, self.hop)
        if not self.envelope_min > ENVELOPE_MIN:
            raise ValueError(f"hop_size = {self.hop}: the window's envelope falls to {self.envelope_min:g} at a kept sample (must stay above "
                             f"{ENVELOPE_MIN:g}): the inverse STFT would divide by it")
        self.n_bins = self.n_fft // 2 + 1
        self.ctx = ctx
        self._mel_hp = {k: hp.get(k) for k in ("audio_num_mel_bins", "fmin", "fmax", "audio_sample_rate")}
        self.inv_mel_basis = None   # built by the first griffin_lim(mel=...), then part of the plan
        self._plan_has_inv = False

    def _plan(self, mel=False):
        """A context holds ONE plan (the window of the last finalise).  The context remembers which object's plan that is, so that several
        ``Spectral`` objects — other configurations, or the vocoder's own — can share a context: whoever is called after another finalises
        again (a host-side repack and upload of the two bases; launches in flight keep the packs they were given).  mel: the plan must
        carry the inverse mel basis too (``griffin_lim(mel=...)``); it is computed once and loaded with every later finalise of this object."""
        if mel and self.inv_mel_basis is None:
            self.inv_mel_basis = inverse_mel_basis(self._mel_hp, self.n_fft)
        if self.ctx is not None and getattr(self.ctx, "_istft_plan_of", None) is self and (self._plan_has_inv or not mel):
            return
        self._device()   # (no PART: which plan the context holds is decided here, call by call)
        self.ctx._istft_plan_of = None   # (a refused finalise leaves no plan behind)
        state = {"window": self.window}
        if self.inv_mel_basis is not None:
            state["inv_mel_basis"] = self.inv_mel_basis
        self.ctx.load_state_dict("istft", state)
        self.ctx.finalize(abi.PART_ISTFT)
        self.ctx._istft_plan_of = self
        self._plan_has_inv = self.inv_mel_basis is not None

    def frames(self, n_samples):
        return 1 + int(n_samples) // self.hop

    @staticmethod
    def _wav(wav):
        if not (torch.is_tensor(wav) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("wav must be a float32 cuda tensor [B, L] (or [L])")
        wav = wav.unsqueeze(0) if wav.dim() == 1 else wav
        if wav.shape[0] < 1:
            raise ValueError("B = 0")
        return wav.contiguous()

    @staticmethod
    def _lens(lens, B, device):
        if lens is None:
            return None
        lens = torch.as_tensor(lens).to(device=device, dtype=torch.int32).contiguous()
        if tuple(lens.shape) != (B,):
            raise ValueError(f"lens of shape {tuple(lens.shape)}, the batch has {B} utterances")
        return lens

    def stft(self, wav, lens=None):
        """wav [B, L] float32 cuda tensor, lens [B] valid samples or None = L for all -> (spec complex64 [B, 1 + L // hop, fft_size // 2 + 1],
        frames int32 [B]): ``torch.stft(wav[b, :lens[b]], center=True, pad_mode='constant', return_complex=True)`` transposed to [T, bins];
        rows >= frames[b] are zero."""
        wav = self._wav(wav)
        B, L = wav.shape
        lens = self._lens(lens, B, wav.device)
        self._plan()
        T = self.frames(L)
        spec = torch.zeros(B, T, self.n_bins, dtype=torch.complex64, device=wav.device)
        frames = torch.empty(B, dtype=torch.int32, device=wav.device)
        self.ctx.spectral(abi.SPECTRAL_FORWARD, B, L, self.hop, T, torch.cuda.current_stream().cuda_stream, wav=wav.data_ptr(),
                          lens=lens.data_ptr() if lens is not None else None, frames=frames.data_ptr(), spec=torch.view_as_real(spec).data_ptr())
        return spec, frames

    def istft(self, spec, frames=None):
        """spec [B, T, fft_size // 2 + 1] complex64 cuda tensor (any spectrum, consistent or not; the imaginary parts of bins 0 and
        fft_size / 2 are ignored), frames [B] rows per utterance or None = T for all -> (wav float32 [B, hop (T - 1)], out_lens int32 [B]):
        ``torch.istft(spec[b, :frames[b]].T, center=True)``; samples >= out_lens[b] = hop (frames[b] - 1) are zero."""
        if not (torch.is_tensor(spec) and spec.is_cuda and spec.dtype == torch.complex64 and spec.dim() in (2, 3)):
            raise ValueError("spec must be a complex64 cuda tensor [B, T, bins] (or [T, bins])")
        spec = spec.unsqueeze(0) if spec.dim() == 2 else spec
        B, T, bins = spec.shape
        if bins != self.n_bins:
            raise ValueError(f"spec of {bins} bins, fft_size = {self.n_fft} gives {self.n_bins}")
        if B < 1 or T < 1:
            raise ValueError(f"spec of shape {tuple(spec.shape)}: at least one utterance of one frame")
        spec = spec.contiguous()
        frames = torch.full((B,), T, dtype=torch.int32, device=spec.device) if frames is None else self._lens(frames, B, spec.device)
        self._plan()
        L = self.hop * (T - 1)
        out = torch.zeros(B, L, dtype=torch.float32, device=spec.device)
        out_lens = torch.empty(B, dtype=torch.int32, device=spec.device)
        self.ctx.spectral(abi.SPECTRAL_INVERSE, B, L, self.hop, T, torch.cuda.current_stream().cuda_stream, frames=frames.data_ptr(),
                          spec=torch.view_as_real(spec).data_ptr(), out=out.data_ptr(), out_lens=out_lens.data_ptr())
        return out, out_lens

    def denoise(self, wav, lens=None, v=0.1):
        """the reference's ``denoise(wav[b, :lens[b]], v)`` for every utterance: wav [B, L] float32 cuda tensor, lens [B] valid samples or
        None -> (wav float32 [B, L], out_lens int32 [B]), out_lens[b] = hop (lens[b] // hop) (the inverse returns whole hops); samples past
        it are zero.  v = 0 is the plain round trip.  The spectrum stays in the context's workspace."""
        v = float(v)
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"v = {v} (must be finite and not negative)")
        wav = self._wav(wav)
        B, L = wav.shape
        lens = self._lens(lens, B, wav.device)
        self._plan()
        out = torch.zeros_like(wav)
        out_lens = torch.empty(B, dtype=torch.int32, device=wav.device)
        self.ctx.spectral(abi.SPECTRAL_FORWARD | abi.SPECTRAL_INVERSE, B, L, self.hop, self.frames(L), torch.cuda.current_stream().cuda_stream,
                          wav=wav.data_ptr(), lens=lens.data_ptr() if lens is not None else None, out=out.data_ptr(),
                          out_lens=out_lens.data_ptr(), floor=v)
        return out, out_lens

    def griffin_lim(self, mag=None, mel=None, frames=None, n_iter=60, init=None, return_spec=False):
        """the reference's ``griffin_lim`` / ``griffin_lim_torch`` (utils/audio.py:35-42, 136-158) for a batch, every transform of it this
        object's ``stft`` / ``istft``: mag [B, T, fft_size // 2 + 1] float32 cuda tensor of target magnitudes, OR mel [B, T, n_mels] float32
        cuda tensor of the project's log10-mels, turned into magnitudes as ``_mel_to_linear(10 ** mel)`` does (utils/audio.py:91-95;
        mel parameters from the hparams); frames [B] rows per utterance or None = T for all; n_iter >= 0 projections (the reference's
        griffin_lim_iters is 60); init [B, T, bins] complex64 cuda tensor, the start's factor on the magnitudes, or None = a random phase
        ``torch.polar(1, 2 pi torch.rand(B, T, bins))`` drawn on the device (``torch.manual_seed`` repeats a run)
        -> (wav float32 [B, hop (T - 1)], out_lens int32 [B] = hop (frames - 1)), samples past out_lens[b] zero; return_spec: also the
        spectrum [B, T, bins] complex64 the waveform was inverted from (rows >= frames[b] zero)."""
        if (mag is None) == (mel is None):
            raise ValueError("griffin_lim takes exactly one of mag= and mel=")
        n_iter = int(n_iter)
        if n_iter < 0:
            raise ValueError(f"n_iter = {n_iter} (must not be negative)")
        src, what, width = (mag, "mag", self.n_bins) if mel is None else (mel, "mel", int(self._mel_hp["audio_num_mel_bins"] or 0))
        if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.float32 and src.dim() in (2, 3)):
            raise ValueError(f"{what} must be a float32 cuda tensor [B, T, {width}] (or [T, {width}])")
        src = (src.unsqueeze(0) if src.dim() == 2 else src).contiguous()
        B, T, cols = src.shape
        if cols != width:
            raise ValueError(f"{what} of {cols} columns, " + (f"fft_size = {self.n_fft} gives {width}" if mel is None else f"audio_num_mel_bins = {width}"))
        if B < 1 or T < 1:
            raise ValueError(f"{what} of shape {tuple(src.shape)}: at least one utterance of one frame")
        if init is not None:
            if not (torch.is_tensor(init) and init.is_cuda and init.dtype == torch.complex64 and tuple(init.shape[-2:]) == (T, self.n_bins)
                    and init.numel() == B * T * self.n_bins):
                raise ValueError(f"init must be a complex64 cuda tensor {(B, T, self.n_bins)}")
            init = init.reshape(B, T, self.n_bins).contiguous()
        frames = None if frames is None else self._lens(frames, B, src.device)
        self._plan(mel=mel is not None)
        if init is None:
            init = torch.polar(torch.ones(B, T, self.n_bins, device=src.device), 2.0 * math.pi * torch.rand(B, T, self.n_bins, device=src.device))
        L = self.hop * (T - 1)
        out = torch.zeros(B, L, dtype=torch.float32, device=src.device)
        out_lens = torch.empty(B, dtype=torch.int32, device=src.device)
        spec = torch.zeros(B, T, self.n_bins, dtype=torch.complex64, device=src.device) if return_spec else None
        self.ctx.griffin_lim(B, T, self.hop, n_iter, L, out.data_ptr(), torch.cuda.current_stream().cuda_stream,
                             mag=src.data_ptr() if mel is None else None, mel=src.data_ptr() if mel is not None else None,
                             n_mels=cols if mel is not None else 0, init=torch.view_as_real(init).data_ptr(),
                             frames=frames.data_ptr() if frames is not None else None, out_lens=out_lens.data_ptr(),
                             spec_out=torch.view_as_real(spec).data_ptr() if return_spec else None)
        return (out, out_lens, spec) if return_spec else (out, out_lens)
