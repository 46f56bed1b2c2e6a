"""Log-mel spectrograms on the device: the reference's ``BaseVocoder.wav2spec`` direction (vocoders/base_vocoder.py:36-53 ->
``process_utterance``, data_gen/tts/data_gen_utils.py:93-147 with vocoder='pwg', loud_norm=False, trim_long_sil=False).

``mel_filterbank`` / ``hann_window`` restate what librosa computes there (no librosa at inference time); ``MelSpectrogram`` loads them
into a context (``abi.PART_MELSPEC``) and runs the fused kernel (dict_tts_amd/csrc/melspec.hip) on a batch of waveforms.
"""
import numpy as np
import torch

from . import abi
from .hparams import BIAOBEI_DEFAULTS
from .unit import DeviceUnit

EPS = 1e-6   # process_utterance(eps=1e-6)


def _hz_to_mel(f):
    """librosa.core.hz_to_mel(htk=False): the Slaney scale — linear below 1 kHz, logarithmic above"""
    f = np.asarray(f, np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """``librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)`` as data_gen_utils.py:128-130 calls it (htk=False, norm='slaney'), in
    float64: [n_mels, n_fft // 2 + 1].  fmin = -1 -> 0, fmax = -1 -> sr / 2, as process_utterance resolves them."""
    fmin = 0 if fmin == -1 else fmin
    fmax = sr / 2 if fmax == -1 else fmax
    fftfreqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]   # norm='slaney': unit area per triangle
    return weights


def hann_window(win_length):
    """scipy.signal.get_window('hann', win_length, fftbins=True): the PERIODIC Hann window librosa.stft builds"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)


def read_wav(path, sample_rate):
    """16-bit / 32-bit / float PCM wav -> float32 mono in [-1, 1).  Nothing here resamples: a file at another rate is refused."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if int(sr) != int(sample_rate):
        raise ValueError(f"{path}: sample rate {sr} Hz, but audio_sample_rate is {sample_rate} Hz (this front end does not resample; "
                         f"the reference's librosa.load would)")
    if data.dtype == np.int16:
        wav = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        wav = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.uint8:
        wav = (data.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(data.dtype, np.floating):
        wav = data.astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported sample format {data.dtype}")
    return wav.mean(axis=1).astype(np.float32) if wav.ndim == 2 else wav   # librosa.load(mono=True)


class MelSpectrogram(DeviceUnit):
    """wav [B, L] -> (log10-mel [B, T, n_mels], frames [B]) with T = 1 + L // hop, one launch per batch, nothing leaves the device.

    hparams keys (the reference's, egs/egs_bases/tts/base.yaml:48-54): fft_size, hop_size, win_size, audio_num_mel_bins, fmin, fmax,
    audio_sample_rate.  ctx: an existing ``abi.Context`` to load the plan into (e.g. the vocoder's), or None for one of its own."""

    PREFIX, PART = "melspec", abi.PART_MELSPEC

    def __init__(self, hparams=None, ctx=None):
        hp = {**BIAOBEI_DEFAULTS, **(hparams or {})}
        self.n_fft, self.hop, self.win = int(hp["fft_size"]), int(hp["hop_size"]), int(hp["win_size"] or hp["fft_size"])
        self.n_mels, self.sample_rate = int(hp["audio_num_mel_bins"]), int(hp["audio_sample_rate"])
        self.fmin, self.fmax = hp["fmin"], hp["fmax"]
        self.ctx = ctx
        self._device()   # (refuses before anything is computed; this unit loads its plan at construction)
        self.mel_basis = mel_filterbank(self.sample_rate, self.n_fft, self.n_mels, self.fmin, self.fmax).astype(np.float32)   # (librosa's dtype)
        self.window = hann_window(self.win).astype(np.float32)
        self._context()

    def _state(self):
        return {"mel_basis": self.mel_basis, "window": self.window}

    def frames(self, n_samples):
        return 1 + int(n_samples) // self.hop

    def __call__(self, wav, lens=None, linear=False):
        """wav: [B, L] (or [L]) float32 tensor / array, host or device; lens: [B] valid samples per utterance or None = L for all.
        -> (mel [B, 1 + L // hop, n_mels] float32 cuda tensor, mel_lens [B] int32 cuda tensor).  Rows >= mel_lens[b] are zero.
        linear=True: a third tensor like mel, the mel values before max(eps, .) and the logarithm."""
        wav = torch.as_tensor(wav, dtype=torch.float32)
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        assert wav.dim() == 2, "wav must be [B, L]"
        wav = wav.to(self.device).contiguous()
        B, L = wav.shape
        if lens is not None:
            lens = torch.as_tensor(lens).to(device=self.device, dtype=torch.int32).contiguous()
        T = self.frames(L)
        mel = torch.zeros(B, T, self.n_mels, dtype=torch.float32, device=self.device)
        mel_lens = torch.empty(B, dtype=torch.int32, device=self.device)
        lin = torch.zeros_like(mel) if linear else None
        self.ctx.melspec(wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, L, self.hop, mel.data_ptr(), T, mel_lens.data_ptr(),
                         torch.cuda.current_stream().cuda_stream, eps=EPS, lin=lin.data_ptr() if linear else None)
        return (mel, mel_lens, lin) if linear else (mel, mel_lens)
