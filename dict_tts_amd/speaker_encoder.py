"""Speaker embeddings on the device: the d-vector encoder behind the reference's ``spk_embed`` — Resemblyzer 0.1.1's ``VoiceEncoder``
(``data_gen/tts/base_binarizer.py:156-168`` calls ``VoiceEncoder().embed_utterance(wav)``), restated from its documented behaviour and run by
dict_tts_amd/csrc/spkenc.hip (dtts_text2mel_fetch(DTTS_OUT_SPKENC)): a 40-band POWER mel at 16 kHz (n_fft 400, hop 160, periodic Hann,
centred frames, Slaney filterbank 0 .. 8000 Hz), partial utterances of 160 frames every ``round(16000 / rate / 160)`` frames, three LSTM
layers of 256 units, ``relu(linear(h_T))`` divided by its norm, the mean over the partials divided by its norm.

The arithmetic is specified in include/dicttts_hip.h and restated in float64 by tests/spkenc_ref.py.  Neither Resemblyzer, its
``pretrained.pt``, librosa nor webrtcvad was available: see INTEGRATION.md ("Known uncertainties of the speaker encoder").

The reference's binariser embeds the float16 waveform at ``audio_sample_rate`` (22050 Hz) AS IF it were 16 kHz and without
``preprocess_wav``; ``embed_utterance(wav)`` on that array reproduces it (it is what a shipped checkpoint was trained on).
``embed_utterance(preprocess_wav(wav, source_sr=22050))`` is the proper form.

A zero vector (every relu output dead) divides to NaN exactly as Resemblyzer's does; nothing hides it.
"""
import numpy as np
import torch

from . import abi, melspec
from .unit import DeviceUnit

SAMPLING_RATE = 16000
MEL_WINDOW_LENGTH, MEL_WINDOW_STEP, MEL_N_CHANNELS = 25, 10, 40
N_FFT, HOP = SAMPLING_RATE * MEL_WINDOW_LENGTH // 1000, SAMPLING_RATE * MEL_WINDOW_STEP // 1000   # 400, 160
PARTIALS_N_FRAMES = 160
HIDDEN, EMBED, LAYERS = 256, 256, 3
AUDIO_NORM_TARGET_DBFS = -30
INT16_MAX = (2 ** 15) - 1
PAD_MODES = {"constant": abi.SPKENC_PAD_CONSTANT, "reflect": abi.SPKENC_PAD_REFLECT}


def state_dict_shapes():
    """the VoiceEncoder's state-dict keys and their shapes"""
    sh = {}
    for k in range(LAYERS):
        sh[f"lstm.weight_ih_l{k}"] = (4 * HIDDEN, MEL_N_CHANNELS if k == 0 else HIDDEN)
        sh[f"lstm.weight_hh_l{k}"] = (4 * HIDDEN, HIDDEN)
        sh[f"lstm.bias_ih_l{k}"] = (4 * HIDDEN,)
        sh[f"lstm.bias_hh_l{k}"] = (4 * HIDDEN,)
    sh["linear.weight"] = (EMBED, HIDDEN)
    sh["linear.bias"] = (EMBED,)
    return sh


def model_state_of(path_or_state):
    """a checkpoint path, a loaded ``{"model_state": ...}`` checkpoint or the state dict itself -> the state dict"""
    st = path_or_state
    if isinstance(st, (str, bytes)) or hasattr(st, "__fspath__"):
        st = torch.load(st, map_location="cpu", weights_only=False)
    if "model_state" in st:
        st = st["model_state"]
    return st


def check_state_dict(state):
    """-> {key: float32 array} of exactly the encoder's tensors; a missing key (KeyError) or another shape (ValueError) is refused by name"""
    out = {}
    for k, shape in state_dict_shapes().items():
        if k not in state:
            raise KeyError(f"the speaker encoder's state dict lacks {k}")
        v = state[k]
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if tuple(a.shape) != shape:
            raise ValueError(f"{k} is {list(a.shape)}; the encoder's is {list(shape)} (nn.LSTM(40, 256, 3), nn.Linear(256, 256))")
        out[k] = np.ascontiguousarray(a, np.float32)
    return out


def frame_step_of(rate):
    """frames between partials: Resemblyzer's int(np.round((sampling_rate / rate) / samples_per_frame))"""
    if not 0 < rate:
        raise ValueError(f"rate = {rate!r} (partials per second, > 0)")
    samples_per_frame = int(SAMPLING_RATE * MEL_WINDOW_STEP / 1000)
    step = int(np.round((SAMPLING_RATE / rate) / samples_per_frame))
    if not 0 < step <= PARTIALS_N_FRAMES:
        raise ValueError(f"rate = {rate!r} gives a step of {step} frames (must lie in 1 .. {PARTIALS_N_FRAMES})")
    return step


def normalize_volume(wav, target_dBFS=AUDIO_NORM_TARGET_DBFS, increase_only=False, decrease_only=False):
    """Resemblyzer's normalize_volume: the level is that of wav * 32767, dBFS = 20 log10(rms / 32767); the gain 10^((target - dBFS) / 20) is
    applied unless it would move the level the excluded way"""
    if increase_only and decrease_only:
        raise ValueError("Both increase only and decrease only are set")
    wav = np.asarray(wav)
    rms = np.sqrt(np.mean((wav.astype(np.float64) * INT16_MAX) ** 2))
    wave_dBFS = 20 * np.log10(rms / INT16_MAX)
    dBFS_change = target_dBFS - wave_dBFS
    if dBFS_change < 0 and increase_only or dBFS_change > 0 and decrease_only:
        return wav
    return wav * (10 ** (dBFS_change / 20))


def preprocess_wav(wav, source_sr=None, trim=False, ctx=None):
    """Resemblyzer's preprocess_wav without its VAD: resample to 16 kHz on the device (wavprep.Resampler, librosa's kaiser_best), then
    normalize_volume(wav, -30, increase_only=True).  -> float32 numpy.  trim=True (trim_long_silences) needs webrtcvad and is not
    implemented, the same gap as ``trim_long_sil`` of the waveform conditioning."""
    if trim:
        raise NotImplementedError("preprocess_wav(trim=True): Resemblyzer's trim_long_silences needs webrtcvad, which is not implemented "
                                  "(the same gap as trim_long_sil); pass trim=False")
    wav = np.asarray(wav, np.float32).reshape(-1)
    if source_sr is not None and int(source_sr) != SAMPLING_RATE:
        from . import wavprep
        out, out_lens = wavprep.Resampler(int(source_sr), SAMPLING_RATE, ctx=ctx)(torch.from_numpy(wav)[None])
        wav = out[0, :int(out_lens[0])].cpu().numpy()
    return np.asarray(normalize_volume(wav, AUDIO_NORM_TARGET_DBFS, increase_only=True), np.float32)


def similarity(a, b):
    """cosine similarity of two embedding batches [N, 256] (or [256]) on their device: sum a b / (|a| |b|), float32 -> [N]"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.is_cuda != b.is_cuda:
        a, b = (a.to(b.device), b) if b.is_cuda else (a, b.to(a.device))
    a, b = a.to(torch.float32), b.to(torch.float32)
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


class VoiceEncoder(DeviceUnit):
    """``VoiceEncoder.from_checkpoint("pretrained.pt").embed_utterance(wav)``: Resemblyzer's interface on the device.

    ctx: an existing ``abi.Context`` or None for one of its own; it is created, and the weights loaded, on the first device call, so that
    argument errors surface without a GPU.  pad_mode: how the mel's centred frames see beyond the waveform's ends — 'constant' (zeros;
    librosa 0.9.2, the version the reference pins) or 'reflect' (librosa <= 0.8)."""

    PREFIX, PART = "spkenc", abi.PART_SPKENC

    def __init__(self, ctx=None, pad_mode="constant"):
        if pad_mode not in PAD_MODES:
            raise ValueError(f"pad_mode = {pad_mode!r} (known: 'constant', 'reflect')")
        self.ctx = ctx
        self.pad_mode = pad_mode
        self.weights = None

    # ---- weights
    def load_state_dict(self, state):
        if self._loaded:
            raise abi.DttsError("VoiceEncoder.load_state_dict: this encoder's weights are already on the device (a context builds the part once)")
        self.weights = check_state_dict(model_state_of(state))
        return self

    @classmethod
    def from_checkpoint(cls, path_or_state, ctx=None, pad_mode="constant"):
        """Resemblyzer's ``pretrained.pt`` (path or loaded: ``{"model_state": state_dict, ...}``) or the state dict itself"""
        return cls(ctx=ctx, pad_mode=pad_mode).load_state_dict(path_or_state)

    def _state(self):
        if self.weights is None:
            raise abi.DttsError("VoiceEncoder: no weights (load_state_dict / from_checkpoint first)")
        w = dict(self.weights)
        w["mel_basis"] = melspec.mel_filterbank(SAMPLING_RATE, N_FFT, MEL_N_CHANNELS, 0, SAMPLING_RATE // 2).astype(np.float32)
        w["window"] = melspec.hann_window(N_FFT).astype(np.float32)
        return w

    # ---- host arithmetic
    @staticmethod
    def compute_partial_slices(n_samples, rate=1.3, min_coverage=0.75):
        """Resemblyzer's compute_partial_slices in exact integer arithmetic -> (wav_slices, mel_slices): lists of ``slice``"""
        if not 0 < min_coverage <= 1:
            raise ValueError(f"min_coverage = {min_coverage!r} (must lie in (0, 1])")
        n_samples = int(n_samples)
        frame_step = frame_step_of(rate)
        n_frames = -(-(n_samples + 1) // HOP)
        steps = max(1, n_frames - PARTIALS_N_FRAMES + frame_step + 1)
        wav_slices, mel_slices = [], []
        for i in range(0, steps, frame_step):
            mel_slices.append(slice(i, i + PARTIALS_N_FRAMES))
            wav_slices.append(slice(i * HOP, (i + PARTIALS_N_FRAMES) * HOP))
        last = wav_slices[-1]
        coverage = (n_samples - last.start) / (last.stop - last.start)
        if coverage < min_coverage and len(mel_slices) > 1:
            mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
        return wav_slices, mel_slices

    # ---- device calls
    def _run(self, mode, x, wav_ld, lens, frame_step, min_coverage, stages, tile_m):
        ctx = self._context()
        dev = self.device
        B = x.shape[0]
        if mode == abi.SPKENC_FROM_WAV:
            P, F, T = abi.spkenc_max_partials(wav_ld, frame_step), abi.spkenc_frames_ld(wav_ld, frame_step), PARTIALS_N_FRAMES
        else:
            P, F, T = 1, wav_ld, wav_ld
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        out = {"embed": torch.empty(B, EMBED, dtype=torch.float32, device=dev), "n_partials": torch.empty(B, dtype=torch.int32, device=dev)}
        if stages or mode == abi.SPKENC_FROM_MELS:
            out["partials"] = nan(B, P, EMBED)
        if stages:
            if mode == abi.SPKENC_FROM_WAV:
                out["mel"] = nan(B, F, MEL_N_CHANNELS)
            out["hseq"] = [nan(B, P, T, HIDDEN) for _ in range(LAYERS)]
        ptr = lambda t: None if t is None else t.data_ptr()
        ctx.spkenc(B, torch.cuda.current_stream().cuda_stream, wav=x.data_ptr(), wav_ld=wav_ld, embed=out["embed"].data_ptr(),
                   n_partials=out["n_partials"].data_ptr(), mode=mode, frame_step=frame_step, min_coverage=min_coverage,
                   pad_mode=PAD_MODES[self.pad_mode], tile_m=tile_m, lens=ptr(lens), partials=ptr(out.get("partials")), mel=ptr(out.get("mel")),
                   hseq=[ptr(t) for t in out.get("hseq", (None, None, None))])
        return out

    def forward(self, mels, stages=False, tile_m=0):
        """mels [N, T, 40] -> unit embeddings [N, 256] float32 on the device (``VoiceEncoder.forward``).  stages=True -> a dict with
        ``partials`` [N, 1, 256] and ``hseq``: every layer's hidden sequence [N, 1, T, 256]"""
        mels = torch.as_tensor(mels)
        if mels.dim() != 3 or mels.shape[2] != MEL_N_CHANNELS:
            raise ValueError(f"mels must be [N, T, {MEL_N_CHANNELS}] (got {tuple(mels.shape)})")
        N, T = mels.shape[0], mels.shape[1]
        if not 1 <= N <= 65535:
            raise ValueError(f"N = {N} (supported: 1 .. 65535)")
        if not 1 <= T <= abi.SPKENC_MAX_T:
            raise ValueError(f"T = {T} frames (supported: 1 .. {abi.SPKENC_MAX_T})")
        self._context()
        x = mels.to(device=self.device, dtype=torch.float32).contiguous()
        out = self._run(abi.SPKENC_FROM_MELS, x, T, None, 1, 1.0, stages, tile_m)
        return out if stages else out["partials"][:, 0]

    __call__ = forward

    def _wav_batch(self, wavs, lens):
        wavs = torch.as_tensor(wavs)
        if wavs.dim() != 2:
            raise ValueError(f"wavs must be [B, L] (got {tuple(wavs.shape)})")
        B, L = wavs.shape
        if not 1 <= B <= 65535:
            raise ValueError(f"B = {B} (supported: 1 .. 65535)")
        if not 1 <= L <= 1 << 24:
            raise ValueError(f"L = {L} samples (supported: 1 .. {1 << 24})")
        if lens is not None:
            lens = torch.as_tensor(lens).reshape(-1)
            if lens.shape[0] != B:
                raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
            if not lens.is_cuda:
                for b, n in enumerate(lens.tolist()):
                    if not 0 <= n <= L:
                        raise ValueError(f"lens[{b}] = {n} samples for waveforms of {L}")
        self._context()
        wd = wavs.to(device=self.device, dtype=torch.float32).contiguous()
        ld = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
        return wd, ld, B, L

    def embed_batch(self, wavs, lens=None, rate=1.3, min_coverage=0.75, return_partials=False, stages=False, tile_m=0):
        """wavs [B, L] (taken as 16 kHz; float16 / float64 are converted), lens [B] valid samples or None (= L) -> dict of device tensors:
        ``embed`` f32 [B, 256], ``n_partials`` i32 [B]; with return_partials ``partials`` f32 [B, P, 256] (rows behind n_partials NaN); with
        stages also ``mel`` f32 [B, F, 40] (rows behind an utterance's frames NaN) and ``hseq``: three f32 [B, P, 160, 256].  No host
        synchronisation when lens is a device tensor (or None)."""
        if not 0 < min_coverage <= 1:
            raise ValueError(f"min_coverage = {min_coverage!r} (must lie in (0, 1])")
        frame_step = frame_step_of(rate)
        wd, ld, B, L = self._wav_batch(wavs, lens)
        return self._run(abi.SPKENC_FROM_WAV, wd, L, ld, frame_step, float(min_coverage), stages or return_partials, tile_m)

    def wav_to_mel_spectrogram(self, wavs, lens=None):
        """wavs [B, L], lens -> (mel f32 [B, F, 40] on the device, frames i32 [B]): the mel of every utterance zero padded to one partial
        (25600 samples) at least, as embed_utterance takes it; an utterance of at least 25600 samples has ``1 + len // 160`` frames, as
        Resemblyzer's wav_to_mel_spectrogram gives it"""
        wd, ld, B, L = self._wav_batch(wavs, lens)
        # partials 160 frames apart that must be covered in full never lengthen an utterance beyond one partial (the encoder runs on them too)
        out = self._run(abi.SPKENC_FROM_WAV, wd, L, ld, PARTIALS_N_FRAMES, 1.0, True, 0)
        n = torch.full((B,), L, dtype=torch.int32, device=self.device) if ld is None else ld
        return out["mel"], 1 + torch.clamp(n, min=PARTIALS_N_FRAMES * HOP) // HOP

    def embed_utterance(self, wav, return_partials=False, rate=1.3, min_coverage=0.75):
        """one waveform (1-D, taken as 16 kHz) -> its embedding float32 [256] as numpy; return_partials -> (embed, partial_embeds
        [n, 256], wav_slices), as Resemblyzer returns them"""
        wav = np.asarray(wav).reshape(-1)
        n = len(wav)
        x = torch.from_numpy(np.ascontiguousarray(wav if n else np.zeros(1, wav.dtype)))[None]
        out = self.embed_batch(x, [n], rate, min_coverage, return_partials=return_partials)
        embed = out["embed"][0].cpu().numpy()
        if not return_partials:
            return embed
        k = int(out["n_partials"][0])
        return embed, out["partials"][0, :k].cpu().numpy(), self.compute_partial_slices(n, rate, min_coverage)[0]

    def embed_speaker(self, wavs, **kwargs):
        """several utterances of one speaker -> the mean of their embeddings, normalised (float32 [256] numpy)"""
        raw = np.mean([self.embed_utterance(w, return_partials=False, **kwargs) for w in wavs], axis=0)
        return raw / np.linalg.norm(raw, 2)
