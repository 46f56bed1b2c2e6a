"""Waveform conditioning on the device: the two steps the reference's ``process_utterance`` / ``trim_long_silences``
(data_gen/tts/data_gen_utils.py) run on a recording before anything else looks at it.

* ``Resampler`` — band-limited resampling, ``librosa.core.load(path, sr=...)``'s ``resample(res_type='kaiser_best')`` of librosa 0.9.2,
  which is resampy 0.4.2's ``resample_f`` with its ``kaiser_best`` table (dict_tts_amd/csrc/resample.hip,
  dtts_text2mel_fetch(DTTS_OUT_RESAMPLE)).
* ``Loudness`` — ITU-R BS.1770 integrated loudness and normalisation to a target, pyloudnorm 0.1.1's ``Meter.integrated_loudness`` and
  ``normalize.loudness``, then the reference's peak rule (dict_tts_amd/csrc/loudness.hip, dtts_text2mel_fetch(DTTS_OUT_LOUDNESS)).

Both compute in fp64.  The arithmetic is specified in include/dicttts_hip.h and restated in float64 by tests/wavprep_ref.py.  Neither
librosa, resampy nor pyloudnorm was available to compare against: what could not be settled is listed in INTEGRATION.md ("Known
uncertainties of the waveform conditioning").  The VAD silence trimming of ``trim_long_silences`` (webrtcvad) is not implemented.
"""
import math
import warnings

import numpy as np
import torch

from . import abi
from .unit import DeviceUnit

KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
KAISER_FAST = dict(num_zeros=16, precision=9, beta=8.555504641634386, rolloff=0.85)
MAX_WAV = 1 << 26


def sinc_window(num_zeros, precision, beta, rolloff):
    """resampy.filters.sinc_window with window = scipy.signal.kaiser(beta): -> (half_window f64 [num_zeros * 2^precision + 1], 2^precision).
    rolloff sinc(rolloff linspace(0, num_zeros, n + 1)) times the right half of the SYMMETRIC Kaiser window of 2 n + 1 points,
    w[k] = I0(beta sqrt(1 - ((k - n) / n)^2)) / I0(beta)."""
    from scipy.special import i0
    num_bits = 2 ** int(precision)
    n = num_bits * int(num_zeros)
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    k = np.arange(n, 2 * n + 1, dtype=np.float64)
    taper = i0(beta * np.sqrt(np.maximum(0.0, 1.0 - ((k - n) / n) ** 2))) / i0(beta)
    return taper * sinc_win, num_bits


def kaiser_best():
    """resampy's kaiser_best: (half_window f64 [32769], 512)"""
    return sinc_window(**KAISER_BEST)


def kaiser_fast():
    """resampy's kaiser_fast: (half_window f64 [8193], 512)"""
    return sinc_window(**KAISER_FAST)


_FILTERS = {"kaiser_best": kaiser_best, "kaiser_fast": kaiser_fast}


def resampled_len(L, sr_in, sr_out):
    """(n_out, out_len) of an L-sample utterance: resampy computes int(L ratio) samples, librosa's fix_length pads to ceil(L ratio)"""
    lr = float(int(L)) * (float(int(sr_out)) / float(int(sr_in)))
    return int(lr), int(math.ceil(lr))


def k_weighting(rate):
    """pyloudnorm's two K-weighting biquads at `rate`, each normalised by its a0: ((b_shelf [3], a_shelf [3]), (b_highpass [3],
    a_highpass [3])) as float64 (csrc/loudness.hip::loud_coefficients, operation for operation, with the same libm)"""
    rate = float(rate)
    G, Q, fc = 4.0, 1.0 / math.sqrt(2.0), 1500.0
    A, w0 = math.pow(10.0, G / 40.0), 2.0 * math.pi * (fc / rate)
    alpha, cw, r = math.sin(w0) / (2.0 * Q), math.cos(w0), math.sqrt(A)
    b = [A * ((A + 1) + (A - 1) * cw + 2 * r * alpha), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - 2 * r * alpha)]
    a = [(A + 1) - (A - 1) * cw + 2 * r * alpha, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - 2 * r * alpha]
    shelf = (np.array([v / a[0] for v in b]), np.array([v / a[0] for v in a]))
    Q, fc = 0.5, 38.0
    w0 = 2.0 * math.pi * (fc / rate)
    alpha, cw = math.sin(w0) / (2.0 * Q), math.cos(w0)
    b = [(1 + cw) / 2, -(1 + cw), (1 + cw) / 2]
    a = [1 + alpha, -2 * cw, 1 - alpha]
    return shelf, (np.array([v / a[0] for v in b]), np.array([v / a[0] for v in a]))


def n_blocks_of(L, rate):
    """pyloudnorm's count of 0.4 s blocks at 75 % overlap for an L-sample utterance (0: shorter than one block, where it raises)"""
    rate = float(rate)
    if L < 0 or float(L) < 0.4 * rate:
        return 0
    T = float(L) / rate
    return int(np.round((T - 0.4) / (0.4 * 0.25)) + 1)


def block_bounds(rate, n):
    """the first n blocks' sample ranges [lo_j, hi_j) as int64 [n, 2]: int(0.4 (j 0.25) rate), int(0.4 (j 0.25 + 1) rate), pyloudnorm's
    truncations"""
    rate = float(rate)
    return np.array([[int(0.4 * (j * 0.25) * rate), int(0.4 * (j * 0.25 + 1) * rate)] for j in range(int(n))], np.int64).reshape(-1, 2)


def _rate(name, v):
    r = int(v)
    if r != v or not 8000 <= r <= 48000:
        raise ValueError(f"{name} = {v!r} (supported: an integer in 8000 .. 48000)")
    return r


def _batch(wavs, lens):
    wavs = torch.as_tensor(wavs)
    if wavs.dim() != 2:
        raise ValueError(f"wavs must be [B, L] (got {tuple(wavs.shape)})")
    B, L = wavs.shape
    if B < 1 or B > 65535:
        raise ValueError(f"B = {B} (supported: 1 .. 65535)")
    if not 1 <= L <= MAX_WAV:
        raise ValueError(f"L = {L} samples (supported: 1 .. {MAX_WAV})")
    if lens is not None:
        lens = torch.as_tensor(lens).reshape(-1)
        if lens.shape[0] != B:
            raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
    return wavs, lens, B, L


class Resampler(DeviceUnit):
    """``Resampler(sr_in, sr_out)(wavs, lens)`` -> (out f32 [B, ceil(L ratio)], out_lens i32 [B]) on the device.

    filter: "kaiser_best" (librosa's default), "kaiser_fast", or a pair (half_window f64 [n_win], num_table).  ctx: an existing
    ``abi.Context`` or None for one of its own; it is created, and the filter loaded into it, on the first call, so that argument errors
    surface without a GPU.  A context holds ONE filter: a unit whose filter is not the one its context holds loads it again before the
    call (the plan is rebuilt; the old table stays allocated until the context goes), so units with different filters may share a context
    but should not alternate call by call."""

    def __init__(self, sr_in, sr_out, filter="kaiser_best", ctx=None):
        self.ctx = ctx
        self.sr_in, self.sr_out = _rate("sr_in", sr_in), _rate("sr_out", sr_out)
        if self.sr_in == self.sr_out:
            raise ValueError(f"sr_in = sr_out = {self.sr_in}: nothing to resample")
        if isinstance(filter, str):
            if filter not in _FILTERS:
                raise ValueError(f"filter = {filter!r} (known: {', '.join(sorted(_FILTERS))}, or a pair (half_window, num_table))")
            self.win, self.num_table = _FILTERS[filter]()
        else:
            win, num_table = filter
            self.win, self.num_table = np.ascontiguousarray(win, np.float64).reshape(-1), int(num_table)
        nt = self.num_table
        if nt < 1 or nt > 1024 or nt & (nt - 1):
            raise ValueError(f"num_table = {nt} (supported: a power of two, 1 .. 1024)")
        if not 2 <= len(self.win) <= 1 << 17 or (len(self.win) - 1) % nt:
            raise ValueError(f"the filter has {len(self.win)} entries (supported: 2 .. {1 << 17}, one more than a multiple of num_table = {nt})")
        self.ratio = float(self.sr_out) / float(self.sr_in)
        self.index_step = int(min(1.0, self.ratio) * nt)
        if self.index_step < 1:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz gives index_step = 0 with num_table = {nt}")
        if (len(self.win) - 1) // self.index_step > 2048:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz gives {(len(self.win) - 1) // self.index_step} taps per wing (supported: up to 2048)")
        self._key = abi.resample_filter_key(self.win, self.num_table)

    def out_len(self, L):
        return resampled_len(L, self.sr_in, self.sr_out)[1]

    def __call__(self, wavs, lens=None, acc64=False, out_ld=None):
        """wavs [B, L] float32 (anything else is converted), lens [B] or None (= L).  -> (out, out_lens), with acc64=True
        (out, out_lens, out64): the fp64 accumulators before their one rounding.  An utterance whose length is outside 1 .. L gets
        out_lens = 0 and a zero row."""
        wavs, lens, B, L = _batch(wavs, lens)
        ld = self.out_len(L) if out_ld is None else int(out_ld)
        if ld < 1:
            raise ValueError(f"out_ld = {ld}")
        ctx = self._context()
        if getattr(ctx, "resample_filter_key", None) != self._key:
            ctx.load_resample_filter(self.win, self.num_table)
        dev = self.device
        wd = wavs.to(device=dev, dtype=torch.float32).contiguous()
        lensd = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(B, ld, dtype=torch.float32, device=dev)
        out_lens = torch.empty(B, dtype=torch.int32, device=dev)
        out64 = torch.empty(B, ld, dtype=torch.float64, device=dev) if acc64 else None
        ctx.resample(B, torch.cuda.current_stream().cuda_stream, wav=wd.data_ptr(), wav_ld=L, out=out.data_ptr(), out_ld=ld, out_lens=out_lens.data_ptr(),
                     sr_in=self.sr_in, sr_out=self.sr_out, lens=None if lensd is None else lensd.data_ptr(), out64=None if out64 is None else out64.data_ptr())
        return (out, out_lens, out64) if acc64 else (out, out_lens)


class Loudness(DeviceUnit):
    """BS.1770 integrated loudness of a batch of mono waveforms at `sample_rate`, and their normalisation.  ctx as for ``Resampler``."""

    def __init__(self, sample_rate, ctx=None):
        self.ctx = ctx
        self.sample_rate = _rate("sample_rate", sample_rate)

    def blocks(self, L):
        return n_blocks_of(L, self.sample_rate)

    def _run(self, wavs, lens, mode, target, stages):
        wavs, lens, B, L = _batch(wavs, lens)
        target = float(target)
        if not math.isfinite(target):
            raise ValueError(f"target = {target} LUFS (must be finite)")
        ctx = self._context()
        dev = self.device
        wd = wavs.to(device=dev, dtype=torch.float32).contiguous()
        lensd = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
        nb = max(1, self.blocks(L))
        r = {"lufs": torch.empty(B, dtype=torch.float64, device=dev), "gain": torch.empty(B, dtype=torch.float64, device=dev),
             "status": torch.empty(B, dtype=torch.int32, device=dev)}
        if mode:
            r["wavs"] = torch.empty(B, L, dtype=torch.float32, device=dev)
        if stages:
            r["z"] = torch.full((B, nb), float("nan"), dtype=torch.float64, device=dev)
            r["n_blocks"] = torch.empty(B, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        ctx.loudness(B, torch.cuda.current_stream().cuda_stream, wav=wd.data_ptr(), wav_ld=L, blocks_ld=nb, sample_rate=self.sample_rate, lufs=ptr(r["lufs"]),
                     gain=ptr(r["gain"]), status=ptr(r["status"]), mode=mode, target_lufs=target, lens=ptr(lensd), out=ptr(r.get("wavs")), z=ptr(r.get("z")),
                     n_blocks=ptr(r.get("n_blocks")))
        return r

    def measure(self, wavs, lens=None, stages=False):
        """-> lufs f64 [B] on the device (NaN: shorter than one 0.4 s block; -inf: no block passes the gates); stages=True: the dict of
        lufs, gain (towards -22 LUFS), status, z f64 [B, blocks] and n_blocks i32 [B]"""
        r = self._run(wavs, lens, 0, -22.0, stages)
        return r if stages else r["lufs"]

    def normalize(self, wavs, lens=None, target=-22.0, check=True, stages=False):
        """-> (wavs f32 [B, L], lufs f64 [B], gain f64 [B], status i32 [B]) on the device: every utterance scaled to `target` LUFS, then
        divided by its peak where that exceeds 1 (status bit abi.LOUD_PEAK); zeros behind its length.  check=True synchronises and raises
        ValueError naming the first utterance shorter than one block (pyloudnorm's error), and warns for one in which no block passes the
        gates; check=False leaves both to the status bits (such rows are copied unchanged)."""
        r = self._run(wavs, lens, 1, target, stages)
        if check:
            st = r["status"].cpu().numpy()
            short = np.nonzero(st & abi.LOUD_TOO_SHORT)[0]
            if len(short):
                raise ValueError(f"utterance {int(short[0])}: audio must have length greater than the block size (0.4 s = "
                                 f"{0.4 * self.sample_rate:g} samples at {self.sample_rate} Hz)")
            silent = np.nonzero(st & abi.LOUD_SILENT)[0]
            if len(silent):
                warnings.warn(f"utterance {int(silent[0])}: no block passes the BS.1770 gates (loudness -inf); left unnormalised")
        return r if stages else (r["wavs"], r["lufs"], r["gain"], r["status"])


def read_wav_native(path):
    """16-bit / 32-bit / 8-bit / float PCM wav -> (sample rate, float32 mono in [-1, 1)) at the file's own rate"""
    from scipy.io import wavfile
    from . import melspec
    sr, _ = wavfile.read(path, mmap=True)
    return int(sr), melspec.read_wav(path, int(sr))


def load_wav(path, sr, resampler_cache=None, ctx=None):
    """``librosa.core.load(path, sr=sr)``: mono float32 at `sr`, resampled on the device (kaiser_best) when the file's rate differs.
    resampler_cache: a dict that keeps the ``Resampler`` per source rate between calls."""
    sr = _rate("sr", sr)
    sr_file, wav = read_wav_native(path)
    if sr_file == sr:
        return wav
    cache = resampler_cache if resampler_cache is not None else {}
    rs = cache.get((sr_file, sr))
    if rs is None:
        rs = cache[(sr_file, sr)] = Resampler(sr_file, sr, ctx=ctx)
    if len(wav) < 1:
        return wav
    out, _ = rs(torch.from_numpy(np.ascontiguousarray(wav))[None])
    return out[0].cpu().numpy()
