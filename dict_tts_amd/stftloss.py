"""Multi-resolution STFT distance between waveforms on the device: the figures ``sc`` (spectral convergence) and ``mag`` (log STFT magnitude)
of the reference's vocoder validation (tasks/vocoder/hifigan.py:62-76 -> modules/hifigan/stft_loss.py: MultiResolutionSTFTLoss), computed by
the fused kernel of dict_tts_amd/csrc/stftdist.hip — no ``torch.stft``, nothing leaves the device, no gradients.

Per resolution (fft_size, hop, win_length), with m = sqrt(clamp(re^2 + im^2, min=1e-7)) of ``torch.stft(sig, fft_size, hop, win_length,
torch.hann_window(win_length))`` (center=True, pad_mode='reflect'):

    sc  = || m_y - m_x ||_F / || m_y ||_F          mag = mean | log m_y - log m_x |

and the mean of each over the resolutions.  The argument order is the module's, ``forward(x, y)``: y is the recording and the normaliser.
"""
import numpy as np
import torch

from . import abi
from .unit import DeviceUnit

FFT_SIZES, HOP_SIZES, WIN_LENGTHS = (1024, 2048, 512), (120, 240, 50), (600, 1200, 240)   # MultiResolutionSTFTLoss.__init__ defaults


def centred_window(fft_size, win_length):
    """the window as torch.stft applies it: torch.hann_window(win_length) (periodic), zero padded to fft_size with
    (fft_size - win_length) // 2 zeros on the left — float32 [fft_size], what "stft.<i>.window" takes"""
    if not 1 <= win_length <= fft_size:
        raise ValueError(f"win_length = {win_length} (supported: 1 .. fft_size = {fft_size})")
    w = np.zeros(fft_size, np.float32)
    left = (fft_size - win_length) // 2
    w[left:left + win_length] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)).astype(np.float32)
    return w


def frame_count(n_samples, hop, fft_size):
    """frames torch.stft(center=True) gives for n_samples: 1 + n // hop; 0 where it refuses the signal (n <= fft_size // 2: the mirror
    would reach past the other end)"""
    n_samples = int(n_samples)
    return 1 + n_samples // int(hop) if n_samples > int(fft_size) // 2 else 0


def scores(sums, count):
    """sums [n_res, B, 3] float64 (sum (m_y - m_x)^2, sum m_y^2, sum |log m_y - log m_x|) and count [n_res, B] int64 as the library
    returns them -> the dict MultiResolutionSTFT.__call__ documents.  A resolution with count 0 gives NaN, and so does a mean it enters."""
    sums, count = torch.as_tensor(sums, dtype=torch.float64), torch.as_tensor(count, dtype=torch.int64)
    nan = torch.full_like(sums[..., 0], float("nan"))
    has = count > 0
    cnt = count.clamp(min=1).to(torch.float64)
    sc_res = torch.where(has, torch.sqrt(sums[..., 0] / torch.where(has, sums[..., 1], torch.ones_like(nan))), nan)
    mag_res = torch.where(has, sums[..., 2] / cnt, nan)
    pooled, pcount = sums.sum(dim=1), count.sum(dim=1)
    phas = pcount > 0
    pnan = torch.full_like(pooled[:, 0], float("nan"))
    sc_pool = torch.where(phas, torch.sqrt(pooled[:, 0] / torch.where(phas, pooled[:, 1], torch.ones_like(pnan))), pnan)
    mag_pool = torch.where(phas, pooled[:, 2] / pcount.clamp(min=1).to(torch.float64), pnan)
    return {"sc": sc_res.mean(dim=0), "mag": mag_res.mean(dim=0), "sc_res": sc_res, "mag_res": mag_res,
            "sc_batch": sc_pool.mean(), "mag_batch": mag_pool.mean(), "sums": sums, "count": count}


class MultiResolutionSTFT(DeviceUnit):
    """(x [B, L], y [B, L]) -> the reference's multi-resolution ``sc`` / ``mag`` per utterance and pooled, one launch per resolution plus
    one reduction launch, no host synchronisation.

    fft_sizes / hop_sizes / win_lengths: up to four resolutions, the reference's three by default; fft sizes 512 / 1024 / 2048, any hop in
    1 .. fft_size, any win_length <= fft_size.  ctx: an existing ``abi.Context`` to load the plans into (e.g. the vocoder's), or None for
    one of its own; it is created on the first call, so that argument errors surface without a GPU."""

    PREFIX, PART = "stft", abi.PART_STFT

    def __init__(self, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, ctx=None):
        self.fft_sizes, self.hop_sizes, self.win_lengths = [int(v) for v in fft_sizes], [int(v) for v in hop_sizes], [int(v) for v in win_lengths]
        if not (len(self.fft_sizes) == len(self.hop_sizes) == len(self.win_lengths)):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")   # (the module asserts the same)
        if not 1 <= len(self.fft_sizes) <= 4:
            raise ValueError(f"{len(self.fft_sizes)} resolutions (supported: 1 .. 4)")
        for n, h in zip(self.fft_sizes, self.hop_sizes):
            if n not in (512, 1024, 2048):
                raise ValueError(f"fft_size = {n} (supported: 512, 1024, 2048)")
            if not 1 <= h <= n:
                raise ValueError(f"hop = {h} (supported: 1 .. fft_size = {n})")
        self.windows = [centred_window(n, w) for n, w in zip(self.fft_sizes, self.win_lengths)]
        self.ctx = ctx

    @property
    def n_res(self):
        return len(self.fft_sizes)

    def _state(self):
        return {f"{i}.window": w for i, w in enumerate(self.windows)}

    def _plan(self):
        self._context()

    def mag_layout(self, B, mag_cap):
        """(offset, shape) of every resolution's block [2 (x, y), B, mag_cap, fft_size // 2 + 1] inside the flat ``mag`` buffer"""
        out, off = [], 0
        for n in self.fft_sizes:
            shape = (2, B, mag_cap, n // 2 + 1)
            out.append((off, shape))
            off += int(np.prod(shape))
        return out, off

    def __call__(self, x, y, lens=None, mag=None, mag_cap=0):
        """x, y: [B, L] (or [L]) float32 tensors / arrays, x the generated waveform and y the recording; lens: [B] valid samples per
        utterance or None = L for all.  -> dict of float64 cuda tensors:
          sc, mag [B]                 per utterance, the mean over the resolutions (NaN where a resolution has no frame: len <= fft_size / 2);
          sc_res, mag_res [n_res, B]  per resolution;
          sc_batch, mag_batch         the sums pooled over the batch first: the reference's batch call when all lengths are L;
          sums [n_res, B, 3], count [n_res, B]   what the library returned.
        mag: an optional flat float32 cuda tensor that receives the clamped magnitudes (``mag_layout``), mag_cap rows per utterance."""
        x, y = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(y, dtype=torch.float32)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if y.dim() == 1:
            y = y.unsqueeze(0)
        if x.dim() != 2 or x.shape != y.shape:
            raise ValueError(f"x and y must both be [B, L] (got {tuple(x.shape)} and {tuple(y.shape)})")
        B, L = x.shape
        if lens is None and L <= max(self.fft_sizes) // 2:
            raise ValueError(f"L = {L} samples: torch.stft's reflect padding needs more than fft_size / 2 = {max(self.fft_sizes) // 2}")
        if B < 1:
            raise ValueError("B = 0")
        self._plan()
        x, y = x.to(self.device).contiguous(), y.to(self.device).contiguous()
        if lens is not None:
            lens = torch.as_tensor(lens).to(device=self.device, dtype=torch.int32).contiguous()
        sums = torch.empty(self.n_res, B, 3, dtype=torch.float64, device=self.device)
        count = torch.empty(self.n_res, B, dtype=torch.int64, device=self.device)
        self.ctx.stft_distance(x.data_ptr(), y.data_ptr(), lens.data_ptr() if lens is not None else None, B, L, self.hop_sizes, sums.data_ptr(),
                               count.data_ptr(), torch.cuda.current_stream().cuda_stream, mag=mag.data_ptr() if mag is not None else None,
                               mag_cap=mag_cap)
        return scores(sums, count)
