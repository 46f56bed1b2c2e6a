"""Plain float64 restatement of the reference's ``FFTBlocks.forward`` at inference (modules/fastspeech/tts_modules.py:458-523; the fp32
oracle of the same stack is oracle/fft_blocks_ref.py), the defects the tests plant in it, and the per-row comparison of
tests/test_fft_blocks_gpu.py (test infrastructure).

``forward`` takes the sinusoid table as an INPUT (``table(n, C)``: built in fp32 exactly as dict_tts_amd.fft.sinusoid_table builds it,
then widened), so that the reference and the GPU read the same table values and the comparison measures the arithmetic of the stack
alone.  Everything else is float64: value-derived or explicit padding, make_positions on x[..., 0], x + alpha * table[pos], EncSALayer
(bias-free projections, keys past the end masked), torch LayerNorm at eps 1e-5, the SAME-padded ffn_1 that reads the LayerNorm bias
of padded frames, (conv + bias) * k**-0.5 -> erf-GELU, ffn_2, the residuals and non-padding masks, the optional last norm.

``defect=`` plants ONE kernel defect (DEFECTS); tests/test_fft_blocks_cpu.py proves that each of them exceeds FFT_BOUNDS on a seam case
of the GPU file, i.e. that the GPU tests would notice a kernel which had it.
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

from acoustic_ref import WIN, rowcmp
from dict_tts_amd import fft as _fft

# the defects forward(defect=...) can plant, one at a time
DEFECTS = ("pos_off_by_one",        # a first-channel-zero frame advances the position count of the frames behind it
           "carry_lost_256",        # the position count restarts at frame 256 (fft_positions_kernel's carry between chunks of 256 frames)
           "gelu_tanh",             # tanh-form GELU instead of the erf form
           "scale_before_bias",     # conv * k**-0.5 + bias instead of (conv + bias) * k**-0.5
           "masked_key_leak",       # the first key past an utterance's end is not masked: it keeps the finite weight of its own score
           "ffn1_pad_zeros",        # ffn_1 reads zeros at padded frames instead of the LayerNorm bias
           "ln_eps_1e-12",          # LayerNorm eps 1e-12 (the S2PA encoders' value) instead of torch's 1e-5
           "last_row_zero")         # the last valid row of every utterance comes out as zeros

# Bounds of GPU - float64 per comparison (whole output, first 8 rows, last 8 rows of every utterance): max abs / largest RMS over 8
# consecutive rows of one utterance / global RMS.  Each is at most 3x the worst figure measured on MI355X over every case of
# tests/test_fft_blocks_gpu.py at that hidden size (the measured figures in the comments and in LABNOTES.md); the margin leaves room
# for another summation order, nothing else.  The fp32 oracle itself is 2.0e-6 / 3.5e-7 / 2.4e-7 from float64 on the same cases
# (1.4e-6 / 2.7e-7 / 1.7e-7 at hidden 768).
# One row per hidden size, because the error follows the longest fp32 summation chain of the stack: conv1d_short_kernel sums a contraction in
# 4 parts, the generic conv1d_cl_kernel in ONE chain of v_mfma_f32_32x32x2 over the whole contraction.  Up to hidden 192 every convolution is on
# the short kernel; at 256 ffn_2 (1024 terms) goes to the generic kernel beyond 256 row tiles, at 384 always (1536 terms), at 768 ffn_2
# (3072 terms) always and ffn_1 (6912 terms) beyond 256 row tiles.  An fp32 chain of that length summed on the CPU is 2.0x (1024, 1536 terms)
# and 2.8x (3072) the RMS error of a blocked sgemm of the same product; the GPU measures 1.3x / 2.0x / 2.9x the oracle's RMS at 256 / 384 / 768.
FFT_BOUNDS = {
    192: {"max": 5.0e-6, "win": 1.0e-6, "rms": 9.2e-7},     # hidden <= 192: 1.67e-6 / 3.43e-7 / 3.09e-7
    256: {"max": 1.1e-5, "win": 1.7e-6, "rms": 1.3e-6},     # 3.76e-6 / 5.67e-7 / 4.65e-7 (ffn_2 on the generic kernel; on the fp32 short kernel 1.93e-6 / 4.06e-7 / 3.36e-7)
    384: {"max": 1.6e-5, "win": 2.0e-6, "rms": 1.9e-6},     # 5.53e-6 / 6.87e-7 / 6.40e-7
    768: {"max": 2.3e-5, "win": 3.3e-6, "rms": 2.7e-6},     # 7.88e-6 / 1.12e-6 / 9.20e-7 (ffn_1 on the generic kernel; on the fp32 short kernel 6.35e-6 / 7.58e-7 / 6.41e-7)
}


def bounds_of(hidden):
    """the row of the smallest listed hidden size >= hidden"""
    return FFT_BOUNDS[min(h for h in FFT_BOUNDS if h >= hidden)]


def table(n, C):
    """the fp32 sinusoid table of dict_tts_amd.fft (bit-identical to the reference's), widened to float64"""
    return _fft.sinusoid_table(n, C, 0).double()


def state(sd_np):
    """numpy state dict (synth.fft_blocks_state_dict) -> float64 torch state dict"""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd_np.items()}


def make_positions(first, defect=None):
    """utils/tts_utils.py:6-18 on x[..., 0]: non-zero frames -> 1, 2, 3, ...; zero frames -> 0 and do not advance the count"""
    nz = first.ne(0).long()
    cnt = torch.cumsum(nz, dim=1)
    if defect == "pos_off_by_one":
        seen_zero = (torch.cumsum(1 - nz, dim=1) > 0).long()
        cnt = cnt + seen_zero
    elif defect == "carry_lost_256" and first.shape[1] > 256:
        cnt = torch.cat([cnt[:, :256], cnt[:, 256:] - cnt[:, 255:256]], dim=1)
    return cnt * nz


def _ln(x, sd, name, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)


def _layer(sd, p, x, pad, lens, heads, K, defect):
    """EncSALayer.forward (common_layers.py:649-673) on [B, T, C]"""
    B, T, C = x.shape
    keep = (~pad).to(x.dtype)[..., None]
    eps = 1e-12 if defect == "ln_eps_1e-12" else 1e-5
    dk = C // heads
    h = _ln(x, sd, p + "layer_norm1", eps)
    q, k, v = F.linear(h, sd[p + "self_attn.in_proj_weight"]).split(C, dim=-1)
    q = q.view(B, T, heads, dk).transpose(1, 2) * dk ** -0.5
    k = k.view(B, T, heads, dk).transpose(1, 2)
    v = v.view(B, T, heads, dk).transpose(1, 2)
    scores = q @ k.transpose(-1, -2)                                    # [B, heads, T, T]
    masked = scores.masked_fill(pad[:, None, None, :], float("-inf"))
    if defect == "masked_key_leak":
        for b, n in enumerate(lens):
            if n < T:
                masked[b, :, :, n] = scores[b, :, :, n]
    o = (torch.softmax(masked, dim=-1) @ v).transpose(1, 2).reshape(B, T, C)
    x = (x + F.linear(o, sd[p + "self_attn.out_proj.weight"])) * keep
    h = _ln(x, sd, p + "layer_norm2", eps)                              # = the LayerNorm bias at padded frames
    if defect == "ffn1_pad_zeros":
        h = h * keep
    w1, b1 = sd[p + "ffn.ffn_1.weight"], sd[p + "ffn.ffn_1.bias"]
    if defect == "scale_before_bias":
        h = F.conv1d(h.transpose(1, 2), w1, None, padding=K // 2).transpose(1, 2) * K ** -0.5 + b1
    else:
        h = F.conv1d(h.transpose(1, 2), w1, b1, padding=K // 2).transpose(1, 2) * K ** -0.5
    h = F.gelu(h, approximate="tanh" if defect == "gelu_tanh" else "none")
    h = F.linear(h, sd[p + "ffn.ffn_2.weight"], sd[p + "ffn.ffn_2.bias"])
    return (x + h) * keep


def forward(sd, x, lens=None, num_heads=2, kernel_size=9, use_pos_embed=True, use_last_norm=True, use_pos_embed_alpha=True, pos_table=None,
            defect=None):
    """FFTBlocks.forward(x [B, T, C], padding_mask) -> [B, T, C] in the dtype of x / sd (float64 for the reference).  lens: None for the
    value-derived padding (x.abs().sum(-1).eq(0)) or the valid length of every utterance (an explicit suffix padding_mask); pos_table:
    table(n > T, C), required with use_pos_embed"""
    assert defect is None or defect in DEFECTS, defect
    with torch.no_grad():
        B, T, C = x.shape
        if lens is None:
            pad = x.abs().sum(-1).eq(0)
            lens = [int(n) for n in (~pad).sum(1)]
            assert bool((pad == (torch.arange(T)[None] >= torch.tensor(lens)[:, None])).all()), "padding must be a suffix"
        else:
            lens = [int(n) for n in lens]
            pad = torch.arange(T)[None] >= torch.tensor(lens)[:, None]
        assert min(lens) >= 1, "an utterance without a valid frame has no softmax"
        keep = (~pad).to(x.dtype)[..., None]
        if use_pos_embed:
            assert pos_table is not None and pos_table.shape[0] > T
            alpha = sd["pos_embed_alpha"] if use_pos_embed_alpha and "pos_embed_alpha" in sd else 1.0
            x = x + alpha * pos_table.to(x.dtype)[make_positions(x[..., 0], defect)]    # the mask plays no part in the positions
        x = x * keep
        n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
        for i in range(n_layers):
            x = _layer(sd, f"layers.{i}.op.", x, pad, lens, num_heads, kernel_size, defect)
        if use_last_norm:
            x = _ln(x, sd, "layer_norm", 1e-12 if defect == "ln_eps_1e-12" else 1e-5) * keep
        if defect == "last_row_zero":
            x = x.clone()
            for b, n in enumerate(lens):
                x[b, n - 1] = 0
        return x


# ---------------------------------------------------------------------------------------------------------------------------------------
def edge_rows(y, lens, last, n=WIN):
    """[B, n, C]: the first (last=False) or last (last=True) n VALID rows of every utterance, zero rows where it has fewer"""
    y = np.asarray(y.detach().cpu() if hasattr(y, "detach") else y)
    out = np.zeros((y.shape[0], n, y.shape[2]), y.dtype)
    for b, m in enumerate(lens):
        m = int(m)
        k = min(n, m)
        out[b, :k] = y[b, m - k:m] if last else y[b, :k]
    return out


def check(case, what, got, want, bounds, win=WIN):
    """acoustic_ref.rowcmp + one FFTMEAS line; -> the bounds exceeded, as '<case> <what> <stat> <value> > <bound>' (empty = within)"""
    v = rowcmp(got, want, win)
    print("FFTMEAS " + json.dumps({"case": case, "what": what, **v}), flush=True)
    return [f"{case} {what} {k} {v[k]:.3g} > {bounds[k]:.3g} (max at {v['at']}, worst window at {v['win_at']})"
            for k in ("max", "win", "rms") if v[k] > bounds[k]]


def compare(case, got, want, lens, bounds):
    """the comparisons of one output: the whole tensor, the first 8 and the last 8 valid rows of every utterance (where the k-tap halo
    of ffn_1 reads the LayerNorm bias of padded frames), and rows past the end exactly 0.  -> list of failures"""
    g = np.asarray(got.detach().cpu() if hasattr(got, "detach") else got)
    bad = check(case, "all", g, want, bounds)
    bad += check(case, "head", edge_rows(g, lens, False), edge_rows(want, lens, False), bounds)
    bad += check(case, "tail", edge_rows(g, lens, True), edge_rows(want, lens, True), bounds)
    for b, n in enumerate(lens):
        if (g[b, int(n):] != 0).any():
            bad.append(f"{case} utterance {b}: rows past its end ({int(n)}) are not exactly 0")
    if not np.isfinite(g).all():
        bad.append(f"{case}: non-finite output")
    return bad
