"""Rounding-point emulator of a ResBlock2 generator as the library computes it (test infrastructure, CPU): tests/vocoder_emul.Emulator
with the ResBlock replaced.  Everything outside the ResBlocks (serial convolutions, stage sums, the fused conv_post, the hook protocol)
is the parent class's; the rounding helpers are its ``act`` / ``_w``.

ResBlock2 as rb2x.hip computes it (both modes; the vconv per-convolution path of the bf16 mode rounds at the same points: its 16-bit
operand is the producer's bf16(leaky_relu(x)) copy, vconv.hip `pack2bf(lrelu(o, p.slope))`):
  * the residual x stays fp32 in registers through the whole block (rb2x.hip: `xr`, "accumulates straight into the residual
    registers"): NO 16-bit stream between the two convolutions in any mode, so tune bit 15 (`stream16`) changes nothing;
  * the operand of convolution m is act(x) taken from the CURRENT x (rb2x.hip: `write_act(xr)` before the loop and again after
    the first convolution — "leaky_relu of the UPDATED x");
  * weights: one 16-bit pack per convolution (vocoder.hip build_vocoder: pack_conv(..., eng_rb, ...) of convs.{0,1}).

``defect`` plants a restatement error for the CPU test of the bounds: "halo" (the second convolution's outermost tap on each side sees
zeros within one dilation step of a tile seam every `tile` rows: a halo short by d1 rows), "stale" (the second convolution fed
leaky_relu of the OLD x), "no_res0" (the first residual add left out), "rb1_order" (ResBlock1's order: conv, activation, conv, ONE add).
"""
import torch
import torch.nn.functional as F

from vocoder_emul import BOUNDS, Emulator, _pad

# GPU - emulator bounds of tests/test_resblock2_gpu.py (per-sample max, largest 256-sample window RMS, global RMS), by the rule of
# vocoder_emul.BOUNDS: at most 3x the worst value measured on an MI355X over every shape of the group, never above the ResBlock1 bound of
# the same group (a ResBlock2 chain is a third as deep).  Measured values: the GPU test's docstring.
BOUNDS_RB2 = {
    "f16": {"max": 1.6e-4, "win": 2.8e-5, "rms": 2.5e-5},          # isolating generators; measured 5.4e-5 / 9.3e-6 / 8.3e-6
    "bf16": {"max": 2.5e-3, "win": 6.5e-4, "rms": 6.5e-4},         # measured 8.4e-4 / 2.2e-4 / 2.2e-4
    "full_f16": {"max": 6.8e-4, "win": 1.8e-4, "rms": 1.4e-4},     # the V3 generator; measured 2.3e-4 / 6.0e-5 / 4.9e-5
    "full_bf16": {"max": 1.0e-2, "win": 2.7e-3, "rms": 2.2e-3},    # measured 4.2e-3 / 1.1e-3 / 8.9e-4 (3x exceeds ResBlock1's bounds: capped at those)
}
for _g, _b in BOUNDS_RB2.items():
    assert all(_b[k] <= BOUNDS[_g][k] for k in _b), _g


class Emulator2(Emulator):
    def __init__(self, sd, cfg, mode="f16", fused_post=None, rounding=True, dtype=torch.float64, hook=None, defect=None, tile=128):
        assert str(cfg.get("resblock", "1")) == "2"
        super().__init__(sd, cfg, mode=mode, stream16=False, h2=False, fused_post=fused_post, rounding=rounding, dtype=dtype, hook=hook)
        self.defect, self.tile = defect, tile

    def per_iteration(self, i):
        return False   # no per-iteration kernel, no inter-launch stream (rb2x.hip header)

    def _conv(self, a, w, b, k, d):
        return F.conv1d(a, w, b, padding=_pad(k, d), dilation=d)

    def resblock(self, i, j, x, operand_hook=None):
        k, dils = self.cfg["resblock_kernel_sizes"][j], self.cfg["resblock_dilation_sizes"][j]
        p = f"resblocks.{i * self.nk + j}"
        w = [self._w(f"{p}.convs.{m}.weight", self.mode) for m in range(2)]      # pack.hip pack_conv: f2h_host / f2bf_host
        b = [self.sd[f"{p}.convs.{m}.bias"] for m in range(2)]
        if self.defect == "rb1_order":
            xt = self._conv(self.act(x), w[0], b[0], k, dils[0])
            return self._conv(self.act(xt), w[1], b[1], k, dils[1]) + x
        x0 = x
        a0 = self.act(x0)                                   # rb2x.hip: write_act(xr) in front of the loop (rb_common.h act4<EL>)
        y = self._conv(a0, w[0], b[0], k, dils[0])
        x = y if self.defect == "no_res0" else y + x0       # rb2x.hip: xr += bias; contraction accumulates into xr
        a1 = a0 if self.defect == "stale" else self.act(x)  # rb2x.hip: write_act(xr) behind the first convolution
        y = self._conv(a1, w[1], b[1], k, dils[1])
        if self.defect == "halo":
            # rows within d1 of a seam lose the outermost tap that crosses it
            d, half = dils[1], (k - 1) // 2
            n = x.shape[-1]
            t = torch.arange(n)
            wk = w[1]
            lo = ((t % self.tile) < d) & (t >= half * d)                       # the tap at -half * d comes from the other tile
            hi = ((t % self.tile) >= self.tile - d) & (t + half * d < n)
            idx_lo, idx_hi = (t - half * d).clamp(min=0), (t + half * d).clamp(max=n - 1)
            y = y - lo.to(y.dtype) * torch.einsum("oc,bct->bot", wk[:, :, 0], a1[:, :, idx_lo])
            y = y - hi.to(y.dtype) * torch.einsum("oc,bct->bot", wk[:, :, k - 1], a1[:, :, idx_hi])
        return y + x
