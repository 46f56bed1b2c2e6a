"""Rounding-point restatement of the HifiGAN generator as the fused vocoder kernels compute it (test infrastructure, CPU).

Same structure as ``oracle/hifigan_ref.generator_forward``.  Every value is carried in float64 EXCEPT at the points where a
kernel rounds to a 16-bit type: there it is rounded exactly as the kernel rounds it (each point cites the kernel line it
restates).  The fp32 steps between those points (MFMA accumulation, bias, residual and stage sums, ÷ num_kernels, the
fused conv_post) are taken in float64: the GPU then differs from this emulator only by fp32 summation order and the rare
16-bit rounding flips that order causes, far below the fp16 operand noise the oracle comparison has to allow for.

Modes (``dtts_config.vocoder_precision``, dict_tts_amd/csrc/vocoder.hip ``build_vocoder`` / ``hifigan_forward_fused`` / ``hifigan_forward_x3``):
  * ``"f16"``  (DTTS_VOC_F16): serial convolutions (conv_pre, the polyphase upsamplers, the unfused conv_post) on bf16
    hi / lo split operands with three products; ResBlock convolutions on single fp16 operands, leaky_relu applied in
    fp16 AFTER the conversion; the residual stream between the three iterations of the per-iteration kernel (vpair:
    C >= 128 and k != 3) stored as fp16 unless ``stream16=False`` (tune_flags bit 15).  ``h2=True`` (tune_flags bit 13):
    ups.1 on fp16 hi / lo activations and a single fp16 weight (two products).
  * ``"bf16"`` (DTTS_VOC_BF16): single bf16 operands everywhere, leaky_relu in fp32 BEFORE the conversion.

``rounding=False`` switches every rounding point off: the emulator is then the oracle itself (in ``dtype``).
``hook(name, x, emu)`` is called with every stage tensor (``conv_pre``, ``ups.{i}``, ``rb.{i}.{j}`` = one ResBlock's
output, ``stage.{i}`` = the stage output after ÷ num_kernels, ``post`` = conv_post's pre-tanh output) and may return a
replacement (the planted-defect tests use it); ``emu.resblock(i, j, x)`` recomputes one ResBlock.
"""
import numpy as np
import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1                  # modules/hifigan/hifigan.py:8
F16_SLOPE = 0.0999755859375        # fp16(0.1): rb_common.h act4, `const _Float16 hs = (_Float16)slope` (slope = 0.1f at every call site)


def to_bf16(x):
    """round-to-nearest-even to bf16 of the fp32 value (rb_common.h rf2bf / pack2bf: v_cvt_pk_bf16_f32)"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def to_f16(x):
    """round-to-nearest-even to fp16 of the fp32 value, overflow to +-inf (rb_common.h pack2<EL_F16>: v_cvt_pk_f16_f32)"""
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


def _pad(k, d=1):
    return (k * d - d) // 2   # get_padding, hifigan.py:23-24


class Emulator:
    def __init__(self, sd, cfg, mode="f16", stream16=True, h2=False, fused_post=None, rounding=True, dtype=torch.float64, hook=None):
        """sd: FOLDED state dict (oracle.hifigan_ref.fold_weight_norm), cfg: the generator config.  fused_post: None = as the library
        decides it (the last stage at C = 32 with >= 2 ResBlock kernels: conv_post + tanh in the last rblock's epilogue, vocoder.hip
        `fusable`); False = conv_post on the serial-convolution path (the unfused bf16 testing mode, or any other last width)."""
        assert mode in ("f16", "bf16")
        self.cfg, self.mode, self.rounding, self.dtype, self.hook = cfg, mode, rounding, dtype, hook
        self.stream16 = stream16 and mode == "f16"
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.nk = len(cfg["resblock_kernel_sizes"])
        c0, nup = cfg["upsample_initial_channel"], len(cfg["upsample_rates"])
        self.last_ch = c0 >> nup
        if fused_post is None:
            fused_post = self.last_ch == 32 and self.nk >= 2
        self.fused_post = fused_post
        # vocoder.hip build_vocoder `h2`: ups.1 only, when its polyphase shape suits the H2 instantiation
        self.h2_stage = None
        if h2 and mode == "f16" and nup >= 2:
            if (cfg["upsample_rates"][1] * (c0 >> 2)) % 256 == 0 and (c0 >> 1) % 128 == 0:
                self.h2_stage = 1
        self._wcache = {}

    # ---- rounding points -----------------------------------------------------------------------------------
    def _w(self, name, kind):
        key = (name, kind)
        if key not in self._wcache:
            w = self.sd[name]
            if self.rounding and kind == "f16":
                w = to_f16(w)            # pack.hip pack_conv: ENG_F16 -> f2h_host(v)
            elif self.rounding and kind == "bf16":
                w = to_bf16(w)           # pack.hip pack_conv: ENG_BF16 -> f2bf_host(v)
            self._wcache[key] = w
        return self._wcache[key]

    def _serial(self, fn, x, name, slope, h2=False):
        """one serial convolution (conv_pre, ups.i, unfused conv_post) of leaky_relu(x, slope)"""
        w, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        a = x if slope == 1.0 else F.leaky_relu(x, slope)
        if not self.rounding:
            return fn(a, w, b)
        if self.mode == "bf16":
            # bf16 mode: the operand is the bf16 copy of leaky_relu taken in fp32 by the producer's epilogue (vconv.hip:409-410 /
            # rblock.hip:482 / vpair.hip:341 `pack2bf(lrelu(o, p.slope))`; conv_pre's input: vocoder.hip f32_to_bf16_pad of the mel);
            # weights a single bf16 pack (pack.hip pack_conv ENG_BF16)
            return fn(to_bf16(a), self._w(name + ".weight", "bf16"), b)
        if h2:
            # vconv.hip:158-165 (H2): hh = fp16(med3(a, -65504, 65504)), lo = fp16(a - hh); weights a single fp16 pack;
            # vconv.hip:238-241: W * Xlo + W * Xhi
            ah = to_f16(a.clamp(-65504.0, 65504.0))
            al = to_f16(a - ah)
            wh = self._w(name + ".weight", "f16")
            return fn(al, wh, None) + fn(ah, wh, b)
        # vconv.hip:168-175 (X3): hi = bf16(lrelu(a)), lo = bf16(a - hi); pack.hip pack_conv ENG_BF16X3: whi = bf16(w),
        # wlo = bf16(w - whi); vconv.hip:243-247: Wlo * Xhi + Whi * Xlo + Whi * Xhi (the lo * lo product is not taken)
        ah = to_bf16(a)
        al = to_bf16(a - ah)
        wh = to_bf16(w)
        wl = to_bf16(w - wh)
        return fn(ah, wl, None) + fn(al, wh, None) + fn(ah, wh, b)

    def act(self, x):
        """the ResBlock convolutions' operand leaky_relu(x, 0.1) (rb_common.h act4<EL>(v, 0.1f), vpair.hip:157 / :184 / :230,
        rblock.hip:305)"""
        if not self.rounding:
            return F.leaky_relu(x, LRELU_SLOPE)
        if self.mode == "f16":
            # rb_common.h:88-92: convert first (v_cvt_pk_f16_f32), then max(h, h * fp16(0.1)) in packed fp16 arithmetic (the
            # product of two fp16 values is exact in fp32, so rounding it once to fp16 is the fp16 multiply)
            h = to_f16(x)
            return torch.maximum(h, to_f16(h * F16_SLOPE))
        # rb_common.h:97-103: max(a, a * slope) in fp32, then one bf16 rounding
        return to_bf16(F.leaky_relu(x, LRELU_SLOPE))

    def _call_hook(self, name, x):
        if self.hook is None:
            return x
        y = self.hook(name, x, self)
        return x if y is None else y

    def per_iteration(self, i):
        """does stage i run its ResBlocks on the per-iteration kernel (vpair), for k != 3?  (vocoder.hip build_vocoder: rblock covers
        C <= 64 every k and k = 3 at C = 128 / 256 (rblock.hip rblock_supported); everything else is vpair)"""
        return (self.cfg["upsample_initial_channel"] >> (i + 1)) >= 128

    # ---- the generator ---------------------------------------------------------------------------------------
    def resblock(self, i, j, x, operand_hook=None):
        """ResBlock1 (hifigan.py:51-58) of stage i, kernel j; the residual x in fp32 (rblock: accumulator registers) except on
        the vpair path, where iterations 0 and 1 store it as fp16 (vpair.hip:335-337 `p.y16`, read back as the next iteration's
        residual at vpair.hip:323-326) unless tune bit 15 (vocoder.hip `s16`).  operand_hook(m, which, a) may replace the 16-bit operand
        of iteration m's convs1 (which = 1) / convs2 (which = 2)"""
        oh = operand_hook or (lambda m, which, a: a)
        k, dils = self.cfg["resblock_kernel_sizes"][j], self.cfg["resblock_dilation_sizes"][j]
        p = f"resblocks.{i * self.nk + j}"
        kind = self.mode
        s16 = self.rounding and self.stream16 and self.per_iteration(i) and k != 3
        for m, d in enumerate(dils):
            w1, b1 = self._w(f"{p}.convs1.{m}.weight", kind), self.sd[f"{p}.convs1.{m}.bias"]
            w2, b2 = self._w(f"{p}.convs2.{m}.weight", kind), self.sd[f"{p}.convs2.{m}.bias"]
            xt = F.conv1d(oh(m, 1, self.act(x)), w1, b1, padding=_pad(k, d), dilation=d)
            xt = F.conv1d(oh(m, 2, self.act(xt)), w2, b2, padding=_pad(k, 1))
            x = xt + x
            if s16 and m < 2:
                x = to_f16(x)
        return x

    def forward(self, mel, return_stages=False):
        """mel [B,80,T] -> wav [B,1,T*hop] (B utterances of the same length, like the oracle)"""
        cfg, stages = self.cfg, {}
        mel = mel.to(self.dtype)
        with torch.no_grad():
            conv = lambda a, w, b: F.conv1d(a, w, b, padding=3)
            # conv_pre: f16 mode reads the fp32 mel with in_slope 1 (vocoder.hip vparams_x3(conv_pre, mel, ..., 1.f))
            x = self._serial(conv, mel, "conv_pre", 1.0)
            x = self._call_hook("conv_pre", x)
            stages["conv_pre"] = x
            for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
                up = lambda a, w, b, u=u, k=k: F.conv_transpose1d(a, w, b, stride=u, padding=(k - u) // 2)
                x = self._serial(up, x, f"ups.{i}", LRELU_SLOPE, h2=self.h2_stage == i)
                x = self._call_hook(f"ups.{i}", x)
                stages[f"ups.{i}"] = x
                xs = None
                for j in range(self.nk):
                    r = self._call_hook(f"rb.{i}.{j}", self.resblock(i, j, x))
                    xs = r if xs is None else xs + r
                x = self._call_hook(f"stage.{i}", xs / self.nk)
                stages[f"stage.{i}"] = x
            w, b = self.sd["conv_post.weight"], self.sd["conv_post.bias"]
            if self.fused_post or not self.rounding:
                # rblock.hip:466 lrelu(o / div, 0.01) in fp32 + rblock.hip:492-530 conv_post in exact fp32 (no 16-bit operand)
                pre = F.conv1d(F.leaky_relu(x, 0.01), w, b, padding=3)
            else:
                # vconv.hip post_tanh on the serial path: f16 mode split operands with in_slope 0.01 (vocoder.hip vparams_x3(conv_post,
                # Sf, ch, 0.01f)); bf16 mode the bf16 copy Sa = bf16(lrelu(x, 0.01))
                pre = self._serial(conv, x, "conv_post", 0.01)
            pre = self._call_hook("post", pre)
            stages["post"] = pre
            wav = torch.tanh(pre)
        return (wav, stages) if return_stages else wav

    def spec2wav(self, mel_T80):
        """one utterance, [T,80] -> 1-D float64 numpy (as oracle.hifigan_ref.spec2wav)"""
        c = torch.as_tensor(np.asarray(mel_T80, dtype=np.float32)).unsqueeze(0).transpose(2, 1)
        return self.forward(c).view(-1).to(torch.float64).numpy()


def seam_check(got, want, bounds, win=256):
    """per-sample max |got - want|, the largest RMS over aligned windows of `win` samples, the global RMS; -> (values, failures)
    where failures lists the bounds ({'max', 'win', 'rms'}) that are exceeded.  `values['argmax']` is the worst sample."""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    assert d.ndim == 1 and d.size > 0
    n = (d.size + win - 1) // win
    dp = np.zeros(n * win)
    dp[:d.size] = d
    cnt = np.full(n, float(win))
    cnt[-1] = d.size - (n - 1) * win
    wrms = np.sqrt(np.square(dp).reshape(n, win).sum(1) / cnt)
    vals = {"max": float(np.abs(d).max()), "win": float(wrms.max()), "rms": float(np.sqrt(np.mean(np.square(d)))),
            "argmax": int(np.abs(d).argmax())}
    fails = [k for k in ("max", "win", "rms") if k in bounds and vals[k] > bounds[k]]
    return vals, fails



# GPU - emulator bounds of tests/test_vocoder_kernels_gpu.py: per-sample max, largest 256-sample windowed RMS, global RMS.  Each is <= 3x the
# worst value measured on an MI355X over every shape of that group (the table in the GPU test's docstring); the planted-defect test of
# tests/test_vocoder_emul_cpu.py shows the defects exceed the "full_f16" bounds.  GPU - emulator is NOT an order of magnitude below
# GPU - oracle: the emulator computed in fp32 instead of fp64 differs from itself by about as much as it differs from the GPU (the fp16
# rounding decisions of a deep chain are re-drawn by any change of fp32 summation order; test_vocoder_emul_cpu.py measures it).
BOUNDS = {
    "f16": {"max": 2.4e-4, "win": 6.3e-5, "rms": 6.3e-5},          # isolating generators; measured 9.7e-5 / 2.1e-5 / 2.1e-5
    "bf16": {"max": 3.1e-3, "win": 7.3e-4, "rms": 7.3e-4},         # measured 1.13e-3 / 2.7e-4 / 2.7e-4
    "full_f16": {"max": 8.6e-4, "win": 1.9e-4, "rms": 1.7e-4},     # the four-stage generator; measured 2.9e-4 / 6.4e-5 / 5.7e-5
    "full_bf16": {"max": 1.0e-2, "win": 2.7e-3, "rms": 2.2e-3},    # measured 3.5e-3 / 8.9e-4 / 7.5e-4
}
