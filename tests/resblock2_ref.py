"""Float64 restatement of a HifiGAN generator built from ResBlock2 (``resblock: "2"``; test infrastructure, CPU).

Reuses oracle/hifigan_ref.py for everything the two block types share (weight-norm folding, paddings, the upsamplers, conv_pre /
conv_post) and restates only what differs (reference file:line):
  * modules/hifigan/hifigan.py:61-66   ResBlock2: ``convs`` = two dilated convolutions (d0, d1), padding get_padding(k, d)
  * modules/hifigan/hifigan.py:67-84   forward: ``for c in convs: xt = leaky_relu(x, 0.1); xt = c(xt); x = xt + x``
  * modules/hifigan/hifigan.py:109     the generator picks the block by ``h['resblock'] == '1'``
Pinned against the reference implementation itself by tests/golden/g13_hifigan_rb2.npz (tools/make_golden_rb2.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.hifigan_ref import LRELU_SLOPE, _pad, fold_weight_norm  # noqa: F401  (fold_weight_norm re-exported for the tests)


def resblock2(sd, p, x, k, dilations):
    for m, d in enumerate(dilations):
        xt = F.leaky_relu(x, LRELU_SLOPE)
        xt = F.conv1d(xt, sd[f"{p}.convs.{m}.weight"], sd[f"{p}.convs.{m}.bias"], padding=_pad(k, d), dilation=d)
        x = xt + x
    return x


def generator_forward(sd, cfg, mel, return_stages=False, dtype=torch.float64, watch=None):
    """sd: folded state dict; mel [B,80,T] -> wav [B,1,T*hop] in ``dtype``.  Stages: conv_pre, ups.{i}, rb.{n} (one ResBlock's output),
    stage.{i}, post (pre-tanh).  watch(name, a): called with every tensor that the fused kernels convert to a 16-bit operand (the input
    of each ResBlock convolution, BEFORE leaky_relu: rb2x.hip write_act converts first in the f16 mode)."""
    assert str(cfg.get("resblock", "1")) == "2"
    sd = {k: v.to(dtype) for k, v in sd.items()}
    stages = {}
    x = F.conv1d(mel.to(dtype), sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    stages["conv_pre"] = x
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, LRELU_SLOPE)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        stages[f"ups.{i}"] = x
        xs = None
        for j, (rk, rd) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            r = x
            for m, d in enumerate(rd):
                if watch is not None:
                    watch(f"{p}.convs.{m}", r)
                r = F.conv1d(F.leaky_relu(r, LRELU_SLOPE), sd[f"{p}.convs.{m}.weight"], sd[f"{p}.convs.{m}.bias"], padding=_pad(rk, d),
                             dilation=d) + r
            stages[f"rb.{i * nk + j}"] = r
            xs = r if xs is None else xs + r
        x = xs / nk
        stages[f"stage.{i}"] = x
    x = F.leaky_relu(x)  # default slope 0.01 (hifigan.py:138)
    x = F.conv1d(x, sd["conv_post.weight"], sd["conv_post.bias"], padding=3)
    stages["post"] = x
    x = torch.tanh(x)
    return (x, stages) if return_stages else x


def spec2wav(sd, cfg, mel_T80, dtype=torch.float64):
    """vocoders/hifigan.py:54-62 for one utterance; mel [T,80] -> 1-D float64 numpy"""
    with torch.no_grad():
        c = torch.as_tensor(np.asarray(mel_T80, dtype=np.float32)).unsqueeze(0).transpose(2, 1)
        return generator_forward(sd, cfg, c, dtype=dtype).view(-1).to(torch.float64).numpy()


def max_operand(sd, cfg, mel_T80):
    """the largest |value| the fused kernels would convert to a 16-bit ResBlock operand, as the float64 reference sees it"""
    worst = [0.0]

    def watch(name, a):
        worst[0] = max(worst[0], float(a.abs().max()))
    with torch.no_grad():
        c = torch.as_tensor(np.asarray(mel_T80, dtype=np.float32)).unsqueeze(0).transpose(2, 1)
        generator_forward(sd, cfg, c, watch=watch)
    return worst[0]
