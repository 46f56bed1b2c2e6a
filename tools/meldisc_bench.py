#!/usr/bin/env python3
"""Time the multi-window mel discriminator (dict_tts_amd/mel_discriminator.py, csrc/meldisc.hip) against the same weights in torch float32
on the same device: one 364-frame pair and 60 x 700 frames, clips at hop win / 2 (``scores``' default), disc_norm ``in``, H = 128.

Both sides start from the same device tensors and end with D per clip on the device; the torch side gathers the clips with ``unfold``, runs
``F.conv2d`` / ``F.leaky_relu`` / ``F.instance_norm`` / ``F.linear`` (MIOpen / rocBLAS) per window.  Times are medians of --iters calls after
--warmup calls, taken with device events around one call each; the lower and upper quartiles are printed next to them.  The implicit GEMM's
rate is a LOWER bound: blocks 2 and 3's flops divided by the whole call's time (the kernel alone is not timed here).

  python tools/meldisc_bench.py [--iters 30] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dict_tts_amd import mel_discriminator as M  # noqa: E402
from dict_tts_amd import synth  # noqa: E402

WINS = M.WINS


def torch_scores(w, mel, lens):
    """the same computation in torch float32: mel [n, T, 80] (all of length lens[0]: the bench's batches are unpadded) -> D per window"""
    out = []
    for i, win in enumerate(WINS):
        L = int(lens[0])
        if L < win:
            continue
        clips = mel[:, :L].unfold(1, win, win // 2)                       # [n, n_clips, 80, win]
        x = clips.permute(0, 1, 3, 2).reshape(-1, 1, win, 80)
        for l in range(3):
            x = F.leaky_relu(F.conv2d(x, w[f"{i}.conv.{l}.weight"], w[f"{i}.conv.{l}.bias"], stride=2, padding=1), 0.2)
            if l:
                x = F.instance_norm(x, weight=w[f"{i}.norm.{l}.weight"], bias=w[f"{i}.norm.{l}.bias"], eps=1e-5)
        out.append(F.linear(x.reshape(x.shape[0], -1), w[f"{i}.adv.weight"], w[f"{i}.adv.bias"]))
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    state = synth.mel_disc_state_dict(1234, "in", 128, 3, "stack")
    disc = M.MelDiscriminator.from_checkpoint(state)
    wt = {k: torch.from_numpy(v).to(dev) for k, v in M.fold_state_dict(state).items()}
    res = {}
    for name, B, T in (("pair_364", 1, 364), ("batch_60x700", 60, 700)):
        g = torch.from_numpy(np.stack([synth.random_mel(1234, T, f"bench.g{b}") for b in range(B)])).to(dev)
        p = (g + 0.3 * torch.randn(g.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))).contiguous()
        both = torch.cat([g, p]).contiguous()
        lens = torch.full((B,), T, dtype=torch.int32)
        ours = disc.scores(g, p, lens, return_d=True)
        ref = torch_scores(wt, both, lens)
        n_clips, flops = 0, 0.0
        for i, win in enumerate(WINS):
            d = ours["d"][i, :, :ref[i].shape[0] // (2 * B), 0].reshape(-1)
            err = float((d - ref[i].reshape(-1)).abs().max() / ref[i].abs().max())
            assert err < 1e-4, (name, win, err)
            n_clips += ref[i].shape[0]
            flops += ref[i].shape[0] * 2.0 * 9 * 128 * 128 * ((win // 4) * 20 + (win // 8) * 10)
        t_ours = timed(lambda: disc.scores(g, p, lens), args.iters, args.warmup)
        t_torch = timed(lambda: torch_scores(wt, both, lens), args.iters, args.warmup)
        res[name] = {"clips": n_clips, "ours": t_ours, "torch_f32": t_torch, "gemm_gflop": flops / 1e9,
                     "gemm_tflops_lower_bound": flops / (t_ours["median_ms"] * 1e-3) / 1e12}
        print(f"{name}: {n_clips} clips; ours {t_ours['median_ms']:.3f} ms [{t_ours['q25_ms']:.3f}, {t_ours['q75_ms']:.3f}], torch float32 "
              f"{t_torch['median_ms']:.3f} ms [{t_torch['q25_ms']:.3f}, {t_torch['q75_ms']:.3f}]; blocks 2 + 3 are {flops / 1e9:.2f} GFLOP: at least "
              f"{res[name]['gemm_tflops_lower_bound']:.2f} TFLOP/s on the fp32 MFMA")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
