#!/usr/bin/env python3
"""Time the validation losses (ValidationLosses.mel / .dur -> dtts_text2mel_fetch(DTTS_OUT_LOSSES)) against the same formulas in torch
on the same device in the same run: the reference's float32 path (the bias in float32, five F.conv2d with the 11 x 11 window, the masked
means of l1 and ssim; scatter_add and the two logarithms for the durations).  Two workloads: 60 x 700 x 80 (the flagship batch of
bench.py) and 1 x 364 x 80.  The two sides ALTERNATE call by call; device time by an event pair around each call, median of --reps after
--warmup.  Also prints both sides' deviation from float64 on utterance 0 (the SSIM loss, relative).  No gate: figures for LABNOTES.md.

    python tools/loss_bench.py [--reps 20] [--warmup 5] [--lib path/to/libdicttts_hip.so]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

from dict_tts_amd import abi


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(fns, reps, warmup):
    """{name: fn} -> {name: (median ms, min ms)}, the functions taking turns call by call"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(one(fn))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="path of the library build to load instead of the in-tree release library")
    a = ap.parse_args()
    if a.lib:
        abi.load_library(os.path.abspath(a.lib))
    from dict_tts_amd import losses as L
    import losses_ref as lr
    v = L.ValidationLosses(hparams={})
    win = torch.from_numpy(L.ssim_window())[None, None].cuda()
    rng = np.random.default_rng(0)
    for B, T, M in ((60, 700, 80), (1, 364, 80)):
        lens = rng.integers(max(1, T // 2), T + 1, B)
        lens[0] = T
        tgt = np.zeros((B, T, M), np.float32)
        for b in range(B):
            tgt[b, :lens[b]] = np.clip(0.8 * rng.standard_normal((lens[b], M)) - 2.5, -5.9, 1.5)
        pred = (tgt + rng.uniform(0.1, 0.3, tgt.shape) * rng.choice([-1.0, 1.0], tgt.shape)).astype(np.float32)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()
        T_w = max(1, T // 20)
        m2w_np = np.zeros((B, T), np.int64)
        for b in range(B):
            m2w_np[b, :lens[b]] = np.minimum(np.arange(lens[b]) * T_w // lens[b] + 1, T_w)
        m2w = torch.from_numpy(m2w_np).cuda()
        wl = torch.full((B,), T_w, dtype=torch.int64, device="cuda")
        dp = torch.log(torch.from_numpy(lr.dur_gt64(m2w_np, T_w)).float() + 1).cuda() + 0.1

        def torch_mel():
            w = t.abs().sum(-1, keepdim=True).ne(0).float().repeat(1, 1, M)
            l1 = (F.l1_loss(p, t, reduction="none") * w).sum() / w.sum()
            x, y = p[:, None] + 6.0, t[:, None] + 6.0
            conv = lambda q: F.conv2d(q, win, padding=5)
            mx, my = conv(x), conv(y)
            sxx, syy, sxy = conv(x * x) - mx.pow(2), conv(y * y) - my.pow(2), conv(x * y) - mx * my
            m = ((2 * mx * my + lr.C1) * (2 * sxy + lr.C2)) / ((mx.pow(2) + my.pow(2) + lr.C1) * (sxx + syy + lr.C2))
            return l1, ((1 - m[:, 0]) * w).sum() / w.sum()

        def torch_dur():
            g = m2w.new_zeros(B, T_w + 1).scatter_add(1, m2w, torch.ones_like(m2w))[:, 1:].float()
            n = (torch.arange(T_w, device="cuda")[None, :] < wl[:, None]).float()
            d, g = dp * n, ((g * n) + 1).log()
            d, g = (d + 1).log(), (g + 1).log()
            k = (g > 0).float()
            return ((d - g).abs() * k).sum() / k.sum(), (d.sum(-1) - g.sum(-1)).abs().mean()

        out = {"B": B, "T": T, "n_mel": M, "T_w": T_w, "gflop_direct": 2.0 * 5 * 121 * B * T * M * 1e-9}
        r = alternated({"unit": lambda: v.mel(p, t), "torch": torch_mel}, a.reps, a.warmup)
        out["mel_unit_ms_median"], out["mel_unit_ms_min"] = r["unit"]
        out["mel_torch_ms_median"], out["mel_torch_ms_min"] = r["torch"]
        r = alternated({"unit": lambda: v.dur(dp, m2w, wl), "torch": torch_dur}, a.reps, a.warmup)
        out["dur_unit_ms_median"], out["dur_torch_ms_median"] = r["unit"][0], r["torch"][0]
        s64, c64, _ = lr.mel_sums64(pred[:1], tgt[:1])
        want = s64[0, 2] / c64[0]
        out["ssim_unit_rel_err_utt0"] = abs(float(v.mel(p[:1], t[:1])["ssim"]) - want) / want
        out["ssim_torch_rel_err_utt0"] = abs(float(torch_mel_utt0(p, t, win, lr)) - want) / want
        print(json.dumps(out))


def torch_mel_utt0(p, t, win, lr):
    """the float32 path's SSIM loss of utterance 0 alone, on the device"""
    p, t = p[:1], t[:1]
    w = t.abs().sum(-1, keepdim=True).ne(0).float().repeat(1, 1, p.shape[2])
    x, y = p[:, None] + 6.0, t[:, None] + 6.0
    conv = lambda q: F.conv2d(q, win, padding=5)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx.pow(2), conv(y * y) - my.pow(2), conv(x * y) - mx * my
    m = ((2 * mx * my + lr.C1) * (2 * sxy + lr.C2)) / ((mx.pow(2) + my.pow(2) + lr.C1) * (sxx + syy + lr.C2))
    return ((1 - m[:, 0]) * w).sum() / w.sum()


if __name__ == "__main__":
    main()
