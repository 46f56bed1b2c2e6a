#!/usr/bin/env python3
"""Time HifiGAN's discriminators on the device (dtts_text2mel_fetch(DTTS_OUT_DISC)) against the same folded weights in torch float32 on the
same device in the same run (F.conv2d for the period discriminators, grouped F.conv1d for the scale discriminators; warm, the two sides
ALTERNATE call by call), and against the unit's own block-diagonal DENSE form of the five grouped layers (DTTS_DISC_DENSE_GROUPED: what
conv1d_launch alone would cost).

Two workloads: one 364-frame sentence pair and 60 pairs of 700 frames (hop 256); MPD and MSD separately.  Device time by an event pair
around each call, median of --reps after --warmup.  No gate: figures for LABNOTES.md.

    python tools/disc_bench.py [--reps 5] [--warmup 2] [--workload sentence|batch] [--no-torch] [--no-dense]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/disc_bench.py --once --workload batch     # per-launch times, one call per side
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

WORKLOADS = {"sentence": (1, 364 * 256), "batch": (60, 700 * 256)}
MSD_SPECS = ((1, 1), (2, 4), (2, 16), (4, 16), (4, 16), (1, 16), (1, 1))   # (stride, groups) of convs.0 .. 6


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(one(fn))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def torch_mpd(W, y2):
    """y2 [2B, L] -> the D outputs of the five period discriminators (float32, F.conv2d)"""
    outs = []
    for i, p in enumerate((2, 3, 5, 7, 11)):
        x = y2[:, None, :]
        if x.shape[2] % p:
            x = F.pad(x, (0, p - x.shape[2] % p), "reflect")
        x = x.view(x.shape[0], 1, -1, p)
        for j in range(5):
            x = F.leaky_relu(F.conv2d(x, W[f"mpd.{i}.convs.{j}.weight"], W[f"mpd.{i}.convs.{j}.bias"], stride=(3 if j < 4 else 1, 1), padding=(2, 0)), 0.1)
        outs.append(F.conv2d(x, W[f"mpd.{i}.conv_post.weight"], W[f"mpd.{i}.conv_post.bias"], padding=(1, 0)).flatten(1))
    return outs


def torch_msd(W, y2):
    outs = []
    x0 = y2[:, None, :]
    for i in range(3):
        if i:
            x0 = F.avg_pool1d(x0, 4, 2, padding=1)
        x = x0
        for j, (s, g) in enumerate(MSD_SPECS):
            w = W[f"msd.{i}.convs.{j}.weight"]
            x = F.leaky_relu(F.conv1d(x, w, W[f"msd.{i}.convs.{j}.bias"], stride=s, padding=w.shape[2] // 2, groups=g), 0.1)
        outs.append(F.conv1d(x, W[f"msd.{i}.conv_post.weight"], W[f"msd.{i}.conv_post.bias"], padding=1).flatten(1))
    return outs


def flops(B, L):
    """algorithmic 2 * MAC of both signals of B pairs at L samples: (mpd, msd, msd grouped layers only)"""
    import disc_ref as dr
    mpd = msd = grouped = 0.0
    for p in dr.PERIODS:
        r = -(-L // p)
        for co, ci, k, s, g in dr.MPD_CONVS + (dr.POST,):
            r = -(-r // s)
            mpd += 2.0 * r * p * co * ci * k
    for i in range(3):
        r = L >> i
        for j, (co, ci, k, s, g) in enumerate(dr.MSD_CONVS + (dr.POST,)):
            r = -(-r // s)
            f = 2.0 * r * co * (ci // g) * k
            msd += f
            if 1 <= j <= 5:
                grouped += f
    return mpd * 2 * B, msd * 2 * B, grouped * 2 * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--once", action="store_true", help="one call per side and workload, no timing: for a kernel trace")
    a = ap.parse_args()
    from dict_tts_amd import abi, synth
    from dict_tts_amd import discriminators as D
    w = D.fold_state_dict(synth.hifigan_disc_state_dict(1616))
    disc = D.Discriminators(w)
    Wt = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    rng = np.random.default_rng(0)
    for name in a.workload or sorted(WORKLOADS, reverse=True):
        B, L = WORKLOADS[name]
        y = torch.from_numpy((0.3 * rng.standard_normal((B, L))).astype(np.float32)).cuda()
        yh = y + 0.05 * torch.randn_like(y)
        y2 = torch.cat([y, yh])
        fns = {"unit_mpd": lambda: disc.scores(y, yh, which=("mpd",)), "unit_msd": lambda: disc.scores(y, yh, which=("msd",)),
               "unit_both_fm": lambda: disc.scores(y, yh, feature_matching=True)}
        if not a.no_dense:
            ctx = disc._context()
            out = {k: torch.empty(s, dtype=t, device="cuda") for k, s, t in (("sums", (B, 8, 4), torch.float64), ("counts", (B, 8), torch.int64),
                                                                                 ("status", (B,), torch.int32))}
            fns["unit_msd_dense_grouped"] = lambda: ctx.disc(B, torch.cuda.current_stream().cuda_stream, y=y.data_ptr(), y_hat=yh.data_ptr(), wav_ld=L,
                                                             which=abi.DISC_MSD | abi.DISC_DENSE_GROUPED, sums=out["sums"].data_ptr(),
                                                             counts=out["counts"].data_ptr(), status=out["status"].data_ptr())
        if not a.no_torch:
            with torch.no_grad():
                fns["torch_mpd"] = lambda: torch_mpd(Wt, y2)
                fns["torch_msd"] = lambda: torch_msd(Wt, y2)
        if a.once:
            with torch.no_grad():
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            continue
        with torch.no_grad():
            r = alternated(fns, a.reps, a.warmup)
            res = {"workload": name, "B": B, "samples": L}
            for k, (med, mn) in r.items():
                res[k + "_ms_median"], res[k + "_ms_min"] = med, mn
            f_mpd, f_msd, f_grp = flops(B, L)
            res.update(mpd_tflop=f_mpd / 1e12, msd_tflop=f_msd / 1e12, msd_grouped_tflop=f_grp / 1e12,
                       unit_mpd_tflops=f_mpd / r["unit_mpd"][0] / 1e9, unit_msd_tflops=f_msd / r["unit_msd"][0] / 1e9)
            if not a.no_dense:
                s1 = disc.scores(y, yh, which=("msd",))["sums"][:, 5:]
                fns["unit_msd_dense_grouped"]()
                res["dense_vs_grouped_max_rel_diff_of_sums"] = float(((out["sums"][:, 5:] - s1).abs() / s1.abs()).max())
            if not a.no_torch:
                got = disc.scores(y, yh, return_d=True)
                dt = torch_mpd(Wt, y2) + torch_msd(Wt, y2)
                res["max_rel_diff_of_D_vs_torch"] = max(float((got["d"][d, 0, :, :dt[d].shape[1]] - dt[d][:B]).abs().max() / dt[d].abs().max()) for d in range(8))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
