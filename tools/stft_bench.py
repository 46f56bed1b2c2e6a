#!/usr/bin/env python3
"""Time the multi-resolution STFT distance (dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE): one launch per resolution + the reduction) against
the same figures from torch.stft — what the reference's stft_loss.py runs — on the same device in the same process.  Workload: --batch waveform
pairs of --frames x 256 samples (default 60 x 400) at the reference's three resolutions.  Device time by event pairs around each call,
median of --reps after --warmup; each resolution's launch is timed alone as well (its FLOP: 2 signals x frames x fft_size outputs x the
contracted samples x 2).  Prints one JSON line; --out appends it to a file.

    python tools/stft_bench.py [--batch 60] [--frames 400] [--reps 20] [--warmup 5] [--lib path/to/libdicttts_hip.so] [--out profiles/stftdist_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from dict_tts_amd import abi


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="path of the library build to load instead of the in-tree release library (A/B runs: nothing is copied over it)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    if a.lib:
        abi.load_library(os.path.abspath(a.lib))
    from dict_tts_amd import stftloss
    L = a.frames * 256
    rng = np.random.default_rng(0)
    y = torch.from_numpy((0.1 * rng.standard_normal((a.batch, L))).astype(np.float32)).cuda()
    x = y + torch.from_numpy((0.01 * rng.standard_normal((a.batch, L))).astype(np.float32)).cuda()
    mr = stftloss.MultiResolutionSTFT()
    res = list(zip(mr.fft_sizes, mr.hop_sizes, mr.win_lengths))
    windows = [torch.hann_window(w, device="cuda") for _, _, w in res]

    def torch_path():
        sc, mag = [], []
        for (n, h, w), win in zip(res, windows):
            m = []
            for s in (x, y):
                X = torch.stft(s, n, h, w, win, return_complex=True)
                m.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-7)).transpose(2, 1))
            sc.append(torch.norm(m[1] - m[0], p="fro") / torch.norm(m[1], p="fro"))
            mag.append(torch.mean(torch.abs(torch.log(m[1]) - torch.log(m[0]))))
        return torch.stack(sc).mean(), torch.stack(mag).mean()

    out = {"batch": a.batch, "samples": L, "resolutions": res}
    got = mr(x, y)
    want = torch_path()
    out["sc_batch"], out["mag_batch"] = float(got["sc_batch"]), float(got["mag_batch"])
    out["torch_sc"], out["torch_mag"] = float(want[0]), float(want[1])
    out["fused_ms_median"], out["fused_ms_min"] = timed(lambda: mr(x, y), a.reps, a.warmup)
    out["torch_ms_median"], out["torch_ms_min"] = timed(torch_path, a.reps, a.warmup)
    out["fused_over_torch"] = out["fused_ms_median"] / out["torch_ms_median"]
    per = []
    for n, h, w in res:   # each resolution alone (a context of its own): which launch bounds the call
        one = stftloss.MultiResolutionSTFT((n,), (h,), (w,))
        ms, _ = timed(lambda: one(x, y), a.reps, a.warmup)
        contracted = (((n - w) // 2 + w + 127) // 128 - ((n - w) // 2 + 1) // 128) * 128   # whole fours of super-groups around the window's support
        gflop = 2.0 * 2 * a.batch * (1 + L // h) * n * contracted * 1e-9
        per.append({"fft_size": n, "hop": h, "win": w, "ms_median": ms, "gflop": gflop, "tflops": gflop / ms})
    out["per_resolution"] = per
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
