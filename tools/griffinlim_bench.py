#!/usr/bin/env python3
"""Time Griffin-Lim on the device (Spectral.griffin_lim -> dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM)) against the reference's
griffin_lim_torch (utils/audio.py:136-158) restated on torch.stft / torch.istft in float32 on the same device, in the same process: the two
ALTERNATE call by call, device time by an event pair around each call (a call is 1 + 2 + 3 n_iter launches, tens of milliseconds and more),
median of --reps after --warmup.  Workloads: --iters iterations (default 60, the reference's griffin_lim_iters) on 60 x 700 frames, the
flagship batch of bench.py, and on one 364-frame sentence; magnitudes of seeded noise through the transform, a random start phase.

The split of an iteration is timed alongside from the pieces that can be called alone: n_iter = 0 (target and start + the inverse's two
launches), Spectral.istft (the inverse's two), Spectral.stft (the forward contraction without the projection epilogue); the iteration itself
is (t(n_iter) - t(0)) / n_iter, and the projection launch is that minus the inverse.  For the time of every KERNEL run this script under
`rocprofv3 --kernel-trace --stats` with --reps 1 --warmup 0 (a run of its own: tracing slows the host).  Also prints both sides'
consistency || |STFT(y)| - A || / || A || on utterance 0 (float64 on the host).  No gate: these are figures for LABNOTES.md.

    python tools/griffinlim_bench.py [--iters 60] [--reps 5] [--warmup 2] [--shapes 60x700,1x364] [--lib path/to/libdicttts_hip.so]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

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
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="60x700,1x364", help="comma separated BxT")
    ap.add_argument("--lib", default=None, help="path of the library build to load instead of the in-tree one")
    a = ap.parse_args()
    if a.lib:
        abi.load_library(os.path.abspath(a.lib))
    if not torch.cuda.is_available():
        raise SystemExit("griffinlim_bench.py needs a ROCm GPU: there is nothing to time without one")
    from dict_tts_amd import spectral
    import griffinlim_ref as gr
    sp = spectral.Spectral()
    N, hop = sp.n_fft, sp.hop
    window = torch.from_numpy(sp.window).cuda()
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(0)
        x = 0.1 * torch.randn(B, hop * (T - 1), device="cuda", generator=g)
        A = sp.stft(x)[0].abs().contiguous()
        init = torch.polar(torch.ones_like(A), 2.0 * math.pi * torch.rand(A.shape, device="cuda", generator=g))
        amp, ang0 = A.transpose(1, 2).contiguous(), torch.angle(init).transpose(1, 2).contiguous()   # [B, bins, T], the reference's layout

        def torch_gl(n=a.iters):
            def inv(ang):
                return torch.istft(amp * torch.exp(1j * ang), N, hop_length=hop, win_length=N, window=window, center=True)
            y = inv(ang0)
            for _ in range(n):
                y = inv(torch.angle(torch.stft(y, N, hop_length=hop, win_length=N, window=window, center=True, pad_mode="constant", return_complex=True)))
            return y

        hip_gl = lambda n=a.iters: sp.griffin_lim(mag=A, init=init, n_iter=n)[0]
        out = {"batch": B, "frames": T, "n_fft": N, "hop": hop, "iters": a.iters, "launches": 3 + 3 * a.iters,
               "gflop": (1 + 2 * a.iters) * 2.0 * B * T * N * N * 1e-9}   # the dense contractions: one inverse, then a forward and an inverse per iteration
        t = alternated({"hip": hip_gl, "torch": torch_gl}, a.reps, a.warmup)
        out["hip_ms_median"], out["hip_ms_min"] = t["hip"]
        out["torch_ms_median"], out["torch_ms_min"] = t["torch"]
        out["hip_over_torch"] = out["hip_ms_median"] / out["torch_ms_median"]
        out["hip_tflops"] = out["gflop"] / out["hip_ms_median"]
        spec0 = torch.view_as_complex(torch.view_as_real(init) * A[..., None])
        y0 = hip_gl(0)
        t = alternated({"n0": lambda: hip_gl(0), "istft": lambda: sp.istft(spec0), "stft": lambda: sp.stft(y0)}, max(5, 2 * a.reps), 2)
        out["n_iter0_ms"], out["istft_ms"], out["stft_ms"] = t["n0"][0], t["istft"][0], t["stft"][0]
        if a.iters:
            out["iteration_ms"] = (out["hip_ms_median"] - out["n_iter0_ms"]) / a.iters
            out["project_ms"] = out["iteration_ms"] - out["istft_ms"]
        out["target_ms"] = out["n_iter0_ms"] - out["istft_ms"]
        A0, w = A[0].cpu().numpy(), sp.window
        out["hip_consistency"] = gr.consistency(hip_gl()[0].cpu().numpy(), A0, w, hop)
        out["torch_consistency"] = gr.consistency(torch_gl()[0].cpu().numpy(), A0, w, hop)
        out["start_consistency"] = gr.consistency(y0[0].cpu().numpy(), A0, w, hop)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
