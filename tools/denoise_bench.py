#!/usr/bin/env python3
"""Time the spectral-subtraction filter (HifiGAN.denoise -> dtts_text2mel_fetch(DTTS_OUT_SPECTRAL)) against the pipeline a user has without
it, on the same device in the same run: torch.stft -> max(|S| - v, 0) with the phase kept -> torch.istft in float32.  Workload: --batch
waveforms of --frames frames as the vocoder returns them (default 60 x 700, the flagship batch of bench.py).  The two pipelines ALTERNATE
call by call; device time by an event pair around each call, median of --reps after --warmup.  The vocoder forward of the same batch and
the filter's two halves alone (Spectral.stft / Spectral.istft) are timed alongside.  Also prints both pipelines' error against float64 on
utterance 0 in the units of tests/test_spectral_gpu.py.  No gate: these are figures for LABNOTES.md.

    python tools/denoise_bench.py [--batch 60] [--frames 700] [--v 0.1] [--reps 20] [--warmup 5] [--lib path/to/libdicttts_hip.so]
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
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--frames", type=int, default=700)
    ap.add_argument("--v", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="path of the library build to load instead of the in-tree release library (A/B runs: nothing is copied over it)")
    a = ap.parse_args()
    if a.lib:
        abi.load_library(os.path.abspath(a.lib))
    from dict_tts_amd import synth, vocoder
    import istft_ref as ir
    T_ = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    voc = vocoder.HifiGAN(state_dict={k: T_(v) for k, v in synth.hifigan_state_dict(1234).items()}, config=synth.hifigan_config())
    rng = np.random.default_rng(0)
    mels = T_((0.8 * rng.standard_normal((a.batch, a.frames, 80)) - 2.0).astype(np.float32)).cuda()
    lens = torch.full((a.batch,), a.frames, dtype=torch.int32, device="cuda")
    wav = voc.forward_batch(mels, lens)
    voc.denoise(wav, lens, a.v)   # builds the plan
    sp = voc._spectral
    window = T_(sp.window).cuda()
    v32 = float(np.float32(a.v))

    def torch_pipeline():
        S = torch.stft(wav, sp.n_fft, hop_length=sp.hop, win_length=sp.n_fft, window=window, center=True, pad_mode="constant", return_complex=True)
        m = S.abs()
        S = torch.where(m > 0, S * ((m - v32).clamp(min=0) / torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(S))
        return torch.istft(S, sp.n_fft, hop_length=sp.hop, win_length=sp.n_fft, window=window, center=True)

    spec, frames = sp.stft(wav)
    out = {"batch": a.batch, "frames": a.frames, "n_fft": sp.n_fft, "hop": sp.hop, "v": a.v,
           "gflop": 2 * 2.0 * a.batch * (a.frames + 1) * sp.n_fft * sp.n_fft * 1e-9}   # two dense contractions of n_fft x n_fft per frame
    t = alternated({"fused": lambda: voc.denoise(wav, lens, a.v), "torch": torch_pipeline}, a.reps, a.warmup)
    out["fused_ms_median"], out["fused_ms_min"] = t["fused"]
    out["torch_ms_median"], out["torch_ms_min"] = t["torch"]
    out["fused_tflops"] = out["gflop"] / out["fused_ms_median"]
    t = alternated({"stft": lambda: sp.stft(wav), "istft": lambda: sp.istft(spec, frames)}, max(3, a.reps // 2), 2)
    out["stft_ms_median"], out["istft_ms_median"] = t["stft"][0], t["istft"][0]
    out["vocoder_ms_median"] = alternated({"voc": lambda: voc.forward_batch(mels, lens)}, max(3, a.reps // 4), 2)["voc"][0]
    out["fused_share_of_vocoder"] = out["fused_ms_median"] / out["vocoder_ms_median"]
    x = wav[0].cpu().numpy()
    y64 = ir.denoise(x, sp.window, sp.hop, a.v)
    out["fused_err"] = ir.unit_error(voc.denoise(wav, lens, a.v)[0][0].cpu().numpy(), y64)
    out["torch_err"] = ir.unit_error(torch_pipeline()[0].cpu().numpy(), y64)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
