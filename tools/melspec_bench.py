#!/usr/bin/env python3
"""Time the fused log-mel launch (dtts_text2mel_fetch(DTTS_OUT_MELSPEC)) against the pipeline a user has without it, on the same device
in the same run: torch.stft + matmul + log10 in float32.  Workload: --batch utterances of --frames frames (default 60 x 700, the
flagship batch of bench.py).  Device time by event pairs around each call, median of --reps after --warmup; the vocoder forward of the
same batch is timed alongside for the launch's share of it (--no-vocoder skips it).  Also prints both pipelines' error against float64
on utterance 0 in the units of tests/test_melspec_gpu.py.

    python tools/melspec_bench.py [--batch 60] [--frames 700] [--reps 20] [--warmup 5] [--no-vocoder] [--lib path/to/libdicttts_hip.so]
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
    ap.add_argument("--frames", type=int, default=700)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-vocoder", action="store_true")
    ap.add_argument("--lib", default=None, help="path of the library build to load instead of the in-tree release library (A/B runs: nothing is copied over it)")
    a = ap.parse_args()
    if a.lib:
        abi.load_library(os.path.abspath(a.lib))
    from dict_tts_amd import melspec, synth, vocoder
    import melspec_ref as mr
    fe = melspec.MelSpectrogram()
    L = a.frames * fe.hop
    rng = np.random.default_rng(0)
    wav_h = (0.1 * rng.standard_normal((a.batch, L))).astype(np.float32)
    wav = torch.from_numpy(wav_h).cuda()
    T = fe.frames(L)
    mel = torch.empty(a.batch, T, fe.n_mels, device="cuda")
    lens = torch.empty(a.batch, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def fused():
        fe.ctx.melspec(wav.data_ptr(), None, a.batch, L, fe.hop, mel.data_ptr(), T, lens.data_ptr(), stream)

    window = torch.from_numpy(fe.window).cuda()
    basis = torch.from_numpy(fe.mel_basis).cuda()

    def torch_pipeline():
        spec = torch.stft(wav, fe.n_fft, hop_length=fe.hop, win_length=fe.win, window=window, center=True, pad_mode="constant", return_complex=True).abs()
        return torch.log10(torch.clamp(torch.matmul(basis, spec), min=melspec.EPS)).transpose(1, 2)

    out = {"batch": a.batch, "frames": T, "gflop": 2.0 * a.batch * T * fe.n_fft * fe.n_fft * 1e-9}
    out["fused_ms_median"], out["fused_ms_min"] = timed(fused, a.reps, a.warmup)
    out["torch_ms_median"], out["torch_ms_min"] = timed(torch_pipeline, a.reps, a.warmup)
    out["fused_tflops"] = out["gflop"] / out["fused_ms_median"]
    lin64 = mr.mel_lin(wav_h[0], fe.n_fft, fe.hop, fe.win, fe.mel_basis)
    sel = mr.log_selection(lin64)
    fused()
    out["fused_log10_err"] = mr.log_error(mel[0].cpu().numpy(), lin64, sel)
    out["torch_log10_err"] = mr.log_error(torch_pipeline()[0].cpu().numpy(), lin64, sel)
    if not a.no_vocoder:
        T_ = lambda v: torch.from_numpy(np.ascontiguousarray(v))
        voc = vocoder.HifiGAN(state_dict={k: T_(v) for k, v in synth.hifigan_state_dict(1234).items()}, config=synth.hifigan_config())
        mels = torch.from_numpy((0.8 * rng.standard_normal((a.batch, a.frames, 80)) - 2.0).astype(np.float32)).cuda()
        out["vocoder_ms_median"], _ = timed(lambda: voc.forward_batch(mels), max(3, a.reps // 4), 2)
        out["fused_share_of_vocoder"] = out["fused_ms_median"] / out["vocoder_ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
