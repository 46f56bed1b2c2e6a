#!/usr/bin/env python3
"""Time the speaker encoder on the device (dtts_text2mel_fetch(DTTS_OUT_SPKENC)) against float32 torch on the same device in the same run:
torch.nn.LSTM(40, 256, 3) (MIOpen) + Linear + the norms fed the SAME partial mels, and torch.stft -> power -> filterbank for the front end.
Warm, the sides ALTERNATE call by call; device time by an event pair around each call, median of --reps after --warmup.

Two workloads at 16 kHz: one recording of a 364-frame sentence (hop 256 at 22050 Hz: 67 617 samples, 4 partials) and 60 recordings of 700
frames (130 031 samples, 9 partials each: 540 sequences).  Both tile sizes of the recurrent kernel (tile_m 16 and 32).  The stages of the
unit (mel, projections, recurrence, epilogue) come from a kernel trace of one call:

    python tools/spkenc_bench.py [--reps 7] [--warmup 2] [--workload sentence|batch]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/spkenc_bench.py --once --workload batch [--tile-m 16]
    python tools/spkenc_bench.py --stages DIR          # sums the trace's kernel_stats by stage

No gate: figures for LABNOTES.md."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

samples = lambda frames: int(round(frames * 256 * 16000 / 22050))
WORKLOADS = {"sentence": (1, samples(364)), "batch": (60, samples(700))}
STAGES = (("mel", ("spkenc_mel",)), ("projections", ("conv1d",)), ("recurrence", ("spkenc_lstm",)), ("epilogue", ("spkenc_embed", "spkenc_utt", "spkenc_plan")))


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


def stages(directory):
    """kernel_stats of a rocprofv3 --kernel-trace --stats run -> total device time per stage (ms)"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    out = {name: 0.0 for name, _ in STAGES}
    out["other"] = 0.0
    for r in rows:
        ns = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0)
        for name, keys in STAGES:
            if any(k in r["Name"] for k in keys):
                out[name] += ns / 1e6
                break
        else:
            out["other"] += ns / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--once", action="store_true", help="one warm call of the unit and nothing else (for a kernel trace)")
    ap.add_argument("--tile-m", type=int, default=0)
    ap.add_argument("--stages", default=None, help="directory of a rocprofv3 --kernel-trace --stats run: print its time per stage")
    ap.add_argument("--seed", type=int, default=2020)
    a = ap.parse_args()
    if a.stages:
        print(json.dumps({"stages_ms": stages(a.stages)}))
        return
    import spkenc_ref as R
    from dict_tts_amd import melspec, synth
    from dict_tts_amd import speaker_encoder as E

    sd = synth.voice_encoder_state_dict(a.seed)
    enc = E.VoiceEncoder.from_checkpoint(sd)
    layers, lin = R.torch_lstm(R.f64(sd))
    lstm = torch.nn.LSTM(40, 256, 3, batch_first=True)
    lstm.load_state_dict({f"{n[:-1]}{k}": v for k, m in enumerate(layers) for n, v in m.state_dict().items()})
    lstm, lin = lstm.cuda(), lin.cuda()
    lstm.flatten_parameters()
    win = torch.from_numpy(melspec.hann_window(400)).float().cuda()
    fb = torch.from_numpy(melspec.mel_filterbank(16000, 400, 40, 0, 8000)).float().cuda()
    for name in ([a.workload] if a.workload else sorted(WORKLOADS)):
        B, L = WORKLOADS[name]
        rng = np.random.default_rng(a.seed)
        t = np.arange(L)
        wav = torch.from_numpy((0.2 * np.sin(2 * np.pi * 150 * t / 16000)[None] + 0.05 * rng.standard_normal((B, L))).astype(np.float32)).cuda()
        starts = R.partial_starts(L)
        stop = (starts[-1] + 160) * 160
        if a.once:
            enc.embed_batch(wav, tile_m=a.tile_m)
            torch.cuda.synchronize()
            continue
        mel = enc.embed_batch(wav, stages=True)["mel"]
        slices = torch.stack([mel[:, s:s + 160] for s in starts], dim=1).reshape(B * len(starts), 160, 40).contiguous()
        padded = torch.nn.functional.pad(wav, (0, max(0, stop - L)))

        def torch_lstm():
            with torch.no_grad():
                _, (hidden, _) = lstm(slices)
                y = torch.relu(lin(hidden[-1]))
                e = (y / torch.norm(y, dim=1, keepdim=True)).view(B, len(starts), 256).mean(dim=1)
                return e / torch.norm(e, dim=1, keepdim=True)

        def torch_mel():
            spec = torch.stft(padded, 400, 160, 400, win, center=True, pad_mode="constant", return_complex=True)
            return (fb @ (spec.real ** 2 + spec.imag ** 2)).transpose(1, 2)

        fns = {"unit, tile_m 32": lambda: enc.embed_batch(wav, tile_m=32), "unit, tile_m 16": lambda: enc.embed_batch(wav, tile_m=16),
               "unit from mels, tile_m 32": lambda: enc.forward(slices, tile_m=32), "unit from mels, tile_m 16": lambda: enc.forward(slices, tile_m=16),
               "torch float32 LSTM (same mels)": torch_lstm, "torch float32 stft + mel": torch_mel}
        res = alternated(fns, a.reps, a.warmup)
        cos = float(E.similarity(enc.embed_batch(wav)["embed"], torch_lstm()).min())
        print(json.dumps({"workload": name, "B": B, "samples": L, "partials": len(starts), "sequences": B * len(starts), "reps": a.reps,
                          "median_ms (min_ms)": {k: f"{v[0]:.3f} ({v[1]:.3f})" for k, v in res.items()}, "min cosine unit vs torch": cos}))


if __name__ == "__main__":
    main()
