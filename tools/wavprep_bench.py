#!/usr/bin/env python3
"""Time the two waveform-conditioning units on the device — dtts_text2mel_fetch(DTTS_OUT_RESAMPLE), 48000 -> 22050 Hz with kaiser_best, and
dtts_text2mel_fetch(DTTS_OUT_LOUDNESS), measuring and normalising at 22050 Hz — against what else is at hand:

  * on the device, for the K-weighting alone: the same filter applied in the frequency domain by float64 torch.fft (rfft of the zero-padded
    batch, times H(e^jw) of the two biquads, irfft: a circular convolution with the impulse response, which a stable IIR's decay makes
    equal to the recurrence far below its rounding), squares and a cumulative sum for the block powers; torch has no recurrence to offer.
    The two sides ALTERNATE call by call;
  * with --host (needs no GPU together with --host-only): scipy.signal.lfilter twice plus numpy block sums for the loudness, and the float64
    restatement tests/wavprep_ref.py for the resampler (vectorised across outputs), measured on --host-utts utterances and SCALED to the batch.

Two workloads: one 364-frame sentence and 60 utterances of 700 frames (hop 256 at 22050 Hz; the resampler's input is the same duration at
48 kHz).  Device time by an event pair around each call, median of --reps after --warmup.  No gate: figures for LABNOTES.md.

    python tools/wavprep_bench.py [--reps 10] [--warmup 3] [--host [--host-only] [--host-utts 2]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

SR_IN, SR, HOP = 48000, 22050, 256
WORKLOADS = (("sentence", 1, 364), ("batch", 60, 700))


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


def speechlike(rng, L, sr):
    t = np.arange(L, dtype=np.float64) / sr
    f = rng.uniform(100, 250) + rng.uniform(20, 60) * np.sin(2 * np.pi * rng.uniform(1, 4) * t + rng.uniform(0, 6))
    ph = 2 * np.pi * np.cumsum(f) / sr
    env = 0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 2) * t)
    return (0.3 * env * sum(np.sin(k * ph) / k for k in range(1, 4)) + 0.003 * rng.standard_normal(L)).astype(np.float32)


def inputs(B, frames, rng, sr):
    L = int(frames * HOP * sr / SR)
    return np.stack([speechlike(rng, L, sr) for _ in range(B)])


def host(utts):
    from scipy.signal import lfilter
    import wavprep_ref as wr
    from dict_tts_amd import wavprep as W
    rng = np.random.default_rng(0)
    win, nt = W.kaiser_best()
    (bs, as_), (bh, ah) = W.k_weighting(SR)
    for name, B, frames in WORKLOADS:
        n = min(B, utts)
        x48, x22 = inputs(n, frames, rng, SR_IN), inputs(n, frames, rng, SR)
        t0 = time.perf_counter()
        for b in range(n):
            wr.resample(x48[b], SR_IN, SR, win, nt)
        t_rs = (time.perf_counter() - t0) / n
        t0 = time.perf_counter()
        for b in range(n):
            y = lfilter(bh, ah, lfilter(bs, as_, x22[b].astype(np.float64)))
            z = [np.sum(np.square(y[lo:hi])) for lo, hi in W.block_bounds(SR, W.n_blocks_of(len(y), SR))]
            wr.gate(np.array(z) / (0.4 * SR))
        t_ld = (time.perf_counter() - t0) / n
        print(json.dumps({"workload": name, "B": B, "frames": frames, "host_utterances_measured": n, "host_resample_restatement_ms_scaled_to_batch": t_rs * B * 1e3,
                          "host_lfilter_loudness_ms_scaled_to_batch": t_ld * B * 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the host yardsticks")
    ap.add_argument("--host-only", action="store_true", help="only the host yardsticks (no GPU needed)")
    ap.add_argument("--host-utts", type=int, default=2)
    a = ap.parse_args()
    if a.host or a.host_only:
        host(a.host_utts)
    if a.host_only:
        return
    from dict_tts_amd import abi
    from dict_tts_amd import wavprep as W
    ctx = abi.Context()
    rs, ln = W.Resampler(SR_IN, SR, ctx=ctx), W.Loudness(SR, ctx=ctx)
    (bs, as_), (bh, ah) = W.k_weighting(SR)
    rng = np.random.default_rng(0)
    for name, B, frames in WORKLOADS:
        x48 = torch.from_numpy(inputs(B, frames, rng, SR_IN)).cuda()
        x22 = torch.from_numpy(inputs(B, frames, rng, SR)).cuda()
        L = x22.shape[1]
        n_fft = 1 << int(np.ceil(np.log2(L + SR)))       # one second of room for the tail: the high pass has decayed by e^-230 there
        w = torch.exp(-2j * np.pi * torch.arange(n_fft // 2 + 1, dtype=torch.float64, device="cuda") / n_fft)
        H = torch.ones_like(w)
        for b_, a_ in ((bs, as_), (bh, ah)):
            H = H * (b_[0] + b_[1] * w + b_[2] * w * w) / (a_[0] + a_[1] * w + a_[2] * w * w)
        bd = torch.from_numpy(W.block_bounds(SR, W.n_blocks_of(L, SR))).cuda()

        def fft_loudness():
            y = torch.fft.irfft(torch.fft.rfft(x22.to(torch.float64), n=n_fft) * H, n=n_fft)[:, :L]
            c = torch.nn.functional.pad(torch.cumsum(y * y, dim=1), (1, 0))
            return (c[:, bd[:, 1].clamp(max=L)] - c[:, bd[:, 0]]) / (0.4 * SR)

        r = alternated({"resample": lambda: rs(x48), "measure": lambda: ln.measure(x22), "normalize": lambda: ln.normalize(x22, check=False),
                        "fft_blocks": fft_loudness}, a.reps, a.warmup)
        st = ln.measure(x22, stages=True)
        dz = float(((fft_loudness() - st["z"]).abs() / st["z"].abs().amax(dim=1, keepdim=True)).max())
        out = {"workload": name, "B": B, "frames": frames, "samples_in_48k": int(x48.shape[1]), "samples_22k": int(L), "fft_n": n_fft,
               "fft_blocks_minus_unit_z_max_rel": dz, "lufs_mean": float(st["lufs"].mean())}
        for k, v in r.items():
            out[f"{k}_ms_median"], out[f"{k}_ms_min"] = v
        print(json.dumps(out))


if __name__ == "__main__":
    main()
