#!/usr/bin/env python3
"""Time the F0 extraction on the device (dtts_text2mel_fetch(DTTS_OUT_PITCH): the whole call, four launches) against two yardsticks:

  * for the autocorrelation stage alone: the same windowed frames through batched float64 torch.fft.rfft -> |.|^2 -> irfft on the same
    device in the same run (the frames are prepared outside the timed span, which favours the FFT); the two sides ALTERNATE call by call;
  * with --host (needs no GPU together with --host-only): the float64 restatement tests/pitch_ref.py on the host for the whole pipeline,
    measured on --host-utts utterances of each workload and SCALED to the batch (reported as scaled).

Two workloads at the reference's parameters (22050 Hz, hop 256, 80 .. 750 Hz): one 364-frame sentence, and 60 utterances of 700 frames.
Device time by an event pair around each call, median of --reps after --warmup.  Also reports how far the FFT's autocorrelation is from
the unit's.  The per-kernel split comes from running this tool under a kernel trace.  No gate: figures for LABNOTES.md.

    python tools/pitch_bench.py [--reps 10] [--warmup 3] [--host [--host-only] [--host-utts 2]]
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

SR, HOP = 22050, 256
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


def speechlike(rng, L):
    """voiced stretches (a gliding three-harmonic tone) between noisy and silent ones"""
    t = np.arange(L, dtype=np.float64) / SR
    f = rng.uniform(100, 250) + rng.uniform(20, 60) * np.sin(2 * np.pi * rng.uniform(1, 4) * t + rng.uniform(0, 6))
    ph = 2 * np.pi * np.cumsum(f) / SR
    x = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 4)) + 0.003 * rng.standard_normal(L)
    pos = 0
    while pos < L:
        seg = int(rng.uniform(0.1, 0.5) * SR)
        kind = rng.integers(0, 4)
        if kind == 0:
            x[pos:pos + seg] = 0.05 * rng.standard_normal(len(x[pos:pos + seg]))
        elif kind == 1:
            x[pos:pos + seg] = 0.0
        pos += seg
    return x.astype(np.float32)


def inputs(B, frames, rng):
    L = (frames + 3) * HOP
    return np.stack([speechlike(rng, L) for _ in range(B)])


def host(utts):
    import pitch_ref as pr
    p = pr.params(SR, HOP, 80.0, 750.0)
    rng = np.random.default_rng(0)
    for name, B, frames in WORKLOADS:
        wav = inputs(min(B, utts), frames, rng)
        t0 = time.perf_counter()
        for b in range(wav.shape[0]):
            pr.pitch(wav[b], p)
        per = (time.perf_counter() - t0) / wav.shape[0]
        print(json.dumps({"workload": name, "B": B, "frames": frames, "host_restatement_s_per_utterance": per, "host_utterances_measured": int(wav.shape[0]),
                          "host_restatement_ms_scaled_to_batch": per * B * 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the float64 restatement on the host")
    ap.add_argument("--host-only", action="store_true", help="only the host yardstick (no GPU needed)")
    ap.add_argument("--host-utts", type=int, default=2)
    a = ap.parse_args()
    if a.host or a.host_only:
        host(a.host_utts)
    if a.host_only:
        return
    from dict_tts_amd import abi
    from dict_tts_amd import pitch as P
    ctx = abi.Context()
    ex = P.PitchAC(ctx)
    g = ex.geo
    nsw, n_lag, half = g["nsw"], g["n_lag"], g["half"]
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    n_fft = 1 << int(np.ceil(np.log2(nsw + n_lag)))
    w = torch.from_numpy(0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(nsw) + 1.0) / (nsw + 1))).cuda()
    for name, B, frames in WORKLOADS:
        wav = torch.from_numpy(inputs(B, frames, rng)).cuda()
        L = wav.shape[1]
        nF = ex.frames(L)
        assert nF == frames
        f0 = torch.empty(B, nF, dtype=torch.float64, device="cuda")
        nfr = torch.empty(B, dtype=torch.int32, device="cuda")
        acf = torch.empty(B, nF, n_lag, dtype=torch.float64, device="cuda")
        kw = dict(wav=wav.data_ptr(), wav_ld=L, frames_ld=nF, f0=f0.data_ptr(), n_frames=nfr.data_ptr(), sample_rate=SR, hop=HOP)
        unit = lambda: ctx.pitch(B, stream, **kw)
        # the FFT yardstick's frames: the unit's own geometry, local mean taken out, windowed (outside the timed span)
        left0 = (L - nF * HOP + HOP - 1) // 2
        fr = wav.to(torch.float64)[:, left0 + 1 - half:].unfold(1, nsw, HOP)[:, :nF]
        lo, hi = half - g["nper"], half - 1 + g["nper"]
        fr = ((fr - fr[:, :, lo:hi + 1].mean(-1, keepdim=True)) * w).reshape(B * nF, nsw).contiguous()

        def fft_acf():
            s = torch.fft.rfft(fr, n=n_fft)
            return torch.fft.irfft(s.real * s.real + s.imag * s.imag, n=n_fft)[:, :n_lag]

        r = alternated({"unit": unit, "fft_acf": fft_acf}, a.reps, a.warmup)
        ctx.pitch(B, stream, acf=acf.data_ptr(), **kw)
        ac = fft_acf()
        # a frame whose centre is silent (localPeak == 0) has by definition r = 0 behind lag 0 in the unit, whatever its edges hold
        live = (ac[:, 0] > 1e-9) & (acf.reshape(B * nF, n_lag)[:, 1:] != 0).any(1)
        _, wr = __import__("pitch_ref").tables(nsw)
        rr = ac[live] / (ac[live][:, :1] * torch.from_numpy(wr).cuda())
        diff = float((rr - acf.reshape(B * nF, n_lag)[live]).abs().max())
        voiced = float((f0 > 0).double().mean())
        print(json.dumps({"workload": name, "B": B, "frames": nF, "unit_ms_median": r["unit"][0], "unit_ms_min": r["unit"][1],
                          "fft_acf_ms_median": r["fft_acf"][0], "fft_acf_ms_min": r["fft_acf"][1], "fft_n": n_fft,
                          "fft_acf_minus_unit_acf_max": diff, "voiced_fraction": voiced}))


if __name__ == "__main__":
    main()
