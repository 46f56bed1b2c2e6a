#!/usr/bin/env python3
"""Time dynamic time warping on the device (dtts_text2mel_fetch(DTTS_OUT_DTW): distance + path) against two yardsticks:

  * a straightforward anti-diagonal loop in torch on the same device in the same run (float64, the cost matrix by broadcasting or
    torch.cdist(p=1), one masked minimum per diagonal; distance only) — the two sides ALTERNATE call by call;
  * with --reference DIR (a checkout of the reference; needs no GPU together with --host-only): the reference's own utils/dtw.py on the
    host, measured on --host-pairs pairs of each workload and SCALED to the batch (reported as scaled).

Three workloads: one 364-frame F0 pair, 60 F0 pairs of 700 x 700, 60 mel pairs of 700 x 700 x 80.  Device time by an event pair around
each call, median of --reps after --warmup.  Also checks that the torch loop and the unit agree bit for bit.  No gate: figures for
LABNOTES.md.

    python tools/dtw_bench.py [--reps 10] [--warmup 3] [--reference DIR [--host-only] [--host-pairs 2]]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

WORKLOADS = (("f0_sentence", 1, 364, 364, 1), ("f0_batch", 60, 700, 700, 1), ("mel_batch", 60, 700, 700, 80))


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


def inputs(B, N, M, F, rng):
    import dtw_shapes as ds
    if F == 1:
        base = np.clip(0.5 + 0.45 * np.sin(2 * np.pi * np.linspace(0, 1.5, 48)), 0, 1)
        return (np.stack([ds.f0_track(rng, N, base, np.float64) for _ in range(B)]), np.stack([ds.f0_track(rng, M, base, np.float64) for _ in range(B)]))
    walk = lambda n: (np.cumsum(rng.standard_normal((B, n, F)), axis=1) * 0.1 - 3.0).astype(np.float32)
    return walk(N), walk(M)


def torch_dtw(x, y):
    """the anti-diagonal loop: x [B, N(, F)], y [B, M(, F)] on the device -> the distances f64 [B]"""
    if x.dim() == 2:
        C = (x[:, :, None] - y[:, None, :]).abs().to(torch.float64)
    else:
        C = torch.cdist(x.to(torch.float64), y.to(torch.float64), p=1)
    B, N, M = C.shape
    inf = float("inf")
    # row i0 of D0 at index i0; diagonal e = i0 + j0.  Cs[:, e, i0] = C[i0 - 1][e - i0 - 1] where that cell exists, inf elsewhere
    i0 = torch.arange(N + 1, device=C.device)[None, :]
    e = torch.arange(N + M + 1, device=C.device)[:, None]
    j0 = e - i0
    ok = (i0 >= 1) & (j0 >= 1) & (j0 <= M)
    Cs = torch.where(ok[None], C[:, (i0 - 1).clamp(0, N - 1).expand_as(j0), (j0 - 1).clamp(0, M - 1)], torch.full((), inf, dtype=C.dtype, device=C.device))
    prev2 = torch.full((B, N + 1), inf, dtype=C.dtype, device=C.device)
    prev2[:, 0] = 0.0
    prev = torch.full_like(prev2, inf)
    pad = torch.full((B, 1), inf, dtype=C.dtype, device=C.device)
    for d in range(2, N + M + 1):
        up_or_left = torch.minimum(torch.cat([pad, prev[:, :-1]], 1), prev)
        cur = Cs[:, d] + torch.minimum(torch.cat([pad, prev2[:, :-1]], 1), up_or_left)
        prev2, prev = prev, cur
    return prev[:, N]


def host_reference(ref_dir, pairs):
    spec = importlib.util.spec_from_file_location("ref_dtw", os.path.join(ref_dir, "utils", "dtw.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(0)
    for name, B, N, M, F in WORKLOADS:
        x, y = inputs(min(B, pairs), N, M, F, rng)
        t0 = time.perf_counter()
        for b in range(x.shape[0]):
            if F == 1:
                ref.dtw(x[b], y[b], lambda a, c: np.abs(a - c))
            else:
                ref.accelerated_dtw(x[b], y[b], "cityblock")
        per = (time.perf_counter() - t0) / x.shape[0]
        print(json.dumps({"workload": name, "B": B, "N": N, "M": M, "F": F, "host_ref_s_per_pair": per, "host_ref_pairs_measured": int(x.shape[0]),
                          "host_ref_ms_scaled_to_batch": per * B * 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference", default=None, help="a checkout of the reference: also time its utils/dtw.py on the host")
    ap.add_argument("--host-only", action="store_true", help="only the host yardstick (no GPU needed)")
    ap.add_argument("--host-pairs", type=int, default=2)
    a = ap.parse_args()
    if a.reference:
        host_reference(a.reference, a.host_pairs)
    if a.host_only:
        return
    from dict_tts_amd import abi
    ctx = abi.Context()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    for name, B, N, M, F in WORKLOADS:
        xh, yh = inputs(B, N, M, F, rng)
        x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
        dist = torch.empty(B, dtype=torch.float64, device="cuda")
        path = torch.empty(B, 2, N + M - 1, dtype=torch.int32, device="cuda")
        plen = torch.empty(B, dtype=torch.int32, device="cuda")
        kw = dict(x=x.data_ptr(), y=y.data_ptr(), x_ld=N, y_ld=M, F=F, dtype=1 if xh.dtype == np.float64 else 0, dist=dist.data_ptr())
        unit = lambda: ctx.dtw(B, stream, path=path.data_ptr(), path_ld=N + M - 1, path_len=plen.data_ptr(), **kw)
        unit_dist = lambda: ctx.dtw(B, stream, **kw)
        r = alternated({"unit": unit, "unit_dist": unit_dist, "torch": lambda: torch_dtw(x, y)}, a.reps, a.warmup)
        unit()
        same = bool(torch.equal(dist.view(torch.int64), torch_dtw(x, y).view(torch.int64)))
        print(json.dumps({"workload": name, "B": B, "N": N, "M": M, "F": F, "unit_ms_median": r["unit"][0], "unit_ms_min": r["unit"][1],
                          "unit_dist_only_ms_median": r["unit_dist"][0], "torch_loop_ms_median": r["torch"][0], "torch_loop_ms_min": r["torch"][1],
                          "torch_equals_unit_bitwise": same, "mean_path_len": float(plen.float().mean())}))


if __name__ == "__main__":
    main()
