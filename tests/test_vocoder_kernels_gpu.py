"""The fused vocoder kernels (vpair.hip, rblock.hip, vconv.hip) sample by sample against the rounding-point emulator
(tests/vocoder_emul.py), which rounds where the kernels round and computes everything else in float64, with per-sample,
256-sample-window and global bounds (vocoder_emul.BOUNDS) instead of the waveform gate's global RMS alone.

Measured on MI355X (worst over all shapes; GPU - emulator beside GPU - oracle, max / window / RMS):
  isolating, f16 / release / bit 15:   9.7e-5 / 2.1e-5 / 2.1e-5   vs   1.3e-4 / 3.4e-5 / 3.4e-5   -> bounds 2.4e-4 / 6.3e-5 / 6.3e-5
  isolating, bf16:                     1.1e-3 / 2.7e-4 / 2.7e-4   vs   2.6e-3 / 7.8e-4 / 7.8e-4   -> bounds 3.1e-3 / 7.3e-4 / 7.3e-4
  four-stage, f16 / release / 15 / 13: 2.9e-4 / 6.5e-5 / 5.7e-5   vs   3.6e-4 / 9.2e-5 / 8.2e-5   -> bounds 8.6e-4 / 1.9e-4 / 1.7e-4
  four-stage, bf16:                    3.5e-3 / 8.9e-4 / 7.5e-4   vs   5.5e-3 / 1.3e-3 / 1.2e-3   -> bounds 1.0e-2 / 2.7e-3 / 2.2e-3
In the fp16 mode GPU - emulator is NOT far below GPU - oracle (0.25-0.97 of it per utterance): computing the emulator in fp32 instead
of fp64 moves it by as much (tests/test_vocoder_emul_cpu.py), i.e. fp32 summation order re-draws the fp16 rounding decisions of the
whole chain; every alternative restatement of a rounding point tried (leaky_relu before the conversion, slope 0.1 instead of fp16(0.1),
exact serial convolutions) moved the emulator further from the GPU.  The bf16 mode's rounding points dominate its error (<= 0.44).
The k = 5 / 9 generators with dilation sums above 9 found the rblock halo defect fixed with them (GPU - emulator 3.8e-4 at the tile
edges before, within the bounds after).

Isolating generators have ONE upsampler (rate 2), so that one stage's ResBlock kernels feed conv_post directly; their
stage rows are the waveform's samples.  Shapes come from the launchers' tile rules (``rblock_tile`` / ``vpair_tile``
restate rblock.hip rb_launch_el / vpair.hip vpair_launch_el): B = 1 (half-size tiles, ``few()``), B = 1 over several
tiles, and a ragged batch of DTTS_MAX_VOCODER_BATCH utterances (several tiles per persistent workgroup) whose lengths put the last tile at 2 rows, exactly
full, or full - 2 (the hop of 2 is the finest step an utterance length can take).

Every measured value is printed as a ``VOCMEAS {json}`` line (run with -s to see them)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from dict_tts_amd import abi, synth, vocoder
from oracle import hifigan_ref as href
from vocoder_emul import BOUNDS, Emulator, seam_check

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
SEED = 1234
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as _f:
    MAX_BATCH = int(re.search(r"#define DTTS_MAX_VOCODER_BATCH (\d+)", _f.read()).group(1))   # utterances per call in the fused modes


def _iso(c0, rk, rd):
    return {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": rk, "resblock_dilation_sizes": rd}


D135 = [[1, 3, 5]] * 3
CONFIGS = {
    # C = 256 / 128: vpair at k = 7 / 11 (one launch per iteration, fp16 stream between them), rblock at k = 3
    "c256": _iso(512, [3, 7, 11], D135),
    "c128": _iso(256, [3, 7, 11], D135),
    # C = 64: rblock 512-row tiles at k = 3, 640-row tiles at k >= 7, 256-row half-size tiles
    "c64": _iso(128, [3, 7, 11], D135),
    # C = 32: rblock 1024-row tiles (k >= 7) with conv_post + tanh fused into the last ResBlock (k = 11)
    "c32": _iso(64, [3, 7, 11], D135),
    # C = 32: the fused conv_post on the 512-row k = 3 tile; k = 9 with other dilations
    "c32_k3post": _iso(64, [11, 9, 3], [[1, 3, 5], [1, 2, 4], [2, 3, 4]]),
    # k = 5 / 9 and dilations other than (1, 3, 5) on both kernel families
    "c128_k59": _iso(256, [5, 9, 3], [[2, 4, 5], [1, 2, 3], [3, 5, 5]]),
    "c64_k59": _iso(128, [5, 9, 3], [[2, 4, 5], [1, 2, 3], [1, 1, 1]]),
}
MODES = {   # name -> (HifiGAN precision, range_guard, tune_flags, emulator options)
    "f16": ("f16", True, 0, dict(mode="f16")),
    "f16_release": ("f16", False, 0, dict(mode="f16")),
    "bf16": ("bf16", False, 0, dict(mode="bf16")),
    "f16_bit15": ("f16", True, 1 << 15, dict(mode="f16", stream16=False)),
    "f16_bit13": ("f16", True, 1 << 13, dict(mode="f16", h2=True)),
}


# ------------------------------------------------------------------------------------------------ tile rules
def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


def _rb_lds(C, W, WT, TT, wav):
    """rblock.hip rb_lds_bytes: dynamic LDS of a configuration without the tile table"""
    act = (W + 2 * 40) * (C * 2 + 16)
    stage = WT * 32 * (C * 4 + 16)
    return (max(TT * C * 4, act) if wav else act) + stage


def rblock_tile(C, k, dils, B, L, wav, cus):
    """rblock.hip rb_launch_el / rb_launch_cfg (single-ResBlock launches): -> output rows per tile (TT, with the fused conv_post TT - 6).
    A persistent configuration whose LDS cannot also hold the tile table of B utterances (12 B each) falls through to the next one."""
    halo = max(6 * (k - 1), (k - 1) // 2 * (sum(dils) + 3))   # rblock.h rblock_halo_of

    def tt(W):
        return W - 2 * halo - (6 if wav else 0)

    def few(W):
        return tt(W) >= 32 and 2 * B * _cdiv(L, tt(W)) <= cus

    def fits(W, WT, PS):
        return _rb_lds(C, W, WT, W - 2 * halo, wav) + (3 * B + 2) * 4 * PS <= 160 * 1024
    if C == 32:
        chain = [(1024, 8, 1)] if (k >= 7 and not few(1024)) else []
        chain += [(512, 4, 0)]
    elif C == 64:
        chain = [(256, 2, 1)] if few(512) else ([(640, 4, 1)] if k >= 7 else []) + [(512, 4, 1), (256, 2, 1)]
    elif C == 128:
        chain = [(128, 1, 1)] if few(256) else [(256, 2, 1), (128, 1, 1)]
    else:
        chain = [(64, 1, 1)] if few(128) else [(128, 1, 1), (64, 1, 1)]
    for W, WT, PS in chain:
        if fits(W, WT, PS):
            break
    return tt(W)


def vpair_tile(C, k, d, B, L, cus):
    """vpair.hip vpair_launch_el: -> valid rows per tile (TT - (k - 1))"""
    def tiles(tt):
        return B * _cdiv(L, tt - (k - 1))
    if C == 256:
        if 2 * tiles(128) <= cus:
            TT = 64
        else:
            lds = lambda tt: (tt + d * (k - 1) + max(d + 1, 4)) * (256 * 2 + 16) + (3 * B + 2) * 4
            TT = 96 if (2 * lds(128) > 160 * 1024 and 2 * lds(96) <= 160 * 1024) else 128
    else:
        if 2 * tiles(256) <= cus:
            TT = 128
        else:
            big = ((256 + d * (k - 1) + max(d + 1, 8)) * (128 * 2 + 16) + (3 * B + 2) * 4) * 2 <= 160 * 1024
            TT = 256 if big else 192
    return TT - (k - 1)


def stage_tiles(cfg, B, L, cus):
    """{launch description: output rows per tile} for the LAST stage's ResBlock launches (L = padded stage length)"""
    C = cfg["upsample_initial_channel"] >> len(cfg["upsample_rates"])
    nk = len(cfg["resblock_kernel_sizes"])
    out = {}
    for j, (k, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
        if C <= 64 or k == 3:
            wav = C == 32 and j == nk - 1
            out[f"rblock<{C}> k={k}{' +post' if wav else ''}"] = rblock_tile(C, k, dils, B, L, wav, cus)
        else:
            for m, d in enumerate(dils):
                out[f"vpair<{C}> k={k} it{m} d={d}"] = vpair_tile(C, k, d, B, L, cus)
    return out


def seam_lengths(cfg, B, n, hop, cus, guess):
    """stage lengths n * s - 2, n * s, n * s + 2 for every distinct tile step s of the last stage at batch size B"""
    steps = sorted(set(stage_tiles(cfg, B, guess, cus).values()))
    out = []
    for s in steps:
        for delta in (-2, 0, 2):
            L = n * s + delta
            if L > 0 and L % hop == 0:
                out.append(L // hop)
    return sorted(set(out))


# ------------------------------------------------------------------------------------------------ helpers
_SD = {}


def _sd(name):
    if name not in _SD:
        cfg = synth.hifigan_config() if name == "full" else CONFIGS[name]
        raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
        _SD[name] = (cfg, raw, href.fold_weight_norm(raw))
    return _SD[name]


def _model(name, mode, unfused=False):
    cfg, raw, _ = _sd(name)
    precision, guard, tune, _ = MODES[mode]
    return vocoder.HifiGAN(state_dict=raw, config={**cfg, "dtts_tune_flags": tune}, precision=precision, range_guard=guard,
                           unfused=unfused)


def _emulate(name, mode, mel):
    cfg, _, fsd = _sd(name)
    return Emulator(fsd, cfg, **MODES[mode][3]).spec2wav(mel)


def _mel(seed, n, tag):
    return synth.random_mel(seed, n, tag)


def _report(got, want, tiles, utt):
    """the worst sample: its utterance, last-stage row (= sample: conv_post keeps the rate) and the row's offset inside its tile"""
    i = int(np.abs(np.asarray(got, np.float64) - want).argmax())
    return {"utt": utt, "row": i, "offset_in_tile": {k: i % s for k, s in tiles.items()}}


def _check_utts(name, mode, model, mels, lens_cases, oracle=False):
    """run every list of mels in lens_cases as one batch, compare each utterance with the emulator; returns the measured table rows"""
    cfg = _sd(name)[0]
    hop = model.hop
    cus = _cus()
    bounds = BOUNDS[("full_" if name == "full" else "") + ("bf16" if mode == "bf16" else "f16")]
    rows, failures = [], []
    for case, idx in lens_cases:
        ms = [mels[i] for i in idx]
        lens = [m.shape[0] for m in ms]
        Tm = max(lens)
        batch = np.zeros((len(ms), Tm, 80), np.float32)
        for b, m in enumerate(ms):
            batch[b, :lens[b]] = m
        full = model.forward_batch(T(batch).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
        assert not model.overflowed()
        assert np.isfinite(full).all() and float(np.abs(full).max()) <= 1.0, case   # every utterance, emulated or not
        tiles = stage_tiles(cfg, len(ms), Tm * hop, cus)
        worst = None
        for b, n in enumerate(lens):
            assert float(np.abs(full[b, n * hop:]).max(initial=0.0)) == 0.0, (case, b)   # exact zeros past lens * hop
            if b not in _emulated(len(ms)):
                continue
            g = full[b, :n * hop]
            assert np.isfinite(g).all()
            assert np.mean(np.abs(g) > 0.9) < 0.01, "tanh saturation would hide errors"
            e = _emulate(name, mode, ms[b])
            vals, fails = seam_check(g, e, bounds)
            rec = {"config": name, "mode": mode, "case": case, "B": len(ms), "utt": b, "samples": n * hop,
                   "emu": {k: vals[k] for k in ("max", "win", "rms")}}
            if oracle:
                ref = href.spec2wav(_sd(name)[2], cfg, ms[b]).numpy()
                rec["oracle"] = {k: seam_check(g, ref, {})[0][k] for k in ("max", "win", "rms")}
                rec["oracle"]["abs_rms_delta"] = abs(rms(g) - rms(ref))
            print("VOCMEAS " + json.dumps(rec), flush=True)
            rows.append(rec)
            if fails:
                failures.append((fails, vals, _report(g, e, tiles, b), case, lens[b]))
            if worst is None or vals["max"] > worst:
                worst = vals["max"]
    assert not failures, f"{name} / {mode}: GPU vs emulator beyond {bounds}: " + "; ".join(
        f"{c} len {n}: {f} {v} worst {r}" for f, v, r, c, n in failures[:6])
    return rows


def _emulated(B):
    """the utterances of a batch that are compared with the emulator (all of a small batch; of a large one the seam-length ones, which
    come first, and the first / middle / last filler)"""
    if B <= 24:
        return set(range(B))
    return set(range(24)) | {B // 2, B - 1}


# ------------------------------------------------------------------------------------------------ isolating generators
ISO_MODES = [(c, m) for c in CONFIGS for m in ("f16", "f16_release", "bf16")] + \
            [(c, "f16_bit15") for c in ("c256", "c128", "c128_k59")]


@pytest.mark.parametrize("name,mode", ISO_MODES)
def test_isolating_generator_vs_emulator(name, mode):
    cfg = CONFIGS[name]
    model = _model(name, mode)
    assert model.precision == abi.VOC_PRECISIONS[MODES[mode][0]]
    hop, cus = model.hop, _cus()
    # B = 1: short (half-size tiles) and over two tiles + a seam remainder, for every tile step of the stage
    b1 = [20] + seam_lengths(cfg, 1, 2, hop, cus, 400)
    # ragged batch: every seam length at the full-size tiles, then fillers of one full tile each so that every persistent
    # workgroup walks several tiles
    B_rag = MAX_BATCH   # (the persistent launches' tile tables at their largest: rblock_tile's fall-through)
    rag = seam_lengths(cfg, B_rag, 1, hop, cus, 4096)
    fill_len = max(rag)   # the longest seam length: two tiles of the widest step
    n_fill = B_rag - len(rag)
    mels = [_mel(700 + i, n, f"iso{n}") for i, n in enumerate(b1)]
    rmels = [_mel(900 + i, n, f"rag{n}") for i, n in enumerate(rag)] + [_mel(5000 + i, fill_len, "fill") for i in range(n_fill)]
    if mode == "f16":
        print(f"\n[{name}] tiles B=1: {stage_tiles(cfg, 1, max(b1) * hop, cus)}  ragged B={len(rmels)}: "
              f"{stage_tiles(cfg, len(rmels), fill_len * hop, cus)}", flush=True)
    rows = _check_utts(name, mode, model, mels, [(f"B=1 len={n}", [i]) for i, n in enumerate(b1)],
                       oracle=mode != "f16_release")
    rows += _check_utts(name, mode, model, rmels, [("ragged", list(range(len(rmels))))])
    if mode == "bf16":
        # bf16 operands: the emulator's rounding points carry most of the error (measured GPU - emulator <= 0.44 x GPU - oracle per utterance)
        for r in rows:
            if "oracle" in r:
                assert r["emu"]["rms"] < 0.6 * r["oracle"]["rms"], r


# ------------------------------------------------------------------------------------------------ the full generator
FULL_CASES = {"f16": [[40], [17, 64, 33]], "f16_release": [[40], [17, 64, 33]], "bf16": [[17, 64, 33]], "f16_bit15": [[40]],
              "f16_bit13": [[40]]}


@pytest.mark.parametrize("mode", list(FULL_CASES))
def test_full_generator_vs_emulator(mode):
    """the default four-stage generator (conv_pre, 4 polyphase upsamplers, vpair + rblock stages, fused conv_post); bit 13 (two-product
    fp16 ups.1) with the default fp16 stream also inside the waveform gate against the oracle"""
    model = _model("full", mode)
    cfg, _, fsd = _sd("full")
    groups = FULL_CASES[mode]
    mels, cases = [], []
    for g in groups:
        idx = []
        for n in g:
            idx.append(len(mels))
            mels.append(_mel(40 + n, n, "full"))
        cases.append((f"B={len(g)} lens={g}", idx))
    rows = _check_utts("full", mode, model, mels, cases, oracle=mode != "f16_release")
    if mode.startswith("f16"):
        for r in rows:   # the waveform gate (BASELINE.json: RMS(gpu - ref) and |RMS(gpu) - RMS(ref)| <= 1e-4) in every fp16 form
            if "oracle" in r:
                assert r["oracle"]["rms"] <= 1e-4 and r["oracle"]["abs_rms_delta"] <= 1e-4, r


@pytest.mark.parametrize("mode", ["f16", "f16_release", "bf16"])
def test_full_generator_at_the_largest_batch(mode):
    """DTTS_MAX_VOCODER_BATCH short utterances in one call.  The persistent ResBlock launches keep a tile table of 12 B per utterance in
    LDS: with it the fused-conv_post 1024-row tile (C = 32) no longer fits above ~940 utterances, the 128-row k = 3 tile of C = 256 above
    ~1730; the launcher falls through to the next configuration that fits (such a call used to fail with DTTS_E_HIP)."""
    rng = np.random.RandomState(11)
    lens = [int(v) for v in rng.randint(1, 7, size=MAX_BATCH)]
    mels = [_mel(20000 + i, n, "bmax") for i, n in enumerate(lens)]
    cfg = _sd("full")[0]
    print(f"\n[B={MAX_BATCH}] last-stage tiles: {stage_tiles(cfg, MAX_BATCH, max(lens) * 256, _cus())}", flush=True)
    _check_utts("full", mode, _model("full", mode), mels, [(f"B={MAX_BATCH}", list(range(MAX_BATCH)))])


# ------------------------------------------------------------------------------------------------ every sample is written
@pytest.mark.parametrize("precision,unfused", [("f16", False), ("bf16", False), ("bf16x3", False), ("bf16", True)])
@pytest.mark.parametrize("name", ["full", "c256"])
def test_every_sample_is_written(name, precision, unfused):
    """dtts_hifigan_forward into a NaN-filled waveform: with lens = NULL no sample is cleared beforehand, so every one
    must come from a kernel; with short lens the samples past lens * hop are exact zeros"""
    cfg, raw, _ = _sd(name)
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision, unfused=unfused)
    hop = model.hop
    lens = [40, 17, 64, 1]
    Tm = max(lens)
    mel = np.zeros((len(lens), Tm, 80), np.float32)
    for b, n in enumerate(lens):
        mel[b] = _mel(60 + b, Tm, "nan")
    mel_d = T(mel).cuda()
    stream = torch.cuda.current_stream()
    for short in (False, True):
        wav = torch.full((len(lens), Tm * hop), float("nan"), dtype=torch.float32, device="cuda")
        lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda") if short else None
        model.ctx.hifigan_forward(mel_d.data_ptr(), lens_d.data_ptr() if short else None, len(lens), Tm, wav.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        w = wav.cpu().numpy()
        assert np.isfinite(w).all(), (name, precision, unfused, short, int((~np.isfinite(w)).sum()))
        if short:
            for b, n in enumerate(lens):
                assert float(np.abs(w[b, n * hop:]).max(initial=0.0)) == 0.0, (b, n)
                assert float(np.abs(w[b, :n * hop]).max()) > 0.0
