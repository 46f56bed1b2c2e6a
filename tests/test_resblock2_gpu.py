"""HifiGAN generators built from ResBlock2 (``resblock: "2"``, the V3 family) on the GPU: the fused kernel rb2x.hip, the
per-convolution paths and the public interface around them.

Per-sample comparisons are against the rounding emulator (tests/resblock2_emul.py) and the float64 reference
(tests/resblock2_ref.py), never against another GPU path; bounds are resblock2_emul.BOUNDS_RB2 (<= 3x the worst value measured
on an MI355X over the group's shapes, never above ResBlock1's bound of the same group).

Measured on MI355X (worst over all shapes of the group; GPU - emulator beside GPU - float64 reference, max / window / RMS):
  isolating, f16 / release (648 utterances): 5.4e-5 / 9.3e-6 / 8.3e-6   vs   1.7e-4 / 5.4e-5 / 5.1e-5   -> bounds 1.6e-4 / 2.8e-5 / 2.5e-5
  isolating, bf16 (327):                     8.4e-4 / 2.2e-4 / 2.2e-4   vs   3.6e-3 / 1.2e-3 / 1.1e-3   -> bounds 2.5e-3 / 6.5e-4 / 6.5e-4
  V3, f16 / release (60):                    2.3e-4 / 6.0e-5 / 4.9e-5   vs   4.6e-4 / 1.1e-4 / 9.7e-5   -> bounds 6.8e-4 / 1.8e-4 / 1.4e-4
  V3, bf16 fused and per convolution (35):   4.2e-3 / 1.1e-3 / 8.9e-4   vs   1.1e-2 / 2.4e-3 / 2.1e-3   -> bounds 1.0e-2 / 2.7e-3 / 2.2e-3 (ResBlock1's: the cap)
  V3 waveform gate on g6_mel against g13 (RMS(gpu - ref), |RMS(gpu) - RMS(ref)|): f16 9.46e-5, 1.6e-5; bf16x3 3.3e-6, 1.0e-8;
  bf16 1.68e-3, 2.0e-4; bf16 per convolution 2.01e-3, 3.3e-4.  The f16 figure is the emulator's (9.43e-5, tests/test_resblock2_cpu.py:
  most of it is made in the last stage, where every fp16 rounding reaches conv_post directly), not a kernel defect: GPU - emulator is
  4.9e-5 there.  Every value is printed as a ``VOCMEAS {json}`` line (run with -s).

Isolating generators have ONE upsampler (rate 2), so that one stage's three ResBlock2 launches feed conv_post directly.  Shapes come
from the kernel's tile rule (tests/rb2x_shapes.py restates rb2x.h / rb2x.hip): B = 1 short, B = 1 over several tiles, and a ragged batch
of DTTS_MAX_VOCODER_BATCH utterances whose lengths put the last tile at 2 rows, exactly full, or full - 2."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import golden_cases as gc
import rb2x_shapes as shp
import resblock2_ref as r2
from dict_tts_amd import abi, synth, vocoder
from oracle import hifigan_ref as href
from resblock2_emul import BOUNDS_RB2, Emulator2
from vocoder_emul import seam_check

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
SEED = 1234
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as _f:
    MAX_BATCH = int(re.search(r"#define DTTS_MAX_VOCODER_BATCH (\d+)", _f.read()).group(1))
V3 = synth.hifigan_config_v3()
V3_K, V3_D = V3["resblock_kernel_sizes"], V3["resblock_dilation_sizes"]


def _iso(c0, rk, rd):
    return {"resblock": "2", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": rk, "resblock_dilation_sizes": [list(d) for d in rd]}


CONFIGS = {
    # V3's three kernels at each width; at C = 32 the fused conv_post sits on the largest-halo kernel (k = 7, (3, 12): 1024-row tiles)
    "r256": _iso(512, V3_K, V3_D),
    "r128": _iso(256, V3_K, V3_D),
    "r64": _iso(128, V3_K, V3_D),
    "r32": _iso(64, V3_K, V3_D),
    # the fused conv_post on the smallest-halo kernel (k = 3, (1, 2): 512-row tiles)
    "r32_k3post": _iso(64, V3_K[::-1], V3_D[::-1]),
    # k = 9 / 11, the pair (1, 1), and the largest pair the predicate admits at that width and kernel size
    "r64_k911": _iso(128, [9, 11, 3], [[1, 1], [2, 3], shp.largest_pair(64, 3)]),
    "r128_k911": _iso(256, [11, 9, 5], [[1, 1], [3, 2], shp.largest_pair(128, 5)]),
    "r256_big": _iso(512, [3, 9, 7], [[1, 1], shp.largest_pair(256, 9), shp.largest_pair(256, 7)]),
    "r32_big": _iso(64, [5, 11, 3], [[4, 1], shp.largest_pair(32, 11), [1, 1]]),
}
MODES = {   # name -> (HifiGAN precision, range_guard, emulator mode)
    "f16": ("f16", True, "f16"),
    "f16_release": ("f16", False, "f16"),
    "bf16": ("bf16", False, "bf16"),
}

_SD = {}


def _sd(name):
    if name not in _SD:
        cfg = V3 if name == "v3" else CONFIGS[name]
        raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
        _SD[name] = (cfg, raw, href.fold_weight_norm(raw))
    return _SD[name]


def _model(name, mode, unfused=False, **extra):
    cfg, raw, _ = _sd(name)
    precision, guard, _ = MODES[mode]
    return vocoder.HifiGAN(state_dict=raw, config={**cfg, **extra}, precision=precision, range_guard=guard, unfused=unfused)


def _gate(got, ref, rec):
    rec.update(rms_diff=rms(np.asarray(got, np.float64) - ref), abs_rms_delta=abs(rms(got) - rms(ref)))
    print("VOCMEAS " + json.dumps(rec), flush=True)
    return rec


def seam_lengths(cfg, B, n, hop):
    """mel lengths that put the last tile of every ResBlock2 launch of the stage at 2 rows short of n tiles, exactly n, and 2 over"""
    out = []
    for s in sorted(set(shp.stage_tiles(cfg, B).values())):
        for delta in (-2, 0, 2):
            L = n * s + delta
            if L > 0 and L % hop == 0:
                out.append(L // hop)
    return sorted(set(out))


def _emulated(B):
    return set(range(B)) if B <= 24 else set(range(24)) | {B // 2, B - 1}


def _check_utts(name, mode, model, mels, lens_cases, group, fused_post=None):
    cfg, _, fsd = _sd(name)
    hop, bounds = model.hop, BOUNDS_RB2[group]
    emu = Emulator2(fsd, cfg, mode=MODES[mode][2], fused_post=fused_post)
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
        tiles = shp.stage_tiles(cfg, len(ms))
        for b, n in enumerate(lens):
            assert float(np.abs(full[b, n * hop:]).max(initial=0.0)) == 0.0, (case, b)   # exact zeros past lens * hop
            if b not in _emulated(len(ms)):
                continue
            g = full[b, :n * hop]
            assert np.mean(np.abs(g) > 0.9) < 0.01, "tanh saturation would hide errors"
            vals, fails = seam_check(g, emu.spec2wav(ms[b]), bounds)
            ref = r2.spec2wav(fsd, cfg, ms[b])
            rec = {"config": name, "mode": mode, "case": case, "B": len(ms), "utt": b, "samples": n * hop,
                   "emu": {k: vals[k] for k in ("max", "win", "rms")},
                   "oracle": {k: seam_check(g, ref, {})[0][k] for k in ("max", "win", "rms")}}
            print("VOCMEAS " + json.dumps(rec), flush=True)
            rows.append(rec)
            if fails:
                i = vals["argmax"]
                failures.append((fails, vals, {k: i % s for k, s in tiles.items()}, case, lens[b]))
    assert not failures, f"{name} / {mode}: GPU vs emulator beyond {bounds}: " + "; ".join(
        f"{c} len {n}: {f} {v} offset in tile {r}" for f, v, r, c, n in failures[:6])
    return rows


# ------------------------------------------------------------------------------------------------ 1. the waveform gate
@pytest.mark.parametrize("precision,unfused", [("f16", False), ("bf16x3", False), ("bf16", False), ("bf16", True)])
def test_v3_waveform_gate(golden_dir, precision, unfused):
    """spec2wav(g6_mel) of the synthetic V3 generator against the golden taken from the reference implementation.  BASELINE.json
    north_star: RMS(gpu - ref) and |RMS(gpu) - RMS(ref)| <= 1e-4 for f16 and bf16x3; bf16 has no project gate: the per-sample bounds of
    the full-generator group against the float64 reference's emulator (test_v3_vs_emulator)."""
    g = np.load(os.path.join(golden_dir, "g13_hifigan_rb2.npz"))
    cfg, raw, fsd = _sd("v3")
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision, unfused=unfused)
    assert model.hop == 256 and model.precision == abi.VOC_PRECISIONS[precision]
    mel = gc.g6_mel()
    wav = model.spec2wav(mel)
    assert wav.shape == g["wav"].shape and np.isfinite(wav).all()
    rec = _gate(wav, g["wav"].astype(np.float64), {"test": "v3_gate", "precision": precision, "unfused": unfused})
    if precision in ("f16", "bf16x3"):
        assert rec["rms_diff"] <= 1e-4 and rec["abs_rms_delta"] <= 1e-4, rec
    else:
        emu = Emulator2(fsd, cfg, mode="bf16", fused_post=not unfused).spec2wav(mel)
        vals, fails = seam_check(wav, emu, BOUNDS_RB2["full_bf16"])
        print("VOCMEAS " + json.dumps({"test": "v3_gate_bf16_vs_emulator", "unfused": unfused, **{k: vals[k] for k in ("max", "win", "rms")}}), flush=True)
        assert not fails, (fails, vals)


# ------------------------------------------------------------------------------------------------ 2. per sample against the emulator
@pytest.mark.parametrize("name,mode", [(c, m) for c in CONFIGS for m in MODES])
def test_isolating_generator_vs_emulator(name, mode):
    cfg = CONFIGS[name]
    model = _model(name, mode)
    assert model.precision == abi.VOC_PRECISIONS[MODES[mode][0]]
    hop = model.hop
    b1 = [20] + seam_lengths(cfg, 1, 2, hop)
    rag = seam_lengths(cfg, MAX_BATCH, 1, hop)
    fill_len = max(rag)
    mels = [synth.random_mel(700 + i, n, f"iso{n}") for i, n in enumerate(b1)]
    rmels = [synth.random_mel(900 + i, n, f"rag{n}") for i, n in enumerate(rag)] + \
            [synth.random_mel(5000 + i, fill_len, "fill") for i in range(MAX_BATCH - len(rag))]
    if mode == "f16":
        print(f"\n[{name}] tiles B=1: {shp.stage_tiles(cfg, 1)}  ragged B={len(rmels)}: {shp.stage_tiles(cfg, len(rmels))}", flush=True)
    group = "bf16" if mode == "bf16" else "f16"
    _check_utts(name, mode, model, mels, [(f"B=1 len={n}", [i]) for i, n in enumerate(b1)], group)
    _check_utts(name, mode, model, rmels, [("ragged", list(range(len(rmels))))], group)


@pytest.mark.parametrize("mode", list(MODES))
def test_v3_vs_emulator(mode):
    """the full V3 generator (conv_pre, three polyphase upsamplers, nine rb2x launches at C = 128 / 64 / 32, the fused conv_post)"""
    model = _model("v3", mode)
    groups = [[40], [17, 64, 33]]
    mels, cases = [], []
    for g in groups:
        idx = []
        for n in g:
            idx.append(len(mels))
            mels.append(synth.random_mel(40 + n, n, "full"))
        cases.append((f"B={len(g)} lens={g}", idx))
    rows = _check_utts("v3", mode, model, mels, cases, "full_bf16" if mode == "bf16" else "full_f16")
    if mode != "bf16":
        for r in rows:   # the waveform gate per utterance against the float64 reference
            assert r["oracle"]["rms"] <= 1e-4, r


@pytest.mark.parametrize("mode", list(MODES))
def test_v3_at_the_largest_batch(mode):
    rng = np.random.RandomState(11)
    lens = [int(v) for v in rng.randint(1, 7, size=MAX_BATCH)]
    mels = [synth.random_mel(20000 + i, n, "bmax") for i, n in enumerate(lens)]
    _check_utts("v3", mode, _model("v3", mode), mels, [(f"B={MAX_BATCH}", list(range(MAX_BATCH)))],
                "full_bf16" if mode == "bf16" else "full_f16")


def test_bf16_unfused_vs_emulator():
    """the per-convolution path (vconv only) of a ResBlock2 generator: the same rounding points, conv_post on the serial path"""
    for name in ("v3", "r128"):
        cfg, raw, _ = _sd(name)
        model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16", unfused=True)
        mels = [synth.random_mel(40 + n, n, "full") for n in (17, 64, 33)]
        _check_utts(name, "bf16", model, mels, [("B=3", [0, 1, 2])], "full_bf16" if name == "v3" else "bf16", fused_post=False)


# ------------------------------------------------------------------------------------------------ 3. every sample is written
@pytest.mark.parametrize("precision,unfused", [("f16", False), ("bf16", False), ("bf16x3", False), ("bf16", True)])
@pytest.mark.parametrize("name", ["v3", "r256"])
def test_every_sample_is_written(name, precision, unfused):
    cfg, raw, _ = _sd(name)
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision, unfused=unfused)
    hop = model.hop
    lens = [40, 17, 64, 1]
    Tm = max(lens)
    mel = np.stack([synth.random_mel(60 + b, Tm, "nan") for b in range(len(lens))])
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


# ------------------------------------------------------------------------------------------------ 4. memory-safety mode
@pytest.mark.parametrize("name", ["v3", "r256", "r128", "r64", "r32", "r32_k3post"])
def test_memory_safety_mode_is_clean(name):
    """dtts_config.debug_redzone: every workspace buffer and weight pack between red zones, workspaces NaN-filled before each forward"""
    for mode in ("f16", "bf16"):
        model = _model(name, mode, dtts_debug_redzone=1)
        lens = [33, 7, 64]
        mels = [synth.random_mel(80 + b, n, "rz") for b, n in enumerate(lens)]
        got = model.spec2wav_batch(mels)
        assert all(np.isfinite(g).all() for g in got)
        n = model.ctx.debug_check(torch.cuda.current_stream().cuda_stream)
        assert n == 0, model.ctx.last_error()


# ------------------------------------------------------------------------------------------------ 5. guards
def test_fp16_bound_overflow_detector_and_range_guard():
    cfg, raw, fsd = _sd("v3")
    mel = gc.g6_mel()
    v = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    # the static bound of dtts_vocoder_fp16_bound walks the ResBlock2 graph and stays a bound: >= the largest operand the float64
    # reference sees on mels inside the stated range
    for m in (mel, synth.random_mel(31, 72, "s16_0"), synth.random_mel(32, 48, "b")):
        wc, est = v.ctx.vocoder_fp16_bound(float(np.abs(m).max()))
        seen = r2.max_operand(fsd, cfg, m)
        print("VOCMEAS " + json.dumps({"test": "fp16_bound", "worst_case": wc, "rms_estimate": est, "seen": seen}), flush=True)
        assert wc >= seen > 0 and v.fp16_bound[0] >= wc
    # a mel scaled until the float64 reference shows an fp16-unrepresentable ResBlock operand
    scale = 1.0
    while r2.max_operand(fsd, cfg, mel * scale) <= 65504.0 * 1.5:
        scale *= 8.0
    hot = (mel * scale).astype(np.float32)
    with pytest.raises(abi.DttsError, match="overflowed"):
        v.spec2wav(hot)
    raw_w = v.forward_batch(T(hot[None]).cuda())
    torch.cuda.synchronize()
    assert v.overflowed() and v.ctx.vocoder_nonfinite() > 0 and not np.isfinite(raw_w.cpu().numpy()).all()
    assert np.isfinite(v.spec2wav(mel)).all() and not v.overflowed()
    auto = vocoder.HifiGAN(state_dict=raw, config=cfg)
    assert auto.precision == abi.VOC_F16
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter("always")
        w_hot = auto.spec2wav(hot)
    assert auto.precision == abi.VOC_BF16X3 and any("overflowed" in str(w.message) for w in ws) and np.isfinite(w_hot).all()
    assert np.array_equal(w_hot, vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16x3").spec2wav(hot))
    # the census instantiations count the unrepresentable activations and the call raises
    census = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16", range_guard=True)
    assert np.isfinite(census.spec2wav(mel)).all()
    with pytest.raises(abi.DttsError, match="exceeded the fp16 range"):
        census.forward_batch(T(hot[None]).cuda())
    stream = torch.cuda.current_stream()
    hot_d, wav_d = T(hot[None]).cuda(), torch.empty(1, hot.shape[0] * 256, device="cuda")
    census.ctx.hifigan_forward(hot_d.data_ptr(), None, 1, hot.shape[0], wav_d.data_ptr(), stream.cuda_stream)
    assert census.ctx.vocoder_clamped(stream.cuda_stream) > 0 and census.ctx.vocoder_clamped(stream.cuda_stream) == 0   # (reset by the first read)


@pytest.mark.parametrize("bits", [1 << 15, 1 << 9, 1 << 12, (1 << 9) | (1 << 15)])
def test_resblock1_tune_bits_do_not_change_a_resblock2_result(bits):
    cfg, raw, _ = _sd("v3")
    mels = [synth.random_mel(40 + n, n, "full") for n in (17, 64, 33)]
    want = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16").spec2wav_batch(mels)
    got = vocoder.HifiGAN(state_dict=raw, config={**cfg, "dtts_tune_flags": bits}, precision="f16").spec2wav_batch(mels)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("what", ["even_k", "pair"])
def test_shapes_outside_the_predicate(what):
    if what == "even_k":
        cfg = _iso(128, [3, 4, 5], [[1, 2], [1, 1], [2, 1]])
    else:
        d0, d1 = shp.largest_pair(256, 7)
        assert not shp.supported(256, 7, d0, d1 + 1)
        cfg = _iso(512, [3, 7, 5], [[1, 2], [d0, d1 + 1], [2, 1]])
    raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
    with pytest.raises(abi.DttsError, match="DTTS_VOC_BF16X3"):
        vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16x3")
    mel = synth.random_mel(5, 48, "refuse")
    if what == "even_k":
        # (an even kernel: get_padding(4, 1) = 1 shortens the sequence in the reference itself — no same-length reference exists)
        assert np.isfinite(model.spec2wav(mel)).all()
        return
    fsd = href.fold_weight_norm(raw)
    ref = r2.spec2wav(fsd, cfg, mel)
    rec = _gate(model.spec2wav(mel), ref, {"test": "refused_pair_bf16x3"})
    assert rec["rms_diff"] <= 1e-4 and rec["abs_rms_delta"] <= 1e-4, rec
    # bf16: the refused block runs convolution by convolution on vconv between its two fused neighbours (same rounding points)
    got = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16").spec2wav(mel)
    vals, fails = seam_check(got, Emulator2(fsd, cfg, mode="bf16").spec2wav(mel), BOUNDS_RB2["bf16"])
    print("VOCMEAS " + json.dumps({"test": "refused_pair_bf16_mixed", **{k: vals[k] for k in ("max", "win", "rms")}}), flush=True)
    assert not fails, (fails, vals)


def test_state_dict_of_the_other_block_type_names_the_first_missing_tensor():
    cfg, raw, _ = _sd("v3")
    raw1 = {k: T(v) for k, v in synth.hifigan_state_dict(SEED).items()}
    with pytest.raises(abi.DttsError, match=r"missing weight tensor 'vocoder\.resblocks\.0\.convs\.0"):
        vocoder.HifiGAN(state_dict=raw1, config={**synth.hifigan_config(), "resblock": "2", "resblock_dilation_sizes": V3_D}, precision="bf16x3")
    with pytest.raises(abi.DttsError, match=r"missing weight tensor 'vocoder\.resblocks\.0\.convs1\.0"):
        vocoder.HifiGAN(state_dict=raw, config={**cfg, "resblock": "1", "resblock_dilation_sizes": [[1, 3, 5]] * 3}, precision="bf16x3")


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_text_to_waveform_with_a_v3_vocoder():
    from dict_tts_amd import model as M
    m = M.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(SEED).items()})
    batch = synth.make_batch(synth.biaobei_struct()["sentences"][:3], SEED)
    tb = {k: T(v) for k, v in batch.items()}
    out = m((tb["word_tokens"], None), tb["pron_modified"], (None, None, None), None, None,
            (tb["keys"], tb["values"], tb["key_map"], tb["pinyin"], tb["pinyin_map"]), infer=True)
    mel = out["mel_out"].float().cpu().numpy()
    lens = [int(v) for v in (out["mel2word"].cpu() > 0).sum(-1)]
    cfg, raw, _ = _sd("v3")
    voc = vocoder.HifiGAN(state_dict=raw, config=cfg)
    wavs = voc.spec2wav_batch([mel[b, :n] for b, n in enumerate(lens)])
    assert [w.shape[0] for w in wavs] == [n * 256 for n in lens] and all(np.isfinite(w).all() for w in wavs)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    wav = voc.forward_batch(T(mel).cuda(), lens_t, check=True)
    pcm = voc.to_int16(wav, lens_t).cpu().numpy()
    assert pcm.dtype == np.int16 and pcm.shape == (len(lens), mel.shape[1] * 256)
    for b, n in enumerate(lens):
        assert np.abs(pcm[b, :n * 256].astype(np.int32)).max() > 0 and not pcm[b, n * 256:].any()
