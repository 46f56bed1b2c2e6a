"""HifiGAN V2 generators (``resblock "1"``, ``upsample_initial_channel`` 128: stage widths 64 / 32 / 16 / 8) on the GPU: the narrow
whole-ResBlock1 kernel rbn.hip (C = 16 / 8, taps folded into the MFMA's contraction index, conv_post + tanh in the last ResBlock's
epilogue), the padded serial convolutions around it, and the host path that selects them.

Same method as tests/test_vocoder_kernels_gpu.py: sample by sample against the rounding-point emulator (tests/vocoder_emul.py, which
takes any cfg; ``fused_post=True`` is passed explicitly because its default rule knows only a last width of 32), with the bounds of
tests/hifigan_v2_bounds.py (vocoder_emul.BOUNDS, one of them tightened: GPU - emulator differs by fp32 summation order only) — and the
waveform gate against the golden taken from the reference implementation (tests/golden/g14_hifigan_v2.npz, tools/make_golden_v2.py).

Isolating generators have ONE upsampler of rate 2 (``_iso(32, ..)`` -> C = 16, ``_iso(16, ..)`` -> C = 8): the stage's three rbn launches
feed the fused conv_post directly, and stage rows are waveform samples.  Shapes come from the launcher's tile rule (tests/rbn_shapes.py
restates rbn_launch_el): 256-, 512- and 1024-row tiles are all reached — B = 1 short, B = 1 over two tiles, B = 3 ragged with stage lengths
n s - 2, n s, n s + 2 for every tile step s of each tile size, and one call of DTTS_MAX_VOCODER_BATCH short utterances.

Every measured value is printed as a ``VOCMEAS {json}`` line (run with -s to see them).  Worst values measured on MI355X over all shapes
of a group (GPU - emulator, max / 256-sample window / RMS):
  isolating C = 16, f16 / release:  9.0e-5 / 2.0e-5 / 1.5e-5     isolating C = 8, f16 / release:  3.4e-5 / 7.0e-6 / 4.8e-6   (bounds 2.4e-4 / 6.3e-5 / 6.3e-5)
  isolating C = 16, bf16:           7.9e-4 / 1.5e-4 / 7.4e-5     isolating C = 8, bf16:           6.9e-4 / 8.0e-5 / 3.3e-5   (bounds 1.3e-3 / 7.3e-4 / 7.3e-4)
  full V2, f16 / release:           1.9e-4 / 4.5e-5 / 3.7e-5     (bounds 8.6e-4 / 1.9e-4 / 1.7e-4)
  full V2, bf16:                    3.1e-3 / 7.1e-4 / 5.8e-4     (bounds 1.0e-2 / 2.7e-3 / 2.2e-3)
  bf16 per convolution (unfused, 24 channels, a refused block): 8.8e-4 / 2.3e-4 / 1.8e-4 (bounds 3.1e-3 / 7.3e-4 / 7.3e-4); full V2 4.0e-3 / 8.3e-4 / 7.0e-4
  waveform gate on g6_mel against g14 (RMS(gpu - ref), |RMS(gpu) - RMS(ref)|): f16 4.77e-5, 5.8e-7; bf16x3 2.2e-6, 5.7e-7; bf16 1.04e-3, 2.0e-4
"""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import golden_cases as gc
import rbn_shapes as shp
from dict_tts_amd import abi, synth, vocoder
from oracle import hifigan_ref as href
from hifigan_v2_bounds import NARROW_BOUNDS
from vocoder_emul import BOUNDS, Emulator, seam_check

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
SEED = 1234
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as _f:
    MAX_BATCH = int(re.search(r"#define DTTS_MAX_VOCODER_BATCH (\d+)", _f.read()).group(1))
V2 = synth.hifigan_config_v2()


def _iso(c0, rk, rd):
    return {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": rk, "resblock_dilation_sizes": [list(d) for d in rd]}


D135 = [[1, 3, 5]] * 3
K59 = ([5, 9, 3], [[2, 4, 5], [1, 2, 3], [3, 5, 5]])   # k = 5 / 9 and dilation sums above 9
CONFIGS = {
    "n16": _iso(32, [3, 7, 11], D135),          # the fused conv_post on the largest halo (k = 11)
    "n8": _iso(16, [3, 7, 11], D135),
    "n16_k59": _iso(32, *K59),
    "n8_k59": _iso(16, *K59),
    "n16_k3post": _iso(32, [11, 9, 3], D135),   # the fused conv_post on a k = 3 tile
    "n8_k3post": _iso(16, [11, 9, 3], D135),
}
MODES = {   # name -> (HifiGAN precision, range_guard, emulator mode)
    "f16": ("f16", True, "f16"),
    "f16_release": ("f16", False, "f16"),
    "bf16": ("bf16", False, "bf16"),
}
_SD, _EMU, _MODEL = {}, {}, {}


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _sd(name):
    if name not in _SD:
        cfg = V2 if name == "v2" else CONFIGS[name]
        raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
        _SD[name] = (cfg, raw, href.fold_weight_norm(raw))
    return _SD[name]


def _model(name, mode, **extra):
    key = (name, mode, tuple(sorted(extra.items())))
    if key not in _MODEL:
        cfg, raw, _ = _sd(name)
        precision, guard, _ = MODES[mode]
        _MODEL[key] = vocoder.HifiGAN(state_dict=raw, config={**cfg, **extra}, precision=precision, range_guard=guard)
    return _MODEL[key]


def _emulate(name, emode, mel, fused_post=True):
    """the emulator's waveform of one utterance: computed once, shared by the tests that need it"""
    key = (name, emode, fused_post, mel.shape[0], float(mel[0, 0]), float(mel[-1, -1]))
    if key not in _EMU:
        cfg, _, fsd = _sd(name)
        _EMU[key] = Emulator(fsd, cfg, mode=emode, fused_post=fused_post).spec2wav(mel)
    return _EMU[key]


_BASE = []


def _mel(n, q=0):
    """an utterance of n frames: a window of one long random mel (generated once), at an offset that differs per utterance"""
    if not _BASE:
        _BASE.append(synth.random_mel(4242, 24000, "v2base"))
    off = 3 * q + (n % 89)
    assert off + n <= _BASE[0].shape[0]
    return np.ascontiguousarray(_BASE[0][off:off + n])


def _bounds(name, mode):
    return NARROW_BOUNDS[("full_" if name == "v2" else "") + ("bf16" if mode == "bf16" else "f16")]


def _run(model, mels):
    lens = [m.shape[0] for m in mels]
    Tm = max(lens)
    batch = np.zeros((len(mels), Tm, 80), np.float32)
    for b, m in enumerate(mels):
        batch[b, :lens[b]] = m
    full = model.forward_batch(T(batch).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    assert not model.overflowed()
    assert np.isfinite(full).all() and float(np.abs(full).max()) <= 1.0
    for b, n in enumerate(lens):
        assert float(np.abs(full[b, n * model.hop:]).max(initial=0.0)) == 0.0, b   # exact zeros past lens * hop
    return full


def _check(name, mode, model, mels, case, emulated=None, fused_post=True, bounds=None):
    """one batch against the emulator, utterance by utterance; -> the batch's waveforms (each cut to its length)"""
    full = _run(model, mels)
    hop, bounds = model.hop, bounds or _bounds(name, mode)
    failures, out = [], []
    for b, m in enumerate(mels):
        g = full[b, :m.shape[0] * hop]
        out.append(g)
        if emulated is not None and b not in emulated:
            continue
        assert np.mean(np.abs(g) > 0.9) < 0.01, "tanh saturation would hide errors"
        vals, fails = seam_check(g, _emulate(name, MODES[mode][2], m, fused_post), bounds)
        print("VOCMEAS " + json.dumps({"config": name, "mode": mode, "case": case, "B": len(mels), "utt": b, "samples": g.size,
                                       "emu": {k: vals[k] for k in ("max", "win", "rms")}}), flush=True)
        if fails:
            failures.append((case, b, m.shape[0], fails, vals))
    assert not failures, f"{name} / {mode}: GPU vs emulator beyond {bounds}: {failures[:6]}"
    return out


# ------------------------------------------------------------------------------------------------ shapes from the tile rule
def regime_lengths(cfg, B, hop, cus):
    """{tile rows W: [mel lengths]}: for each of the launcher's tile sizes a batch size B reaches, stage lengths n s - 2, n s, n s + 2 for every
    tile step s of the stage's launches at a padded length that makes the LAST launch (the one with the fused conv_post) pick W"""
    C = cfg["upsample_initial_channel"] >> 1
    k, dils = cfg["resblock_kernel_sizes"][-1], cfg["resblock_dilation_sizes"][-1]
    h = shp.halo(k, dils)
    first = {}
    for L in range(64, 400000, 64):   # the shortest padded length at which each tile size is picked
        first.setdefault(shp.tile_rows(C, k, dils, B, L, True, cus) + 2 * h + 6, L)
    out = {}
    for W, L0 in first.items():
        guess = max(L0 + L0 // 8, 2 * W)
        steps = sorted(set(shp.stage_tiles(cfg, B, guess, cus).values()))
        lens = sorted({(max(2, round(guess / s)) * s + d) // hop for s in steps for d in (-2, 0, 2) if (max(2, round(guess / s)) * s + d) % hop == 0})
        assert shp.tile_rows(C, k, dils, B, max(lens) * hop, True, cus) + 2 * h + 6 == W, (W, lens)
        out[W] = lens
    return out


def test_v2_constructs_in_f16_and_auto_keeps_f16():
    """FAILS WITHOUT THE FEATURE: the parent refuses V2 in DTTS_VOC_F16 ("needs ResBlock widths 32/64/128/256") and AUTO falls back to bf16x3"""
    cfg, raw, _ = _sd("v2")
    v = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    assert v.precision == abi.VOC_F16 and v.hop == 256
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter("always")
        auto = vocoder.HifiGAN(state_dict=raw, config=cfg)
    assert auto.precision == abi.VOC_F16 and auto.fp16_status in ("proven", "checked")
    assert not any("do not cover" in str(w.message) for w in ws)
    assert np.isfinite(auto.spec2wav(gc.g6_mel())).all()


# ------------------------------------------------------------------------------------------------ the waveform gate
@pytest.mark.parametrize("precision", ["f16", "bf16x3", "bf16"])
def test_v2_waveform_gate(golden_dir, precision):
    """spec2wav(g6_mel) of the synthetic V2 generator against the golden taken from the reference implementation.  BASELINE.json
    north_star: RMS(gpu - ref) and |RMS(gpu) - RMS(ref)| <= 1e-4 for f16 and bf16x3; bf16 has no project gate (reported, as for V1)."""
    g = np.load(os.path.join(golden_dir, "g14_hifigan_v2.npz"))
    cfg, raw, _ = _sd("v2")
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision)
    assert model.hop == 256 and model.precision == abi.VOC_PRECISIONS[precision]
    wav = model.spec2wav(gc.g6_mel())
    ref = g["wav"].astype(np.float64)
    assert wav.shape == ref.shape and np.isfinite(wav).all()
    rec = {"test": "v2_gate", "precision": precision, "rms_diff": rms(wav.astype(np.float64) - ref), "abs_rms_delta": abs(rms(wav) - rms(ref))}
    print("VOCMEAS " + json.dumps(rec), flush=True)
    if precision != "bf16":
        assert rec["rms_diff"] <= 1e-4 and rec["abs_rms_delta"] <= 1e-4, rec


# ------------------------------------------------------------------------------------------------ per sample against the emulator
@pytest.mark.parametrize("name,mode", [(c, m) for c in CONFIGS for m in MODES])
def test_isolating_generator_vs_emulator(name, mode):
    cfg = CONFIGS[name]
    model = _model(name, mode)
    assert model.precision == abi.VOC_PRECISIONS[MODES[mode][0]]
    hop, cus = model.hop, _cus()
    b1 = regime_lengths(cfg, 1, hop, cus)
    if mode == "f16":
        print(f"\n[{name}] B=1 {b1}  B=3 {regime_lengths(cfg, 3, hop, cus)}", flush=True)
    # B = 1: shorter than one tile, then two tiles and a seam remainder of the smallest tile size
    for n in [20] + b1[min(b1)]:
        _check(name, mode, model, [_mel(n)], f"B=1 len={n}")
    # B = 3 ragged at every tile size; each utterance alone (another tile size) is bit-identical to itself inside the batch
    for W, lens in regime_lengths(cfg, 3, hop, cus).items():
        for i in range(0, len(lens), 3):
            grp = lens[i:i + 3]
            grp = grp + grp[:3 - len(grp)]
            mels = [_mel(n, q) for q, n in enumerate(grp)]
            got = _check(name, mode, model, mels, f"B=3 W={W} lens={grp}")
            for q in ((0, 2) if mode == "f16_release" else (1,)):
                alone = _run(model, [mels[q]])[0]
                assert np.array_equal(alone, got[q]), (name, mode, W, grp[q], "alone != inside the batch")


@pytest.mark.parametrize("name,mode", [("n16", "f16"), ("n8", "f16"), ("n16", "bf16"), ("n8_k59", "f16_release"), ("n16_k3post", "bf16")])
def test_isolating_generator_at_the_largest_batch(name, mode):
    """one call of DTTS_MAX_VOCODER_BATCH short ragged utterances (the tile table at its largest, the large tiles, several tiles per
    persistent workgroup); index 0, the last index and the seam lengths of that batch size are emulated (at most 8)"""
    cfg = CONFIGS[name]
    model = _model(name, mode)
    hop, cus = model.hop, _cus()
    reg = regime_lengths(cfg, MAX_BATCH, hop, cus)
    seams = reg[max(reg)][:6]
    rng = np.random.RandomState(11)
    lens = [int(rng.randint(1, 7))] + seams + [int(v) for v in rng.randint(1, 7, size=MAX_BATCH - 1 - len(seams))]
    mels = [_mel(n, q % 16) for q, n in enumerate(lens)]
    got = _check(name, mode, model, mels, f"B={MAX_BATCH}", emulated=set(range(1 + len(seams))) | {MAX_BATCH - 1})
    alone = _run(model, [mels[1]])[0]
    assert np.array_equal(alone, got[1]), "alone != inside the largest batch"


FULL_MELS = lambda: [gc.g6_mel(), synth.random_mel(57, 17, "full"), synth.random_mel(104, 33, "full")]


@pytest.mark.parametrize("mode", list(MODES))
def test_full_v2_vs_emulator(mode):
    """the whole V2 generator: conv_pre, four padded polyphase upsamplers, rblock at C = 64 / 32, rbn at C = 16 / 8, the fused conv_post"""
    model = _model("v2", mode)
    mels = FULL_MELS()
    _check("v2", mode, model, mels[:1], "B=1 g6_mel")
    got = _check("v2", mode, model, mels, "B=3")
    assert np.array_equal(got[1], _run(model, [mels[1]])[0])


# ------------------------------------------------------------------------------------------------ the per-convolution path below 32 channels
OUTSIDE = {
    # 24 channels: no fused kernel at all; every ResBlock convolution by convolution, rows of 24 channels under packs padded to 32
    "c24": _iso(48, [3, 7, 11], D135),
    # C = 16 with one dilation triple outside rbn_supported (halo 110: 30 rows left): that block on vconv between two rbn launches
    "n16_mixed": _iso(32, [3, 11, 7], [[1, 3, 5], [7, 6, 6], [1, 3, 5]]),
}
CONFIGS_ALL = {**CONFIGS, **OUTSIDE}


@pytest.mark.parametrize("name,unfused", [("n16", True), ("n8", True), ("v2", True), ("c24", False), ("n16_mixed", False)])
def test_bf16_per_convolution_path_vs_emulator(name, unfused):
    """DTTS_VOC_BF16 convolution by convolution (vconv; conv_post on the serial path) at widths below 32 — with vocoder_unfused = 1, and for shapes
    outside rbn_supported: activation rows of 8 / 16 / 24 channels under packs whose C_in_pad is 32.  The rows are read at their own pitch and the
    pad channels as zeros (before: at the pack's pitch, the pad channels being the next row's values).  Bounds: vocoder_emul.BOUNDS, the ones the
    per-convolution path of the wider generators is held to."""
    if name in OUTSIDE:
        assert not all(shp.supported(CONFIGS_ALL[name]["upsample_initial_channel"] >> 1, k, d)
                       for k, d in zip(CONFIGS_ALL[name]["resblock_kernel_sizes"], CONFIGS_ALL[name]["resblock_dilation_sizes"]))
        CONFIGS[name] = OUTSIDE[name]
    cfg, raw, _ = _sd(name)
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16", unfused=unfused)
    mels = FULL_MELS() if name == "v2" else [_mel(n, q) for q, n in enumerate((150, 33, 401))]
    _check(name, "bf16", model, mels, f"per convolution unfused={unfused}", fused_post=False, bounds=BOUNDS["full_bf16" if name == "v2" else "bf16"])


def test_census_counts_each_row_once_at_every_tile_size():
    """the range guard's count is a function of the input, not of the tiles: three copies of an utterance in one batch (512-row tiles) count three
    times what the utterance alone counts (256-row tiles) — with the fused conv_post the tiles overlap by 6 rows, which are counted once"""
    cfg, raw, _ = _sd("n16")
    c = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16", range_guard=True)
    n = regime_lengths(cfg, 3, c.hop, _cus())[512][0]
    hot = (_mel(n) * 3e4).astype(np.float32)
    stream = torch.cuda.current_stream()

    def count(B):
        mel_d = T(np.stack([hot] * B)).cuda()
        wav = torch.empty(B, n * c.hop, device="cuda")
        c.ctx.hifigan_forward(mel_d.data_ptr(), None, B, n, wav.data_ptr(), stream.cuda_stream)
        return c.ctx.vocoder_clamped(stream.cuda_stream)
    one, three = count(1), count(3)
    print("VOCMEAS " + json.dumps({"test": "census_tile_sizes", "alone": one, "three": three}), flush=True)
    assert one > 0 and three == 3 * one


# ------------------------------------------------------------------------------------------------ bit identities
@pytest.mark.parametrize("name", ["n16", "n8", "v2"])
def test_census_equals_release_and_forwards_repeat(name):
    mels = FULL_MELS()[1:] if name == "v2" else [synth.random_mel(300 + n, n, "bits") for n in (150, 33, 401)]
    census, release = _model(name, "f16"), _model(name, "f16_release")
    a, b = _run(census, mels), _run(release, mels)
    assert np.array_equal(a, b)
    assert census.ctx.vocoder_clamped(torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(b, _run(release, mels))   # two consecutive forwards


@pytest.mark.parametrize("bits", [1 << 15, 1 << 9, 1 << 12, 1 << 14])
def test_tune_bits_do_not_change_a_narrow_result(bits):
    for name in ("n16", "n8"):
        mels = [synth.random_mel(300 + n, n, "bits") for n in (150, 33, 401)]
        want = _run(_model(name, "f16_release"), mels)
        got = _run(_model(name, "f16_release", dtts_tune_flags=bits), mels)
        assert np.array_equal(want, got), (name, bits)


# ------------------------------------------------------------------------------------------------ every sample is written
@pytest.mark.parametrize("precision", ["f16", "bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["v2", "n16", "n8"])
def test_every_sample_is_written(name, precision):
    cfg, raw, _ = _sd(name)
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision)
    hop = model.hop
    lens = [40, 17, 64, 1]
    Tm = max(lens)
    mel_d = T(np.stack([synth.random_mel(60 + b, Tm, "nan") for b in range(len(lens))])).cuda()
    stream = torch.cuda.current_stream()
    for short in (False, True):
        wav = torch.full((len(lens), Tm * hop), float("nan"), dtype=torch.float32, device="cuda")
        lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda") if short else None
        model.ctx.hifigan_forward(mel_d.data_ptr(), lens_d.data_ptr() if short else None, len(lens), Tm, wav.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        w = wav.cpu().numpy()
        assert np.isfinite(w).all(), (name, precision, short, int((~np.isfinite(w)).sum()))
        if short:
            for b, n in enumerate(lens):
                assert float(np.abs(w[b, n * hop:]).max(initial=0.0)) == 0.0, (b, n)
                assert float(np.abs(w[b, :n * hop]).max()) > 0.0


# ------------------------------------------------------------------------------------------------ memory-safety mode
@pytest.mark.parametrize("name", ["n16", "n8", "v2"])
def test_memory_safety_mode_is_clean(name):
    """dtts_config.debug_redzone: every workspace buffer and weight pack between red zones; 0 damaged bytes, the same bits as the release context"""
    lens = [33, 7, 64]
    mels = [synth.random_mel(80 + b, n, "rz") for b, n in enumerate(lens)]
    for mode in ("f16_release", "bf16"):
        model = _model(name, mode, dtts_debug_redzone=1)
        got = _run(model, mels)
        n = model.ctx.debug_check(torch.cuda.current_stream().cuda_stream)
        assert n == 0, model.ctx.last_error()
        assert np.array_equal(got, _run(_model(name, mode), mels))


def test_a_pack_in_another_order_is_refused():
    """dtts_config.debug_redzone = 2: the whole-ResBlock launches declare another fragment order; rbn_launch refuses, nothing runs"""
    cfg, raw, _ = _sd("n16")
    model = vocoder.HifiGAN(state_dict=raw, config={**cfg, "dtts_debug_redzone": 2}, precision="f16")
    with pytest.raises(abi.DttsError):
        model.spec2wav(synth.random_mel(5, 48, "misorder"))


# ------------------------------------------------------------------------------------------------ fp16 validity
def test_fp16_overflow_is_counted_poisoned_and_redone():
    cfg, raw, fsd = _sd("v2")
    mel = gc.g6_mel()
    exact = Emulator(fsd, cfg, rounding=False)
    scale = 1.0

    def peak(m):   # the largest ResBlock operand x (an upsampler's output) of the float64 reference
        st = exact.forward(torch.as_tensor(m, dtype=torch.float32).unsqueeze(0).transpose(2, 1), return_stages=True)[1]
        return max(float(v.abs().max()) for k, v in st.items() if k.startswith("ups."))
    while peak(mel * scale) <= 65504.0 * 1.5:
        scale *= 8.0
    hot = (mel * scale).astype(np.float32)
    v = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
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
    census = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16", range_guard=True)
    assert np.isfinite(census.spec2wav(mel)).all()
    with pytest.raises(abi.DttsError, match="exceeded the fp16 range"):
        census.forward_batch(T(hot[None]).cuda())
    # the narrow stages' own census: an isolating C = 8 generator, where no other kernel family counts
    cfg8, raw8, fsd8 = _sd("n8")
    c8 = vocoder.HifiGAN(state_dict=raw8, config=cfg8, precision="f16", range_guard=True)
    hot8 = (synth.random_mel(3, 40, "hot") * 1e7).astype(np.float32)
    stream = torch.cuda.current_stream()
    hot_d, wav_d = T(hot8[None]).cuda(), torch.empty(1, hot8.shape[0] * 2, device="cuda")
    c8.ctx.hifigan_forward(hot_d.data_ptr(), None, 1, hot8.shape[0], wav_d.data_ptr(), stream.cuda_stream)
    assert c8.ctx.vocoder_clamped(stream.cuda_stream) > 0 and c8.ctx.vocoder_clamped(stream.cuda_stream) == 0   # (reset by the first read)
    assert c8.ctx.vocoder_nonfinite() > 0 and not np.isfinite(wav_d.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ outside the predicate
@pytest.mark.parametrize("what", ["even_k", "24ch", "resblock2"])
def test_shapes_outside_the_predicate(what):
    if what == "even_k":
        cfg, match = _iso(32, [3, 4, 5], D135), "ResBlock widths"
    elif what == "24ch":
        cfg, match = _iso(48, [3, 7, 11], D135), "ResBlock widths"
    else:
        cfg, match = {**_iso(32, [3, 5, 7], [[1, 2], [2, 6], [3, 12]]), "resblock": "2"}, "ResBlock2 widths"
    raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
    with pytest.raises(abi.DttsError, match=match) as e:
        vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    assert "use DTTS_VOC_BF16X3" in str(e.value)
    assert np.isfinite(vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16x3").spec2wav(synth.random_mel(5, 48, "refuse"))).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_text_to_waveform_with_a_v2_vocoder():
    from dict_tts_amd import model as M
    m = M.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(SEED).items()})
    batch = synth.make_batch(synth.biaobei_struct()["sentences"][:3], SEED)
    tb = {k: T(v) for k, v in batch.items()}
    out = m((tb["word_tokens"], None), tb["pron_modified"], (None, None, None), None, None,
            (tb["keys"], tb["values"], tb["key_map"], tb["pinyin"], tb["pinyin_map"]), infer=True)
    mel = out["mel_out"].float().cpu().numpy()
    lens = [int(v) for v in (out["mel2word"].cpu() > 0).sum(-1)]
    cfg, raw, _ = _sd("v2")
    voc = vocoder.HifiGAN(state_dict=raw, config=cfg)
    assert voc.precision == abi.VOC_F16
    wavs = voc.spec2wav_batch([mel[b, :n] for b, n in enumerate(lens)])
    assert [w.shape[0] for w in wavs] == [n * 256 for n in lens] and all(np.isfinite(w).all() for w in wavs)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    wav = voc.forward_batch(T(mel).cuda(), lens_t, check=True)
    pcm = voc.to_int16(wav, lens_t).cpu().numpy()
    assert pcm.dtype == np.int16 and pcm.shape == (len(lens), mel.shape[1] * 256)
    for b, n in enumerate(lens):
        assert np.abs(pcm[b, :n * 256].astype(np.int32)).max() > 0 and not pcm[b, n * 256:].any()
