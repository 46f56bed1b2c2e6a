"""The vocoder's polyphase upsamplers on the GPU at every accepted form (single: k = u; half: k = 2u on whole waves; general: everything else,
k < 2u included) and every stage width (256 .. 8), where the rest of the suite runs k = 2u with an even rate only: pack.hip pack_transposed,
every vconv_launch branch an upsampler reaches (tests/ups_shapes.py restates the rule; tests/test_upsampler_forms_cpu.py holds the table to
it), the stores of C_out < C_out_pad rows at 16 and 8 channels, conv1d.hip under bf16x3, and the phase rule of the static fp16 bound.

Same method as tests/test_vocoder_kernels_gpu.py: isolating generators (ONE upsampler; resblock_kernel_sizes [3, 7, 11], dilations (1, 3, 5): the
ResBlock side is what the suite already runs, stage rows are waveform samples), compared per sample with the rounding-point emulator
(tests/vocoder_emul.py) under the project's own bounds: vocoder_emul.BOUNDS, hifigan_v2_bounds.NARROW_BOUNDS at 16 / 8 channels, `full_*` for
the mixed three-stage generator (rates 4 / 5 / 3, kernels 4 / 9 / 5: another form per stage, hop 60).  Lengths come from the upsampler's own
input-row tile TT (ups_shapes.vconv_config): TT - 1, TT, TT + 1, 2 TT + 1 alone, and ragged behind a longer utterance, so that every short
utterance's end has real neighbour rows in the padded batch (a +1 tap that read them instead of zero, a store past C_out, rotated phases, p off
by one, a tap dropped at a tile seam: test_upsampler_forms_cpu.py plants each and shows it 7x .. 1000x beyond these bounds).

Forms the reference cannot match are refused by name in every precision (pack.hip): an odd k - u (ConvTranspose1d yields T u + 1 rows) and
k < u were accepted before and computed something else than the reference; k > 2u was refused already.

Every measured value is printed as a ``VOCMEAS {json}`` line (run with -s to see them).
Worst values measured on MI355X over all shapes of a group (GPU - emulator: max / 256-sample window / RMS); no group was added or widened:
  stage widths 256 .. 32, f16 / release:  8.3e-5 / 2.4e-5 / 2.4e-5   (bounds 2.4e-4 / 6.3e-5 / 6.3e-5)      bf16:  1.1e-3 / 2.6e-4 / 2.6e-4   (bounds 3.1e-3 / 7.3e-4 / 7.3e-4)
  stage widths 16 / 8,    f16 / release:  5.8e-5 / 1.4e-5 / 1.1e-5   (bounds 2.4e-4 / 6.3e-5 / 6.3e-5)      bf16:  5.8e-4 / 6.6e-5 / 4.9e-5   (bounds 1.3e-3 / 7.3e-4 / 7.3e-4)
  mixed three-stage,      f16 / release:  1.9e-4 / 4.6e-5 / 4.1e-5   (bounds 8.6e-4 / 1.9e-4 / 1.7e-4)      bf16:  2.6e-3 / 6.2e-4 / 5.2e-4   (bounds 1.0e-2 / 2.7e-3 / 2.2e-3)
  bf16 per convolution (unfused): initial width 64  7.4e-4 / 1.6e-4 / 1.3e-4,  initial width 16  1.2e-3 / 2.0e-4 / 2.0e-4   (bounds 3.1e-3 / 7.3e-4 / 7.3e-4)
  bf16x3 against the float64 oracle: control (2, 4)  4.5e-6 / 1.6e-6 / 1.4e-6 (initial width 64), 4.1e-6 / 1.4e-6 / 1.3e-6 (16);  new forms at most
    6.0e-6 / 1.9e-6 / 1.8e-6 (1.33 / 1.42 / 1.45 x the control)   -> X3_BOUNDS 1.8e-5 / 5.8e-6 / 5.5e-6
FAILED BEFORE THE FIX, found here: test_static_fp16_bound_general_forms at M = 6 in all nine cases (dtts_vocoder_fp16_bound 4e-5 .. 2e-4 BELOW the
independently evaluated peak, e.g. (8, 12): 174845187 against 174872835): vocoder.hip took the slope of every bound as value(1) - value(0) behind the
upsampler's maximum over output phases, which underestimates it when another phase leads at M = 6 than at M = 1.  The analysis now propagates the
bias part and the slope separately.  Nothing else failed: no kernel or pack change was needed for any accepted form.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rbn_shapes
import test_vocoder_kernels_gpu as vk
import ups_shapes as ups
from dict_tts_amd import abi, synth, vocoder
from hifigan_v2_bounds import NARROW_BOUNDS
from oracle import hifigan_ref as href
from vocoder_emul import BOUNDS, Emulator, seam_check

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SEED = 1234
MODES = {   # name -> (HifiGAN precision, range_guard, emulator mode)
    "f16": ("f16", True, "f16"),
    "f16_release": ("f16", False, "f16"),
    "bf16": ("bf16", False, "bf16"),
}
# DTTS_VOC_BF16X3 (conv1d.hip, hi / lo split operands) against the float64 oracle: 3 x the worst value measured on an MI355X over the control (2, 4)
# and the forms of test_forms_in_bf16x3_and_unfused (the table in the docstring: worst 5.96e-6 / 1.92e-6 / 1.83e-6)
X3_BOUNDS = {"max": 1.8e-5, "win": 5.8e-6, "rms": 5.5e-6}
_SD, _EMU, _BASE = {}, {}, []


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _cfg(case):
    if isinstance(case, tuple):   # (c0, u, k): a generator outside the table (the controls)
        return ups.iso(*case)
    return ups.MIXED if case == "mixed" else ups.CASES[case]["cfg"]


def _sd(case, weight_norm=True):
    key = (case, weight_norm)
    if key not in _SD:
        cfg = _cfg(case)
        raw = {k: T(v) for k, v in synth.hifigan_state_dict(SEED, weight_norm=weight_norm, cfg=cfg).items()}
        _SD[key] = (cfg, raw, href.fold_weight_norm(raw))
    return _SD[key]


def _narrow(case):
    return _cfg(case)["upsample_initial_channel"] >> len(_cfg(case)["upsample_rates"]) in (16, 8)


def _model(case, mode, unfused=False, **extra):
    cfg, raw, _ = _sd(case)
    precision, guard, _ = MODES[mode]
    return vocoder.HifiGAN(state_dict=raw, config={**cfg, **extra}, precision=precision, range_guard=guard, unfused=unfused)


def _mel(n, q=0):
    """an utterance of n frames: a window of one long random mel (generated once), at an offset that differs per utterance"""
    if not _BASE:
        _BASE.append(synth.random_mel(4343, 4000, "upsbase"))
    off = 7 * q + (n % 89)
    assert off + n <= _BASE[0].shape[0]
    return np.ascontiguousarray(_BASE[0][off:off + n])


def _emulate(case, emode, mel, fused_post=None, rounding=True):
    """the emulator's waveform of one utterance: computed once, shared by the tests and modes that need it"""
    key = (case, emode, fused_post, rounding, mel.shape[0], float(mel[0, 0]), float(mel[-1, -1]))
    if key not in _EMU:
        cfg, _, fsd = _sd(case)
        if fused_post is None and _narrow(case):
            fused_post = True   # (the emulator's default rule knows only a last width of 32)
        _EMU[key] = Emulator(fsd, cfg, mode=emode, fused_post=fused_post, rounding=rounding).spec2wav(mel)
    return _EMU[key]


def _bounds(case, mode):
    group = "bf16" if mode == "bf16" else "f16"
    if case == "mixed":
        return BOUNDS["full_" + group]
    return (NARROW_BOUNDS if _narrow(case) else BOUNDS)[group]


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


def _check(case, mode, model, mels, what, bounds=None, want=None, tt=None):
    """one batch against the emulator (or `want(mel)`), utterance by utterance; -> the measured rows.  A failure reports where the worst sample
    lies: its input row's offset inside the upsampler's tile and its distance from the utterance's end"""
    full = _run(model, mels)
    hop, bounds = model.hop, bounds or _bounds(case, mode)
    rows, failures = [], []
    for b, m in enumerate(mels):
        g = full[b, :m.shape[0] * hop]
        assert np.mean(np.abs(g) > 0.9) < 0.01, "tanh saturation would hide errors"
        e = want(m) if want else _emulate(case, MODES[mode][2], m)
        vals, fails = seam_check(g, e, bounds)
        rec = {"case": str(case), "mode": mode, "what": what, "B": len(mels), "utt": b, "frames": m.shape[0],
               "emu": {k: vals[k] for k in ("max", "win", "rms")}, "worst_frame": vals["argmax"] // hop, "frames_from_end": m.shape[0] - 1 - vals["argmax"] // hop}
        if tt:
            rec["offset_in_tile"] = (vals["argmax"] // hop) % tt
        print("VOCMEAS " + json.dumps(rec), flush=True)
        rows.append(rec)
        if fails:
            failures.append((fails, rec))
    assert not failures, f"{case} / {mode}: GPU vs emulator beyond {bounds}: {failures[:6]}"
    return rows


# ------------------------------------------------------------------------------------------------ every form, every width, at the upsampler's seams
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(ups.CASES))
def test_form_vs_emulator(case, mode):
    model = _model(case, mode)
    assert model.precision == abi.VOC_PRECISIONS[MODES[mode][0]] and model.hop == ups.CASES[case]["u"]
    (cfg_l, tt), (short, longer) = ups.launch_of(case, mode), ups.tile_lengths(case, mode)
    mels = [_mel(n, q) for q, n in enumerate(short)]
    for m in mels:   # B = 1: one row short of a tile, exactly one, one row into the second, one row into the third
        _check(case, mode, model, [m], f"B=1 vconv{cfg_l}", tt=tt)
    # ragged: the longer utterance first, so that the rows behind every short utterance's end hold a neighbour's values in the padded batch
    _check(case, mode, model, [_mel(longer, 9)] + mels, "ragged", tt=tt)


SEAM_CASES = ["u3k5_c512", "u5k9_c256", "u3k5_c128", "u6k10_c64", "u5k9_c32", "u3k5_c16"]   # one per stage width: 256, 128, 64, 32, 16, 8


def _resblock_steps(case, B, L):
    cfg = _cfg(case)
    st = rbn_shapes.stage_tiles(cfg, B, L, _cus()) if _narrow(case) else vk.stage_tiles(cfg, B, L, _cus())
    return sorted(set(st.values()))


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("case", SEAM_CASES)
def test_resblock_seams_at_stage_lengths_of_odd_rates(case, mode):
    """the ResBlock kernels' own tile seams (the existing helpers' tile steps) met by stage lengths that are multiples of 3, 5 or 6 instead of 2:
    for every tile step s the utterance lengths whose stage rows end just below and just at / above 2 s"""
    u, B = ups.CASES[case]["u"], 6
    lens = []
    for _ in range(2):   # (the steps depend on the padded length: settle it once)
        steps = _resblock_steps(case, B, max(lens) * u if lens else 4096)
        lens = sorted({n for s in steps for n in ((2 * s) // u, -(-(2 * s) // u), (2 * s) // u + 1)})[-B:]
    lens = lens + lens[:B - len(lens)]
    model = _model(case, mode)
    _check(case, mode, model, [_mel(n, q) for q, n in enumerate(lens)], f"resblock seams steps={steps}")


# ------------------------------------------------------------------------------------------------ a used workspace
@pytest.mark.parametrize("case", ["u3k5_c64", "u5k9_c64", "u3k5_c128", "u5k9_c128", "u3k5_c32", "u5k9_c32", "u3k5_c16", "u5k9_c16"])
def test_dirty_workspace(case):
    """a long batch, then the ragged batch on the same model (its workspace now holds the long batch's rows behind every utterance's end): the
    same bits as on a fresh model"""
    for mode in ("f16_release", "bf16"):
        short, longer = ups.tile_lengths(case, mode)
        ragged = [_mel(longer, 9)] + [_mel(n, q) for q, n in enumerate(short)]
        used = _model(case, mode)
        _run(used, [_mel(longer + 16 + 3 * q, 20 + q) for q in range(6)])
        assert np.array_equal(_run(used, ragged), _run(_model(case, mode), ragged)), (case, mode)


# ------------------------------------------------------------------------------------------------ conv1d.hip: bf16x3, and bf16 per convolution
X3_CASES = {64: ["u4k4_c64", "u3k5_c64", "u6k12_c64"], 16: ["u4k4_c16", "u3k5_c16", "u6k12_c16"]}


@pytest.mark.parametrize("c0", [64, 16])
def test_forms_in_bf16x3_and_unfused(c0):
    """DTTS_VOC_BF16X3 runs every convolution on conv1d.hip (K = 1 for the single form, the 3-tap pack otherwise) and is compared with the
    float64 oracle (Emulator(rounding=False)); the control (2, 4) is measured in the same run and each form stays within 2 x its values (the
    arithmetic is the same, only the tap pattern differs).  DTTS_VOC_BF16 convolution by convolution (vocoder_unfused) against the bf16 emulator
    with conv_post on the serial path."""
    lens = (150, 33, 401)
    mels = [_mel(n, q) for q, n in enumerate(lens)]
    worst = {}
    for case in [(c0, 2, 4)] + X3_CASES[c0]:
        cfg, raw, _ = _sd(case)
        model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16x3")
        assert model.precision == abi.VOC_BF16X3
        full = _run(model, mels)
        vals = [seam_check(full[b, :m.shape[0] * model.hop], _emulate(case, "f16", m, rounding=False), {})[0] for b, m in enumerate(mels)]
        worst[case] = {k: max(v[k] for v in vals) for k in ("max", "win", "rms")}
        print("VOCMEAS " + json.dumps({"case": str(case), "mode": "bf16x3", "what": "vs float64", "x3": worst[case]}), flush=True)
    control = worst[(c0, 2, 4)]
    for case in X3_CASES[c0]:
        for k in ("max", "win", "rms"):
            assert worst[case][k] <= 2 * control[k], (case, k, worst[case], control)
            assert worst[case][k] <= X3_BOUNDS[k], (case, k, worst[case])
    for k in ("max", "win", "rms"):
        assert control[k] <= X3_BOUNDS[k], control
    for case in X3_CASES[c0]:
        model = _model(case, "bf16", unfused=True)
        _check(case, "bf16", model, mels, "bf16 per convolution", bounds=BOUNDS["bf16"], want=lambda m, case=case: _emulate(case, "bf16", m, fused_post=False))


# ------------------------------------------------------------------------------------------------ three stages, a form each
@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_three_stage_generator(mode):
    model = _model("mixed", mode)
    assert model.hop == 60
    _check("mixed", mode, model, [_mel(40)], "B=1")
    _check("mixed", mode, model, [_mel(n, q) for q, n in enumerate((17, 64, 33, 5, 48))], "ragged B=5")


# ------------------------------------------------------------------------------------------------ memory-safety mode
@pytest.mark.parametrize("case", ["u4k4_c512", "u3k5_c512", "u5k9_c128", "u6k12_c64", "u3k3_c64", "u5k9_c32", "u4k4_c32", "u3k5_c16", "u5k9_c16", "u4k4_c16"])
def test_memory_safety_mode_is_clean(case):
    """dtts_config.debug_redzone: every workspace buffer and weight pack between red zones, the workspace filled with NaN (a read of a row no kernel
    wrote shows); 0 damaged bytes, the same bits as the release context.  Every form, and the stage widths 256, 64, 16 and 8."""
    mels = [_mel(n, q) for q, n in enumerate((33, 7, 64))]
    for mode in ("f16_release", "bf16"):
        model = _model(case, mode, dtts_debug_redzone=1)
        got = _run(model, mels)
        n = model.ctx.debug_check(torch.cuda.current_stream().cuda_stream)
        assert n == 0, model.ctx.last_error()
        assert np.array_equal(got, _run(_model(case, mode), mels)), (case, mode)


# ------------------------------------------------------------------------------------------------ every sample is written
@pytest.mark.parametrize("precision,unfused", [("f16", False), ("bf16", False), ("bf16x3", False), ("bf16", True)])
@pytest.mark.parametrize("case", ["u3k5_c32", "u5k9_c32", "u3k5_c16", "u5k9_c16"])
def test_every_sample_is_written(case, precision, unfused):
    """dtts_hifigan_forward into a NaN-filled waveform where the upsampler's rows are narrower than its pack (u C_out = 48, 80, 24, 40 under 64, 96,
    32, 64): with lens = NULL every sample comes from a kernel; with short lens the samples past lens * hop are exact zeros"""
    cfg, raw, _ = _sd(case)
    model = vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision, unfused=unfused)
    hop = model.hop
    lens = [40, 17, 64, 1]
    Tm = max(lens)
    mel_d = T(np.stack([_mel(Tm, b) for b in range(len(lens))])).cuda()
    stream = torch.cuda.current_stream()
    for short in (False, True):
        wav = torch.full((len(lens), Tm * hop), float("nan"), dtype=torch.float32, device="cuda")
        lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda") if short else None
        model.ctx.hifigan_forward(mel_d.data_ptr(), lens_d.data_ptr() if short else None, len(lens), Tm, wav.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        w = wav.cpu().numpy()
        assert np.isfinite(w).all(), (case, precision, unfused, short, int((~np.isfinite(w)).sum()))
        if short:
            for b, n in enumerate(lens):
                assert float(np.abs(w[b, n * hop:]).max(initial=0.0)) == 0.0, (b, n)
                assert float(np.abs(w[b, :n * hop]).max()) > 0.0


# ------------------------------------------------------------------------------------------------ the static fp16 bound's phase rule
def _peak_by_convolution(fsd, cfg, M):
    """the largest worst-case bound of any fp16 ResBlock operand for |mel| <= M, the upsamplers taken by an independent route: F.conv_transpose1d
    of |w| (and |b|) on a constant input of the per-channel bounds, the interior rows' maximum per channel — no phase slicing"""
    g = lambda k: fsd[k].double()
    conv = lambda name, u: g(name + ".bias").abs() + g(name + ".weight").abs().sum(2) @ u
    nk = len(cfg["resblock_kernel_sizes"])
    u = conv("conv_pre", torch.full((80,), float(M), dtype=torch.float64))
    peak = 0.0
    for i, (r, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        y = F.conv_transpose1d(u.view(1, -1, 1).expand(1, -1, 16).contiguous(), g(f"ups.{i}.weight").abs(), g(f"ups.{i}.bias").abs(), stride=r,
                               padding=(k - r) // 2)
        assert y.shape[2] == 16 * r
        x0 = y[0, :, 4 * r:12 * r].max(dim=1).values   # rows whose three input offsets all exist
        us = 0.0
        for j in range(nk):
            x = x0.clone()
            for m in range(3):
                peak = max(peak, float(x.max()))
                xt = conv(f"resblocks.{i * nk + j}.convs1.{m}", x)
                peak = max(peak, float(xt.max()))
                x = x + conv(f"resblocks.{i * nk + j}.convs2.{m}", xt)
            us = us + x / nk
        u = us
    return peak


@pytest.mark.parametrize("case", ["u3k5_c64", "u5k9_c64", "u4k6_c64", "u5k7_c64", "u6k10_c64", "u8k12_c64", "u3k3_c64", "u5k9_c16", "mixed"])
def test_static_fp16_bound_general_forms(case):
    """dtts_vocoder_fp16_bound (vocoder.hip: output phase ph collects the taps k == ph + pad mod r) is at least the peak found without that rule.
    The checkpoint carries plain weights (no weight norm to fold), so that both sides start from the same fp32 values.  FAILED BEFORE THE FIX at
    M = 6 in every case (the slope taken behind the maximum over phases: the file's docstring)."""
    cfg, raw, fsd = _sd(case, weight_norm=False)
    v = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    for M in (1.0, 6.0):
        got, want = v.ctx.vocoder_fp16_bound(M)[0], _peak_by_convolution(fsd, cfg, M)
        print("VOCMEAS " + json.dumps({"case": case, "what": "fp16 bound", "M": M, "library": got, "independent": want}), flush=True)
        assert got >= want * (1 - 1e-9), (case, M, got, want)
        assert got <= 2 * want, (case, M, got, want)   # (max a + M max b <= peak(0) + peak(M) <= 2 peak(M))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("u,k", ups.REFUSED)
def test_unsupported_forms_are_refused_by_name(u, k):
    """refused at dtts_finalize_weights with the layer, k and the stride in the message, in every precision; AUTO raises too (no fallback to bf16x3:
    the shape is wrong, not the arithmetic).  FAILED BEFORE THE FIX for odd k - u and k < u: the model was built and its waveform had the length
    T u, which the reference does not produce.  A supported model still builds and runs afterwards."""
    cfg = ups.iso(64, u, k)
    raw = {n: T(v) for n, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}
    for precision in ("f16", "bf16", "bf16x3", None):
        with pytest.raises(abi.DttsError) as e:
            vocoder.HifiGAN(state_dict=raw, config=cfg, precision=precision)
        msg = str(e.value)
        assert "ups.0" in msg and f"k={k}" in msg and f"stride={u}" in msg, msg
    model = _model("u3k5_c64", "f16_release")
    _check("u3k5_c64", "f16_release", model, [_mel(40)], "after a refusal")
