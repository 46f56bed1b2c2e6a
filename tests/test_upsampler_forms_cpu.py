"""The vocoder's polyphase upsamplers at every accepted form and width, on the CPU: the case table of tests/ups_shapes.py against the
launcher's rules, the reference and the rounding-point emulator at those forms, and the planted upsampler defects that the bounds of
tests/test_upsampler_forms_gpu.py must catch."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ups_shapes as ups
from dict_tts_amd import synth
from hifigan_v2_bounds import NARROW_BOUNDS
from oracle import hifigan_ref as href
from vocoder_emul import BOUNDS, Emulator, seam_check

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SEED = 1234
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_SD = {}


def _sd(case):
    if case not in _SD:
        cfg = ups.MIXED if case == "mixed" else ups.CASES[case]["cfg"]
        _SD[case] = (cfg, href.fold_weight_norm({k: T(v) for k, v in synth.hifigan_state_dict(SEED, cfg=cfg).items()}))
    return _SD[case]


def _emu(case, mode, **kw):
    cfg, fsd = _sd(case)
    return Emulator(fsd, cfg, mode=mode, fused_post=True if ups.narrow(case) else None, **kw)


def _bounds(case, mode):
    return (NARROW_BOUNDS if ups.narrow(case) else BOUNDS)[mode]


# ------------------------------------------------------------------------------------------------ the table
def test_every_case_has_the_form_its_row_claims():
    for name, c in ups.CASES.items():
        assert ups.accepted(c["u"], c["k"]), name
        assert ups.polyphase_form(c["u"], c["k"], c["c0"] // 2) == c["form"], name
    assert {c["form"] for c in ups.CASES.values()} == {"single", "half", "general"}
    # the forms of the issue's table, each at upsample_initial_channel = 64, and three of them at every other width
    assert {(c["u"], c["k"]) for c in ups.CASES.values() if c["c0"] == 64} == {(4, 4), (3, 3), (6, 12), (4, 6), (8, 12), (3, 5), (5, 7), (5, 9), (6, 10), (2, 4)}
    for c0 in (512, 256, 128, 32, 16):
        assert {(c["u"], c["k"]) for c in ups.CASES.values() if c["c0"] == c0} >= {(3, 5), (5, 9), (4, 4)}
    # k = 2u is `half` only where the packed channels split into whole waves: at 8 channels (6, 12) would be `general`
    assert ups.polyphase_form(6, 12, 8) == "general" and ups.polyphase_form(2, 4, 32) == "half" and ups.polyphase_form(8, 16, 256) == "half"
    # the mixed generator: a different form per stage
    widths = [ups.MIXED["upsample_initial_channel"] >> (i + 1) for i in range(3)]
    assert widths == [128, 64, 32] and int(np.prod(ups.MIXED["upsample_rates"])) == 60
    assert [ups.polyphase_form(u, k, w) for u, k, w in zip(ups.MIXED["upsample_rates"], ups.MIXED["upsample_kernel_sizes"], widths)] == ["single", "general", "general"]


def test_the_restated_launcher_lists_the_sources_instantiations():
    """ups_shapes.ALL_BRANCHES is what vconv_launch can return: every `vlaunch<..>` (both operand forms) and `vlaunch_x<.., true>` of its text"""
    src = open(os.path.join(ROOT, "dict_tts_amd", "csrc", "vconv.hip")).read()
    body = src[src.index("hipError_t vconv_launch("):src.index("// mel fp32 [rows][C]")]
    found = set()
    for x, args in re.findall(r"return vlaunch(_x)?<([^>]+)>\(p, stream\)", body):
        a = [s.strip() for s in args.split(",")]
        if x:
            assert a[5] == "true" and len(a) == 6
            found.add(tuple(int(v) for v in a[:5]) + (True,))
        else:
            assert len(a) == 5
            found |= {tuple(int(v) for v in a) + (x3,) for x3 in (True, False)}
    assert found == ups.ALL_BRANCHES
    assert body.count("return vlaunch") == 17


def test_the_table_reaches_every_launcher_branch_an_upsampler_can_reach():
    """over the table, in DTTS_VOC_F16 (split operands, small_tiles) and in DTTS_VOC_BF16: exactly the instantiations an upsampler of a
    generator with upsample_initial_channel in {16 .. 512} and u <= 8 can reach; every other one is listed by name with the reason"""
    table = {m: {ups.launch_of(c, m)[0] for c in ups.CASES} for m in ("f16", "bf16")}
    assert table["f16"] == ups.reachable_branches(True), ups.reachable_branches(True) - table["f16"]
    assert table["bf16"] == ups.reachable_branches(False), ups.reachable_branches(False) - table["bf16"]
    assert all(b[5] for b in table["f16"]) and not any(b[5] for b in table["bf16"])
    assert ups.ALL_BRANCHES - table["f16"] - table["bf16"] == set(ups.NOT_AN_UPSAMPLER)
    assert all(len(why) > 20 for why in ups.NOT_AN_UPSAMPLER.values())
    # the tile sizes the lengths of the GPU tests come from: 64, 128, 256 and 512 input rows
    assert {ups.launch_of(c, m)[1] for c in ups.CASES for m in ("f16", "bf16")} == {64, 128, 256, 512}
    # C_out < C_out_pad (the stores that must stop at C_out) at 16 and 8 channels
    pads = {(c["u"] * c["c0"] // 2, ups.pad32(c["u"] * c["c0"] // 2)) for c in ups.CASES.values() if c["c0"] <= 32}
    assert {(24, 32), (40, 64), (48, 64), (80, 96)} <= pads


# ------------------------------------------------------------------------------------------------ the reference and the emulator
def test_polyphase_sum_is_conv_transpose1d():
    g = torch.Generator().manual_seed(3)
    for u, k in sorted({(c["u"], c["k"]) for c in ups.CASES.values()}):
        a = torch.randn(2, 6, 9, generator=g, dtype=torch.float64)
        w = torch.randn(6, 5, k, generator=g, dtype=torch.float64)
        b = torch.randn(5, generator=g, dtype=torch.float64)
        want = F.conv_transpose1d(a, w, b, stride=u, padding=(k - u) // 2)
        assert want.shape[2] == 9 * u
        assert float((ups.polyphase(a, w, b, u, k) - want).abs().max()) <= 1e-12, (u, k)


@pytest.mark.parametrize("case", list(ups.CASES))
def test_reference_and_emulator_at_every_form(case):
    """the oracle yields exactly T * hop samples, far from tanh saturation (it would hide errors); the emulator in f16 mode is within the
    GPU tests' f16 bounds of it (measured at 40 frames: max 6e-5 .. 1.5e-4, RMS <= 4.7e-5)"""
    cfg, fsd = _sd(case)
    mel = synth.random_mel(500, 40, "upsform")
    ref = href.spec2wav(fsd, cfg, mel).numpy().astype(np.float64)
    assert ref.shape == (40 * ups.CASES[case]["u"],)
    assert np.mean(np.abs(ref) > 0.9) < 0.01
    emu = _emu(case, "f16").spec2wav(mel)
    vals, fails = seam_check(emu, ref, BOUNDS["f16"])
    print(f"\n[{case}] oracle peak {np.abs(ref).max():.3f}; emulator - oracle max {vals['max']:.2e} win {vals['win']:.2e} rms {vals['rms']:.2e}")
    assert not fails, (case, vals)


def test_reference_of_the_mixed_generator():
    cfg, fsd = _sd("mixed")
    mel = synth.random_mel(501, 40, "upsform")
    ref = href.spec2wav(fsd, cfg, mel).numpy().astype(np.float64)
    assert ref.shape == (40 * 60,) and np.mean(np.abs(ref) > 0.9) < 0.01
    vals, fails = seam_check(Emulator(fsd, cfg, mode="f16").spec2wav(mel), ref, BOUNDS["full_f16"])
    assert not fails, vals


# ------------------------------------------------------------------------------------------------ planted defects
_TT = ups.launch_of("u3k5_c64", "f16")[1]
PLANTED = [   # (case, defect, frames, input row the defect concerns)
    ("u3k5_c64", "plus_tap_at_end", 40, None), ("u3k5_c64", "minus_tap_at_start", 40, None), ("u3k5_c64", "phase_rotated", 40, None),
    ("u3k5_c64", "pad_off_by_one", 40, None), ("u3k5_c64", "seam_tap_dropped", _TT + 8, _TT - 1),
    ("u6k12_c64", "plus_tap_at_end", 40, None), ("u6k12_c64", "minus_tap_at_start", 40, None),
    ("u4k4_c64", "phase_rotated", 40, None), ("u4k4_c64", "pad_off_by_one", 40, None),
    ("u5k9_c16", "pad_channel_store", 40, 20), ("u5k9_c16", "plus_tap_at_end", 40, None), ("u5k9_c16", "phase_rotated", 40, None),
]
_CLEAN = {}


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("case,defect,frames,at", PLANTED, ids=[f"{c}-{d}" for c, d, _, _ in PLANTED])
def test_planted_upsampler_defects_exceed_the_gpu_bounds(case, defect, frames, at, mode):
    """an upsampler defect planted through the emulator's hook (ups.0 replaced by the restated polyphase sum carrying it) against the clean
    emulator: beyond the bounds the GPU tests hold this case to, in the fp16 and in the bf16 group"""
    assert at is None or defect != "seam_tap_dropped" or at == ups.launch_of(case, mode)[1] - 1   # (the last row of the case's first tile in this mode)
    mel = synth.random_mel(600 + frames, frames, "upsdefect")
    if (case, mode, frames) not in _CLEAN:
        _CLEAN[(case, mode, frames)] = _emu(case, mode).spec2wav(mel)
        # the hook without a defect changes nothing but the summation order
        same = _emu(case, mode, hook=ups.planted(None)).spec2wav(mel)
        assert seam_check(same, _CLEAN[(case, mode, frames)], {})[0]["max"] <= 0.1 * _bounds(case, mode)["max"]
    clean = _CLEAN[(case, mode, frames)]
    bad = _emu(case, mode, hook=ups.planted(defect, at)).spec2wav(mel)
    bounds = _bounds(case, mode)
    vals, fails = seam_check(bad, clean, bounds)
    print(f"\n[{case} {defect} {mode}] max {vals['max']:.3e} win {vals['win']:.3e} rms {vals['rms']:.3e} at sample {vals['argmax']}; bounds {bounds}")
    assert "max" in fails and vals["max"] >= 5 * bounds["max"], (vals, bounds)   # (measured: 7x the bf16 bound at the least, 95x the f16 one)


# ------------------------------------------------------------------------------------------------ refusals (the rule)
def test_refused_forms_are_the_ones_the_reference_cannot_match():
    """odd k - u: ConvTranspose1d(padding=(k - u) // 2) yields T u + 1 rows, one more than every stage of the library holds; k < u: its padding
    would be negative, which PyTorch refuses; k > 2u: more than the three taps of the polyphase pack.  The GPU test checks the refusal itself."""
    x = torch.zeros(1, 4, 40)
    for u, k in ups.REFUSED:
        assert not ups.accepted(u, k), (u, k)
        w = torch.zeros(4, 2, k)
        if k < u:
            with pytest.raises(RuntimeError):
                F.conv_transpose1d(x, w, stride=u, padding=(k - u) // 2)   # (the reference's floor division: -1 for both (4, 2) and (4, 3))
        elif (k - u) % 2:
            assert F.conv_transpose1d(x, w, stride=u, padding=(k - u) // 2).shape[2] == 40 * u + 1
    for u in range(1, 9):
        for k in range(1, 20):
            if ups.accepted(u, k):
                assert F.conv_transpose1d(x, torch.zeros(4, 2, k), stride=u, padding=(k - u) // 2).shape[2] == 40 * u
    assert all(ups.accepted(c["u"], c["k"]) for c in ups.CASES.values())
    assert all(ups.accepted(u, k) for u, k in zip(ups.MIXED["upsample_rates"], ups.MIXED["upsample_kernel_sizes"]))
