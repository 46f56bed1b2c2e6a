"""CPU side of the FFT-block tests (tests/test_fft_blocks_gpu.py): the shape table reaches the branches it names, by the launch rules
restated in tests/fft_shapes.py from constants READ out of conv1d.hip and ops.hip; the float64 reference (tests/fft_ref.py) is the fp32
oracle up to the oracle's own rounding; and every defect the reference can plant exceeds FFT_BOUNDS on a seam case of the GPU file, so
a kernel with that defect would fail there."""
import json

import numpy as np
import pytest
import torch

import fft_ref as fr
import fft_shapes as fs
import golden_cases as gc
from dict_tts_amd import synth
from oracle import fft_blocks_ref as oref

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def test_launch_rule_constants_are_read_from_the_sources():
    """the numbers the rule was restated with; another value in conv1d.hip / ops.hip means the table has to be looked at again"""
    assert fs.constants() == {"SHORT_LDS_KB": 150, "SHORT_TILES": 256, "MHX_DK": 96, "MHA_DK_MAX": 96, "MHA_SPLIT_T": 128}
    # the two figures of the issue: ffn_2 at hidden 192 just fits the three-piece tile, at hidden 256 it does not
    assert 32 * (768 * 2 + 16) * 3 == 148992 and fs.conv_kernel(768, 1, 1, 32) == "short_x6"
    assert fs.conv_kernel(1024, 1, 8, 1024) == "short_f32" and fs.conv_kernel(1024, 1, 8, 1025) == "generic"


@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_every_shape_reaches_the_branch_in_its_name(name):
    s = fs.SHAPES[name]
    assert 1 <= s["layers"] <= 2 and max(s["lens"]) == s["T"] and min(s["lens"]) >= 1
    assert f"h{s['hidden']}" in name.split("_")[0] and s["hidden"] % s["heads"] == 0 and s["hidden"] // s["heads"] <= 96
    small = fs.kernels(s, len(s["lens"]), s["T"])
    for launch, kern in s["expect"].items():
        assert small[launch] == kern, (name, launch, small)
    if s["repeat"]:
        big = fs.kernels(s, len(s["lens"]) * s["repeat"], s["T"])
        for launch, kern in s["big"].items():
            assert big[launch] == kern, (name, launch, big)
    # what the name says
    dk = s["hidden"] // s["heads"]
    if "mha_dk" in name:
        assert f"mha_dk{dk}" in name and small["mha"] == "scalar"
    if "mfma_c384" in name:
        assert s["hidden"] == 384 and small["mha"] == "mfma"
    if "ffn2_f32_short_or_generic" in name:
        assert small["ffn2"] == "short_f32" and big["ffn2"] == "generic"
    if "ffn2_generic" in name:
        assert small["ffn2"] == "generic"
    if "ffn1_generic_gelu" in name:
        assert small["ffn1"] == "short_f32" and big["ffn1"] == "generic"
    if "_k" in name:
        assert name.endswith(f"_k{s['k']}")
    if s["hidden"] == 192:   # every convolution keeps the three-piece short kernel at any batch
        for B in (1, len(s["lens"]), 90, 4096):
            assert set(v for k, v in fs.kernels(s, B, s["T"]).items() if k != "mha") == {"short_x6"}


def test_table_covers_every_conv_and_attention_branch():
    seen = set()
    for s in fs.SHAPES.values():
        for B in (len(s["lens"]), len(s["lens"]) * s["repeat"]):
            if B:
                seen |= set(fs.kernels(s, B, s["T"]).items())
    for need in (("ffn1", "generic"), ("ffn1", "short_f32"), ("ffn1", "short_x6"), ("ffn2", "short_f32"), ("ffn2", "generic"), ("ffn2", "short_x6"),
                 ("mha", "mfma"), ("mha", "mfma_split"), ("mha", "scalar")):
        assert need in seen, need
    assert {s["k"] for s in fs.SHAPES.values()} >= {1, 3, 9, 13}


@pytest.mark.parametrize("which", ["dec", "enc"])
def test_float64_reference_is_the_fp32_oracle_up_to_its_rounding(golden_dir, which):
    """on the G8 inputs: fft_ref.forward in fp32 and the oracle differ by fp32 rounding only, the float64 reference and the oracle by the
    oracle's own error; the golden output (the reference repository's own FFTBlocks) lies as close"""
    import os
    cfg = gc.G8_CASES[which]
    sd_np = synth.fft_blocks_state_dict(gc.SEED, 192, **cfg)
    sd_np.pop("embed_positions._float_tensor", None)
    x, lens = gc.g8_inputs(which)
    kw = dict(num_heads=2, kernel_size=cfg["kernel_size"], use_pos_embed=cfg["use_pos_embed"], use_last_norm=cfg["use_last_norm"])
    want32 = oref.fft_blocks({k: T(v) for k, v in sd_np.items()}, T(x), **kw)
    tab = fr.table(2000, 192)
    got64 = fr.forward(fr.state(sd_np), T(x).double(), pos_table=tab, **kw)
    got64m = fr.forward(fr.state(sd_np), T(x).double(), lens=lens, pos_table=tab, **kw)
    assert torch.equal(got64, got64m)
    got32 = fr.forward({k: T(v) for k, v in sd_np.items()}, T(x), pos_table=tab.float(), **kw)
    gold = np.load(os.path.join(golden_dir, "g8_fft_blocks.npz"))[which + ".out"]
    e = {"oracle32_vs_ref64": fr.rowcmp(want32, got64), "ref32_vs_oracle32": fr.rowcmp(got32, want32), "golden_vs_ref64": fr.rowcmp(gold, got64)}
    for k, v in e.items():
        print("FFTMEAS " + json.dumps({"case": "g8." + which, "what": k, **v}), flush=True)
    # fp32 rounding of values of magnitude <= ~4 through 2 / 4 layers: a few 1e-6; a semantic difference would be 1e-3 or more
    assert e["oracle32_vs_ref64"]["max"] <= 2e-5 and e["oracle32_vs_ref64"]["rms"] <= 2e-6, e
    assert e["ref32_vs_oracle32"]["max"] <= 2e-5 and e["golden_vs_ref64"]["max"] <= 2e-5, e
    for b, n in enumerate(lens):
        assert not (got64[b, n:] != 0).any()


def _seam_cases():
    """the seam cases of the GPU file the planted defects are tried on: name -> (state dict, x, lens, forward kwargs)"""
    s = fs.SEAM_SHAPE
    sd = fr.state(fs.state_np(s))
    kw = dict(num_heads=s["heads"], kernel_size=s["k"], pos_table=fr.table(2000, s["hidden"]))
    x, _ = fs.seam_input(False)
    xm, lens = fs.seam_input(True)
    xq, qlens = fs.quiet_input()
    sdq = fr.state(fs.state_np(s, use_pos_embed=False))
    return {"seam.derived": (sd, T(x).double(), None, kw), "seam.mask": (sd, T(xm).double(), lens, kw),
            "switch.no_pos_quiet": (sdq, T(xq).double(), None, dict(num_heads=s["heads"], kernel_size=s["k"], use_pos_embed=False))}


@pytest.fixture(scope="module")
def seam_refs():
    cases = _seam_cases()
    return cases, {k: fr.forward(sd, x, lens=lens, **kw) for k, (sd, x, lens, kw) in cases.items()}


@pytest.mark.parametrize("defect", fr.DEFECTS)
def test_every_planted_defect_exceeds_the_bounds_on_a_seam_case(seam_refs, defect):
    """the GPU tests compare with FFT_BOUNDS: a kernel with this defect would differ from the float64 reference by what the defective
    reference differs from the clean one, far more than the bounds, on at least one seam case"""
    cases, clean = seam_refs
    caught = []
    for name, (sd, x, lens, kw) in cases.items():
        bad_out = fr.forward(sd, x, lens=lens, defect=defect, **kw)
        true_lens = lens if lens is not None else [int(n) for n in x.abs().sum(-1).ne(0).sum(1)]
        if fr.compare(f"{defect}@{name}", bad_out, clean[name], true_lens, fr.bounds_of(192)):
            caught.append(name)
    assert caught, f"{defect} stays inside FFT_BOUNDS on every seam case: strengthen the cases"
    if defect in ("pos_off_by_one", "carry_lost_256"):      # the position defects must show under BOTH kinds of padding
        assert {"seam.derived", "seam.mask"} <= set(caught), caught
    if defect == "ln_eps_1e-12":
        assert "switch.no_pos_quiet" in caught, caught


def test_position_seams_sit_on_the_wave_and_chunk_boundaries():
    """the seam input: first-channel-zero frames next to the 64-lane and 256-frame boundaries of fft_positions_kernel; the positions of
    the reference skip them without advancing, whatever the explicit mask says"""
    x, _ = fs.seam_input(False)
    pos = fr.make_positions(T(x)[..., 0])
    assert {t for b, t in fs.SEAM_ZERO if b == 0} == {0, 63, 64, 255, 256, 511, 512} and (1, fs.SEAM_LENS[1] - 1) in fs.SEAM_ZERO
    for b, t in fs.SEAM_ZERO:
        assert pos[b, t] == 0
    assert pos[0, 1] == 1 and pos[0, 62] == 62 and pos[0, 65] == 63 and pos[0, 254] == 252 and pos[0, 257] == 253 and pos[0, 510] == 506
    assert pos[1, 255] == 256 and pos[1, 257:].eq(0).all() and pos[2, 255] == 256 and pos[2, 256:].eq(0).all()
    xm, lens = fs.seam_input(True)
    posm = fr.make_positions(T(xm)[..., 0])
    assert list(lens) == list(fs.SEAM_LENS) and posm[1, 299] == 299 and posm[2, 270] == 0 and posm[2, 289] == 289   # counted past the mask
    # ... and the defective position rules differ from it exactly where they should
    assert (fr.make_positions(T(x)[..., 0], "carry_lost_256")[0, :256] == pos[0, :256]).all()
    assert fr.make_positions(T(x)[..., 0], "carry_lost_256")[0, 257] == 1
    assert fr.make_positions(T(x)[..., 0], "pos_off_by_one")[2, 255] == 256 and fr.make_positions(T(x)[..., 0], "pos_off_by_one")[0, 1] == 2
