"""HifiGAN V2 generators (``resblock "1"``, ``upsample_initial_channel`` 128: stage widths 64 / 32 / 16 / 8) on the CPU: the configuration,
the synthetic checkpoint, the oracle against the golden taken from the reference implementation (tests/golden/g14_hifigan_v2.npz,
tools/make_golden_v2.py), the rounding emulator's waveform error, the tile rule of the narrow whole-ResBlock kernel (tests/rbn_shapes.py
restates dict_tts_amd/csrc/rbn.h / rbn.hip) and — the point of the per-sample bounds — defects the new kernel could have, planted through
the emulator, which must exceed the bounds the GPU test (tests/test_hifigan_v2_gpu.py) applies."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import rbn_shapes as shp
from dict_tts_amd import hparams as hp
from dict_tts_amd import synth
from oracle import hifigan_ref as href
from hifigan_v2_bounds import NARROW_BOUNDS
from vocoder_emul import BOUNDS, Emulator, seam_check

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
V2 = synth.hifigan_config_v2()


def _iso(c0, rk=(3, 7, 11), rd=((1, 3, 5),) * 3):
    return {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": list(rk), "resblock_dilation_sizes": [list(d) for d in rd]}


def _folded(cfg, seed=gc.SEED):
    return href.fold_weight_norm({k: T(v) for k, v in synth.hifigan_state_dict(seed, cfg=cfg).items()})


@pytest.fixture(scope="module")
def v2():
    return V2, _folded(V2)


def test_v2_config_is_the_released_one():
    assert V2 == hp.HIFIGAN_V2 == {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
                                   "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 7, 11],
                                   "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
    assert {**synth.hifigan_config(), "upsample_initial_channel": 128} == V2   # V1 at a quarter of the width


def test_synthetic_state_dict_names_and_shapes(golden_dir):
    sd = synth.hifigan_state_dict(gc.SEED, cfg=V2)
    g = np.load(os.path.join(golden_dir, "g14_hifigan_v2.npz"))
    assert sorted(sd) == [str(n) for n in g["state_dict_names"]]   # the reference generator's own names
    assert sd["conv_pre.weight_v"].shape == (128, 80, 7) and sd["conv_post.weight_v"].shape == (1, 8, 7)
    for i, (ch, k) in enumerate(zip((64, 32, 16, 8), (16, 16, 4, 4))):
        assert sd[f"ups.{i}.weight_v"].shape == (2 * ch, ch, k)
        for j, rk in enumerate((3, 7, 11)):
            for m in range(3):
                assert sd[f"resblocks.{3 * i + j}.convs1.{m}.weight_v"].shape == (ch, ch, rk)
                assert sd[f"resblocks.{3 * i + j}.convs2.{m}.weight_v"].shape == (ch, ch, rk)
    assert len(sd) == 3 * (2 + 4 + 12 * 6)


def test_oracle_reproduces_the_reference_golden(v2, golden_dir):
    cfg, fsd = v2
    g = np.load(os.path.join(golden_dir, "g14_hifigan_v2.npz"))
    w = href.spec2wav(fsd, cfg, gc.g6_mel()).numpy()
    assert w.shape == g["wav"].shape == (gc.g6_mel().shape[0] * 256,)
    assert np.abs(w - g["wav"]).max() <= 2e-5   # the oracle's tolerance against G6 / G13 (tests/test_oracle_golden.py)
    _, st = Emulator(fsd, cfg, rounding=False, dtype=torch.float32).forward(T(gc.g6_mel()).T.unsqueeze(0), return_stages=True)
    for name in ["ups.0", "ups.1", "ups.2", "ups.3", "post"]:
        assert np.abs(st[name][0, :, :64].numpy() - g[name + ".head"]).max() <= 2e-5 * max(1.0, float(np.abs(g[name + ".head"]).max())), name
        assert abs(float(st[name].pow(2).mean().sqrt()) - float(g[name + ".rms"])) <= 1e-5, name


def test_rounding_off_is_the_oracle_in_float64(v2):
    cfg, fsd = v2
    mel = T(gc.g6_mel()).T.unsqueeze(0).double()
    want = href.generator_forward({k: v.double() for k, v in fsd.items()}, cfg, mel)
    got = Emulator(fsd, cfg, rounding=False, fused_post=True).forward(mel)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12


def test_emulated_f16_waveform_error_is_inside_the_gate(v2):
    """BASELINE.json north_star: RMS(gpu - ref) <= 1e-4.  The rounding scheme of rblock, which rbn.hip keeps, emulated on the synthetic V2
    weights: 4.75e-5 on g6_mel whether conv_post is fused or serial (V1: 6.7e-5); bf16 operands ~1e-3, outside it as on V1."""
    cfg, fsd = v2
    mel = gc.g6_mel()
    ref = href.spec2wav(fsd, cfg, mel).numpy()
    for fused in (True, False):
        w = Emulator(fsd, cfg, fused_post=fused).spec2wav(mel)
        e = rms(w - ref)
        print(f"\n[V2 emulator vs oracle] fused_post={fused}: f16 {e:.3e}")
        assert 3.5e-5 <= e <= 6.5e-5 and abs(rms(w) - rms(ref)) <= 1e-4, e
    ebf = rms(Emulator(fsd, cfg, mode="bf16", fused_post=True).spec2wav(mel) - ref)
    assert 5e-4 <= ebf <= 2e-3, ebf


# ------------------------------------------------------------------------------------------------ the tile rule
def test_tile_rule_by_hand():
    D = [1, 3, 5]
    assert [shp.padded_taps(C, k) for C in (16, 8) for k in (3, 7, 11)] == [4, 8, 12, 4, 8, 12]
    assert (shp.padded_taps(16, 5), shp.padded_taps(8, 5), shp.padded_taps(16, 9), shp.padded_taps(8, 9)) == (6, 8, 10, 12)
    assert [shp.halo(k, D) for k in (3, 7, 11)] == [12, 36, 60] and shp.halo(5, [2, 4, 5]) == 28 and shp.halo(3, [3, 5, 5]) == 16
    assert shp.guard(16, 11, D) == (12 - 1 - 5) * 5 and shp.guard(16, 3, D) == (4 - 1 - 1) * 5 and shp.guard(8, 5, [2, 4, 5]) == (8 - 1 - 2) * 5
    # six packs + the activation tile with its guard bands + the fp32 output tile
    assert shp.lds_bytes(16, 1024, 11, D, True) == 6 * 6 * 1024 + (1024 + 60) * 32 + 904 * 64 == 129408
    assert shp.lds_bytes(8, 256, 3, D, False) == 6 * 1 * 1024 + (256 + 20) * 16
    # B = 1, a short utterance: 1024- and 512-row tiles would each leave more than half of 256 CUs idle -> 256-row tiles
    assert shp.tile_rows(16, 11, D, 1, 400, True, 256) == 256 - 120 - 6
    assert shp.tile_rows(8, 3, D, 1, 400, False, 256) == 256 - 24
    # B = 3 x 18140 rows: 21 tiles of 898 each (126 <= 256) but 47 of 386 (282 > 256) -> 512-row tiles
    assert shp.tile_rows(16, 11, D, 3, 18140, True, 256) == 512 - 120 - 6
    # a large batch: 1024-row tiles, whose LDS with the largest tile table still fits (129408 + 24584 <= 163840)
    assert shp.tile_rows(16, 11, D, 2048, 12, True, 256) == 1024 - 120 - 6
    assert shp.lds_bytes(16, 1024, 11, D, True) + shp.table_bytes(2048) == 153992
    # the predicate: widths, odd kernels, and >= 32 output rows left in the 256-row tile under the fused conv_post
    assert all(shp.supported(C, k, D) for C in (16, 8) for k in (3, 5, 7, 9, 11))
    assert not shp.supported(32, 3, D) and not shp.supported(24, 3, D) and not shp.supported(16, 4, D) and not shp.supported(16, 13, D)
    assert not shp.supported(8, 3, [0, 1, 1])
    assert shp.supported(16, 11, [6, 6, 6]) and not shp.supported(16, 11, [7, 6, 6])   # halo 105 -> 40 rows; 110 -> 30 rows
    for cfg in (_iso(32), _iso(16), _iso(32, (5, 9, 3), ((2, 4, 5), (1, 2, 3), (3, 5, 5)))):
        tiles = shp.stage_tiles(cfg, 3, 600, 256)
        assert len(tiles) == 3 and sum("+post" in k for k in tiles) == 1 and all(v >= 32 for v in tiles.values())


# ------------------------------------------------------------------------------------------------ bounds
def test_narrow_bounds_do_not_exceed_resblock1s():
    for group, b in NARROW_BOUNDS.items():
        assert set(b) == {"max", "win", "rms"}
        for k, v in b.items():
            assert 0 < v <= BOUNDS[group][k], (group, k)


def test_narrow_bounds_against_the_emulators_own_noise():
    """the one tightened bound (bf16, per sample) is not inside what fp32 summation order alone does to the bf16 rounding points: the float64
    and the float32 evaluation of the emulator differ by 4.4e-4 at most here, a third of it"""
    cfg = _iso(32, (5, 9, 3), ((2, 4, 5), (1, 2, 3), (3, 5, 5)))
    fsd = _folded(cfg)
    mel = synth.random_mel(9, 9000, "x")
    a = Emulator(fsd, cfg, mode="bf16", fused_post=True).spec2wav(mel)
    b = Emulator(fsd, cfg, mode="bf16", fused_post=True, dtype=torch.float32).spec2wav(mel)
    vals, _ = seam_check(a, b, {})
    print(f"\n[bf16 emulator, float64 vs float32] max {vals['max']:.3e} win {vals['win']:.3e} rms {vals['rms']:.3e}")
    assert 2 * vals["max"] <= NARROW_BOUNDS["bf16"]["max"] and 2 * vals["win"] <= NARROW_BOUNDS["bf16"]["win"]


# ------------------------------------------------------------------------------------------------ planted defects
def _resblock(emu, i, j, x, drop_res0=False, w_edit=None, operand_hook=None):
    """Emulator.resblock restated (rblock's rounding points, which rbn.hip keeps) with the defects it cannot express: the iteration-0
    residual left out; an edited convs1 weight of iteration 1"""
    oh = operand_hook or (lambda m, which, a: a)
    k, dils = emu.cfg["resblock_kernel_sizes"][j], emu.cfg["resblock_dilation_sizes"][j]
    p = f"resblocks.{i * emu.nk + j}"
    for m, d in enumerate(dils):
        w1, b1 = emu._w(f"{p}.convs1.{m}.weight", emu.mode), emu.sd[f"{p}.convs1.{m}.bias"]
        w2, b2 = emu._w(f"{p}.convs2.{m}.weight", emu.mode), emu.sd[f"{p}.convs2.{m}.bias"]
        if w_edit is not None and m == 1:
            w1 = w_edit(w1.clone())
        xt = F.conv1d(oh(m, 1, emu.act(x)), w1, b1, padding=(k * d - d) // 2, dilation=d)
        xt = F.conv1d(oh(m, 2, emu.act(xt)), w2, b2, padding=(k - 1) // 2)
        x = xt if (drop_res0 and m == 0) else xt + x
    return x


def _defect_hook(kind, C, s, tt):
    """a stage hook that replaces ResBlock j = 1 (k = 7) of the isolating generator by a defective one.  s: first row of a tile, tt: its rows"""
    k, pad = 7, 3
    tps = 32 // C

    def hook(name, x, emu):
        if name == "ups.0":
            emu.defect_input = x
        if name != "rb.0.1":
            return None
        xin = emu.defect_input
        if kind == "residual0":                       # the iteration-0 residual missing (x = xt instead of xt + x)
            return _resblock(emu, 0, 1, xin, drop_res0=True)
        if kind == "last_tap":                        # the last real tap dropped (read as one of the zero taps the k-steps are padded with)
            def edit(w):
                w[:, :, k - 1] = 0
                return w
            return _resblock(emu, 0, 1, xin, w_edit=edit)
        if kind == "taps_swapped":                    # two taps of one folded k-step swapped (step 1: taps tps .. 2 tps - 1)
            def edit(w):
                w[:, :, [tps, tps + 1]] = w[:, :, [tps + 1, tps]]
                return w
            return _resblock(emu, 0, 1, xin, w_edit=edit)
        if kind == "halo_short":                      # the tile at row s: the last convolution's farthest halo row (s - pad) read as zero
            def oh(m, which, a):
                if (m, which) == (2, 2):
                    a = a.clone()
                    a[:, :, s - pad] = 0
                return a
        elif kind == "stale_tile":                    # the tile at row s runs iteration 1's first convolution on the previous tile's operand
            def oh(m, which, a):
                if (m, which) == (1, 1):
                    a = a.clone()
                    a[:, :, s:s + tt] = a[:, :, s - tt:s].clone()
                return a
        else:
            raise ValueError(kind)
        r = _resblock(emu, 0, 1, xin, operand_hook=oh)
        out = x.clone()
        out[:, :, s:s + tt] = r[:, :, s:s + tt]       # only that tile's rows leave the defective tile
        return out
    return hook


@pytest.mark.parametrize("kind", ["halo_short", "stale_tile", "residual0", "last_tap", "taps_swapped"])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("c0", [32, 16])
def test_planted_defects_exceed_the_gpu_tests_bounds(c0, mode, kind):
    """each defect, planted in ONE ResBlock (k = 7) of the isolating C = 16 / C = 8 generator, against the clean emulator: beyond
    NARROW_BOUNDS["f16"] / ["bf16"], the bounds the GPU test holds the isolating generators to (BOUNDS["bf16"]'s per-sample 3.1e-3 would
    hide the C = 8 halo defect, 1.4e-3: hifigan_v2_bounds.py)"""
    cfg = _iso(c0)
    fsd = _folded(cfg)
    C = c0 >> 1
    tt = shp.tile_rows(C, 7, [1, 3, 5], 1, 400, False, 256)   # 256-row tiles: 184 rows each
    assert tt == 256 - 72
    mel = synth.random_mel(77, 300, "defect")                 # 600 stage rows: tiles at 0, 184, 368, 552
    clean = Emulator(fsd, cfg, mode=mode, fused_post=True).spec2wav(mel)
    bad = Emulator(fsd, cfg, mode=mode, fused_post=True, hook=_defect_hook(kind, C, 2 * tt, tt)).spec2wav(mel)
    bounds = NARROW_BOUNDS[mode]
    vals, fails = seam_check(bad, clean, bounds)
    print(f"\n[C={C} {mode} {kind}] max {vals['max']:.3e} win {vals['win']:.3e} rms {vals['rms']:.3e} at {vals['argmax']}; bounds {bounds}")
    assert "max" in fails, (vals, bounds)
    if kind != "halo_short":                                  # (one row of one tile: the per-sample bound is the one that sees it)
        assert "win" in fails, (vals, bounds)
