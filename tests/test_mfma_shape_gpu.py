"""Two properties of the fused ResBlock kernels (vpair.hip, rblock.hip) that hold for every MFMA shape a kernel family may use
(rb_common.h MfmaShape: v_mfma_f32_32x32x16 or v_mfma_f32_16x16x32) and that a wrong lane map or a per-tile-size choice of shape breaks.

1. Tile-size independence.  The launchers give a single utterance half-size tiles and a large batch full-size tiles; both must sum every
   layer in the same order, so an utterance alone is BIT-identical to the same utterance inside the batch.  The batch is sized from the
   device's CU count with the launchers' own rules, restated below (vpair_tile, rblock_tile_wide): the precondition asserts that EVERY
   ResBlock launch of the stage changes its tile size between the two runs.

2. Exact lane maps.  A generator whose every output channel takes ONE input channel at ONE tap (a different (channel, tap) per output
   channel), with weights 1 or 2, biases on a 1/256 grid and a mel of zeros and 1/256: every value is a non-negative multiple of 1/256
   below 2048/256, so every leaky_relu is the identity and every product, sum and 16-bit rounding is exact (the rounding emulator equals
   the float64 oracle before the test touches the GPU).  Four ResBlocks make the stage mean a division by 4.  The GPU output then differs
   from the float64 oracle only by the final tanh in fp32.
   Measured on MI355X: max |GPU - oracle| = 1.03e-7 over all cases, the same with every kernel on 32x32x16 (the commit before this
   file) and with vpair on 16x16x32; bound LANE_BOUND = 2e-7.
"""
import numpy as np
import pytest
import torch

import test_vocoder_kernels_gpu as vk
from dict_tts_amd import abi, vocoder
from oracle import hifigan_ref as href
from vocoder_emul import Emulator

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ 1. tile-size independence
def _cdiv(a, b):
    return -(-a // b)


def vpair_tile(C, k, d, B, L, cus):
    """vpair.hip vpair_launch_el: valid output rows per tile (TT - (k - 1)) of one iteration (kernel size k, dilation d) for B utterances
    padded to L rows on a device with `cus` CUs"""
    tiles = lambda tt: B * _cdiv(L, tt - (k - 1))
    table = (3 * B + 2) * 4                                    # the persistent configurations' tile table behind the LDS tile
    if C == 256:
        if 2 * tiles(128) <= cus:                              # few tiles: half-size ones
            TT = 64
        else:                                                  # 96 rows where only those leave room for two workgroups per CU
            lds = lambda tt: (tt + d * (k - 1) + max(d + 1, 4)) * (256 * 2 + 16) + table
            TT = 96 if (2 * lds(128) > 160 * 1024 and 2 * lds(96) <= 160 * 1024) else 128
    else:
        if 2 * tiles(256) <= cus:
            TT = 128
        else:                                                  # 256 rows while two workgroups fit 160 KB of LDS, else 192
            TT = 256 if ((256 + d * (k - 1) + max(d + 1, 8)) * (128 * 2 + 16) + table) * 2 <= 160 * 1024 else 192
    return TT - (k - 1)


def rblock_tile_wide(C, k, dils, B, L, cus):
    """rblock.hip rb_launch_el at C = 128 / 256 (the k = 3 ResBlock of these stages): output rows per tile.  W-row windows lose a halo of
    max(6 (k - 1), (k - 1) / 2 (d0 + d1 + d2 + 3)) rows on either side; half-size windows while 2 x tiles <= CUs"""
    halo = max(6 * (k - 1), (k - 1) // 2 * (sum(dils) + 3))
    full, half = (256, 128) if C == 128 else (128, 64)
    few = full - 2 * halo >= 32 and 2 * B * _cdiv(L, full - 2 * halo) <= cus
    W = half if few else full
    assert (W + 2 * 40) * (C * 2 + 16) + 32 * (C * 4 + 16) + (3 * B + 2) * 4 <= 160 * 1024   # the configuration fits: no fall-through
    return W - 2 * halo


def stage_tiles(cfg, B, L, cus):
    """{launch: output rows per tile} of the one stage's ResBlock launches"""
    C = cfg["upsample_initial_channel"] >> 1
    out = {}
    for k, dils in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
        if k == 3:
            out[f"rblock<{C}> k={k}"] = rblock_tile_wide(C, k, dils, B, L, cus)
        else:
            for m, d in enumerate(dils):
                out[f"vpair<{C}> k={k} it{m} d={d}"] = vpair_tile(C, k, d, B, L, cus)
    return out


def _full_tile_batch(cfg, L, cus):
    """the smallest batch at which every ResBlock launch of the stage uses another tile size than a single utterance does"""
    alone = stage_tiles(cfg, 1, L, cus)
    for B in range(2, 257):
        batch = stage_tiles(cfg, B, L, cus)
        if all(batch[k] != alone[k] for k in alone):
            return B, alone, batch
    raise AssertionError(f"no batch up to 256 utterances moves every launch off its half-size tiles: {alone}")


@pytest.mark.parametrize("name", ["c256", "c128"])
def test_alone_equals_in_batch_across_tile_sizes(name):
    cfg = vk.CONFIGS[name]
    C = cfg["upsample_initial_channel"] >> 1
    cus = vk._cus()
    hop = 2
    # the compared utterance ends two rows short of a full-size tile of the stage's first k = 7 launch, after several whole tiles
    frames = 375
    B, _, batch_tiles = _full_tile_batch(cfg, frames * hop, cus)
    step = batch_tiles[f"vpair<{C}> k=7 it0 d=1"]
    n_rows = (frames * hop // step) * step - 2
    assert n_rows % hop == 0 and step < n_rows < frames * hop
    n = n_rows // hop
    # precondition, with the lengths actually run (the batch is padded to `frames`): every launch switches its tile size
    one = stage_tiles(cfg, 1, n * hop, cus)
    assert all(one[k] != batch_tiles[k] for k in batch_tiles), (one, batch_tiles)
    print(f"\n[{name}] CUs {cus}: B = {B}; tiles alone {one}; in the batch {batch_tiles}", flush=True)
    model = vk._model(name, "f16")
    assert model.precision == abi.VOC_F16 and model.hop == hop
    mel = np.zeros((B, frames, 80), np.float32)
    lens = [frames] * B
    for b in range(B):
        mel[b] = vk._mel(4000 + b, frames, f"shape{b}")
    lens[B // 2] = n            # in the middle of the batch: its tiles are claimed among the others'
    mel[B // 2, n:] = 0.0
    full = model.forward_batch(T(mel).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    alone = model.spec2wav(mel[B // 2, :n])
    assert not model.overflowed()
    assert np.isfinite(full).all()
    assert alone.shape == (n * hop,)
    assert np.array_equal(alone, full[B // 2, :n * hop])
    assert float(np.abs(full[B // 2, n * hop:]).max(initial=0.0)) == 0.0


# ------------------------------------------------------------------------------------------------ 2. exact lane maps
G = 1.0 / 256          # the value grid
# max |GPU - float64 oracle| allowed.  The pre-tanh values are exact and the outputs stay below 0.13, where an fp32 ulp is 7.5e-9; the
# kernels' tanh (hardware exp2 and rcp in fp32) measured 1.03e-7 at worst on the 32x32x16 kernels, every case below.  The bound is
# that plus a dozen ulp; a wrong lane map moves a sample by a grid step through conv_post (1/4096 = 2.4e-4) or more.
LANE_BOUND = 2e-7


def _lane_cfg(c0):
    return {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": [3, 7, 11, 7], "resblock_dilation_sizes": [[1, 3, 5]] * 4}


def _one_tap(rng, c_out, c_in, k, weights, transposed=False):
    """weight [c_out, c_in, k] ([c_in, c_out, k] transposed) with one non-zero per output channel, at a (channel, tap) that differs
    from its neighbours'; bias: 16 levels of the grid, different for channels 1, 4, 8, 16, 32, 64 and 128 apart"""
    w = np.zeros((c_in, c_out, k) if transposed else (c_out, c_in, k), np.float32)
    ci = rng.permutation(max(c_in, c_out))[:c_out] % c_in
    for co in range(c_out):
        tap = (co * 3 + co // 7 + int(rng.randint(k))) % k
        v = weights[(co + co // 5) % len(weights)]
        if transposed:
            w[ci[co], co, tap] = v
        else:
            w[co, ci[co], tap] = v
    co = np.arange(c_out)
    b = (G * (1 + (5 * co + 3 * (co // 16)) % 16)).astype(np.float32)
    return w, b


def _lane_sd(c0):
    """plain (weight-norm folded) state dict of the lane-map generator"""
    rng = np.random.RandomState(c0)
    cfg = _lane_cfg(c0)
    C = c0 // 2
    sd = {}
    sd["conv_pre.weight"], sd["conv_pre.bias"] = _one_tap(rng, c0, 80, 7, [1.0, 2.0])
    sd["ups.0.weight"], sd["ups.0.bias"] = _one_tap(rng, C, c0, 4, [1.0, 2.0], transposed=True)
    for j, k in enumerate(cfg["resblock_kernel_sizes"]):
        for m in range(3):
            # x <- x + c2(c1(x)): at most 3 x + 2 b1 + b2 per iteration
            sd[f"resblocks.{j}.convs1.{m}.weight"], sd[f"resblocks.{j}.convs1.{m}.bias"] = _one_tap(rng, C, C, k, [1.0, 2.0])
            sd[f"resblocks.{j}.convs2.{m}.weight"], sd[f"resblocks.{j}.convs2.{m}.bias"] = _one_tap(rng, C, C, k, [1.0])
    w, _ = _one_tap(rng, 1, C, 7, [1.0 / 16])
    sd["conv_post.weight"], sd["conv_post.bias"] = w, np.array([G], np.float32)
    return cfg, sd


def _lane_mel(seed, n):
    return (np.random.RandomState(seed).randint(0, 2, size=(n, 80)) * G).astype(np.float32)


def _oracle_post(sd64, stages):
    """the pre-tanh value of the oracle from its last stage (generator_forward returns the waveform only)"""
    return torch.nn.functional.conv1d(torch.nn.functional.leaky_relu(stages["stage.0"]), sd64["conv_post.weight"], sd64["conv_post.bias"], padding=3)


_LANE = {}


def _lane_case(c0):
    """-> (cfg, state dict, mels, float64 oracle outputs); computed once per width, checked on the CPU before any GPU work"""
    if c0 not in _LANE:
        cfg, sd = _lane_sd(c0)
        lens = [37, 150, 64, 1, 93]       # B = 1 uses the first two; the ragged batch all of them
        mels = [_lane_mel(100 * c0 + i, n) for i, n in enumerate(lens)]
        sd64 = {k: T(v).double() for k, v in sd.items()}
        sd32 = {k: T(v) for k, v in sd.items()}
        want = []
        for m in mels:
            x = T(m).double().unsqueeze(0).transpose(2, 1)
            with torch.no_grad():
                wav, stages = href.generator_forward(sd64, cfg, x, return_stages=True)
            w = wav.view(-1).numpy()
            assert float(np.abs(w).max()) < 0.9, "tanh saturation would hide errors"
            assert float(stages["ups.0"].min()) >= 0.0 and float(stages["stage.0"].min()) >= 0.0   # every leaky_relu the identity
            # every rounding point exact: the emulator (16-bit operands, fp16 stream, split serial convolutions) reproduces float64
            emu = Emulator(sd32, cfg, mode="f16").forward(T(m).unsqueeze(0).transpose(2, 1), return_stages=True)[1]
            assert torch.equal(emu["stage.0"], stages["stage.0"]) and torch.equal(emu["post"], _oracle_post(sd64, stages))
            assert float(stages["stage.0"].max()) < 2048 * G
            want.append(w)
        _LANE[c0] = (cfg, sd, mels, want)
    return _LANE[c0]


@pytest.mark.parametrize("c0", [512, 256, 128, 64])
def test_lane_maps_exact(c0):
    cfg, sd, mels, want = _lane_case(c0)
    model = vocoder.HifiGAN(state_dict={k: T(v) for k, v in sd.items()}, config=cfg, precision="f16", range_guard=True)
    assert model.precision == abi.VOC_F16 and model.hop == 2
    worst = 0.0
    for i in (0, 1):   # B = 1
        got = model.spec2wav(mels[i])
        d = float(np.abs(got.astype(np.float64) - want[i]).max())
        print(f"LANEMEAS C={c0 // 2} B=1 len={mels[i].shape[0]} max|GPU - oracle| {d:.3e}", flush=True)
        worst = max(worst, d)
    lens = [m.shape[0] for m in mels]
    batch = np.zeros((len(mels), max(lens), 80), np.float32)
    for b, m in enumerate(mels):
        batch[b, :lens[b]] = m
    full = model.forward_batch(T(batch).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    assert not model.overflowed()
    for b, n in enumerate(lens):
        d = float(np.abs(full[b, :2 * n].astype(np.float64) - want[b]).max())
        print(f"LANEMEAS C={c0 // 2} ragged utt={b} len={n} max|GPU - oracle| {d:.3e}", flush=True)
        worst = max(worst, d)
        assert float(np.abs(full[b, 2 * n:]).max(initial=0.0)) == 0.0
    assert worst <= LANE_BOUND, worst
