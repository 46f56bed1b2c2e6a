"""vpair.hip on v_mfma_f32_16x16x32 at BOTH widths (C = 128 and now C = 256), with the C = 256 census running 96-row tiles where the release
path runs 128-row ones (the guarded 128-row kernel does not fit the register file on this shape and is not instantiated).

(a) Exact lane maps (the generator of test_mfma_shape_gpu.py: one (channel, tap) per output channel, weights 1 / 2, values on a 1/256
    grid below 8 — the rounding emulator equals the float64 oracle on the CPU, the GPU differs from it by the fp32 tanh only), at
    utterance lengths that end inside, at and next to the 4-row blocks, the 16-row halves and the 32-row tiles of the MFMA's row map and
    next to a tile edge, k = 7 and k = 11 with dilations 1, 3, 5: alone (the half-size tiles), in one ragged batch, and repeated in a batch
    large enough for the full-size tiles.  The generator's hop is 2, so a stage has an even number of rows: for the odd row counts 1, 3,
    15, 17, 31, 33 the even ones on either side run (2, 4, 14, 16, 18, 30, 32, 34), next to 12 and 16 themselves; the same numbers are
    also used as FRAME counts (rows 2 ... 66).  Bound: that of test_mfma_shape_gpu.py (2e-7; the 32x32x16 kernels measured 1.03e-7).
    Measured on MI355X: max |GPU - oracle| = 4.0e-9 at both widths (these utterances are short: fewer samples meet the tanh's worst case).
    Any placement of the LDS tile that permutes rows or 16-byte chunks between the MFMA's lanes (the conflict-free one of
    tools/experiments/vpair_lds_placement.patch, measured and not adopted) has to pass this unchanged.
(b) C = 256, census == release where their tile sizes differ: identical bits, clamp count 0 on healthy input, and on an input with
    planted out-of-range activations the same non-zero count from the 96-row tiles (in the batch) and the 64-row tiles (alone).
    Measured: 29,100 from both (an overflow spreads: inf operands make inf / NaN sums in every later convolution of the stage).
(d) The shapes of (a) in memory-safety mode (debug_redzone): no red zone damaged, bits identical to the release context's.
(rblock<64> stays on 32x32x16: there is no alone == in-batch case for it here.)
"""
import numpy as np
import pytest
import torch

import test_mfma_shape_gpu as ms
import test_vocoder_kernels_gpu as vk
from dict_tts_amd import abi, vocoder
from oracle import hifigan_ref as href
from vocoder_emul import Emulator

pytestmark = pytest.mark.gpu
T = ms.T
LANE_BOUND = 2e-7      # as test_mfma_shape_gpu.py: exact pre-tanh values, the kernels' fp32 tanh measured 1.03e-7 on the 32x32x16 kernels


def _half_tile_rows(C, k):
    """valid rows of a half-size vpair tile (vpair_launch_el at B = 1): TT - (k - 1) with TT = 64 (C = 256) or 128 (C = 128)"""
    return (64 if C == 256 else 128) - (k - 1)


def _lane_frames(C):
    """frame counts of the cases (stage rows = 2 x frames)"""
    rows = [2, 4, 12, 14, 16, 18, 30, 32, 34]                          # the block edges of the row map, as ROW counts
    frames = [1, 3, 12, 15, 16, 17, 31, 33]                            # ... and as FRAME counts
    edge = [_half_tile_rows(C, 7) // 2 + d for d in (-1, 0, 1)]        # a k = 7 half-size tile - 2, + 0, + 2 rows
    edge += [_half_tile_rows(C, 11) // 2 + 1]                          # one row pair past a k = 11 tile
    return sorted(set([r // 2 for r in rows] + frames + edge)) + [150]  # 150: several tiles of every size


_CASE = {}


def _case(c0):
    """-> (cfg, state dict, mels, float64 oracle outputs), once per width; the exactness of the inputs is checked on the CPU"""
    if c0 not in _CASE:
        cfg, sd = ms._lane_sd(c0)
        mels = [ms._lane_mel(1000 * c0 + n, n) for n in _lane_frames(c0 // 2)]
        sd64 = {k: T(v).double() for k, v in sd.items()}
        sd32 = {k: T(v) for k, v in sd.items()}
        want = []
        for i, m in enumerate(mels):
            x = T(m).double().unsqueeze(0).transpose(2, 1)
            with torch.no_grad():
                wav, stages = href.generator_forward(sd64, cfg, x, return_stages=True)
            w = wav.view(-1).numpy()
            assert float(np.abs(w).max()) < 0.9, "tanh saturation would hide errors"
            assert float(stages["ups.0"].min()) >= 0.0 and float(stages["stage.0"].min()) >= 0.0 and float(stages["stage.0"].max()) < 2048 * ms.G
            if i % 4 == 0 or i == len(mels) - 1:   # every rounding point exact: the emulator reproduces float64 (a sample of the cases)
                emu = Emulator(sd32, cfg, mode="f16").forward(T(m).unsqueeze(0).transpose(2, 1), return_stages=True)[1]
                assert torch.equal(emu["stage.0"], stages["stage.0"]) and torch.equal(emu["post"], ms._oracle_post(sd64, stages))
            want.append(w)
        _CASE[c0] = (cfg, sd, mels, want)
    return _CASE[c0]


def _model(c0, guard, **extra):
    cfg, sd, _, _ = _case(c0)
    m = vocoder.HifiGAN(state_dict={k: T(v) for k, v in sd.items()}, config={**cfg, **extra}, precision="f16", range_guard=guard)
    assert m.precision == abi.VOC_F16 and m.hop == 2
    return m


def _batch(mels, idx):
    lens = [mels[i].shape[0] for i in idx]
    batch = np.zeros((len(idx), max(lens), 80), np.float32)
    for b, i in enumerate(idx):
        batch[b, :lens[b]] = mels[i]
    return batch, lens


def _run_batch(model, mels, idx):
    batch, lens = _batch(mels, idx)
    full = model.forward_batch(T(batch).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    assert not model.overflowed()
    return full, lens


def _worst(tag, full, lens, idx, want):
    worst = 0.0
    for b, (i, n) in enumerate(zip(idx, lens)):
        d = float(np.abs(full[b, :2 * n].astype(np.float64) - want[i]).max())
        worst = max(worst, d)
        assert float(np.abs(full[b, 2 * n:]).max(initial=0.0)) == 0.0
    print(f"LANE2MEAS {tag}: {len(idx)} utterances, max|GPU - oracle| {worst:.3e}", flush=True)
    return worst


def _full_tile_B(C, L, cus):
    """the smallest batch of L-row utterances at which every vpair launch of the lane generator's stage leaves its half-size tile"""
    for B in range(2, 513):
        if all(vk.vpair_tile(C, k, d, B, L, cus) != vk.vpair_tile(C, k, d, 1, L, cus) for k in (7, 11) for d in (1, 3, 5)):
            return B
    raise AssertionError("no batch up to 512 utterances moves every vpair launch off its half-size tiles")


# ------------------------------------------------------------------------------------------------ (a) exact lane maps
@pytest.mark.parametrize("c0", [512, 256])
def test_lane_maps_exact_at_block_and_tile_edges(c0):
    C = c0 // 2
    cfg, sd, mels, want = _case(c0)
    guarded, release = _model(c0, True), _model(c0, False)
    worst = 0.0
    for i, m in enumerate(mels[:-1]):   # alone: half-size tiles
        got = guarded.spec2wav(m)
        d = float(np.abs(got.astype(np.float64) - want[i]).max())
        print(f"LANE2MEAS C={C} alone frames={m.shape[0]} max|GPU - oracle| {d:.3e}", flush=True)
        worst = max(worst, d)
        assert np.array_equal(got, release.spec2wav(m)), m.shape[0]
    idx = list(range(len(mels)))
    full, lens = _run_batch(guarded, mels, idx)   # one ragged batch
    worst = max(worst, _worst(f"C={C} ragged", full, lens, idx, want))
    # full-size tiles (C = 256: 128-row tiles in release, 96-row ones under the census): every case again, padded to the longest
    cus = vk._cus()
    B = _full_tile_B(C, 2 * mels[-1].shape[0], cus)
    idx = [len(mels) - 1 if b % 2 == 0 else (b // 2) % (len(mels) - 1) for b in range(B)]   # the long utterance in every other slot
    print(f"C={C}: CUs {cus}, full-size tiles from B = {B}", flush=True)
    for tag, model in (("census", guarded), ("release", release)):
        full, lens = _run_batch(model, mels, idx)
        worst = max(worst, _worst(f"C={C} B={B} {tag}", full, lens, idx, want))
    assert worst <= LANE_BOUND, worst


# ------------------------------------------------------------------------------------------------ (b) census == release at C = 256
def _c256_batch(cus, frames):
    """B at which the release path of vpair<256> takes 128-row tiles (vpair_launch_el: more than CUs / 2 tiles of 128 rows) for k = 7
    at dilations 1, 3 and k = 11 at dilation 1 (the other three take 96-row tiles in both paths: two workgroups per CU)"""
    B = _full_tile_B(256, 2 * frames, cus)
    tiles = {(k, d): vk.vpair_tile(256, k, d, B, 2 * frames, cus) + (k - 1) for k in (7, 11) for d in (1, 3, 5)}
    assert tiles[(7, 1)] == 128 and tiles[(7, 3)] == 128 and tiles[(11, 1)] == 128 and tiles[(7, 5)] == 96, tiles
    return B


def test_c256_census_equals_release_across_their_tile_sizes():
    cus = vk._cus()
    frames = 150
    B = _c256_batch(cus, frames)
    model = vk._model("c256", "f16_release")
    stream = torch.cuda.current_stream().cuda_stream
    mel = np.stack([vk._mel(7000 + b % 6, frames, f"census{b % 6}") for b in range(B)])
    lens = [frames - 7 * (b % 5) for b in range(B)]
    lens_t = torch.tensor(lens, dtype=torch.int32)
    release = model.forward_batch(T(mel).cuda(), lens_t, check=True).cpu().numpy()
    model.ctx.vocoder_range_guard(True)
    census = model.forward_batch(T(mel).cuda(), lens_t, check=True).cpu().numpy()
    assert model.ctx.vocoder_clamped(stream) == 0
    assert np.isfinite(release).all() and np.array_equal(release, census)
    # planted: a few frames of ONE utterance far outside the range a mel has -> stage activations beyond 65504 around those rows, at a tile
    # seam of the 96-row tiles (rows 90 .. 97) and inside a tile.  The count of the batch (96-row tiles; every other utterance counts 0, as
    # just shown) equals the count of that utterance alone (64-row tiles)
    u = B // 2
    bad = mel.copy()
    for f in (45, 46, 48, 101):
        bad[u, f] = 1e8 * np.sign(bad[u, f] + 3.0)
    model.forward_batch(T(bad).cuda(), lens_t)
    n_batch = model.ctx.vocoder_clamped(stream)
    model.forward_batch(T(bad[u:u + 1, :lens[u]]).cuda())
    n_alone = model.ctx.vocoder_clamped(stream)
    model.overflowed()
    print(f"C=256 census: B = {B}, planted clamp count {n_batch} in the batch (96-row tiles), {n_alone} alone (64-row tiles)", flush=True)
    assert n_batch > 0 and n_batch == n_alone


# ------------------------------------------------------------------------------------------------ (d) memory-safety mode
@pytest.mark.parametrize("c0", [512, 256])
def test_lane_shapes_under_redzone(c0):
    cfg, sd, mels, want = _case(c0)
    rel, dbg = _model(c0, False), _model(c0, False, dtts_debug_redzone=1)
    stream = torch.cuda.current_stream().cuda_stream
    for m in mels[:-1]:
        assert np.array_equal(dbg.spec2wav(m), rel.spec2wav(m)), m.shape[0]
    idx = list(range(len(mels)))
    assert np.array_equal(_run_batch(dbg, mels, idx)[0], _run_batch(rel, mels, idx)[0])
    B = _full_tile_B(c0 // 2, 2 * mels[-1].shape[0], vk._cus())
    idx = [len(mels) - 1 if b % 2 == 0 else (b // 2) % (len(mels) - 1) for b in range(B)]
    assert np.array_equal(_run_batch(dbg, mels, idx)[0], _run_batch(rel, mels, idx)[0])
    assert dbg.ctx.debug_check(stream) == 0, dbg.ctx.last_error()
