"""rblock.hip on the MFMA shape trait (rb_common.h MfmaShape; rblock.h rblock_mfma_shape picks the shape per width), with C = 64 on
v_mfma_f32_16x16x32 and its range-guard census on 512-row tiles where the release path runs 640-row ones (the guarded 640-row kernel does
not fit the register file on this shape and is not instantiated).

(a) Exact lane maps on the FULL-SIZE tiles of C = 64 (test_mfma_shape_gpu.py covers the 256-row half-size tiles a small batch gets): the
    one-(channel, tap)-per-output-channel generator of that file (`_lane_sd(128)`, hop 2), in a batch just large enough that the launcher's
    `few(512)` fails — k = 7 / 11 then run 640-row tiles (568 / 520 output rows; 440 / 392 under the census), k = 3 the 512-row tile (488).
    Utterance row counts ending inside, at and next to the 4-row blocks, 16-row halves and 32-row tiles of the row map (2 ... 34), next to
    every tile edge (output rows - 2, + 0, + 2) and one utterance of several tiles; each alone and in the batch, census and release.
    Bound: LANE_BOUND of test_mfma_shape_gpu.py (2e-7 against the float64 oracle; the emulator equals the oracle on the CPU first).
(b) alone == in-batch, bit for bit, across the tile-size switch at C = 64 (random-weight isolating generator, upsample_initial_channel 128):
    the compared utterance ends two rows short of a full k = 7 tile after several whole tiles, in the middle of the batch.
(c) census == release bits where their tile sizes differ (C = 64, k >= 7), clamp count 0 on healthy input; with planted out-of-range
    activations the same non-zero count from the 512-row tiles (in the batch) and the 256-row tiles (alone).
(d) The shapes of (a) under debug_redzone: no red zone damaged, bits identical to the release context's.
(e) A pack declared in the wrong fragment order is refused by the launcher with an error code, not run.
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
LANE_BOUND = ms.LANE_BOUND
C0, C, HOP = 128, 64, 2
D135 = [1, 3, 5]
KS = (3, 7, 11)


def _halo(k):
    return max(6 * (k - 1), (k - 1) // 2 * (sum(D135) + 3))   # rblock.h rblock_halo_of


def _tile(k, B, L, cus, census):
    """output rows per tile of the C = 64 launch of kernel size k: test_vocoder_kernels_gpu.rblock_tile (rb_launch_el), and for the
    range-guard census the 512-row tile wherever that rule gives the 640-row one"""
    tt = vk.rblock_tile(C, k, D135, B, L, False, cus)
    return 512 - 2 * _halo(k) if census and tt == 640 - 2 * _halo(k) else tt


FULL = {3: 488, 7: 568, 11: 520}       # output rows of the full-size release tiles: 512 - 24, 640 - 72, 640 - 120
CENSUS = {3: 488, 7: 440, 11: 392}     # ... of the census's: 512 rows for every k


def _full_tile_B(L, cus, at_least=2):
    """the smallest batch of L-row utterances at which few(512) fails for every kernel size: all three launches on their full-size tiles"""
    for B in range(at_least, vk.MAX_BATCH + 1):
        if all(_tile(k, B, L, cus, False) == FULL[k] and _tile(k, B, L, cus, True) == CENSUS[k] for k in KS):
            assert all(_tile(k, 1, L, cus, g) == 256 - 2 * _halo(k) for k in KS for g in (False, True))   # alone: the half-size tile
            return B
    raise AssertionError(f"no batch up to {vk.MAX_BATCH} utterances of {L} rows leaves the half-size tiles on {cus} CUs")


def _lane_rows():
    rows = [2, 4, 12, 14, 16, 18, 30, 32, 34]                                      # the block edges of the new row map
    rows += [t + d for t in sorted(set(FULL.values()) | set(CENSUS.values())) for d in (-2, 0, 2)]   # every tile edge
    return sorted(set(rows)) + [1500]                                              # ... and one utterance of several tiles


_CASE = {}


def _case():
    """-> (cfg, state dict, mels, float64 oracle outputs); the exactness of the inputs is checked on the CPU before any GPU work"""
    if not _CASE:
        cfg, sd = ms._lane_sd(C0)
        mels = [ms._lane_mel(3000 + r, r // HOP) for r in _lane_rows()]
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
            if i % 6 == 0 or i == len(mels) - 1:   # every rounding point exact: the emulator reproduces float64 (a sample of the cases)
                emu = Emulator(sd32, cfg, mode="f16").forward(T(m).unsqueeze(0).transpose(2, 1), return_stages=True)[1]
                assert torch.equal(emu["stage.0"], stages["stage.0"]) and torch.equal(emu["post"], ms._oracle_post(sd64, stages))
            want.append(w)
        _CASE["v"] = (cfg, sd, mels, want)
    return _CASE["v"]


def _model(guard, **extra):
    cfg, sd, _, _ = _case()
    m = vocoder.HifiGAN(state_dict={k: T(v) for k, v in sd.items()}, config={**cfg, **extra}, precision="f16", range_guard=guard)
    assert m.precision == abi.VOC_F16 and m.hop == HOP
    return m


def _run_batch(model, mels, idx):
    lens = [mels[i].shape[0] for i in idx]
    batch = np.zeros((len(idx), max(lens), 80), np.float32)
    for b, i in enumerate(idx):
        batch[b, :lens[b]] = mels[i]
    full = model.forward_batch(T(batch).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    assert not model.overflowed()
    return full, lens


def _batch_idx(mels, cus):
    """every case once, the long one first, then the cases again until few(512) fails for a batch padded to the long one"""
    B = _full_tile_B(HOP * mels[-1].shape[0], cus, at_least=len(mels))
    return [len(mels) - 1] + [b % (len(mels) - 1) for b in range(B - 1)]


# ------------------------------------------------------------------------------------------------ (a) exact lane maps, full-size tiles
def test_lane_maps_exact_on_full_size_tiles():
    cfg, sd, mels, want = _case()
    cus = vk._cus()
    idx = _batch_idx(mels, cus)
    print(f"\nC=64: CUs {cus}, B = {len(idx)} padded to {HOP * mels[-1].shape[0]} rows: release tiles {FULL}, census tiles {CENSUS}", flush=True)
    guarded, release = _model(True), _model(False)
    worst = 0.0
    for i, m in enumerate(mels):   # alone: half-size tiles
        got = guarded.spec2wav(m)
        d = float(np.abs(got.astype(np.float64) - want[i]).max())
        print(f"LANE3MEAS C=64 alone rows={HOP * m.shape[0]} max|GPU - oracle| {d:.3e}", flush=True)
        worst = max(worst, d)
        assert np.array_equal(got, release.spec2wav(m)), m.shape[0]
    for tag, model in (("census", guarded), ("release", release)):
        full, lens = _run_batch(model, mels, idx)
        for b, (i, n) in enumerate(zip(idx, lens)):
            d = float(np.abs(full[b, :HOP * n].astype(np.float64) - want[i]).max())
            if b < len(mels):
                print(f"LANE3MEAS C=64 B={len(idx)} {tag} rows={HOP * n} max|GPU - oracle| {d:.3e}", flush=True)
            worst = max(worst, d)
            assert float(np.abs(full[b, HOP * n:]).max(initial=0.0)) == 0.0
    print(f"LANE3MEAS C=64 worst {worst:.3e}", flush=True)
    assert worst <= LANE_BOUND, worst


# ------------------------------------------------------------------------------------------------ (b) alone == in-batch at C = 64
@pytest.mark.parametrize("mode", ["f16_release", "f16"])
def test_c64_alone_equals_in_batch_across_tile_sizes(mode):
    cfg = vk.CONFIGS["c64"]
    assert cfg["upsample_initial_channel"] == C0 and list(cfg["resblock_kernel_sizes"]) == [3, 7, 11]
    census = vk.MODES[mode][1]
    cus = vk._cus()
    frames = 900
    B = _full_tile_B(frames * HOP, cus)
    step = _tile(7, B, frames * HOP, cus, census)
    n_rows = (frames * HOP // step) * step - 2      # two rows short of a full k = 7 tile, after several whole tiles
    assert n_rows % HOP == 0 and 2 * step < n_rows < frames * HOP
    n = n_rows // HOP
    # precondition, with the lengths actually run: EVERY ResBlock launch of the stage changes its tile size between the two runs
    one = {k: _tile(k, 1, n_rows, cus, census) for k in KS}
    batch = {k: _tile(k, B, frames * HOP, cus, census) for k in KS}
    assert all(one[k] != batch[k] for k in KS), (one, batch)
    if not census:   # (the release rule is test_vocoder_kernels_gpu's own)
        assert sorted(vk.stage_tiles(cfg, B, frames * HOP, cus).values()) == sorted(batch.values())
    print(f"\n[c64 {mode}] CUs {cus}: B = {B}; tiles alone {one}; in the batch {batch}", flush=True)
    model = vk._model("c64", mode)
    assert model.precision == abi.VOC_F16 and model.hop == HOP
    mel = np.stack([vk._mel(5000 + b % 7, frames, f"shape3_{b % 7}") for b in range(B)])
    lens = [frames] * B
    lens[B // 2] = n            # in the middle of the batch: its tiles are claimed among the others'
    mel[B // 2, n:] = 0.0
    full = model.forward_batch(T(mel).cuda(), torch.tensor(lens, dtype=torch.int32), check=True).cpu().numpy()
    alone = model.spec2wav(mel[B // 2, :n])
    assert not model.overflowed()
    assert np.isfinite(full).all()
    assert alone.shape == (n * HOP,)
    assert np.array_equal(alone, full[B // 2, :n * HOP])
    assert float(np.abs(full[B // 2, n * HOP:]).max(initial=0.0)) == 0.0


# ------------------------------------------------------------------------------------------------ (c) census == release at C = 64
def test_c64_census_equals_release_across_their_tile_sizes():
    cus = vk._cus()
    frames = 600
    B = _full_tile_B(frames * HOP, cus)
    rel = {k: _tile(k, B, frames * HOP, cus, False) for k in KS}
    cen = {k: _tile(k, B, frames * HOP, cus, True) for k in KS}
    assert rel == FULL and cen == CENSUS and all(rel[k] != cen[k] for k in (7, 11))
    model = vk._model("c64", "f16_release")
    stream = torch.cuda.current_stream().cuda_stream
    mel = np.stack([vk._mel(7100 + b % 6, frames, f"census3_{b % 6}") for b in range(B)])
    lens = [frames - 7 * (b % 5) for b in range(B)]
    lens_t = torch.tensor(lens, dtype=torch.int32)
    release = model.forward_batch(T(mel).cuda(), lens_t, check=True).cpu().numpy()
    model.ctx.vocoder_range_guard(True)
    census = model.forward_batch(T(mel).cuda(), lens_t, check=True).cpu().numpy()
    assert model.ctx.vocoder_clamped(stream) == 0
    assert np.isfinite(release).all() and np.array_equal(release, census)
    # planted: a few frames of ONE utterance far outside the range a mel has -> stage activations beyond 65504 around those rows, at the
    # seam of the census's k = 7 tiles (rows 440 = frame 220) and inside a tile.  The count of the batch (512-row tiles; every other
    # utterance counts 0, as just shown) equals the count of that utterance alone (256-row tiles)
    u = B // 2
    bad = mel.copy()
    for f in (219, 220, 222, 401):
        bad[u, f] = 1e8 * np.sign(bad[u, f] + 3.0)
    model.forward_batch(T(bad).cuda(), lens_t)
    n_batch = model.ctx.vocoder_clamped(stream)
    model.forward_batch(T(bad[u:u + 1, :lens[u]]).cuda())
    n_alone = model.ctx.vocoder_clamped(stream)
    model.overflowed()
    print(f"\nC=64 census: B = {B}, planted clamp count {n_batch} in the batch (512-row tiles), {n_alone} alone (256-row tiles)", flush=True)
    assert n_batch > 0 and n_batch == n_alone


# ------------------------------------------------------------------------------------------------ (d) memory-safety mode
def test_full_size_tile_shapes_under_redzone():
    cfg, sd, mels, want = _case()
    rel, dbg = _model(False), _model(False, dtts_debug_redzone=1)
    stream = torch.cuda.current_stream().cuda_stream
    for m in mels:
        assert np.array_equal(dbg.spec2wav(m), rel.spec2wav(m)), m.shape[0]
    idx = _batch_idx(mels, vk._cus())
    assert np.array_equal(_run_batch(dbg, mels, idx)[0], _run_batch(rel, mels, idx)[0])
    assert dbg.ctx.debug_check(stream) == 0, dbg.ctx.last_error()


# ------------------------------------------------------------------------------------------------ (e) host refusal
def test_launcher_refuses_a_pack_in_the_wrong_fragment_order():
    cfg, sd, mels, want = _case()
    m = mels[5]
    bad = _model(False, dtts_debug_redzone=2)   # its whole-ResBlock launches declare the other order than their packs are in
    with pytest.raises(abi.DttsError) as e:
        bad.spec2wav(m)
    assert "rblock_launch" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    got = _model(False).spec2wav(m)             # (the same packs, declared as they are)
    assert float(np.abs(got.astype(np.float64) - want[5]).max()) <= LANE_BOUND
