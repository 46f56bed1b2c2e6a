"""The multi-resolution STFT distance on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE) against the float64
restatement of modules/hifigan/stft_loss.py (tests/stft_ref.py).

Every accuracy bound is set against the reference's OWN arithmetic, not against what the kernel delivers.  Magnitudes: per signal, the error
max |m - m64| / max(frame's largest m64, 1e-6) of the float32 torch.stft path is the unit and the kernel may use 4 x that (the factor
tests/test_melspec_gpu.py derives for a direct fp32 sum against a float32 FFT).  Scalars: the unit is the largest relative deviation of the
float32 path's sc / mag from the float64 figures over all pairs, resolutions and lengths of the set (pooled: about 1e-3, it depends on the host's FFT; set by the DC / Nyquist
pair, whose side lobes cross the 1e-7 clamp), the bound again 4 x that; a figure that is exactly 0 in float64 must be exactly 0.

Measured on the MI355X (every figure is printed before it is asserted): see MEASURED below.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stft_ref as sr
from dict_tts_amd import abi, stftloss, synth, vocoder

pytestmark = pytest.mark.gpu

MEASURED = """On the MI355X (348 magnitude figures, 174 pairs of scalars; the host's float32 torch.stft gave the pooled scalar unit 1.345e-3):
magnitudes, kernel error / float32-path error (bound 4): 0.34 - 1.13 over everything; by pair speech 0.34 - 0.98, noise 0.42 - 0.77,
tone 0.46 - 1.00, equal signals 0.40 - 0.70, DC / Nyquist 0.80 - 1.13 (the largest: (2048, 240, 1200)); silence 1.00 (both are sqrt(1e-7f)).
Scalars, deviation from float64 in units (bound 4): mag of the DC / Nyquist pair 0.90 (1.2e-3: bins at the clamp), everything else below
0.01 units: speech 4.7e-6 (sc) / 3.8e-6 (mag), tone 4.8e-8 / 2.7e-6, noise 3.0e-9 / 1.8e-7, equal signals exactly 0; pooled batch figures 1.0e-8 / 7.9e-7.
Vocoder (synthetic V2): fp16 against bf16x3 sc 1.9e-4, mag 4.7e-4; against an unrelated waveform 0.25 / 0.51."""

SENTINEL = 777.0
ALL = tuple(range(len(sr.RESOLUTIONS)))


@functools.lru_cache(maxsize=None)
def _front(which):
    """one MultiResolutionSTFT (with a context of its own) per set of resolutions: (0,), (1,), (2,) and (0, 1, 2)"""
    f, h, w = zip(*[sr.RESOLUTIONS[i] for i in which])
    return stftloss.MultiResolutionSTFT(f, h, w)


def _run(m, x, y, lens=None, extra_rows=0):
    """-> (scores dict on the host as numpy, [per resolution: magnitudes [2, B, cap, bins]]); the magnitude buffer is pre-filled with SENTINEL"""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    B, L = x.shape
    cap = 1 + L // min(m.hop_sizes) + extra_rows
    m._plan()
    layout, total = m.mag_layout(B, cap)
    mag = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    r = m(x, y, lens=lens, mag=mag, mag_cap=cap)
    torch.cuda.synchronize()
    mag = mag.cpu().numpy()
    return {k: v.cpu().numpy() for k, v in r.items()}, [mag[o:o + int(np.prod(s))].reshape(s) for o, s in layout]


@functools.lru_cache(maxsize=None)
def _alone(i, name, L):
    """pair `name` of L samples at resolution i alone, B = 1"""
    x, y = sr.pair(name, L)
    return _run(_front((i,)), x, y)


def _judge(tag, res, name, L, sc, mag, count, mags):
    """test 1's criteria for one utterance at one resolution: mags [2, rows, bins] from the GPU"""
    n_fft, hop, _ = res
    r = sr.reference(name, res, L)
    T = 1 + L // hop
    assert count == T * (n_fft // 2 + 1), (tag, count)
    unit = sr.scalar_unit()
    for s in range(2):
        got = mags[s, :T]
        assert np.isfinite(got).all() and np.all(mags[s, T:] == SENTINEL), tag
        e, e32 = sr.mag_error(got, r["m64"][s]), r["e32"][s]
        print(f"{tag} {name}[{'xy'[s]}] L={L}: magnitude error gpu {e:.3e}  float32 path {e32:.3e}  ratio {e / e32 if e32 else 0:.2f}")
        assert e <= sr.FACTOR * e32, (tag, name, s, e, e32)
    for k, v in (("sc", float(sc)), ("mag", float(mag))):
        v64 = r[k + "64"]
        dev = sr.rel_dev(v, v64)
        print(f"{tag} {name} L={L}: {k} gpu {v:.9e}  float64 {v64:.9e}  float32 path {r[k + '32']:.9e}  deviation {dev:.3e} = {dev / unit:.2f} units")
        if v64 == 0:
            assert v == 0, (tag, name, k, v)
        else:
            assert dev <= sr.FACTOR * unit, (tag, name, k, v, v64, unit)


# ---- 1. accuracy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", ALL)
def test_accuracy_of_each_resolution_alone(i):
    res = sr.RESOLUTIONS[i]
    print(f"scalar unit (float32 path, pooled): {sr.scalar_unit():.3e}")
    for L in sr.lengths(res):
        for name in sr.PAIRS:
            r, mags = _alone(i, name, L)
            _judge(f"{res} alone", res, name, L, r["sc_res"][0, 0], r["mag_res"][0, 0], r["count"][0, 0], mags[0][:, 0])
            assert r["sc"][0] == r["sc_res"][0, 0] and r["mag"][0] == r["mag_res"][0, 0]


def test_accuracy_of_the_three_resolutions_together():
    """every length of every resolution through the three-resolution call; a resolution the signal is too short for has count 0 and NaN, and
    every other one gives the bits of the same resolution alone"""
    m = _front(ALL)
    for L in sorted({L for res in sr.RESOLUTIONS for L in sr.lengths(res)}):
        for name in sr.PAIRS:
            x, y = sr.pair(name, L)
            r, mags = _run(m, x, y, lens=[L])
            valid = [L > res[0] // 2 for res in sr.RESOLUTIONS]
            for i, res in enumerate(sr.RESOLUTIONS):
                if not valid[i]:
                    assert r["count"][i, 0] == 0 and not r["sums"][i, 0].any() and np.isnan(r["sc_res"][i, 0]) and np.isnan(r["mag_res"][i, 0])
                    assert np.all(mags[i] == SENTINEL)
                    continue
                _judge(f"{res} of three", res, name, L, r["sc_res"][i, 0], r["mag_res"][i, 0], r["count"][i, 0], mags[i][:, 0])
                if L in sr.lengths(res):
                    assert np.array_equal(r["sums"][i, 0], _alone(i, name, L)[0]["sums"][0, 0]), (res, name, L)
            if all(valid):
                assert r["sc"][0] == pytest.approx(r["sc_res"][:, 0].mean(), rel=1e-15) and r["mag"][0] == pytest.approx(r["mag_res"][:, 0].mean(), rel=1e-15)
            else:
                assert np.isnan(r["sc"][0]) and np.isnan(r["mag"][0])


# ---- 2. counts and bin coverage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", ALL)
def test_counts_and_both_edge_bins(i):
    """the DC / Nyquist pair: bins 0 and fft_size / 2 carry half of the energy — each must enter every sum exactly once"""
    res = sr.RESOLUTIONS[i]
    n_fft, hop, _ = res
    for L in sr.lengths(res):
        r, mags = _alone(i, "dcnyq", L)
        T = 1 + L // hop
        assert r["count"].tolist() == [[T * (n_fft // 2 + 1)]]
        ref = sr.reference("dcnyq", res, L)
        s64, _ = sr.sums_of(*ref["m64"])
        edge = ref["m64"][1][:, 0] ** 2, ref["m64"][1][:, -1] ** 2
        for k, bin_sum in (("bin 0", edge[0].sum()), ("bin fft_size / 2", edge[1].sum())):
            # dropping the bin, or counting it twice, moves sum m_y^2 by this share: several times the bound below
            assert bin_sum / s64[1] > 0.05 > 4 * 2 * sr.FACTOR * sr.scalar_unit(), k
        dev = sr.rel_dev(r["sums"][0, 0, 1], s64[1])
        print(f"{res} dcnyq L={L}: sums gpu {r['sums'][0, 0]}  float64 {s64}  deviation of sum m_y^2 {dev:.3e}")
        assert dev <= 2 * sr.FACTOR * sr.scalar_unit()   # (sc is the root of a ratio with this sum: twice the bound of sc)
        _judge(f"{res} edge bins", res, "dcnyq", L, r["sc_res"][0, 0], r["mag_res"][0, 0], r["count"][0, 0], mags[0][:, 0])


# ---- 3. ragged batch ------------------------------------------------------------------------------------------------------------------------
RAGGED_LENS = (69 * 240 + 7, 600, 0, 33 * 240)
RAGGED_PAIRS = ("speech", "noise", "tone", "dcnyq")


@functools.lru_cache(maxsize=None)
def _ragged_inputs():
    """samples past each length are 1.0 (x) and -1.0 (y): they must not be read as signal"""
    L = max(RAGGED_LENS)
    x, y = np.ones((len(RAGGED_LENS), L), np.float32), -np.ones((len(RAGGED_LENS), L), np.float32)
    for b, (n, name) in enumerate(zip(RAGGED_LENS, RAGGED_PAIRS)):
        if n:
            x[b, :n], y[b, :n] = sr.pair(name, n)
    return x, y


@functools.lru_cache(maxsize=None)
def _ragged():
    x, y = _ragged_inputs()
    return _run(_front(ALL), x, y, lens=list(RAGGED_LENS), extra_rows=3)


def test_ragged_batch_every_utterance_as_alone():
    r, mags = _ragged()
    x, y = _ragged_inputs()
    m = _front(ALL)
    for b, n in enumerate(RAGGED_LENS):
        xa, ya = (x[b:b + 1, :n], y[b:b + 1, :n]) if n else (np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32))
        r1, mags1 = _run(m, xa, ya, lens=[n])
        assert np.array_equal(r1["count"][:, 0], r["count"][:, b]), b
        assert np.array_equal(r1["sums"][:, 0].view(np.int64), r["sums"][:, b].view(np.int64)), (b, r1["sums"][:, 0], r["sums"][:, b])
        for i, (n_fft, hop, _) in enumerate(sr.RESOLUTIONS):
            T = 1 + n // hop if n > n_fft // 2 else 0
            assert r["count"][i, b] == T * (n_fft // 2 + 1)
            assert np.array_equal(mags1[i][:, 0, :T], mags[i][:, b, :T]) and np.all(mags[i][:, b, T:] == SENTINEL), (b, i)
            if T == 0:
                assert not r["sums"][i, b].any() and np.isnan(r["sc_res"][i, b]) and np.isnan(r["mag_res"][i, b])
            else:
                assert np.isfinite(r["sc_res"][i, b]) and np.isfinite(r["mag_res"][i, b])
    assert np.isnan(r["sc"][1]) and np.isnan(r["sc"][2]) and np.isfinite(r["sc"][0]) and np.isfinite(r["sc"][3])
    assert np.isfinite(r["sc_res"][0, 1]) and np.isfinite(r["sc_res"][2, 1]) and np.isnan(r["sc_res"][1, 1])   # 600 samples: too short for 2048 only


def test_pooled_figures_equal_the_reference_batch_call():
    L = 33 * 240
    names = ("speech", "noise", "tone")
    x, y = np.stack([sr.pair(n, L)[0] for n in names]), np.stack([sr.pair(n, L)[1] for n in names])
    r, _ = _run(_front(ALL), x, y)
    want = [sr.sc_mag(sr.stft_mag(x, res), sr.stft_mag(y, res)) for res in sr.RESOLUTIONS]   # the module on the batch, float64
    sc64, mag64 = np.mean([w[0] for w in want]), np.mean([w[1] for w in want])
    unit = sr.scalar_unit()
    for k, v, v64 in (("sc_batch", float(r["sc_batch"]), sc64), ("mag_batch", float(r["mag_batch"]), mag64)):
        print(f"{k}: gpu {v:.9e}  float64 {v64:.9e}  deviation {sr.rel_dev(v, v64):.3e} = {sr.rel_dev(v, v64) / unit:.2f} units")
        assert sr.rel_dev(v, v64) <= sr.FACTOR * unit


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    x, y = _ragged_inputs()
    r1, m1 = _ragged()
    r2, m2 = _run(_front(ALL), x, y, lens=list(RAGGED_LENS), extra_rows=3)
    assert np.array_equal(r1["sums"].view(np.int64), r2["sums"].view(np.int64)) and np.array_equal(r1["count"], r2["count"])
    for a, b in zip(m1, m2):
        assert np.array_equal(a, b)
    for i, (n_fft, hop, _) in enumerate(sr.RESOLUTIONS):   # rows past T_b, the three spare rows included, keep the sentinel
        for b, n in enumerate(RAGGED_LENS):
            T = 1 + n // hop if n > n_fft // 2 else 0
            assert np.all(m1[i][:, b, T:] == SENTINEL) and not np.any(m1[i][:, b, :T] == SENTINEL)


# ---- 5. memory-safety mode ------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_in_a_red_zone_context():
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    try:
        f, h, w = zip(*sr.RESOLUTIONS)
        m = stftloss.MultiResolutionSTFT(f, h, w, ctx=ctx)
        x, y = _ragged_inputs()
        r, mags = _run(m, x, y, lens=list(RAGGED_LENS), extra_rows=3)
        assert ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, ctx.last_error()
        ref, ref_mags = _ragged()
        assert np.array_equal(r["sums"].view(np.int64), ref["sums"].view(np.int64)) and np.array_equal(r["count"], ref["count"])
        for a, b in zip(mags, ref_mags):
            assert np.array_equal(a, b)
    finally:
        ctx.close()


# ---- 6. vocoder level -----------------------------------------------------------------------------------------------------------------------
def test_vocoder_stft_distance_and_argument_errors():
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cfg = synth.hifigan_config_v2()
    raw = {k: T(v) for k, v in synth.hifigan_state_dict(1234, cfg=cfg).items()}
    voc = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="f16")
    exact = vocoder.HifiGAN(state_dict=raw, config=cfg, precision="bf16x3")
    rng = np.random.default_rng(5)
    mels = torch.from_numpy((0.8 * rng.standard_normal((2, 40, 80)) - 2.0).astype(np.float32)).cuda()
    own = voc.forward_batch(mels)
    assert own.shape == (2, 40 * voc.hop)
    r = voc.stft_distance(mels, own)
    assert r["sc"].shape == (2,) and r["sc_res"].shape == (3, 2)
    for k in ("sc", "mag", "sc_res", "mag_res", "sc_batch", "mag_batch"):
        assert not r[k].cpu().numpy().any(), (k, r[k])                      # the same waveform: exactly 0
    near = voc.stft_distance(mels, exact.forward_batch(mels))                # fp16 against bf16x3 of the same mels
    other_mels = torch.from_numpy((0.8 * rng.standard_normal((2, 40, 80)) - 2.0).astype(np.float32)).cuda()
    far = voc.stft_distance(mels, exact.forward_batch(other_mels))           # against an unrelated waveform
    for k in ("sc", "mag"):
        a, b = near[k].cpu().numpy(), far[k].cpu().numpy()
        print(f"{k}: fp16 against bf16x3 {a}  against another waveform {b}")
        assert np.isfinite(a).all() and (a > 0).all() and (a < b).all(), (k, a, b)
    lens = torch.tensor([40, 25], dtype=torch.int32, device="cuda")
    rl = voc.stft_distance(mels, voc.forward_batch(mels, lens), lens)
    assert not rl["sc"].cpu().numpy().any() and rl["count"][0, 1].item() == (1 + 25 * voc.hop // 120) * 513

    # argument errors, in the library's style
    ctx = abi.Context()
    try:
        stream = torch.cuda.current_stream().cuda_stream
        sums, count = torch.zeros(3, 2, 3, dtype=torch.float64, device="cuda"), torch.zeros(3, 2, dtype=torch.int64, device="cuda")
        args = (own.data_ptr(), own.data_ptr(), None, 2, own.shape[1])
        with pytest.raises(abi.DttsError, match=r"\(-1\).*DTTS_PART_STFT"):          # DTTS_E_STATE: no plan yet
            ctx.stft_distance(*args, [120], sums.data_ptr(), count.data_ptr(), stream)
        with pytest.raises(abi.DttsError, match=r"\(-2\).*stft\.0\.window"):         # DTTS_E_NOENT
            ctx.finalize(abi.PART_STFT)
        ctx.load_state_dict("stft", {"0.window": np.ones(768, np.float32)})
        with pytest.raises(abi.DttsError, match=r"\(-22\).*n_fft = 768"):
            ctx.finalize(abi.PART_STFT)
        ctx.load_state_dict("stft", {"0.window": stftloss.centred_window(1024, 600)})
        ctx.finalize(abi.PART_STFT)
        for hop in (0, 1025):
            with pytest.raises(abi.DttsError, match=rf"\(-22\).*hop\[0\] = {hop}"):
                ctx.stft_distance(*args, [hop], sums.data_ptr(), count.data_ptr(), stream)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*n_res = 2"):
            ctx.stft_distance(*args, [120, 240], sums.data_ptr(), count.data_ptr(), stream)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*B = 0"):
            ctx.stft_distance(own.data_ptr(), own.data_ptr(), None, 0, own.shape[1], [120], sums.data_ptr(), count.data_ptr(), stream)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mag_cap = 3"):
            ctx.stft_distance(*args, [120], sums.data_ptr(), count.data_ptr(), stream, mag=own.data_ptr(), mag_cap=3)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*null"):
            ctx.stft_distance(*args, [120], None, count.data_ptr(), stream)
        a = abi.StftArgs(C.sizeof(abi.StftArgs) - 8, 1, (C.c_int32 * 4)(120, 0, 0, 0), 2, own.shape[1], 0, 0, own.data_ptr(), own.data_ptr(), None,
                         sums.data_ptr(), count.data_ptr(), None)
        assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_STFT_DISTANCE, C.byref(a), stream) == -22
        assert f"size = {C.sizeof(abi.StftArgs) - 8}" in ctx.last_error()
        ctx.stft_distance(*args, [120], sums.data_ptr(), count.data_ptr(), stream)   # and the good call goes through
        torch.cuda.synchronize()
        got = sums[0].cpu().numpy()                                                  # x = y: only sum m_y^2 is not zero
        assert count[0].tolist() == [(1 + own.shape[1] // 120) * 513] * 2 and not got[:, 0].any() and not got[:, 2].any() and (got[:, 1] > 0).all()
    finally:
        ctx.close()
