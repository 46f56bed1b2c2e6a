"""The multi-resolution STFT distance without a GPU: the float64 restatement (tests/stft_ref.py) against closed forms, the host logic of
dict_tts_amd/stftloss.py, the argument block against the header, and a CPU emulation of the kernel's summation inside the bounds that
tests/test_stftdist_gpu.py applies to the kernel itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stft_ref as sr
from dict_tts_amd import abi, stftloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against closed forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", sr.RESOLUTIONS)
def test_a_scaled_copy_gives_log_a_and_one_minus_one_over_a(res):
    """y = a x with every bin above the clamp: m_y = a m_x, so mag = |ln a| and sc = ||a m - m|| / ||a m|| = |1 - 1 / a|"""
    L = sr.lengths(res)[1]
    x = sr.pair("noise", L)[0].astype(np.float64)
    mx = sr.stft_mag(x, res)
    assert 0.25 * float(mx.min()) ** 2 > sr.CLAMP      # (white noise: no bin at the clamp, nor at half the amplitude)
    for a in (0.5, 3.0):
        sc, mag = sr.sc_mag(mx, sr.stft_mag(a * x, res))
        assert abs(mag - abs(np.log(a))) <= 1e-12 and abs(sc - abs(1 - 1 / a)) <= 1e-12, (a, sc, mag)


def test_equal_signals_give_zero_and_the_order_matters():
    res = sr.RESOLUTIONS[0]
    L = sr.lengths(res)[1]
    x, y = sr.pair("noise", L)
    mx, my = sr.stft_mag(x, res), sr.stft_mag(y, res)
    assert sr.sc_mag(mx, mx) == (0.0, 0.0)
    sc_xy, mag_xy = sr.sc_mag(mx, my)     # forward(x, y): y = x / 2 normalises -> |1 - 2| = 1
    sc_yx, mag_yx = sr.sc_mag(my, mx)     # forward(y, x): -> |1 - 1 / 2|
    assert abs(sc_xy - 1.0) <= 1e-12 and abs(sc_yx - 0.5) <= 1e-12
    assert abs(mag_xy - mag_yx) <= 1e-15 and abs(mag_xy - np.log(2.0)) <= 1e-12


def test_the_restatement_is_torch_stft_with_reflect_padding_and_a_centred_window():
    """frames, padding and window spelled out with numpy against torch.stft: 1 + L // hop frames, fft_size / 2 + 1 bins"""
    for res in sr.RESOLUTIONS:
        n_fft, hop, win = res
        for L in sr.lengths(res)[1:]:
            x = sr.pair("speech", L)[0]
            fr = sr.reflect_frames(x, n_fft, hop).astype(np.float64) * sr.mr.window_of(n_fft, win)[None, :]
            want = np.sqrt(np.maximum(np.abs(np.fft.rfft(fr, axis=1)) ** 2, sr.CLAMP))
            got = sr.stft_mag(x, res).numpy()
            assert got.shape == want.shape == (1 + L // hop, n_fft // 2 + 1)
            assert np.max(np.abs(got - want)) <= 1e-11


def test_the_dc_nyquist_pair_lives_at_the_two_edges_of_the_spectrum():
    """the main lobe of a 600-sample Hann window is +-3.4 bins of 1024 wide: four bins at each end carry the energy, and bin 0 and bin
    fft_size / 2 themselves so much of it that losing either shows"""
    res = sr.RESOLUTIONS[0]
    x, _ = sr.pair("dcnyq", sr.lengths(res)[0])
    p = sr.stft_mag(x, res).numpy() ** 2
    assert (p[:, :4].sum() + p[:, -4:].sum()) / p.sum() > 0.999
    assert p[:, 0].sum() / p.sum() > 0.1 and p[:, -1].sum() / p.sum() > 0.4


# ---- host logic of stftloss ---------------------------------------------------------------------------------------------------------------
def test_window_centring_matches_torch_stft():
    for n_fft, _, win in sr.RESOLUTIONS + ((512, 50, 511), (512, 50, 512)):
        w = stftloss.centred_window(n_fft, win)
        left = (n_fft - win) // 2
        assert w.dtype == np.float32 and w.shape == (n_fft,)
        assert not w[:left].any() and not w[left + win:].any()
        assert np.array_equal(w[left:left + win], torch.hann_window(win, dtype=torch.float64).numpy().astype(np.float32))
    with pytest.raises(ValueError, match="win_length = 513"):
        stftloss.centred_window(512, 513)


def test_frame_counts():
    assert stftloss.frame_count(69 * 120 + 7, 120, 1024) == 70
    assert stftloss.frame_count(33 * 240, 240, 2048) == 34
    assert stftloss.frame_count(1025, 240, 2048) == 5
    assert stftloss.frame_count(1024, 240, 2048) == 0 and stftloss.frame_count(0, 50, 512) == 0


def test_sums_become_scores_with_nan_where_a_resolution_has_no_frame():
    sums = torch.tensor([[[4.0, 16.0, 6.0], [1.0, 4.0, 2.0]], [[9.0, 36.0, 8.0], [0.0, 0.0, 0.0]]], dtype=torch.float64)
    count = torch.tensor([[3, 2], [4, 0]])
    r = stftloss.scores(sums, count)
    assert torch.equal(r["sc_res"][:, 0], torch.tensor([0.5, 0.5], dtype=torch.float64))
    assert torch.equal(r["mag_res"][:, 0], torch.tensor([2.0, 2.0], dtype=torch.float64))
    assert float(r["sc_res"][0, 1]) == 0.5 and float(r["mag_res"][0, 1]) == 1.0
    assert torch.isnan(r["sc_res"][1, 1]) and torch.isnan(r["mag_res"][1, 1])
    assert float(r["sc"][0]) == 0.5 and float(r["mag"][0]) == 2.0 and torch.isnan(r["sc"][1]) and torch.isnan(r["mag"][1])
    # pooled: the sums and the counts of the batch first, then the mean over the resolutions
    assert float(r["sc_batch"]) == pytest.approx(0.5 * (np.sqrt(5.0 / 20.0) + np.sqrt(9.0 / 36.0)), abs=1e-15)
    assert float(r["mag_batch"]) == pytest.approx(0.5 * (8.0 / 5.0 + 8.0 / 4.0), abs=1e-15)


def test_pooled_scores_equal_the_reference_batch_call():
    res = sr.RESOLUTIONS[2]
    L = sr.lengths(res)[1]
    names = ("speech", "noise", "tone")
    mx = torch.stack([sr.stft_mag(sr.pair(n, L)[0], res) for n in names])
    my = torch.stack([sr.stft_mag(sr.pair(n, L)[1], res) for n in names])
    sc, mag = sr.sc_mag(mx, my)     # the module on the batch
    per = [sr.sums_of(mx[b].numpy(), my[b].numpy()) for b in range(len(names))]
    r = stftloss.scores(np.stack([s for s, _ in per])[None], np.array([[c for _, c in per]]))
    assert float(r["sc_batch"]) == pytest.approx(sc, rel=1e-12) and float(r["mag_batch"]) == pytest.approx(mag, rel=1e-12)


def test_a_short_signal_is_refused_before_the_gpu_is_touched():
    m = stftloss.MultiResolutionSTFT()
    assert (m.fft_sizes, m.hop_sizes, m.win_lengths) == ([1024, 2048, 512], [120, 240, 50], [600, 1200, 240])
    with pytest.raises(ValueError, match="L = 1024"):
        m(np.zeros((2, 1024), np.float32), np.zeros((2, 1024), np.float32))
    assert m.ctx is None      # nothing was created
    with pytest.raises(ValueError, match="fft_size = 768"):
        stftloss.MultiResolutionSTFT((768,), (100,), (300,))
    with pytest.raises(ValueError, match="hop = 513"):
        stftloss.MultiResolutionSTFT((512,), (513,), (300,))
    with pytest.raises(ValueError, match="same length"):
        stftloss.MultiResolutionSTFT((512, 1024), (50,), (240, 600))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as f:
        return f.read()


def test_the_argument_block_matches_the_header(tmp_path):
    text = _header()
    body = re.search(r"typedef struct dtts_stft_args \{(.*?)\} dtts_stft_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        if "*" in decl:
            fields.append((decl.replace("*", " ").split()[-1], C.c_void_p))
            continue
        ctype = decl.split()[0]
        for nm in decl[len(ctype):].split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", nm)
            base = {"int32_t": C.c_int32, "float": C.c_float}[ctype]
            fields.append((arr.group(1), base * int(arr.group(2))) if arr else (nm, base))
    assert [n for n, _ in fields] == [n for n, _ in abi.StftArgs._fields_]

    class Mirror(C.Structure):
        _fields_ = fields
    assert C.sizeof(Mirror) == C.sizeof(abi.StftArgs) == 88
    for n, _ in fields:
        assert getattr(Mirror, n).offset == getattr(abi.StftArgs, n).offset, n
    assert int(re.search(r"#define DTTS_PART_STFT (\d+)", text).group(1)) == abi.PART_STFT == 16
    assert int(re.search(r"#define DTTS_OUT_STFT_DISTANCE (\d+)", text).group(1)) == abi.OUT_STFT_DISTANCE == 11


def test_no_new_export():
    names = re.findall(r"DTTS_API\s+[\w\s\*]+?\b(dtts_\w+)\s*\(", _header())
    assert sorted(names) == sorted(abi.EXPORTS) and len(abi.EXPORTS) == 32


# ---- the kernel's summation, emulated ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", sr.RESOLUTIONS)
def test_the_emulated_kernel_summation_meets_the_gpu_bounds(res):
    unit = sr.scalar_unit()
    print(f"scalar unit (float32 path, pooled): {unit:.3e}")
    for L in (sr.lengths(res)[0], sr.lengths(res)[2]):
        for name in sr.PAIRS:
            r = sr.reference(name, res, L)
            x, y = sr.pair(name, L)
            mx = sr.emulate_mag(x, res)
            my = mx if name == "same" else sr.emulate_mag(y, res)
            for s, (m, m64, e32) in enumerate(zip((mx, my), r["m64"], r["e32"])):
                e = sr.mag_error(m, m64)
                print(f"{res} L={L} {name}[{'xy'[s]}]: magnitude error emulation {e:.3e}  float32 path {e32:.3e}  ratio {e / e32 if e32 else 0:.2f}")
                assert e <= sr.FACTOR * e32, (name, s, e, e32)
            sc, mag = sr.sc_mag_of_sums(*sr.emulate_sums(mx, my))
            for k, v in (("sc", sc), ("mag", mag)):
                v64 = r[k + "64"]
                dev = sr.rel_dev(v, v64)
                print(f"{res} L={L} {name}: {k} emulation {v:.9e}  float64 {v64:.9e}  deviation {dev:.3e} = {dev / unit:.2f} units")
                if v64 == 0:
                    assert v == 0
                else:
                    assert dev <= sr.FACTOR * unit, (name, k, v, v64, unit)
