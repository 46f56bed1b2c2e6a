"""Waveform conditioning, the parts that need no GPU: the ABI surface of dtts_text2mel_fetch(DTTS_OUT_RESAMPLE / DTTS_OUT_LOUDNESS) with the
refusals of their argument blocks (checked before the handle, so a NULL handle reaches them), the Python layer's argument checks, and the
float64 restatements (tests/wavprep_ref.py) themselves, anchored physically: sines against the analytic sine, an impulse against the
interpolated table, the 997 Hz conformance tone, the BS.1770 coefficient table.

Neither librosa, resampy nor pyloudnorm is on the build machine: the restatements ARE the definition (include/dicttts_hip.h).
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import wavprep_ref as wr
import wavprep_shapes as ws
from dict_tts_amd import abi
from dict_tts_amd import wavprep as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |resampled - analytic sine| of the restatement away from the edges, as measured (kaiser_best, 4000 input samples, unit amplitude; the
# input is the float32 sine, whose own quantisation is 3e-8); the test asserts 2 x these
SINE_ERR = {(44100, 22050, 5000.0): 4.10e-8,    # index_step exactly 256
            (48000, 22050, 5000.0): 6.53e-4,    # index_step 235, truncated from 235.2: resampy's own inaccuracy at this ratio
            (16000, 22050, 5000.0): 1.90e-6,
            (48000, 22050, 15000.0): 1.09e-4}   # above the new Nyquist frequency: what is left of it (against zero)
# the 997 Hz full-scale sine, 5 s: LKFS of the restatement, as measured
TONE_LKFS = {48000: -3.0517, 44100: -3.0524, 22050: -3.0664, 16000: -3.0832}


def _struct_names(hdr, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.search(r"([A-Za-z_0-9]+)$", part.strip()).group(1) for part in decl.split(",")]
    return names


def test_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    d = lambda n: int(re.search(rf"#define {n} (\d+)", hdr).group(1))
    assert d("DTTS_PART_RESAMPLE") == abi.PART_RESAMPLE == 64
    assert d("DTTS_OUT_RESAMPLE") == abi.OUT_RESAMPLE == 17
    assert d("DTTS_OUT_LOUDNESS") == abi.OUT_LOUDNESS == 18
    assert d("DTTS_F64") == abi.DTTS_F64 == 2
    assert d("DTTS_RESAMPLE_TILE") == abi.RESAMPLE_TILE and d("DTTS_LOUD_SEGMENT") == abi.LOUD_SEGMENT
    assert (d("DTTS_LOUD_TOO_SHORT"), d("DTTS_LOUD_SILENT"), d("DTTS_LOUD_PEAK")) == (abi.LOUD_TOO_SHORT, abi.LOUD_SILENT, abi.LOUD_PEAK) == (1, 2, 4)
    assert _struct_names(hdr, "dtts_resample_args") == [f[0] for f in abi.ResampleArgs._fields_]
    assert _struct_names(hdr, "dtts_loudness_args") == [f[0] for f in abi.LoudnessArgs._fields_]
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(abi.ResampleArgs) == 6 * 4 + 5 * vp and abi.ResampleArgs.wav_dev.offset == 24 and abi.ResampleArgs.out64_dev.offset == 24 + 4 * vp
    assert C.sizeof(abi.LoudnessArgs) == 6 * 4 + 8 + 8 * vp and abi.LoudnessArgs.target_lufs.offset == 24 and abi.LoudnessArgs.wav_dev.offset == 32
    assert abi.LoudnessArgs.n_blocks_dev.offset == 32 + 7 * vp
    # the ABI keeps its entry points: both units are items of dtts_text2mel_fetch
    assert len(set(abi.EXPORTS)) == 32 and not [s for s in abi.EXPORTS if "resample" in s or "loud" in s]
    emap = open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()
    assert "resample" not in emap and "loud" not in emap


def test_resample_refusals_name_their_field():
    lib = abi.load_library()
    good = dict(B=2, wav=0x1000, wav_ld=4096, out=0x2000, out_ld=2000, out_lens=0x3000, sr_in=48000, sr_out=22050, lens=0x4000, out64=0x5000)

    def refused(match, **kw):
        a = abi.resample_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_RESAMPLE, C.byref(a), None) == -22   # DTTS_E_INVAL
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"B = 0 ", B=0)
    refused(r"B = 65536", B=65536)
    refused(r"wav_ld = 0 ", wav_ld=0)
    refused(rf"wav_ld = {(1 << 26) + 1}", wav_ld=(1 << 26) + 1)
    refused(r"out_ld = 0 ", out_ld=0)
    refused(r"sr_in = 7999", sr_in=7999)
    refused(r"sr_out = 48001", sr_out=48001)
    refused(r"sr_out = sr_in = 22050", sr_in=22050)
    refused(r"null wav_dev", wav=None)
    refused(r"null wav_dev / out_dev", out=None)
    refused(r"out_lens_dev", out_lens=None)
    refused(r"wav_dev = 0x1002 is not aligned to 4", wav=0x1002)
    refused(r"lens_dev = 0x4001 is not aligned to 4", lens=0x4001)
    refused(r"out_dev = 0x2002 is not aligned to 4", out=0x2002)
    refused(r"out_lens_dev = 0x3001 is not aligned to 4", out_lens=0x3001)
    refused(r"out64_dev = 0x5004 is not aligned to 8", out64=0x5004)
    a = abi.resample_args(**good)
    a.size -= 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_RESAMPLE, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.ResampleArgs) - 8}" in lib.dtts_last_error(None).decode()
    refused(r"null handle")                                      # a good block: only then is the handle looked at
    for sr_in, sr_out in ws.RATIOS:
        refused(r"null handle", sr_in=sr_in, sr_out=sr_out)
    assert lib.dtts_text2mel_fetch(None, abi.OUT_RESAMPLE, None, None) == -22


def test_loudness_refusals_name_their_field():
    lib = abi.load_library()
    good = dict(B=2, wav=0x1000, wav_ld=48000, blocks_ld=27, sample_rate=16000, lufs=0x2000, gain=0x3000, status=0x4000, mode=1, lens=0x5000,
                out=0x6000, z=0x7000, n_blocks=0x8000)

    def refused(match, **kw):
        a = abi.loudness_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_LOUDNESS, C.byref(a), None) == -22
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"B = 0 ", B=0)
    refused(r"B = 65536", B=65536)
    refused(r"wav_ld = 0 ", wav_ld=0)
    refused(rf"wav_ld = {(1 << 26) + 1}", wav_ld=(1 << 26) + 1)
    refused(r"sample_rate = 7999", sample_rate=7999)
    refused(r"sample_rate = 48001", sample_rate=48001)
    refused(r"mode = 2", mode=2)
    refused(r"target_lufs = nan", target_lufs=float("nan"))
    refused(r"blocks_ld = 26 blocks .*wav_ld = 48000 samples give 27", blocks_ld=26)
    refused(r"blocks_ld = 0 ", blocks_ld=0, wav_ld=100)
    refused(r"null wav_dev", wav=None)
    refused(r"lufs_dev", lufs=None)
    refused(r"gain_dev", gain=None)
    refused(r"status_dev", status=None)
    refused(r"null out_dev with mode = 1", out=None)
    refused(r"wav_dev = 0x1002 is not aligned to 4", wav=0x1002)
    refused(r"lens_dev = 0x5001 is not aligned to 4", lens=0x5001)
    refused(r"status_dev = 0x4002 is not aligned to 4", status=0x4002)
    refused(r"out_dev = 0x6002 is not aligned to 4", out=0x6002)
    refused(r"n_blocks_dev = 0x8002 is not aligned to 4", n_blocks=0x8002)
    refused(r"lufs_dev = 0x2004 is not aligned to 8", lufs=0x2004)
    refused(r"gain_dev = 0x3004 is not aligned to 8", gain=0x3004)
    refused(r"z_dev = 0x7004 is not aligned to 8", z=0x7004)
    a = abi.loudness_args(**good)
    a.size += 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_LOUDNESS, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.LoudnessArgs) + 8}" in lib.dtts_last_error(None).decode()
    refused(r"null handle")
    refused(r"null handle", mode=0, out=None, z=None, n_blocks=None, lens=None)
    assert lib.dtts_text2mel_fetch(None, abi.OUT_LOUDNESS, None, None) == -22


def test_python_layer_argument_errors_surface_without_a_gpu():
    z = lambda *s: np.zeros(s, np.float32)
    for a, b, match in ((7000, 22050, "sr_in"), (48000, 50000, "sr_out"), (22050.5, 16000, "sr_in"), (22050, 22050, "nothing to resample")):
        with pytest.raises(ValueError, match=match):
            W.Resampler(a, b)
    with pytest.raises(ValueError, match="filter = 'sinc_best'"):
        W.Resampler(48000, 22050, filter="sinc_best")
    with pytest.raises(ValueError, match="num_table = 3"):
        W.Resampler(48000, 22050, filter=(np.zeros(7), 3))
    with pytest.raises(ValueError, match="7 entries"):
        W.Resampler(48000, 22050, filter=(np.zeros(7), 4))
    with pytest.raises(ValueError, match="index_step = 0"):
        W.Resampler(48000, 8000, filter=(np.zeros(9), 4))
    rs = W.Resampler(48000, 22050)
    assert rs.index_step == 235 and rs.num_table == 512 and len(rs.win) == 32769 and rs.out_len(321) == 148
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        rs(z(100))
    with pytest.raises(ValueError, match="lens has 3 entries"):
        rs(z(2, 1000), lens=[1, 2, 3])
    with pytest.raises(ValueError, match="sample_rate"):
        W.Loudness(4000)
    ln = W.Loudness(16000)
    assert ln.blocks(7200) == 1 and ln.blocks(8800) == 3 and ln.blocks(6399) == 0
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        ln.measure(z(100))
    with pytest.raises(ValueError, match="lens has 1 entries"):
        ln.normalize(z(2, 8000), lens=[8000])
    with pytest.raises(ValueError, match="target"):
        ln.normalize(z(2, 8000), target=float("inf"))


def test_wav2spec_defaults_still_refuse_another_rate(tmp_path):
    from scipy.io import wavfile
    from dict_tts_amd.vocoder import HifiGAN
    fn = str(tmp_path / "a16k.wav")
    wavfile.write(fn, 16000, (np.sin(np.arange(8000) / 10.0) * 10000).astype(np.int16))
    with pytest.raises(ValueError, match=r"16000.*22050"):
        HifiGAN.wav2spec(fn)
    with pytest.raises(NotImplementedError):
        HifiGAN.wav2spec(fn, return_linear=True, resample=True)
    sr, wav = W.read_wav_native(fn)
    assert sr == 16000 and wav.dtype == np.float32 and wav.shape == (8000,) and np.abs(wav).max() < 0.31
    assert W.load_wav(fn, 16000) is not None and np.array_equal(W.load_wav(fn, 16000), wav)      # the file's own rate: no device needed
    with pytest.raises(ValueError, match="does not resample"):
        from dict_tts_amd import melspec
        melspec.read_wav(fn, 22050)


def test_filter_tables():
    win, nt = W.kaiser_best()
    assert win.dtype == np.float64 and win.shape == (32769,) and nt == 512
    assert win[0] == 0.9475937167399596 and abs(win[-1]) < 1e-7           # rolloff sinc(0) I0(beta) / I0(beta); the window's foot
    z = win[512::512]                                                      # sinc(rolloff k): no exact zeros, but small next to the lobes
    assert np.all(np.abs(z[:8]) < 0.06)
    wf, ntf = W.kaiser_fast()
    assert wf.shape == (8193,) and ntf == 512 and wf[0] == 0.85
    d = wr.delta_table(win)
    assert d[-1] == 0.0 and np.array_equal(d[:-1], win[1:] - win[:-1])


def test_k_weighting_against_the_bs1770_table():
    """48 kHz: the shelf within 1e-3 of the coefficients ITU-R BS.1770 tabulates (b0 = 1.53518 against 1.53512: pyloudnorm designs the
    stage from (G, Q, fc), the standard lists the rounded result of another design)"""
    (bs, as_), (bh, ah) = W.k_weighting(48000)
    assert np.allclose(bs, [1.53512485958697, -2.69169618940638, 1.19839281085285], atol=1e-3, rtol=0)
    assert np.allclose(as_, [1.0, -1.69065929318241, 0.73248077421585], atol=1e-3, rtol=0)
    assert abs(bs[0] - 1.53518) < 1e-5
    assert np.allclose(ah, [1.0, -1.99004745483398, 0.99007225036621], atol=1e-4, rtol=0)
    assert abs(bh.sum()) < 1e-12 and abs(bh[0] * 4 / (1 + ah[1] * -1 + ah[2]) - 1) < 1e-9   # a zero at DC; gain 1 at the Nyquist end
    assert [W.n_blocks_of(L, 16000) for L in (6399, 6400, 7200, 8800, 7360)] == [0, 1, 1, 3, 2]
    b = W.block_bounds(11025, 4)
    assert b.tolist() == [[0, 4410], [1102, 5512], [2205, 6615], [3307, 7717]]


@pytest.mark.parametrize("rate", sorted(TONE_LKFS))
def test_restatement_meets_the_997_hz_conformance_tone(rate):
    """a full-scale 997 Hz sine of 5 s measures -3.01 LKFS within the EBU band of +- 0.1; measured: 48 kHz -3.0517, 44.1 kHz -3.0524,
    22.05 kHz -3.0664, 16 kHz -3.0832 (the fixed analogue prototype warps with the rate)"""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * rate) / rate).astype(np.float32)
    r = wr.loudness(x, rate)
    print(f"997 Hz at {rate} Hz: {r['lufs']:.4f} LKFS")
    assert abs(r["lufs"] - -3.01) <= 0.1 and abs(r["lufs"] - TONE_LKFS[rate]) < 2e-4 and r["status"] == 0


def test_restatement_gates_the_quiet_half_away():
    """6 s, the second half 60 dB down: every block inside the quiet half is gated away, every block inside the loud half counts, and the
    figure is the loud half's own within the share of the three straddling blocks (measured: -7.976 against -7.748 LUFS)"""
    rate = 16000
    x = np.concatenate([ws._noise(3 * rate, 77, 0.3), ws._noise(3 * rate, 78, 0.3e-3)])
    r, r1 = wr.loudness(x, rate), wr.loudness(x[:3 * rate], rate)
    bd = W.block_bounds(rate, r["n_blocks"])
    passed = (r["levels"] > r["gamma"]) & (r["levels"] > -70.0)
    assert passed[bd[:, 1] <= 3 * rate].all() and not passed[bd[:, 0] >= 3 * rate].any()
    print(f"half loud, half quiet: {r['lufs']:.4f} LUFS, the loud half alone {r1['lufs']:.4f}")
    assert abs(r["lufs"] - r1["lufs"]) < 0.5


def test_biquad_restatement_is_scipys_lfilter():
    from scipy.signal import lfilter
    x = ws._noise(5000, 5, 0.3)
    (bs, as_), (bh, ah) = W.k_weighting(22050)
    y = lfilter(bh, ah, lfilter(bs, as_, x.astype(np.float64)))
    assert np.allclose(wr.k_filter(x, 22050), y, rtol=0, atol=1e-12 * np.abs(y).max())


def _table_value(win, nt, step, tscale, pos):
    """the interpolated table at `pos` table entries from the centre, with resampy's cut: an entry is used while idx + step <= n_win"""
    idx = int(pos)
    if idx + step > len(win):
        return 0.0
    nxt = win[idx + 1] if idx + 1 < len(win) else win[idx]              # the last delta is 0
    return tscale * (win[idx] + (pos - idx) * (nxt - win[idx]))


@pytest.mark.parametrize("sr_in,sr_out,filt", [(16000, 22050, "kaiser_best"), (44100, 22050, "kaiser_best"), (8000, 12000, "tiny")])
def test_impulse_returns_the_interpolated_table(sr_in, sr_out, filt):
    """x = an impulse at p: y[t] is the table read at |t inc - p| scale num_table entries.  Where scale num_table is an integer (every ratio
    >= 1, and 44100 -> 22050) that position is what off + i index_step and eta add up to; a table with num_table = 1 reaches the last
    entry and its zero delta"""
    win, nt = (np.array([1.0, 0.5, -0.25, 0.125, 0.0625]), 1) if filt == "tiny" else ws.table(filt)
    L, p = 300, 150
    x = np.zeros(L, np.float32)
    x[p] = 1.0
    r = wr.resample(x, sr_in, sr_out, win, nt)
    g = wr.resample_geometry(L, sr_in, sr_out, len(win), nt)
    assert g["scale"] * nt == g["index_step"]
    want = np.array([_table_value(win, nt, g["index_step"], g["tscale"], abs(t * g["inc"] - p) * g["scale"] * nt) for t in range(r["n_out"])])
    assert np.abs(r["y64"]).max() > 0.4 and np.abs(r["y64"] - want).max() < 1e-12
    if filt == "tiny":
        assert (np.abs(want) == 0.0625).any()                             # the last entry itself was read


def test_lengths():
    for sr_in, sr_out in ws.RATIOS:
        for L in (1, 2, 319, 320, 321, 1000):
            x = np.zeros(L, np.float32)
            r = wr.resample(x, sr_in, sr_out, *ws.table("kaiser_fast"))
            lr = L * (sr_out / sr_in)
            assert r["n_out"] == len(r["y64"]) == int(lr) and r["out_len"] == len(r["out"]) == math.ceil(lr) == W.resampled_len(L, sr_in, sr_out)[1]
    assert [ws.rs_ref(f"len_{L}")["n_out"] for L in (319, 320, 321, 640, 960, 961)] == [146, 147, 147, 294, 441, 441]
    assert [ws.rs_ref(f"len_{L}")["out_len"] for L in (319, 320, 321, 640, 960, 961)] == [147, 147, 148, 294, 441, 442]
    assert [ws.rs_ref(f"outputs_{n}")["n_out"] for n in (255, 256, 257, 773)] == [255, 256, 257, 773]
    c = ws.RS_BY_NAME["len_321"]
    assert np.array_equal(wr.resample_scalar(c["x"], c["sr_in"], c["sr_out"], *ws.table("kaiser_best")), ws.rs_ref("len_321")["y64"])


@pytest.mark.parametrize("sr_in,sr_out,f", sorted(SINE_ERR))
def test_restatement_resamples_a_sine(sr_in, sr_out, f):
    """max |y - analytic| away from the edges, measured: 44100 -> 22050 4.10e-8 (5 kHz), 48000 -> 22050 6.53e-4 (5 kHz; the truncated
    index_step), 16000 -> 22050 1.90e-6 (5 kHz), and 1.09e-4 left of a 15 kHz sine at 48000 -> 22050.  The bound is 2 x the measured."""
    win, nt = ws.table("kaiser_best")
    x = np.sin(2 * np.pi * f * np.arange(4000) / sr_in).astype(np.float32)
    r = wr.resample(x, sr_in, sr_out, win, nt)
    edge = int(math.ceil((len(win) - 1) / r["index_step"] * max(1.0, sr_out / sr_in))) + 2
    t = np.arange(r["n_out"]) / sr_out
    want = np.sin(2 * np.pi * f * t) if f < sr_out / 2 else np.zeros_like(t)
    err = float(np.abs(r["y64"] - want)[edge:-edge].max())
    print(f"{sr_in} -> {sr_out}, {f:g} Hz: max error {err:.3e}")
    assert r["n_out"] > 4 * edge and err <= 2 * SINE_ERR[(sr_in, sr_out, f)]


def test_reference_rounding_variants():
    """How far the libraries' own rounding lies from the float64 restatement, on the GPU cases (the figures INTEGRATION.md quotes).
    Resampler, float32 y[t] after every tap: at most 13.7 float32 ulps of the row's peak (48000 -> 8000, 770 taps; 2 .. 6 ulps at the
    other ratios).  Loudness, float32 storage after each filter stage with float32 squares and numpy's float32 sum: at most 2.6e-7 LU."""
    worst = 0.0
    for c in ws.RS_CASES:
        a, b = ws.rs_ref(c["name"]), ws.rs_ref(c["name"], True)
        if a["n_out"] and np.abs(a["y64"]).max() > 0:
            worst = max(worst, float(np.abs(a["y64"] - b["y64"]).max() / np.spacing(np.float32(np.abs(a["y64"]).max()))))
    print(f"resampler, per-tap float32: {worst:.2f} ulps of the row's peak")
    assert worst <= 32.0                      # sqrt(770 taps) half-ulp steps of a random walk is 14; 2 x that and a little
    worst = 0.0
    for c in ws.LD_CASES:
        a, b = ws.ld_ref(c["name"]), ws.ld_ref(c["name"], True)
        assert a["status"] == b["status"]
        if not a["status"] & 3:
            worst = max(worst, abs(a["lufs"] - b["lufs"]))
    print(f"loudness, float32 storage: {worst:.3e} LU")
    assert worst <= 1e-6                      # 2^-24 relative per sample, averaged over >= 3200 squares; 1e-6 LU is 2.3e-7 relative


def test_case_lists_cover_the_specification():
    names = {c["name"] for c in ws.RS_CASES}
    assert {f"noise_{a}_{b}" for a, b in ws.RATIOS} <= names and "fast_48000_22050" in names
    assert all(c["x"].dtype == np.float32 and c["L"] <= 3001 for c in ws.RS_CASES)
    wing = (32769 - 1) // 235
    assert ws.RS_BY_NAME["len_50"]["L"] < wing and (ws.rs_ref("len_50")["taps"] == 50).all()   # both wings clipped by the utterance: L taps
    assert ws.rs_ref("noise_48000_8000")["taps"].max() >= 769                                  # the longest wings of the supported rates
    assert len(ws.RS_BATCH) >= 10 and len({ws.RS_BY_NAME[n]["L"] for n in ws.RS_BATCH}) >= 8
    rates = {c["rate"] for c in ws.LD_CASES}
    assert rates == {22050, 16000, 48000, 44100, 11025}
    assert all(c["L"] <= 3 * 16000 for c in ws.LD_CASES)
    assert [ws.ld_ref(n)["n_blocks"] for n in ("one_block", "one_block_less", "one_block_more", "tie_7200", "tie_8800", "cut_7360")] == [1, 0, 1, 1, 3, 2]
    assert ws.LD_BY_NAME["seg_exact"]["L"] % abi.LOUD_SEGMENT == 0 and ws.LD_BY_NAME["one_block"]["L"] % abi.LOUD_SEGMENT == 0
    for c in ws.LD_CASES:
        want = {"ok": 0, "short": 1, "silent": 2, "peak": 4}[c["kind"]]
        st = ws.ld_ref(c["name"])["status"]
        assert st == want or (c["kind"] == "ok" and st == 4 and c["name"] == "seam_impulse"), (c["name"], st)
    r = ws.ld_ref("loud_quiet")
    assert ((r["levels"] > -70) & ~(r["levels"] > r["gamma"])).any()       # the relative gate drops blocks the absolute gate passed
    assert (ws.ld_ref("zeros_first")["z"] == 0.0).sum() >= 4
    assert ws.LD_BY_NAME["seam_impulse"]["x"][5 * abi.LOUD_SEGMENT - 1] == np.float32(0.9)


@pytest.mark.parametrize("case", ws.LD_CASES, ids=lambda c: c["name"])
def test_gate_margins_of_the_restatement(case):
    """every gate decision the device must reproduce is well-posed: |l_j + 70| and |l_j - Gamma_r| >= 1e-6 LU, or z_j == 0 exactly (which
    the margin leaves out: -inf is on the right side of any gate).  The cases built to be silent have no Gamma_r; their distance to -70
    is checked alone."""
    r = ws.ld_ref(case["name"])
    print(f"{case['name']}: {r['n_blocks']} blocks, margin {r['margin']:.3e} LU")
    assert r["margin"] >= 1e-6
