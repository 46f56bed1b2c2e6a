"""F0 extraction, the parts that need no GPU: the ABI surface of dtts_text2mel_fetch(DTTS_OUT_PITCH) with every refusal of its argument block
(the block is checked before the handle, so a NULL handle reaches them all), the Python layer's argument checks, f0_to_coarse, and the
float64 restatement (tests/pitch_ref.py) itself: against the true frequency of synthetic tones, and with the decision margin of its path on
every case of tests/pitch_shapes.py.

There is no Praat on the build machine: the restatement IS the definition (include/dicttts_hip.h), and the tones are its sanity check.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pitch_ref as pr
import pitch_shapes as ps
from dict_tts_amd import abi
from dict_tts_amd import pitch as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |f0 - true| of the restatement over the nine frames of each five-harmonic tone, as measured (Hz); the test asserts 3 x these
TONE_ERR = {90.0: 0.011657, 123.4: 0.002769, 220.5: 0.001182, 440.0: 0.000148, 700.0: 0.0000059}


def test_argument_block_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert int(re.search(r"#define DTTS_OUT_PITCH (\d+)", hdr).group(1)) == abi.OUT_PITCH == 16
    assert int(re.search(r"#define DTTS_PITCH_CANDIDATES (\d+)", hdr).group(1)) == abi.PITCH_CANDIDATES == pr.NCAND == 15
    assert int(re.search(r"#define DTTS_PITCH_MAX_WINDOW (\d+)", hdr).group(1)) == abi.PITCH_MAX_WINDOW
    assert int(re.search(r"#define DTTS_PITCH_MAX_FRAMES (\d+)", hdr).group(1)) == abi.PITCH_MAX_FRAMES == abi.DTW_MAX_LEN
    body = re.search(r"typedef struct dtts_pitch_args \{(.*?)\} dtts_pitch_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.search(r"([A-Za-z_0-9]+)$", part.strip()).group(1) for part in decl.split(",")]
    assert names == [f[0] for f in abi.PitchArgs._fields_], names
    assert C.sizeof(abi.PitchArgs) == 6 * 4 + 7 * 8 + 9 * C.sizeof(C.c_void_p)
    assert abi.PitchArgs.pitch_floor.offset == 24 and abi.PitchArgs.wav_dev.offset == 80 and abi.PitchArgs.selected_dev.offset == 144
    # the ABI keeps its entry points: the unit is an item of dtts_text2mel_fetch
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "pitch" in s]
    assert "pitch" not in open(os.path.join(ROOT, "dict_tts_amd", "csrc", "exports.map")).read()


def test_every_refusal_names_its_field():
    lib = abi.load_library()
    good = dict(B=2, wav=0x1000, wav_ld=4096, frames_ld=13, f0=0x2000, n_frames=0x3000, lens=0x4000, acf=0x5000, cand=0x6000, n_cand=0x7000,
                intensity=0x8000, selected=0x9000)

    def refused(match, **kw):
        a = abi.pitch_args(**{**good, **kw})
        assert lib.dtts_text2mel_fetch(None, abi.OUT_PITCH, C.byref(a), None) == -22   # DTTS_E_INVAL
        msg = lib.dtts_last_error(None).decode()
        assert re.search(match, msg), (match, msg)

    refused(r"B = 0 ", B=0)
    refused(r"B = -3", B=-3)
    refused(r"B = 65536", B=65536)
    refused(r"wav_ld = 0 ", wav_ld=0)
    refused(rf"wav_ld = {(1 << 26) + 1}", wav_ld=(1 << 26) + 1)
    refused(r"sample_rate = 7999", sample_rate=7999)
    refused(r"sample_rate = 48001", sample_rate=48001)
    refused(r"hop = 0 ", hop=0)
    refused(r"hop = 4097", hop=4097)
    refused(r"pitch_floor = 5 ", pitch_floor=5.0)
    refused(r"pitch_floor = nan", pitch_floor=float("nan"))
    refused(r"pitch_floor = 20 gives a window of 3304 samples", pitch_floor=20.0)
    refused(r"pitch_ceiling = 80 ", pitch_ceiling=80.0)
    refused(r"pitch_ceiling = inf", pitch_ceiling=float("inf"))
    refused(r"voicing_threshold = 0 ", voicing_threshold=0.0)
    refused(r"silence_threshold = -1", silence_threshold=-1.0)
    refused(r"octave_cost = -0.5", octave_cost=-0.5)
    refused(r"octave_jump_cost = nan", octave_jump_cost=float("nan"))
    refused(r"voiced_unvoiced_cost = -1", voiced_unvoiced_cost=-1.0)
    refused(r"frames_ld = 12 frames .*wav_ld = 4096 samples give 13", frames_ld=12)
    refused(r"frames_ld = 0 ", frames_ld=0)
    refused(rf"frames_ld = {abi.PITCH_MAX_FRAMES + 1}", frames_ld=abi.PITCH_MAX_FRAMES + 1)
    refused(r"null wav_dev", wav=None)
    refused(r"null wav_dev / f0_dev", f0=None)
    refused(r"n_frames_dev", n_frames=None)
    refused(r"wav_dev = 0x1002 is not aligned to 4", wav=0x1002)
    refused(r"lens_dev = 0x4001 is not aligned to 4", lens=0x4001)
    refused(r"n_frames_dev = 0x3002 is not aligned to 4", n_frames=0x3002)
    refused(r"n_cand_dev = 0x7002 is not aligned to 4", n_cand=0x7002)
    refused(r"selected_dev = 0x9001 is not aligned to 4", selected=0x9001)
    refused(r"f0_dev = 0x2004 is not aligned to 8", f0=0x2004)
    refused(r"acf_dev = 0x5004 is not aligned to 8", acf=0x5004)
    refused(r"cand_dev = 0x6004 is not aligned to 8", cand=0x6004)
    refused(r"intensity_dev = 0x8004 is not aligned to 8", intensity=0x8004)
    a = abi.pitch_args(**good)
    a.size -= 8
    assert lib.dtts_text2mel_fetch(None, abi.OUT_PITCH, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.PitchArgs) - 8}" in lib.dtts_last_error(None).decode()
    refused(r"null handle")                                      # a good block: only then is the handle looked at
    for p in ps.PARAM_SETS.values():                             # the four parameter sets the unit must take
        refused(r"null handle", sample_rate=p["sr"], hop=p["hop"], pitch_floor=p["floor"], pitch_ceiling=p["ceiling"], frames_ld=40)
    assert lib.dtts_text2mel_fetch(None, abi.OUT_PITCH, None, None) == -22


def test_geometry_of_the_four_parameter_sets():
    g = pr.geometry(22050, 80.0)
    assert (g["nsw"], g["half"], g["nper"], g["halfper"], g["maxlag"], g["brent"], g["n_lag"], g["first"]) == (824, 412, 275, 138, 276, 412, 413, 827)
    for p in ps.PARAM_SETS.values():
        g = pr.geometry(p["sr"], p["floor"])
        assert g == P.geometry(p["sr"], p["floor"])
        assert g["brent"] - g["maxlag"] >= 70 and g["nper"] < g["half"] and 32 <= g["nsw"] <= abi.PITCH_MAX_WINDOW      # depth 70 is never clipped
    # the frame counts the specification quotes
    g = pr.geometry(22050, 80.0)
    assert [pr.n_frames(L, g, 256) for L in (0, 826, 827, 1082, 1083)] == [0, 0, 1, 1, 2]
    assert all(pr.n_frames(T * 256, g, 256) == T - 3 == P.n_frames_of(T * 256, g["first"], 256) for T in range(4, 40))


def test_python_layer_argument_errors_surface_without_a_gpu():
    z = lambda *s: np.zeros(s, np.float32)
    for kw, match in ((dict(sample_rate=7000), "sample_rate"), (dict(sample_rate=22050.5), "sample_rate"), (dict(hop_size=0), "hop_size"),
                      (dict(f0_min=5), "f0_min"), (dict(f0_min=20), "window of 3304 samples"), (dict(f0_max=80), "f0_max"),
                      (dict(voicing_threshold=0), "voicing_threshold"), (dict(silence_threshold=float("nan")), "silence_threshold"),
                      (dict(octave_cost=-1), "octave_cost"), (dict(octave_jump_cost=-1), "octave_jump_cost"),
                      (dict(voiced_unvoiced_cost=float("inf")), "voiced_unvoiced_cost")):
        with pytest.raises(ValueError, match=match):
            P.PitchAC(**kw)
    ex = P.PitchAC()
    assert ex.geo["nsw"] == 824 and ex.frames(12 * 256) == 9
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        ex(z(100))
    with pytest.raises(ValueError, match="lens has 3 entries"):
        ex(z(2, 1000), lens=[1, 2, 3])
    with pytest.raises(ValueError, match="frames"):
        ex(z(1, 256 * (abi.PITCH_MAX_FRAMES + 10)))
    for ext in ("harvest", "dio"):
        with pytest.raises(NotImplementedError, match="pyworld"):
            P.PitchAC.from_hparams({"pitch_extractor": ext})
        with pytest.raises(NotImplementedError, match="pyworld"):
            P.get_pitch(z(4000), z(15, 80), {"pitch_extractor": ext})
    with pytest.raises(ValueError, match="pitch_extractor"):
        P.PitchAC.from_hparams({"pitch_extractor": "crepe"})
    assert P.PitchAC.from_hparams({"audio_sample_rate": 16000, "hop_size": 128}).geo["nsw"] == 598
    with pytest.raises(ValueError, match="hop_size = 200"):
        P.get_pitch(z(4000), z(15, 80), {"hop_size": 200})
    with pytest.raises(ValueError, match=r"one utterance \[L\]"):
        P.get_pitch(z(2, 4000), z(15, 80), {})
    with pytest.raises(ValueError, match="too short for one analysis frame"):
        P.get_pitch(z(826), z(3, 80), {})
    with pytest.raises(ValueError, match=r"\[B, L\] with one B"):
        P.pitch_dtw_from_wavs(z(2, 4000), None, z(3, 4000), None)
    with pytest.raises(ValueError, match="wav_gt: 500 samples are too short"):
        P.pitch_dtw_from_wavs(z(2, 4000), None, z(2, 500), None)


def test_align_to_mel():
    f0 = np.arange(1.0, 11.0)[None].repeat(2, 0)             # [2, 10]
    n = np.array([9, 4])
    a = P.align_to_mel(f0, n, 12)                            # the default: shift 2 (a whole number of hops)
    assert a.shape == (2, 12) and a[0].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0] and a[1].tolist() == [0, 0, 1, 2, 3, 4] + [0] * 6
    # with the lengths the shift is round(c_0 / hop): 2 for 12 hops and for 12 hops + 255 samples; 827 samples (one frame, centred on
    # sample 413) -> 2, and still 2 with 255 samples more (centre 540.5)
    assert P.align_to_mel(f0, [9, 9], 12, lens=[12 * 256, 12 * 256 + 255])[1].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0]
    assert P.align_to_mel(f0[:1], [1], 5, lens=[827])[0].tolist() == [0, 0, 1, 0, 0]
    assert P.align_to_mel(f0[:1], [1], 5, lens=[827 + 255])[0].tolist() == [0, 0, 1, 0, 0]
    # the reference's lpad; a negative right pad truncates
    assert P.align_to_mel(f0, n, 12, lpad=4)[0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert P.align_to_mel(f0, n, 12, lpad=8)[1].tolist() == [0] * 8 + [1, 2, 3, 4]
    import torch
    t = P.align_to_mel(torch.from_numpy(f0), torch.from_numpy(n), 3, lpad=4)
    assert torch.is_tensor(t) and not t.any()
    with pytest.raises(ValueError, match=r"\[B, nF\]"):
        P.align_to_mel(f0[0], n, 12)
    with pytest.raises(ValueError, match="n_frames has 3 entries"):
        P.align_to_mel(f0, [1, 2, 3], 12)
    with pytest.raises(ValueError, match="lpad"):
        P.align_to_mel(f0, n, 12, lpad=-1)


def test_waveforms_pair_by_the_same_rule():
    from dict_tts_amd import dtw as D
    names = ["b_gt.wav", "a.wav", "b.wav", "a_gt.wav", "a.npy", "notes.txt"]
    assert D.pair_f0_files(names, ext=".wav") == [("a.wav", "a_gt.wav"), ("b.wav", "b_gt.wav")]
    with pytest.raises(FileNotFoundError, match="c.wav has no recording c_gt.wav"):
        D.pair_f0_files(["a.wav", "a_gt.wav", "c.wav"], ext=".wav")
    with pytest.raises(FileNotFoundError, match="b_gt.wav has no prediction b.wav"):
        D.pair_f0_files(["b_gt.wav"], ext=".wav")
    with pytest.raises(FileNotFoundError, match=r"no \*_gt.wav"):
        D.pair_f0_files(["a.npy", "a_gt.npy"], ext=".wav")


def test_f0_to_coarse_hand_computed_bins():
    # 1127 ln(1 + f / 700): 50 Hz -> 77.755 (bin 1), 1100 Hz -> 1064.408 (bin 255); 100 Hz -> 150.49 -> (150.49 - 77.755) 254 / 986.653 + 1 =
    # 19.72 -> 20; 440 Hz -> 549.64 -> 122.48 -> 122; unvoiced (0) and anything below 50 Hz -> 1; above 1100 Hz -> 255
    got = P.f0_to_coarse(np.array([0.0, 40.0, 50.0, 100.0, 440.0, 1100.0, 2000.0]))
    assert got.dtype == np.int64 and got.tolist() == [1, 1, 1, 20, 122, 255, 255]
    assert P.f0_to_coarse(np.array([52.0]))[0] == 2


def test_restatement_finds_the_tones():
    """max |f0 - true| over the nine frames of each tone, measured: 90 Hz 0.011657, 123.4 Hz 0.002769, 220.5 Hz 0.001182, 440 Hz 0.000148,
    700 Hz 0.0000059 (Hz).  The bound is 3 x the measured value."""
    for f in ps.TONES:
        o = ps.ref(f"tone_{f:g}")
        err = float(np.abs(o["f0"] - f).max())
        print(f"tone {f:g} Hz: max |f0 - true| = {err:.3e} Hz over {o['nF']} frames")
        assert o["nF"] == 9 and (o["f0"] > 0).all() and err <= 3 * TONE_ERR[f], (f, err)


def test_case_list_covers_the_specification():
    names = {c["name"] for c in ps.CASES}
    assert {f"len_{L}" for L in (827, 1082, 1083, 3072, 3073, 3327)} | {"short_826", "short_0"} <= names
    assert all(c["L"] <= ps.MAX_SAMPLES and c["x"].dtype == np.float32 for c in ps.CASES)
    assert [ps.ref(f"len_{L}")["nF"] for L in (827, 1082, 1083, 3072, 3073, 3327)] == [1, 1, 2, 9, 9, 10]
    assert ps.ref("short_826")["nF"] == 0 and ps.ref("short_0")["nF"] == 0
    assert (3073 - 9 * 256 + 256 - 1) % 2 == 0                         # odd length, even hop: the frame centres fall on samples
    o = ps.ref("sine_1500")                                            # more maxima than slots: the replacement rule runs
    assert (o["maxima"] > pr.NCAND - 1).all() and (o["n_cand"] == pr.NCAND).all() and np.allclose(o["f0"], 500.0, atol=0.01)
    assert (o["cand"][:, 1:, 0].max(axis=1) > 750.0).all()             # over-ceiling candidates were there to be chosen
    o = ps.ref("glide")
    v = o["f0"] > 0
    assert v.any() and (~v).any() and (o["intensity"] == 0.0).any()    # voicing transitions, and a frame with localPeak == 0
    assert (o["n_cand"][o["intensity"] == 0.0] == 1).all()
    assert not ps.ref("noise")["f0"].any() and ps.ref("noise")["gpeak"] > 0
    o = ps.ref("zeros")
    assert o["gpeak"] == 0.0 and not o["f0"].any() and all(np.isfinite(o[k]).all() for k in ("acf", "cand", "intensity"))
    assert np.allclose(ps.ref("tone_dc")["f0"], ps.ref("tone_220.5")["f0"], atol=1e-3)       # the local mean takes the DC out
    assert {id(c["p"]) for c in ps.CASES} == {id(p) for p in ps.PARAM_SETS.values()}
    wav, lens = ps.batch_inputs()
    assert wav.shape[1] > lens.max() and len(set(lens.tolist())) >= 5 and (lens == 0).any() and (lens == 826).any()
    assert all(np.isnan(wav[b, lens[b]:]).all() and not np.isnan(wav[b, :lens[b]]).any() for b in range(len(lens)))


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c["name"])
def test_path_margin_of_the_restatement(case):
    """the smallest gap between the best and the second-best value at the decisions on the chosen path (each backpointer on it, and the final
    argmax) is far above rounding: the path the device must reproduce is not a coin toss"""
    o = ps.ref(case["name"])
    print(f"{case['name']}: {o['nF']} frames, margin {o['margin']:.3e}")
    assert o["margin"] > 1e-9


def test_sign_change_maximiser_agrees_with_the_converged_one():
    """The device finds a slot's maximiser as the sign change of the analytic derivative (pitch_ref.maximise_signchange restates it); the
    restatement's golden-section search with its derivative polish must land on the same point.  Bound: a tenth of the 1e-5 samples the
    device test allows, so that the method itself uses up little of that budget (measured: <= 6e-11)."""
    worst = 0.0
    for c in ps.CASES:
        o = ps.ref(c["name"])
        for k in range(o["nF"]):
            for i in range(1, int(o["n_cand"][k])):
                worst = max(worst, abs(pr.maximise_signchange(o["acf"][k], int(o["lag"][k, i])) - o["x"][k, i]))
    print(f"sign-change against converged maximiser: max |dlag| = {worst:.3e}")
    assert worst <= 1e-6
