"""F0 extraction on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_PITCH) and ``dict_tts_amd.pitch`` against the
float64 restatement (tests/pitch_ref.py) over the cases of tests/pitch_shapes.py.  Each stage's reference consumes the DEVICE's own
previous stage, so no rounding is carried from one stage into the next one's bound.

Bounds.
  acf: per lag |dr[l]| <= 4 nsw 2^-53 / wr[l].  A fixed-order fp64 sum of nsw products is within nsw 2^-53 ac[0] of the exact one; that
    enters once through ac[l] and once through ac[0]; the factor 2 on top is margin.  wr[brent_ixmax] is about 0.167.  intensity: 1e-12
    relative.
  candidates: the same slots from the same integer lags; |dlag| <= 1e-5 samples (the interpolant is flat at its maximum: with a curvature
    >= (2 pi / maxlag)^2 and 1e-15 of evaluation noise, function values define the maximiser to about 2e-6 samples; x 5); strength 1e-10.
  path: selected and f0 identical in every frame, and the restatement's decision margin on that input > 1e-9.
  end to end: the voiced / unvoiced pattern identical, |df0| <= 2e-5 f0^2 / sr Hz (the lag bound carried through f = sr / lag).
  a batch: every utterance bit-identical to itself run alone.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pitch_ref as pr
import pitch_shapes as ps
from dict_tts_amd import abi
from dict_tts_amd import dtw as D
from dict_tts_amd import pitch as P

pytestmark = pytest.mark.gpu
T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SENT = -7.0   # the fill of every output buffer (guard bands, and the frames a call must leave untouched)
NC = abi.PITCH_CANDIDATES
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    return abi.Context()


def _run(ctx, wav, lens, p, stages=True, frames_ld=None):
    """raw ABI call on a host array wav [B, wav_ld] float32 -> dict of numpy outputs; checks the guard bands and that the input stays"""
    B, wav_ld = wav.shape
    g = pr.geometry(p["sr"], p["floor"])
    ldf = frames_ld or max(pr.n_frames(wav_ld, g, p["hop"]), 1)
    n_lag = g["n_lag"]
    wd = T_(wav).cuda()
    ld = None if lens is None else T_(np.asarray(lens, np.int32)).cuda()
    f64 = lambda n: torch.full((n + 16,), SENT, dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")
    f0, nfr = f64(B * ldf), i32(B)
    acf, cand, ncand, inten, sel = (f64(B * ldf * n_lag), f64(B * ldf * NC * 2), i32(B * ldf), f64(B * ldf), i32(B * ldf)) if stages else (None,) * 5
    ptr = lambda t: None if t is None else t.data_ptr()
    ctx.pitch(B, _stream(), wav=wd.data_ptr(), wav_ld=wav_ld, frames_ld=ldf, f0=f0.data_ptr(), n_frames=nfr.data_ptr(), sample_rate=p["sr"], hop=p["hop"],
              pitch_floor=p["floor"], pitch_ceiling=p["ceiling"], voicing_threshold=p["voicing_threshold"], silence_threshold=p["silence_threshold"],
              octave_cost=p["octave_cost"], octave_jump_cost=p["octave_jump_cost"], voiced_unvoiced_cost=p["voiced_unvoiced_cost"], lens=ptr(ld),
              acf=ptr(acf), cand=ptr(cand), n_cand=ptr(ncand), intensity=ptr(inten), selected=ptr(sel))
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu().view(torch.int32), T_(wav).view(torch.int32))              # the input, bit for bit (NaN tails included)
    assert (f0[B * ldf:] == SENT).all() and (nfr[B:] == -7).all()
    out = {"f0": f0[:B * ldf].reshape(B, ldf).cpu().numpy(), "n_frames": nfr[:B].cpu().numpy()}
    if stages:
        assert (acf[B * ldf * n_lag:] == SENT).all() and (cand[B * ldf * NC * 2:] == SENT).all() and (ncand[B * ldf:] == -7).all()
        assert (inten[B * ldf:] == SENT).all() and (sel[B * ldf:] == -7).all()
        out.update(acf=acf[:B * ldf * n_lag].reshape(B, ldf, n_lag).cpu().numpy(), cand=cand[:B * ldf * NC * 2].reshape(B, ldf, NC, 2).cpu().numpy(),
                   n_cand=ncand[:B * ldf].reshape(B, ldf).cpu().numpy(), intensity=inten[:B * ldf].reshape(B, ldf).cpu().numpy(),
                   selected=sel[:B * ldf].reshape(B, ldf).cpu().numpy())
    return out


def _check_tail(out, b, nF):
    """behind n_frames: f0 = 0, selected = -1, the optional float outputs and n_cand untouched; before it: everything finite"""
    assert out["n_frames"][b] == nF
    assert (out["f0"][b, nF:] == 0.0).all() and np.isfinite(out["f0"][b]).all()
    if "acf" in out:
        assert (out["selected"][b, nF:] == -1).all() and (out["n_cand"][b, nF:] == -7).all()
        for k in ("acf", "cand", "intensity"):
            assert (out[k][b, nF:] == SENT).all() and np.isfinite(out[k][b, :nF]).all(), k
        assert ((out["n_cand"][b, :nF] >= 1) & (out["n_cand"][b, :nF] <= NC)).all()
        assert ((out["selected"][b, :nF] >= 0) & (out["selected"][b, :nF] < out["n_cand"][b, :nF])).all()
        for k in range(nF):                                                               # unused slots are (0, 0)
            assert not out["cand"][b, k, out["n_cand"][b, k]:].any() and not out["cand"][b, k, 0].any()


_DEV = {}


def _alone(ctx, name):
    """the case run alone at B = 1, at its own leading dimension; once"""
    if name not in _DEV:
        c = ps.BY_NAME[name]
        wav = np.zeros((1, max(c["L"], 1)), np.float32)
        wav[0, :c["L"]] = c["x"]
        out = _run(ctx, wav, [c["L"]], c["p"])
        _check_tail(out, 0, ps.ref(name)["nF"])
        _DEV[name] = out
    return _DEV[name]


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c["name"])
def test_acf_and_intensity(ctx, case):
    want, got = ps.ref(case["name"]), _alone(ctx, case["name"])
    nF, p = want["nF"], case["p"]
    g = pr.geometry(p["sr"], p["floor"])
    _, wr = pr.tables(g["nsw"])
    bound = 4.0 * g["nsw"] * 2.0 ** -53 / wr
    if nF:
        err = np.abs(got["acf"][0, :nF] - want["acf"])
        print(f"{case['name']}: max |dr| / bound = {(err / bound).max():.3f}; max |dr| = {err.max():.2e}")
        assert (got["acf"][0, :nF, 0] == 1.0).all() and (err <= bound).all()
        assert (np.abs(got["intensity"][0, :nF] - want["intensity"]) <= 1e-12 * want["intensity"]).all()


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c["name"])
def test_candidates_from_the_device_acf(ctx, case):
    got, p = _alone(ctx, case["name"]), case["p"]
    nF = int(got["n_frames"][0])
    worst_lag = worst_s = 0.0
    for k in range(nF):
        want = pr.candidates(got["acf"][0, k], p)
        n = want["n"]
        assert got["n_cand"][0, k] == n, (k, got["n_cand"][0, k], n)
        f, s = got["cand"][0, k, 1:n, 0], got["cand"][0, k, 1:n, 1]
        assert (f > 0).all()
        worst_lag = max(worst_lag, float(np.abs(p["sr"] / f - want["x"][1:n]).max(initial=0.0)))
        worst_s = max(worst_s, float(np.abs(s - want["cand"][1:n, 1]).max(initial=0.0)))
    print(f"{case['name']}: max |dlag| = {worst_lag:.2e} samples, max |dstrength| = {worst_s:.2e}")
    assert worst_lag <= 1e-5 and worst_s <= 1e-10


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c["name"])
def test_path_from_the_device_candidates(ctx, case):
    got, p = _alone(ctx, case["name"]), case["p"]
    nF = int(got["n_frames"][0])
    want = pr.path(got["cand"][0, :nF], got["n_cand"][0, :nF], got["intensity"][0, :nF], p)
    assert want["margin"] > 1e-9, want["margin"]
    assert np.array_equal(got["selected"][0, :nF], want["selected"])
    assert np.array_equal(bits(got["f0"][0, :nF]), bits(want["f0"]))


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c["name"])
def test_end_to_end_against_the_restatement(ctx, case):
    want, got = ps.ref(case["name"]), _alone(ctx, case["name"])
    nF = want["nF"]
    assert got["n_frames"][0] == nF
    f0 = got["f0"][0, :nF]
    assert np.array_equal(f0 > 0, want["f0"] > 0) and np.array_equal(got["selected"][0, :nF], want["selected"])
    v = want["f0"] > 0
    if v.any():
        err = np.abs(f0[v] - want["f0"][v]) / (2e-5 * want["f0"][v] ** 2 / case["p"]["sr"])
        print(f"{case['name']}: max |df0| / bound = {err.max():.2e}")
        assert (err <= 1.0).all()


def _same_as_alone(ctx, out, b, name):
    one = _alone(ctx, name)
    nF = int(one["n_frames"][0])
    _check_tail(out, b, nF)
    for k in ("f0", "acf", "cand", "intensity"):
        assert np.array_equal(bits(out[k][b, :nF]), bits(one[k][0, :nF])), (name, k)
    for k in ("n_cand", "selected"):
        assert np.array_equal(out[k][b, :nF], one[k][0, :nF]), (name, k)


def test_batch_with_poisoned_padding_equals_each_utterance_alone(ctx):
    wav, lens = ps.batch_inputs()
    out = _run(ctx, wav, lens, ps.P0)
    for b, name in enumerate(ps.BATCH):
        _same_as_alone(ctx, out, b, name)
    # another order, other neighbours, a wider output; and without the stage outputs (the workspace holds them)
    perm = [3, 0, 3, 6]
    o2 = _run(ctx, wav[perm], lens[perm], ps.P0, frames_ld=17)
    for i, b in enumerate(perm):
        _same_as_alone(ctx, o2, i, ps.BATCH[b])
    o3 = _run(ctx, wav, lens, ps.P0, stages=False)
    assert np.array_equal(bits(o3["f0"]), bits(out["f0"])) and np.array_equal(o3["n_frames"], out["n_frames"])
    # no lens: every row runs over the whole leading dimension
    full = np.stack([ps.BY_NAME["tone_440"]["x"], ps.BY_NAME["noise"]["x"]])
    o4 = _run(ctx, full, None, ps.P0)
    _same_as_alone(ctx, o4, 0, "tone_440")
    _same_as_alone(ctx, o4, 1, "noise")
    # a length above the leading dimension, or negative: no frame, a zero row; the neighbour is untouched by it
    o5 = _run(ctx, wav[:3], np.array([ps.BATCH_LD + 1, lens[1], -5], np.int32), ps.P0)
    _check_tail(o5, 0, 0)
    _check_tail(o5, 2, 0)
    _same_as_alone(ctx, o5, 1, ps.BATCH[1])


def test_other_parameter_sets_in_a_batch(ctx):
    for name in ("p_22050_128", "p_16000_128", "p_22050_50_1100"):
        c = ps.BY_NAME[name]
        wav = np.full((3, c["L"] + 37), np.nan, np.float32)
        lens = np.array([c["L"], c["L"] - 300, c["L"]], np.int32)
        for b in range(3):
            wav[b, :lens[b]] = c["x"][:lens[b]]
        out = _run(ctx, wav, lens, c["p"])
        _same_as_alone(ctx, out, 0, name)
        _same_as_alone(ctx, out, 2, name)
        _check_tail(out, 1, pr.n_frames(int(lens[1]), pr.geometry(c["p"]["sr"], c["p"]["floor"]), c["p"]["hop"]))


def test_memory_safety_pitch(ctx):
    """debug_redzone = 1: the workspace sits between red zones and starts out as 0xFF; no launch damages a zone, no stale word reaches an
    output, and the results are the plain context's, bit for bit"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg = abi.Context(cfg)
    wav, lens = ps.batch_inputs()
    for stages in (True, False):
        got = _run(dbg, wav, lens, ps.P0, stages=stages)
        assert dbg.debug_check(_stream()) == 0, dbg.last_error()
        want = _run(ctx, wav, lens, ps.P0, stages=stages)
        for k in got:
            assert np.array_equal(got[k].view(np.int64 if got[k].dtype == np.float64 else np.int32), want[k].view(np.int64 if want[k].dtype == np.float64 else np.int32)), k
    c = ps.BY_NAME["p_22050_50_1100"]
    got = _run(dbg, c["x"][None], None, c["p"])
    assert dbg.debug_check(_stream()) == 0, dbg.last_error()
    assert np.array_equal(bits(got["f0"]), bits(_alone(ctx, c["name"])["f0"]))
    dbg.close()


def test_invalid_arguments_are_refused_and_write_nothing(ctx):
    c = ps.BY_NAME["tone_440"]
    wd = T_(c["x"]).cuda()
    f0 = torch.zeros(16, dtype=torch.float64, device="cuda")
    nfr = torch.zeros(4, dtype=torch.int32, device="cuda")
    good = dict(wav=wd.data_ptr(), wav_ld=c["L"], frames_ld=9, f0=f0.data_ptr(), n_frames=nfr.data_ptr())

    def refused(match, B=1, **kw):
        with pytest.raises(abi.DttsError, match=match):
            ctx.pitch(B, _stream(), **{**good, **kw})

    refused(r"\(-22\).*B = 0", B=0)
    refused(r"\(-22\).*frames_ld = 8 frames", frames_ld=8)
    refused(r"\(-22\).*pitch_floor = 20 gives a window", pitch_floor=20.0)
    refused(r"\(-22\).*f0_dev = 0x[0-9a-f]+ is not aligned to 8", f0=f0.data_ptr() + 4)
    a = abi.pitch_args(1, **good)
    a.size += 8
    assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_PITCH, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.PitchArgs) + 8}" in ctx.last_error()
    torch.cuda.synchronize()
    assert not f0.any() and not nfr.any()
    ctx.pitch(1, _stream(), **good)
    torch.cuda.synchronize()
    assert nfr[0].item() == 9 and np.array_equal(bits(f0[:9].cpu().numpy()), bits(_alone(ctx, "tone_440")["f0"][0, :9]))


def test_pitch_dtw_tool_reads_a_directory_of_waveforms(tmp_path, monkeypatch, capsys):
    """tools/pitch_dtw.py --wavs DIR: NAME.wav against NAME_gt.wav by name, the four lines scripts/pitch_dtw.py prints"""
    import importlib.util
    import os
    import sys
    from scipy.io import wavfile
    pcm = lambda x: np.round(np.asarray(x, np.float64) * 32767.0).astype(np.int16)
    pairs = {"zz_utt": (pcm(ps.BY_NAME["glide"]["x"]), pcm(ps.BY_NAME["tone_220.5"]["x"])), "a_utt": (pcm(ps.BY_NAME["tone_123.4"]["x"]), pcm(ps.tone(130.0, 3400)))}
    for name, (pred, gt) in pairs.items():                             # written so that directory order is not name order
        wavfile.write(tmp_path / f"{name}_gt.wav", 22050, gt)
        wavfile.write(tmp_path / f"{name}.wav", 22050, pred)
    spec = importlib.util.spec_from_file_location("pitch_dtw_tool_wavs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pitch_dtw.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["pitch_dtw.py", "--wavs", str(tmp_path)])
    tool.main()
    got = [float(line) for line in capsys.readouterr().out.split()]
    order = sorted(pairs)
    f32 = lambda a: a.astype(np.float32) / 32768.0
    pred, gt = np.zeros((2, ps.MAX_SAMPLES), np.float32), np.zeros((2, 3400), np.float32)
    for b, n in enumerate(order):
        pred[b, :len(pairs[n][0])], gt[b, :len(pairs[n][1])] = f32(pairs[n][0]), f32(pairs[n][1])
    want = P.pitch_dtw_from_wavs(pred, [len(pairs[n][0]) for n in order], gt, [len(pairs[n][1]) for n in order])
    assert got == [want[k] for k in ("dtw", "std", "skew", "kurtosis")] and np.isfinite(got).all()


def test_python_layer_and_pitch_dtw_from_wavs(ctx):
    wav, lens = ps.batch_inputs()
    ex = P.PitchAC(ctx)
    out = ex(np.nan_to_num(wav), lens, stages=True)
    nF = ex.frames(wav.shape[1])
    assert out["f0"].shape == (len(lens), nF) and out["f0"].dtype == torch.float64 and out["acf"].shape == (len(lens), nF, 413)
    assert out["cand"].shape == (len(lens), nF, NC, 2) and out["selected"].dtype == torch.int32 and out["f0"].is_cuda
    for b, name in enumerate(ps.BATCH):
        one = _alone(ctx, name)
        n = int(one["n_frames"][0])
        assert int(out["n_frames"][b]) == n and np.array_equal(bits(out["f0"][b, :n].cpu().numpy()), bits(one["f0"][0, :n]))
        assert torch.isnan(out["acf"][b, n:]).all() and (out["selected"][b, n:] == -1).all() and not out["f0"][b, n:].any()
    # get_pitch: the reference's shift of 4 frames at hop 256, cut to the mel's length
    c = ps.BY_NAME["tone_220.5"]
    f0, coarse = P.get_pitch(c["x"], np.zeros((12, 80), np.float32), {}, ctx=ctx)
    one = _alone(ctx, c["name"])["f0"][0, :9]
    assert f0.shape == (12,) and not f0[:4].any() and np.array_equal(bits(f0[4:]), bits(one[:8])) and np.array_equal(coarse, P.f0_to_coarse(f0))
    assert P.PitchAC(ctx)(c["x"][None, :500])["f0"].shape == (1, 0)                     # too short for a frame: an empty track, n_frames = 0
    # three pairs: the tracks go from the extractor to the DTW on the device; the same tracks downloaded give the same figures, bit for bit
    pred = np.zeros((3, ps.MAX_SAMPLES), np.float32)
    gt = np.zeros((3, 3400), np.float32)
    pl, gl = np.array([ps.MAX_SAMPLES, 3072, 3073], np.int32), np.array([3072, 3400, 2000], np.int32)
    pred[0], pred[1, :3072], pred[2, :3073] = ps.BY_NAME["glide"]["x"], ps.BY_NAME["tone_123.4"]["x"], ps.BY_NAME["len_3073"]["x"]
    gt[0, :3072], gt[1], gt[2, :2000] = ps.BY_NAME["tone_220.5"]["x"], ps.tone(130.0, 3400).astype(np.float32), ps.BY_NAME["glide"]["x"][:2000]
    got = P.pitch_dtw_from_wavs(pred, pl, gt, gl, ctx=ctx)
    tp, tg = ex(pred, pl), ex(gt, gl)
    tracks = lambda t: [t["f0"][b, :int(t["n_frames"][b])].cpu().numpy() for b in range(3)]
    want = D.pitch_dtw(tracks(tp), tracks(tg), ctx=ctx)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.isfinite(got["dtw"]) and got["dtw"] > 0
