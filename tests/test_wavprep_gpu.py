"""Waveform conditioning on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_RESAMPLE / DTTS_OUT_LOUDNESS) and
``dict_tts_amd.wavprep`` against the float64 restatements (tests/wavprep_ref.py) over the cases of tests/wavprep_shapes.py.  Each stage of
the loudness unit is judged from the DEVICE's own previous stage, so no rounding is carried from one stage into the next one's bound.

Bounds.
  resampler, out64: |d acc| <= (taps + 2) 2^-53 sum |w x|.  Device and restatement form the same weights w from the same operations (table
    entry times ratio, eta times delta, one addition; nothing contracted) and meet the same samples in the same order; they differ in how
    a tap is added (one fma on the device; a rounded product and a rounded sum in the restatement).  Every partial sum is bounded by
    sum |w x|, so each of the `taps` additions contributes at most 2^-53 sum |w x| on either side and the products as much once more
    in total; + 2 is margin.  out == (float)out64 bit for bit; out_lens exact; zeros behind.
  loudness, z: with u = 2^-53, m = the largest |x|, |y_shelf|, |y| of the utterance and cs = 1 + sum |b| + sum |a| of the shelf (every
    state and every term of a step is at most cs m), a step of the recurrence rounds each state three times: device and restatement
    part by at most 6 u cs m per step, and the device once more per segment by 5 u (||M^S|| + 1) cs m where it carries the state through
    M^S (four products and sums, and e_k).  Each such error is carried on by powers of M, so all of them together stay below R times
    the largest, R = sum_m ||M^m||_inf (a convergent series: 4.4e3 at 11025 Hz, 8.1e4 at 48 kHz).  With the output's own rounding,
    |dy| <= delta = u cs m (R (6 + 5 (||M^S|| + 1)) + 2).  A block of n samples then differs by at most 2 delta sum |y| + n delta^2,
    and by 2 n u sum y^2 for the two orders of its sum (sample order in the restatement; sample order inside a segment, then segment
    order, on the device).  The tolerance is that bound over 0.4 rate, or 1e-9 of the utterance's mean square where the bound is looser.
  LUFS and gain: the restatement's gating of the device's own z, 1e-12 LU and 1e-13 relative (two log10 / one pow of libm against the
    device's, a few ulp each, on values of order 10 .. 100 LU).  The normalised samples: numpy float32 arithmetic on the device's own gain,
    bit for bit.  Status bits, n_blocks exact.
  a batch: every utterance bit-identical to itself run alone, at another leading dimension.
"""
import numpy as np
import pytest
import torch

import melspec_ref as mr
import wavprep_ref as wr
import wavprep_shapes as ws
from dict_tts_amd import abi
from dict_tts_amd import wavprep as W

pytestmark = pytest.mark.gpu
T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SENT = -7.0
U = 2.0 ** -53
bits64 = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
bits32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context()
    c.load_resample_filter(*ws.table("kaiser_best"))
    return c


@pytest.fixture(scope="module")
def ctx_fast():
    c = abi.Context()
    c.load_resample_filter(*ws.table("kaiser_fast"))
    return c


# ---------------------------------------------------------------- resampler
def _resample(ctx, wav, lens, sr_in, sr_out, out_ld=None):
    """raw ABI call on a host array wav [B, wav_ld] -> dict of numpy outputs; checks the guard bands and that the input stays"""
    B, wav_ld = wav.shape
    ld = out_ld or max(W.resampled_len(wav_ld, sr_in, sr_out)[1], 1)
    wd = T_(wav).cuda()
    lensd = None if lens is None else T_(np.asarray(lens, np.int32)).cuda()
    out = torch.full((B * ld + 16,), SENT, dtype=torch.float32, device="cuda")
    out64 = torch.full((B * ld + 16,), SENT, dtype=torch.float64, device="cuda")
    ol = torch.full((B + 16,), -7, dtype=torch.int32, device="cuda")
    ctx.resample(B, _stream(), wav=wd.data_ptr(), wav_ld=wav_ld, out=out.data_ptr(), out_ld=ld, out_lens=ol.data_ptr(), sr_in=sr_in, sr_out=sr_out,
                 lens=None if lensd is None else lensd.data_ptr(), out64=out64.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu().view(torch.int32), T_(wav).view(torch.int32))              # the input, bit for bit (NaN tails included)
    assert (out[B * ld:] == SENT).all() and (out64[B * ld:] == SENT).all() and (ol[B:] == -7).all()
    return dict(out=out[:B * ld].reshape(B, ld).cpu().numpy(), out64=out64[:B * ld].reshape(B, ld).cpu().numpy(), out_lens=ol[:B].cpu().numpy())


_RS_DEV = {}


def _rs_alone(ctx, name):
    if name not in _RS_DEV:
        c = ws.RS_BY_NAME[name]
        _RS_DEV[name] = _resample(ctx, c["x"][None], None, c["sr_in"], c["sr_out"])
    return _RS_DEV[name]


def _rs_check(got, b, ref, what):
    n_out, ol = ref["n_out"], ref["out_len"]
    assert got["out_lens"][b] == ol, (what, got["out_lens"][b], ol)
    o64, o32 = got["out64"][b], got["out"][b]
    assert np.isfinite(o64).all() and np.isfinite(o32).all(), what
    assert not o64[n_out:].any() and not o32[n_out:].any(), what                               # fix_length's zero, and everything behind
    assert np.array_equal(bits32(o32), bits32(o64.astype(np.float32))), what                   # one rounding
    tol = (ref["taps"] + 2) * U * ref["absum"]
    err = np.abs(o64[:n_out] - ref["y64"])
    worst = float((err / np.maximum(tol, 1e-300)).max()) if n_out else 0.0
    print(f"{what}: {n_out} outputs, up to {int(ref['taps'].max()) if n_out else 0} taps, worst error {worst:.3f} of its bound")
    assert (err <= tol).all(), (what, worst)


@pytest.mark.parametrize("case", [c for c in ws.RS_CASES if c["filter"] == "kaiser_best"], ids=lambda c: c["name"])
def test_resampler_against_the_restatement(ctx, case):
    _rs_check(_rs_alone(ctx, case["name"]), 0, ws.rs_ref(case["name"]), case["name"])


def test_resampler_kaiser_fast_and_refinalising(ctx_fast):
    c = ws.RS_BY_NAME["fast_48000_22050"]
    got = _resample(ctx_fast, c["x"][None], None, c["sr_in"], c["sr_out"])
    _rs_check(got, 0, ws.rs_ref(c["name"]), c["name"])
    ctx_fast.load_resample_filter(*ws.table("kaiser_best"))                                   # every finalize that names the part rebuilds the plan
    c = ws.RS_BY_NAME["len_321"]
    _rs_check(_resample(ctx_fast, c["x"][None], None, c["sr_in"], c["sr_out"]), 0, ws.rs_ref(c["name"]), "len_321 after refinalising")
    ctx_fast.load_resample_filter(*ws.table("kaiser_fast"))


def test_resampler_batch_is_the_utterances_alone(ctx):
    """mixed lengths at one ratio, NaN behind every utterance, other leading dimensions: bit-identical rows, zeros behind out_lens; an
    utterance of length 0 or above wav_ld, or too long for out_ld, gets out_lens = 0 and a zero row"""
    wav, lens = ws.rs_batch_inputs(ws.RS_BATCH)
    wav = np.concatenate([wav, wav[:2]])
    lens = np.concatenate([lens, [0, wav.shape[1] + 1]]).astype(np.int32)
    got = _resample(ctx, wav, lens, ws.A, ws.Bq, out_ld=W.resampled_len(wav.shape[1], ws.A, ws.Bq)[1] + 7)
    for b, name in enumerate(ws.RS_BATCH):
        ref, alone = ws.rs_ref(name), _rs_alone(ctx, name)
        ol = ref["out_len"]
        assert got["out_lens"][b] == ol
        assert np.array_equal(bits64(got["out64"][b, :ol]), bits64(alone["out64"][0, :ol])), name
        assert np.array_equal(bits32(got["out"][b, :ol]), bits32(alone["out"][0, :ol])), name
        assert not got["out"][b, ol:].any() and not got["out64"][b, ol:].any(), name
    for b in (len(ws.RS_BATCH), len(ws.RS_BATCH) + 1):
        assert got["out_lens"][b] == 0 and not got["out"][b].any() and not got["out64"][b].any()
    c = ws.RS_BY_NAME["len_321"]                                                               # 148 samples do not fit 147
    short = _resample(ctx, c["x"][None], None, ws.A, ws.Bq, out_ld=147)
    assert short["out_lens"][0] == 0 and not short["out"].any() and not short["out64"].any()


def test_resampler_python_layer(ctx):
    c = ws.RS_BY_NAME["outputs_773"]
    rs = W.Resampler(c["sr_in"], c["sr_out"], ctx=ctx)
    out, ol = rs(c["x"][None])
    alone = _rs_alone(ctx, c["name"])
    assert out.is_cuda and out.dtype == torch.float32 and ol.cpu().tolist() == [ws.rs_ref(c["name"])["out_len"]]
    assert np.array_equal(bits32(out.cpu().numpy()), bits32(alone["out"]))
    out, ol, acc = rs(c["x"][None], acc64=True)
    assert np.array_equal(bits64(acc.cpu().numpy()), bits64(alone["out64"]))
    # two units with different filters on one context: each loads its own before its call, neither computes with the other's table
    c_fast = ws.RS_BY_NAME["fast_48000_22050"]
    fast = W.Resampler(48000, 22050, filter="kaiser_fast", ctx=ctx)
    of, _, accf = fast(c_fast["x"][None], acc64=True)
    ref = ws.rs_ref(c_fast["name"])
    assert np.abs(accf.cpu().numpy()[0, :ref["n_out"]] - ref["y64"]).max() <= ((ref["taps"] + 2) * U * ref["absum"]).max()
    out, _ = rs(c["x"][None])                                                                  # (leaves kaiser_best in the shared context)
    assert np.array_equal(bits32(out.cpu().numpy()), bits32(alone["out"]))
    own = W.Resampler(16000, 22050)                                                            # a context of its own, made on the first call
    c = ws.RS_BY_NAME["noise_16000_22050"]
    o2, _ = own(c["x"][None])
    assert np.array_equal(bits32(o2.cpu().numpy()), bits32(_rs_alone(ctx, c["name"])["out"]))
    bare = abi.Context()                                                                       # no filter finalised: DTTS_E_NOENT, nothing written
    with pytest.raises(abi.DttsError, match=r"\(-2\).*no filter"):
        _resample(bare, c["x"][None], None, 16000, 22050)
    with pytest.raises(abi.DttsError, match=r"\(-2\).*missing weight resample.filter"):
        bare.finalize(abi.PART_RESAMPLE)
    bare.close()


# ---------------------------------------------------------------- loudness
def _loudness(ctx, wav, lens, rate, mode=1, target=-22.0, blocks_ld=None):
    B, wav_ld = wav.shape
    nb = blocks_ld or max(W.n_blocks_of(wav_ld, rate), 1)
    wd = T_(wav).cuda()
    lensd = None if lens is None else T_(np.asarray(lens, np.int32)).cuda()
    f64 = lambda n: torch.full((n + 16,), SENT, dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")
    lufs, gain, z, st, nbl = f64(B), f64(B), f64(B * nb), i32(B), i32(B)
    out = torch.full((B * wav_ld + 16,), SENT, dtype=torch.float32, device="cuda")
    ctx.loudness(B, _stream(), wav=wd.data_ptr(), wav_ld=wav_ld, blocks_ld=nb, sample_rate=rate, lufs=lufs.data_ptr(), gain=gain.data_ptr(),
                 status=st.data_ptr(), mode=mode, target_lufs=target, lens=None if lensd is None else lensd.data_ptr(),
                 out=out.data_ptr() if mode else None, z=z.data_ptr(), n_blocks=nbl.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu().view(torch.int32), T_(wav).view(torch.int32))
    assert (lufs[B:] == SENT).all() and (gain[B:] == SENT).all() and (z[B * nb:] == SENT).all() and (st[B:] == -7).all() and (nbl[B:] == -7).all()
    assert (out[B * wav_ld:] == SENT).all() and (mode == 1 or (out == SENT).all())
    return dict(lufs=lufs[:B].cpu().numpy(), gain=gain[:B].cpu().numpy(), status=st[:B].cpu().numpy(), n_blocks=nbl[:B].cpu().numpy(),
                z=z[:B * nb].reshape(B, nb).cpu().numpy(), out=out[:B * wav_ld].reshape(B, wav_ld).cpu().numpy())


_LD_DEV = {}
PAD = 5


def _ld_alone(ctx, name):
    """the case alone, B = 1, NaN behind its length"""
    if name not in _LD_DEV:
        c = ws.LD_BY_NAME[name]
        wav = np.full((1, c["L"] + PAD), np.nan, np.float32)
        wav[0, :c["L"]] = c["x"]
        _LD_DEV[name] = _loudness(ctx, wav, [c["L"]], c["rate"])
    return _LD_DEV[name]


_TOL = {}


def _z_tolerance(name):
    """the bound of the module docstring for every block of the case: f64 [n_blocks]"""
    if name in _TOL:
        return _TOL[name]
    c, r = ws.LD_BY_NAME[name], ws.ld_ref(name)
    rate, L, y = c["rate"], c["L"], r["y"]
    (bs, as_), _ = W.k_weighting(rate)
    cs = 1.0 + np.abs(bs).sum() + np.abs(as_[1:]).sum()
    M = wr.state_matrix(rate)
    ms_norm = float(np.abs(np.linalg.matrix_power(M, abi.LOUD_SEGMENT)).sum(axis=1).max())
    delta = U * cs * r["peak"] * (wr.rounding_gain(rate) * (6 + 5 * (ms_norm + 1)) + 2)
    mean_sq = float((y * y).sum()) / L
    tol = np.zeros(r["n_blocks"])
    for j, (lo, hi) in enumerate(W.block_bounds(rate, r["n_blocks"])):
        seg = y[lo:min(hi, L)]
        n = len(seg)
        tol[j] = (2 * delta * np.abs(seg).sum() + n * delta * delta + 2 * n * U * (seg * seg).sum()) / (0.4 * rate)
    _TOL[name] = np.minimum(tol, 1e-9 * mean_sq)
    return _TOL[name]


def _ld_check(got, b, c, what):
    ref, x, L = ws.ld_ref(c["name"]), c["x"], c["L"]
    nb = ref["n_blocks"]
    assert got["n_blocks"][b] == nb, (what, got["n_blocks"][b], nb)
    z = got["z"][b]
    assert (z[nb:] == SENT).all() and np.isfinite(z[:nb]).all() and (z[:nb] >= 0).all(), what
    tol = _z_tolerance(c["name"])
    err = np.abs(z[:nb] - ref["z"])
    worst = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    print(f"{what}: {nb} blocks, worst z error {worst:.3e} of its bound (the bound: up to {float((tol / max(ref['z'].max(), 1e-300)).max()) if nb else 0:.1e} of the largest z)")
    assert (err <= tol).all(), (what, worst)
    assert np.array_equal(z[:nb] == 0.0, ref["z"] == 0.0), what
    g = wr.gate(z[:nb], -22.0)                                                                 # the restatement's gating of the device's own z
    st = int(got["status"][b])
    assert st & 3 == g["status"], (what, st, g["status"])
    if g["status"] == 1:
        assert np.isnan(got["lufs"][b]) and got["gain"][b] == 1.0
    elif g["status"] == 2:
        assert got["lufs"][b] == -np.inf and got["gain"][b] == 1.0
    else:
        assert g["margin"] >= 1e-6, (what, g["margin"])
        assert abs(got["lufs"][b] - g["lufs"]) <= 1e-12 and abs(got["gain"][b] / g["gain"] - 1.0) <= 1e-13, (what, got["lufs"][b], g["lufs"])
    want, st_want = wr.apply_gain(x, got["gain"][b], g["status"])                              # numpy float32 arithmetic on the device's own gain
    assert st == st_want == ref["status"], (what, st, st_want, ref["status"])
    assert np.array_equal(bits32(got["out"][b, :L]), bits32(want)), what
    assert not got["out"][b, L:].any(), what                                                   # zeros behind L, where the input holds NaN
    if st & 3:
        assert np.array_equal(bits32(got["out"][b, :L]), bits32(x)), what                      # the refused kinds: copied unchanged
    if st & 4:
        assert np.abs(got["out"][b, :L]).max() == 1.0, what


@pytest.mark.parametrize("case", ws.LD_CASES, ids=lambda c: c["name"])
def test_loudness_against_the_restatement(ctx, case):
    _ld_check(_ld_alone(ctx, case["name"]), 0, case, case["name"])


def test_loudness_batch_is_the_utterances_alone(ctx):
    wav, lens = ws.ld_batch_inputs(ws.LD_BATCH)
    got = _loudness(ctx, wav, lens, 16000)
    assert len(ws.LD_BATCH) >= 8
    for b, name in enumerate(ws.LD_BATCH):
        alone, L, nb = _ld_alone(ctx, name), ws.LD_BY_NAME[name]["L"], ws.ld_ref(name)["n_blocks"]
        for k in ("lufs", "gain"):
            assert np.array_equal(bits64(got[k][b]), bits64(alone[k][0])), (name, k)
        assert got["status"][b] == alone["status"][0] and got["n_blocks"][b] == alone["n_blocks"][0] == nb
        assert np.array_equal(bits64(got["z"][b, :nb]), bits64(alone["z"][0, :nb])) and (got["z"][b, nb:] == SENT).all(), name
        assert np.array_equal(bits32(got["out"][b, :L]), bits32(alone["out"][0, :L])) and not got["out"][b, L:].any(), name
    # measuring alone (mode 0, no stage outputs wanted back) gives the same figures and writes no samples
    m = _loudness(ctx, wav, lens, 16000, mode=0)
    assert np.array_equal(bits64(m["lufs"]), bits64(got["lufs"])) and np.array_equal(m["status"], got["status"] & 3)


def test_loudness_python_layer(ctx):
    c = ws.LD_BY_NAME["rate_22050"]
    ln = W.Loudness(22050, ctx=ctx)
    alone = _ld_alone(ctx, c["name"])
    lufs = ln.measure(c["x"][None])
    assert lufs.is_cuda and np.array_equal(bits64(lufs.cpu().numpy()), bits64(alone["lufs"]))
    wavs, lufs, gain, st = ln.normalize(c["x"][None])
    assert np.array_equal(bits32(wavs.cpu().numpy()[0]), bits32(alone["out"][0, :c["L"]])) and st.cpu().tolist() == [0]
    again = ln.measure(wavs)                                                                   # the normalised utterance sits on the target
    assert abs(float(again[0]) - -22.0) < 1e-3
    ln16 = W.Loudness(16000, ctx=ctx)
    with pytest.raises(ValueError, match="utterance 1: audio must have length greater than the block size"):
        ln16.normalize(np.stack([ws.LD_BY_NAME["one_block"]["x"], np.pad(ws.LD_BY_NAME["one_block_less"]["x"], (0, 1))]), lens=[6400, 6399])
    with pytest.warns(UserWarning, match="utterance 0: no block passes"):
        w, l, g, s = ln16.normalize(ws.LD_BY_NAME["all_zero"]["x"][None])
    assert s.cpu().tolist() == [abi.LOUD_SILENT] and float(l[0]) == -np.inf


# ---------------------------------------------------------------- integration
def test_wav2spec_resamples_and_normalises(ctx, tmp_path, monkeypatch):
    """a 48 kHz 16-bit file -> wav2spec(fn, resample=True): the mel of the restated resampling, in the melspec suite's own terms (entries
    >= 1e-3 of the frame's maximum within 4e-4 in log10: tests/test_melspec_gpu.py); with loud_norm the mel of the restated normalisation"""
    from scipy.io import wavfile
    from dict_tts_amd import hparams as hparams_mod
    from dict_tts_amd import melspec, vocoder
    rate = 48000
    t = np.arange(30000) / rate
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.05 * np.random.RandomState(5).randn(len(t))
    pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    fn = str(tmp_path / "u48k.wav")
    wavfile.write(fn, rate, pcm)
    with pytest.raises(ValueError, match=r"48000.*22050"):
        vocoder.HifiGAN.wav2spec(fn)
    ref = wr.resample(pcm.astype(np.float32) / 32768.0, rate, 22050, *ws.table("kaiser_best"))
    fb = melspec.mel_filterbank(22050, 1024, 80, 80, 7600).astype(np.float32)
    w, m = vocoder.HifiGAN.wav2spec(fn, resample=True)
    n = ref["out_len"]
    assert w.dtype == np.float32 and m.shape == (1 + n // 256, 80) and len(w) == m.shape[0] * 256 and not w[n:].any()
    assert np.abs(w[:n] - ref["out"]).max() <= np.spacing(np.float32(np.abs(ref["out"]).max()))
    lin64 = mr.mel_lin(ref["out"], 1024, 256, 1024, fb)
    assert mr.log_error(m, lin64, mr.log_selection(lin64)) <= 4e-4
    monkeypatch.setitem(hparams_mod.hparams, "loud_norm", True)
    w2, m2 = vocoder.HifiGAN.wav2spec(fn, resample=True)
    lr = wr.loudness(ref["out"], 22050, -22.0)
    assert lr["status"] == 0 and abs(lr["gain"] - 1.0) > 0.05
    assert np.abs(w2[:n] - lr["out"]).max() <= 2 * np.spacing(np.float32(np.abs(lr["out"]).max())) and not w2[n:].any()
    lin64 = mr.mel_lin(lr["out"], 1024, 256, 1024, fb)
    assert mr.log_error(m2, lin64, mr.log_selection(lin64)) <= 4e-4


def test_chain_on_one_stream_without_a_host_copy(ctx):
    """Resampler -> Loudness -> MelSpectrogram -> PitchAC on one context and one stream: every stage consumes the device tensor of the one
    before; the results are those of the stages run one by one from host copies"""
    from dict_tts_amd import melspec
    from dict_tts_amd import pitch as P
    rate = 48000
    t = np.arange(40000) / rate
    x = (0.2 * np.sign(np.sin(2 * np.pi * 150.0 * t)) * np.hanning(len(t))).astype(np.float32)
    rs, ln = W.Resampler(rate, 22050, ctx=ctx), W.Loudness(22050, ctx=ctx)
    ms, pa = melspec.MelSpectrogram(ctx=ctx), P.PitchAC(ctx)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = T_(x)[None].cuda()
        y, yl = rs(xd)
        wn, lufs, gain, st = ln.normalize(y, yl, check=False)
        mel, frames = ms(wn, yl)
        f0 = pa(wn, yl)
    s.synchronize()
    assert y.is_cuda and wn.is_cuda and mel.is_cuda and f0["f0"].is_cuda
    n = int(yl[0])
    assert n == W.resampled_len(len(x), rate, 22050)[1] and int(st[0]) == 0 and abs(float(lufs[0]) - -22.0) > 1.0
    wn_h = wn.cpu().numpy()
    mel2, _ = ms(wn_h)
    f02 = pa(wn_h)
    assert torch.equal(mel2, mel) and torch.equal(f02["f0"], f0["f0"])
    v = f0["f0"][0].cpu().numpy()
    v = v[v > 0]
    assert len(v) > 20 and abs(np.median(v) - 150.0) < 1.0                                      # the tone survives both conditioning steps


def test_memory_safety_wavprep(ctx):
    """debug_redzone = 1: the workspaces and the tables sit between red zones and start out as 0xFF; no launch damages a zone, no stale
    word reaches an output, and the results are the plain context's, bit for bit"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg = abi.Context(cfg)
    dbg.load_resample_filter(*ws.table("kaiser_best"))
    wav, lens = ws.rs_batch_inputs(ws.RS_BATCH[:8])
    got = _resample(dbg, wav, lens, ws.A, ws.Bq)
    assert dbg.debug_check(_stream()) == 0, dbg.last_error()
    want = _resample(ctx, wav, lens, ws.A, ws.Bq)
    assert all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in got)
    wav, lens = ws.ld_batch_inputs(ws.LD_BATCH)
    got = _loudness(dbg, wav, lens, 16000)
    assert dbg.debug_check(_stream()) == 0, dbg.last_error()
    want = _loudness(ctx, wav, lens, 16000)
    assert all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in got)
    dbg.close()
