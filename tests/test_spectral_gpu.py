"""STFT -> magnitude edit -> inverse STFT on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_SPECTRAL) against the
float64 restatement of the reference's denoise (tests/istft_ref.py).

The accuracy bound follows tests/test_melspec_gpu.py: the unit is the error of the reference's OWN arithmetic on the same input,
e_ref = max |y32 - y64| / max(peak |y64|, 1e-6) with y32 the float32 torch.stft -> edit -> torch.istft path on the CPU, and the kernels
may take FACTOR = 4 of it (a direct fp32 sum of n_fft products against an FFT's log2(n_fft) stages: 1.5 - 1.8 x, times 2 for the order).
Every ratio is printed before it is asserted.

Measured on the MI355X (LABNOTES.md "Spectral denoise"): the float32 path's error is 1.2e-7 - 4.2e-7 of the peak; ratios of the filter
0.38 - 0.70 (the largest: the tone at v = median, 2.47e-7 against 3.52e-7), of v = 0 against the input 0.25 - 0.50, of the spectrum per
frame 0.40 - 0.58, of the inverse alone on an inconsistent spectrum 0.41 - 0.48, of the edge batch 0.44 - 0.50, of a one-tile utterance in a batch of 4098
(one workgroup per tile in both launchers) 0.56.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import istft_ref as ir
import melspec_ref as mr
from dict_tts_amd import abi, infer, spectral, synth, vocoder

pytestmark = pytest.mark.gpu

CONFIGS = {   # (n_fft, hop, win) of tests/test_melspec_gpu.py::CONFIGS, with the sample rate the signals are drawn at
    "default": dict(audio_sample_rate=22050, fft_size=1024, hop_size=256, win_size=1024),
    "short_window": dict(audio_sample_rate=22050, fft_size=512, hop_size=128, win_size=400),
    "hop200_nyquist": dict(audio_sample_rate=16000, fft_size=1024, hop_size=200, win_size=800),
    "n2048_hop300": dict(audio_sample_rate=22050, fft_size=2048, hop_size=300, win_size=1200),
}
FACTOR = 4.0
SENTINEL = 777.0
EDGE_LENS = (0, 100, 256 * 9, 256 * 40 + 77, 256 * 300)
EDGE_V = 0.1
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _sp(name):
    return spectral.Spectral(CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _signals(name):
    c = CONFIGS[name]
    return mr.signals(c["audio_sample_rate"], c["hop_size"])


def _judge(what, got, want64, ref32):
    """one waveform against the oracle in units of the float32 path's error"""
    assert got.shape == want64.shape == ref32.shape, (what, got.shape, want64.shape, ref32.shape)
    assert np.isfinite(got).all(), what
    e_ref, e_gpu = ir.unit_error(ref32, want64), ir.unit_error(got, want64)
    print(f"{what}: error gpu {e_gpu:.3e}  float32 path {e_ref:.3e}  ratio {e_gpu / e_ref if e_ref else 0:.2f}")
    assert e_gpu <= FACTOR * e_ref, (what, e_gpu, e_ref)


def _denoise_checks(name, keys):
    sp, sig = _sp(name), _signals(name)
    w, hop = sp.window, sp.hop
    for k in keys:
        x = sig[k]
        n_out = ir.out_len(len(x), hop)
        m = np.abs(ir.stft(x, w, hop))
        for label, v in (("median", float(np.median(m))), ("0.1", 0.1)):
            if label == "median":   # both branches of the edit run
                clipped = float(np.mean(m <= v))
                assert 0.25 <= clipped <= 0.75, (name, k, clipped)
            got, lens = sp.denoise(T(x).cuda(), v=v)
            assert lens.cpu().tolist() == [n_out] and got.shape == (1, len(x))
            got = got[0].cpu().numpy()
            assert not got[n_out:].any()
            _judge(f"{name}/{k}/v={label}", got[:n_out], ir.denoise(x, w, hop, v), ir.denoise_f32(x, w, hop, v))
        # v = 0: the round trip gives the input back, within the same bound
        got, _ = sp.denoise(T(x).cuda(), v=0.0)
        _judge(f"{name}/{k}/v=0 against the input", got[0, :n_out].cpu().numpy(), x[:n_out].astype(np.float64), ir.denoise_f32(x, w, hop, 0.0))
        # a floor above every magnitude: exact zeros
        got, _ = sp.denoise(T(x).cuda(), v=2.0 * float(m.max()))
        assert not got.cpu().numpy().any(), (name, k)


def test_accuracy_against_float64_in_units_of_the_reference_arithmetic():
    _denoise_checks("default", ("noise", "clipped", "quiet", "speech", "tone"))
    sp, x = _sp("default"), _signals("default")["silence"]
    for v in (0.0, 0.1):   # silence has no magnitude to take a median of: it must come back as exact zeros at any floor
        got, lens = sp.denoise(T(x).cuda(), v=v)
        assert lens.cpu().tolist() == [ir.out_len(len(x), sp.hop)] and not got.cpu().numpy().any()


@pytest.mark.parametrize("name", ["short_window", "hop200_nyquist", "n2048_hop300"])
def test_other_configurations(name):
    _denoise_checks(name, ("noise", "speech"))


@pytest.mark.parametrize("name", ["default", "short_window", "hop200_nyquist", "n2048_hop300"])
def test_forward_alone_against_torch_float64(name):
    """mode 1: the spectrum per frame, in units of the float32 torch.stft's error against float64 (each frame scaled by its largest magnitude)"""
    sp, sig = _sp(name), _signals(name)
    N, hop = sp.n_fft, sp.hop
    for k in ("noise", "speech", "tone") if name == "default" else ("noise",):
        x = sig[k]
        spec, frames = sp.stft(T(x).cuda())
        assert frames.cpu().tolist() == [ir.frame_count(len(x), hop)] and spec.shape == (1, frames[0].item(), N // 2 + 1)
        got = spec[0].cpu().numpy()
        assert not got[:, 0].imag.any() and not got[:, -1].imag.any()
        w64 = torch.as_tensor(sp.window.astype(np.float64))
        S64 = torch.stft(T(x.astype(np.float64)), N, hop_length=hop, win_length=N, window=w64, center=True, pad_mode="constant", return_complex=True).numpy().T
        S32 = torch.stft(T(x), N, hop_length=hop, win_length=N, window=T(sp.window), center=True, pad_mode="constant", return_complex=True).numpy().T
        assert np.max(np.abs(S64 - ir.stft(x, sp.window, hop))) <= 1e-12 * np.abs(S64).max()
        scale = np.maximum(np.abs(S64).max(axis=1, keepdims=True), 1e-6)
        e_ref, e_gpu = float(np.max(np.abs(S32 - S64) / scale)), float(np.max(np.abs(got - S64) / scale))
        print(f"{name}/{k}: spectrum error gpu {e_gpu:.3e}  float32 torch.stft {e_ref:.3e}  ratio {e_gpu / e_ref:.2f}")
        assert e_gpu <= FACTOR * e_ref, (name, k, e_gpu, e_ref)


@pytest.mark.parametrize("name", ["default", "n2048_hop300"])
def test_inverse_alone_on_an_inconsistent_spectrum(name):
    """mode 2 on a spectrum no signal has, with imaginary parts in bins 0 and n_fft / 2: they are ignored (same bits with them zeroed)"""
    sp = _sp(name)
    N, hop, n_frames = sp.n_fft, sp.hop, 41
    rng = np.random.default_rng(17)
    S = (rng.standard_normal((n_frames, N // 2 + 1)) + 1j * rng.standard_normal((n_frames, N // 2 + 1))).astype(np.complex64)
    assert S[:, 0].imag.all() and S[:, -1].imag.all()
    S0 = S.copy()
    S0[:, 0] = S0[:, 0].real
    S0[:, -1] = S0[:, -1].real
    got, lens = sp.istft(T(S).cuda())
    got0, lens0 = sp.istft(T(S0).cuda())
    assert lens.cpu().tolist() == lens0.cpu().tolist() == [hop * (n_frames - 1)] and got.shape == (1, hop * (n_frames - 1))
    assert torch.equal(got, got0)
    y32 = torch.istft(T(S0.T), N, hop_length=hop, win_length=N, window=T(sp.window), center=True).numpy()
    _judge(f"{name}/inconsistent", got[0].cpu().numpy(), ir.istft(S, sp.window, hop), y32)
    # fewer frames than rows: frames[b] rules, the rest of the row stays zero
    part, plens = sp.istft(T(np.stack([S, S])).cuda(), frames=[n_frames, 10])
    assert plens.cpu().tolist() == [hop * (n_frames - 1), hop * 9]
    assert torch.equal(part[0], got[0]) and not part[1, hop * 9:].any()
    _judge(f"{name}/inconsistent, 10 frames", part[1, :hop * 9].cpu().numpy(), ir.istft(S[:10], sp.window, hop),
           torch.istft(T(S0[:10].T), N, hop_length=hop, win_length=N, window=T(sp.window), center=True).numpy())


# ---- the edge batch of tests/test_melspec_gpu.py: an empty utterance, one shorter than n_fft / 2, an exact multiple of hop, a partial
# tile, one that spans several tiles (301 frames: three or five of the forward kernel's, ten of the inverse's).  Samples past each length are 1.0.
@functools.lru_cache(maxsize=None)
def _edge_wavs():
    rng = np.random.default_rng(11)
    wav = np.ones((len(EDGE_LENS), max(EDGE_LENS)), np.float32)
    for b, n in enumerate(EDGE_LENS):
        wav[b, :n] = 0.1 * rng.standard_normal(n)
    return wav


def _edge_run(sp, wav, lens, reps=1, internal=False):
    """-> (out, out_lens, frames) as host arrays of a batch that repeats (wav, lens) reps times through mode FORWARD | INVERSE at v = EDGE_V;
    out pre-filled with the sentinel.  internal: the spectrum and the frame counts stay in the context's workspace (frames comes back None)."""
    sp._plan()
    dev = torch.device("cuda")
    w = T(np.tile(wav, (reps, 1))).to(dev)
    ln = torch.tensor(list(lens) * reps, dtype=torch.int32, device=dev)
    B, L = w.shape
    cap = 1 + L // sp.hop
    out = torch.full((B, L), SENTINEL, dtype=torch.float32, device=dev)
    out_lens = torch.full((B,), -1, dtype=torch.int32, device=dev)
    frames = None if internal else torch.full((B,), -1, dtype=torch.int32, device=dev)
    spec = None if internal else torch.full((B, cap, sp.n_bins, 2), SENTINEL, dtype=torch.float32, device=dev)
    sp.ctx.spectral(abi.SPECTRAL_FORWARD | abi.SPECTRAL_INVERSE, B, L, sp.hop, cap, torch.cuda.current_stream().cuda_stream,
                    wav=w.data_ptr() if L else None, lens=ln.data_ptr(), frames=None if internal else frames.data_ptr(),
                    spec=None if internal else spec.data_ptr(), out=out.data_ptr() if L else None, out_lens=out_lens.data_ptr(), floor=EDGE_V)
    torch.cuda.synchronize()
    if spec is not None:   # rows >= T_b of the spectrum are untouched
        fr = frames.cpu().tolist()
        for b in range(min(B, len(lens))):
            assert bool((spec[b, fr[b]:] == SENTINEL).all()) and not bool((spec[b, :fr[b]] == SENTINEL).any()), b
    return out.cpu().numpy(), out_lens.cpu().numpy(), None if internal else frames.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _edge_batch():
    return _edge_run(_sp("default"), _edge_wavs(), EDGE_LENS)


def _full_tiles_need():
    """utterances of 301 frames it takes before the forward launcher leaves the half-size tile (istft.hip: spectral_forward_launch, the rule
    of melspec_launch): 2 x B x ceil(301 / 128) > CUs"""
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count // 6 + 1


def test_edges_frame_counts_untouched_samples_and_values():
    sp = _sp("default")
    out, out_lens, frames = _edge_batch()
    assert frames.tolist() == [1 + n // sp.hop for n in EDGE_LENS] == [1, 1, 10, 41, 301]
    assert out_lens.tolist() == [sp.hop * (n // sp.hop) for n in EDGE_LENS] == [0, 0, 2304, 10240, 76800]
    wav = _edge_wavs()
    for b, n in enumerate(EDGE_LENS):
        assert np.all(out[b, out_lens[b]:] == SENTINEL), b
        if out_lens[b]:
            _judge(f"len{n}", out[b, :out_lens[b]], ir.denoise(wav[b, :n], sp.window, sp.hop, EDGE_V), ir.denoise_f32(wav[b, :n], sp.window, sp.hop, EDGE_V))


def test_batch_invariance_alone_in_the_batch_and_at_both_tile_sizes():
    sp = _sp("default")
    out, out_lens, frames = _edge_batch()     # B = 5: few tiles, the half-size tile of the forward kernel
    wav = _edge_wavs()
    for b, n in enumerate(EDGE_LENS):         # alone, its own length as the leading dimension
        o1, l1, f1 = _edge_run(sp, wav[b:b + 1, :n], (n,))
        assert l1.tolist() == [out_lens[b]] and f1.tolist() == [frames[b]]
        assert np.array_equal(o1[0, :l1[0]], out[b, :out_lens[b]]) and np.all(o1[0, l1[0]:] == SENTINEL), b
    reps = (_full_tiles_need() + len(EDGE_LENS) - 1) // len(EDGE_LENS)
    big, big_lens, big_frames = _edge_run(sp, wav, EDGE_LENS, reps=reps)   # enough utterances for the full-size tile
    assert 2 * big.shape[0] * 3 > torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    for r in range(reps):
        sl = slice(r * len(EDGE_LENS), (r + 1) * len(EDGE_LENS))
        assert np.array_equal(big[sl], out) and np.array_equal(big_lens[sl], out_lens) and np.array_equal(big_frames[sl], frames), r
    # and with the spectrum in the context's workspace instead of the caller's buffer
    o2, l2, _ = _edge_run(sp, wav, EDGE_LENS, internal=True)
    assert np.array_equal(o2, out) and np.array_equal(l2, out_lens)


def _split(tiles, blocks, want):
    """istft.hip: istft_split — the workgroups a tile's independent blocks are handed to: the smallest power of two that reaches `want`
    workgroups, at most `blocks`"""
    s = 1
    while s < blocks and tiles * s < want:
        s *= 2
    return s


def test_batch_invariance_at_every_work_split():
    """The launchers hand the n_fft / 64 = 16 blocks of a tile to 16, 8, 4, 2 or 1 workgroups, depending on how many tiles the batch has
    (forward: until 4 workgroups per CU, inverse: until 16).  The other tests of this file are small batches: the largest split, one block per
    workgroup.  Here the batch grows until a workgroup walks all 16 blocks itself — the loop over blocks, its prefetch across the block
    boundary and the re[n_fft / 2] substitution on re-entry — and every utterance must keep its bits."""
    sp = _sp("default")
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    out, out_lens, frames = _edge_batch()
    wav, nb = _edge_wavs(), sp.n_fft // 64
    # (a) one-tile utterances: 100 samples, 9 hops, 9 hops of another signal; wav_ld = 9 hops -> one tile per utterance in both launchers
    L = sp.hop * 9
    w3, l3 = np.ascontiguousarray(wav[1:4, :L]), (100, L, L)
    ref, ref_lens, ref_frames = _edge_run(sp, w3, l3)
    assert ref_lens.tolist() == [0, L, L] and ref_frames.tolist() == [1, 10, 10] and np.array_equal(ref[1], out[2, :L])
    fwd_seen, inv_seen = {_split(3, nb, 4 * cus)}, {_split(3, nb, 16 * cus)}
    for need in [4 * cus // 8] + [16 * cus // k for k in (16, 8, 4, 2, 1)]:   # the batch at which a launcher moves to the next split
        reps = (need + 2) // 3
        B = 3 * reps
        f, i = _split(B, nb, 4 * cus), _split(B, nb, 16 * cus)
        fwd_seen.add(f)
        inv_seen.add(i)
        big, big_lens, big_frames = _edge_run(sp, w3, l3, reps=reps)
        assert np.array_equal(big.reshape(reps, 3, L), np.broadcast_to(ref, (reps, 3, L))), (B, f, i)
        assert np.array_equal(big_lens.reshape(reps, 3), np.broadcast_to(ref_lens, (reps, 3))), (B, f, i)
        assert np.array_equal(big_frames.reshape(reps, 3), np.broadcast_to(ref_frames, (reps, 3))), (B, f, i)
        if f == i == 1:
            _judge("9 hops at split 1", big[-1, :L], ir.denoise(w3[2], sp.window, sp.hop, EDGE_V), ir.denoise_f32(w3[2], sp.window, sp.hop, EDGE_V))
    assert inv_seen == fwd_seen == {16, 8, 4, 2, 1}, (fwd_seen, inv_seen)
    # (b) the edge batch itself, utterances of several tiles: 3 forward and 10 inverse tiles per utterance at wav_ld = 300 hops
    for k in (4, 1):
        reps = (16 * cus // (10 * k) + len(EDGE_LENS) - 1) // len(EDGE_LENS) + 1
        B = reps * len(EDGE_LENS)
        assert _split(10 * B, nb, 16 * cus) == k and _split(3 * B, nb, 4 * cus) in (k, k // 2, 1)
        fwd_seen.add(_split(3 * B, nb, 4 * cus))
        big, big_lens, _ = _edge_run(sp, wav, EDGE_LENS, reps=reps, internal=True)
        assert np.array_equal(big.reshape(reps, *out.shape), np.broadcast_to(out, (reps, *out.shape))), k
        assert np.array_equal(big_lens.reshape(reps, -1), np.broadcast_to(out_lens, (reps, len(EDGE_LENS)))), k
    assert 1 in fwd_seen


def test_edges_in_a_red_zone_context():
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    try:
        sp = spectral.Spectral(CONFIGS["default"], ctx=ctx)
        out, out_lens, _ = _edge_run(sp, _edge_wavs(), EDGE_LENS, internal=True)
        assert ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, ctx.last_error()
        assert not np.isnan(out).any()
        ref_out, ref_lens, _ = _edge_batch()
        assert np.array_equal(out, ref_out) and np.array_equal(out_lens, ref_lens)
    finally:
        ctx.close()


def test_misuse_is_refused_with_the_value_named():
    ctx = abi.Context()
    try:
        stream = torch.cuda.current_stream().cuda_stream
        F, I = abi.SPECTRAL_FORWARD, abi.SPECTRAL_INVERSE
        wav = torch.zeros(1, 1000, device="cuda")
        out = torch.zeros(1, 1000, device="cuda")
        spec = torch.zeros(1, 4, 513, 2, device="cuda")
        frames = torch.zeros(1, dtype=torch.int32, device="cuda")
        ptr = dict(wav=wav.data_ptr(), out=out.data_ptr(), spec=spec.data_ptr(), frames=frames.data_ptr())
        call = lambda mode=F | I, B=1, L=1000, hop=256, cap=4, floor=0.1, **kw: ctx.spectral(mode, B, L, hop, cap, stream, floor=floor, **{**ptr, **kw})
        with pytest.raises(abi.DttsError, match=r"\(-1\).*DTTS_PART_ISTFT"):        # DTTS_E_STATE: no plan yet
            call()
        with pytest.raises(abi.DttsError, match=r"\(-2\).*istft\.window"):         # DTTS_E_NOENT: no tensor
            ctx.finalize(abi.PART_ISTFT)
        ctx.load_state_dict("istft", {"window": np.ones(768, np.float32)})
        with pytest.raises(abi.DttsError, match=r"\(-22\).*n_fft = 768"):
            ctx.finalize(abi.PART_ISTFT)
        with pytest.raises(abi.DttsError, match=r"\(-1\)"):                         # the refused plan left nothing behind
            call()
        ctx.load_state_dict("istft", {"window": spectral.centred_hann(1024, 1024)})
        ctx.finalize(abi.PART_ISTFT)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mode = 0"):
            call(mode=0)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mode = 4"):
            call(mode=4)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*B = 0"):
            call(B=0)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*hop = 1025"):
            call(hop=1025)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*hop = 0"):
            call(hop=0)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*hop = 1024.*falls to 0 "):   # Hann: w[0] = 0 alone covers a kept sample
            call(hop=1024, cap=1)
        call(mode=F, hop=1024, cap=1)                                                # the forward half has no envelope to divide by
        with pytest.raises(abi.DttsError, match=r"\(-22\).*spec_cap = 3"):          # 1 + 1000 // 256 = 4 rows are needed
            call(cap=3)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*floor = -0\.5"):
            call(floor=-0.5)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*floor = (inf|nan)"):
            call(floor=float("inf"))
        with pytest.raises(abi.DttsError, match=r"\(-22\).*floor = (inf|nan|-nan)"):
            call(floor=float("nan"))
        with pytest.raises(abi.DttsError, match=r"\(-22\).*null wav_dev"):
            call(wav=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*null out_dev"):
            call(out=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*null spec_dev"):
            call(mode=F, spec=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*null frames_dev"):
            call(mode=I, frames=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*out_dev == wav_dev \+0 samples"):
            call(out=wav.data_ptr())
        two = torch.zeros(3, 1000, device="cuda")                                    # a partial overlap: shifted by one row of a B = 2 batch
        with pytest.raises(abi.DttsError, match=r"\(-22\).*out_dev overlaps wav_dev.*\+1000 samples"):
            call(B=2, wav=two.data_ptr(), out=two[1:].data_ptr(), spec=None, frames=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*out_dev overlaps wav_dev.*-1000 samples"):
            call(B=2, wav=two[1:].data_ptr(), out=two.data_ptr(), spec=None, frames=None)
        call(B=1, wav=two.data_ptr(), out=two[1:].data_ptr())                        # disjoint rows of one tensor are fine
        a = abi.SpectralArgs(C.sizeof(abi.SpectralArgs) - 8, 3, 256, 1, 1000, 4, 0.1, wav.data_ptr(), None, None, None, out.data_ptr(), None)
        assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_SPECTRAL, C.byref(a), stream) == -22
        assert f"size = {C.sizeof(abi.SpectralArgs) - 8}" in ctx.last_error()
        out.fill_(SENTINEL)
        call(spec=None, frames=None)                                                 # and the good call goes through
        torch.cuda.synchronize()
        assert not out[0, :768].any().item() and bool((out[0, 768:] == SENTINEL).all())
    finally:
        ctx.close()


def test_refinalising_replaces_the_plan_on_one_stream():
    """two configurations finalised one after the other into ONE context, each run right behind its finalisation with no synchronisation
    of the caller's in between: both right (the first plan's packs stay alive while its launches may still read them)"""
    ctx = abi.Context()
    try:
        outs = {}
        for name in ("default", "short_window"):
            sp = spectral.Spectral(CONFIGS[name], ctx=ctx)
            x = _signals(name)["noise"]
            outs[name] = (sp, x, sp.denoise(T(x).cuda(), v=0.1))
        for name, (sp, x, (got, lens)) in outs.items():
            n = lens.cpu().tolist()[0]
            _judge(f"{name}/noise", got[0, :n].cpu().numpy(), ir.denoise(x, sp.window, sp.hop, 0.1), ir.denoise_f32(x, sp.window, sp.hop, 0.1))
    finally:
        ctx.close()


def test_objects_sharing_a_context_each_get_their_own_plan():
    """a context holds one plan: two Spectral objects of different configurations on ONE context, called in turn and again, each
    finalise their own plan back in (the first must not go on with the second's n_fft and window)"""
    ctx = abi.Context()
    try:
        a, b = spectral.Spectral(CONFIGS["default"], ctx=ctx), spectral.Spectral(CONFIGS["short_window"], ctx=ctx)
        xa, xb = _signals("default")["noise"], _signals("short_window")["noise"]
        want_a, _ = _sp("default").denoise(T(xa).cuda(), v=0.1)
        want_b, _ = _sp("short_window").denoise(T(xb).cuda(), v=0.1)
        for _ in range(2):
            assert torch.equal(a.denoise(T(xa).cuda(), v=0.1)[0], want_a) and ctx._istft_plan_of is a
            assert torch.equal(b.denoise(T(xb).cuda(), v=0.1)[0], want_b) and ctx._istft_plan_of is b
        assert torch.equal(a.stft(T(xa).cuda())[0], _sp("default").stft(T(xa).cuda())[0])
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _voc():
    return vocoder.HifiGAN(state_dict={k: T(v) for k, v in synth.hifigan_state_dict(1234).items()}, config=synth.hifigan_config())


def test_vocoder_denoise_equals_spectral_denoise():
    voc = _voc()
    assert voc.hop == 256
    rng = np.random.default_rng(3)
    mels = T((0.8 * rng.standard_normal((2, 33, 80)) - 2.0).astype(np.float32)).cuda()
    lens = torch.tensor([20, 33], dtype=torch.int32, device="cuda")
    wav = voc.forward_batch(mels, lens)
    got, got_lens = voc.denoise(wav, lens, v=0.05)
    assert voc._spectral.ctx is voc.ctx                      # the plan lives in the vocoder's context
    want, want_lens = spectral.Spectral().denoise(wav, lens * voc.hop, v=0.05)
    assert got_lens.cpu().tolist() == want_lens.cpu().tolist() == [20 * 256, 33 * 256]
    assert torch.equal(got, want) and got.abs().max().item() > 0 and not got[0, 20 * 256:].any().item()
    assert not torch.equal(got, wav)
    # another plan loaded into the vocoder's context does not derail the vocoder's own
    other = spectral.Spectral(CONFIGS["short_window"], ctx=voc.ctx)
    other.denoise(wav, v=0.05)
    assert torch.equal(voc.denoise(wav, lens, v=0.05)[0], want)
    # hparams whose hop_size is not the generator's: refused, not a silently shortened utterance
    from dict_tts_amd import hparams as hparams_mod
    saved, voc._spectral = dict(hparams_mod.hparams), None
    try:
        hparams_mod.hparams["hop_size"] = 128
        with pytest.raises(abi.DttsError, match=r"hop_size=128.*upsamples by 256"):
            voc.denoise(wav, lens, v=0.05)
    finally:
        hparams_mod.hparams.clear()
        hparams_mod.hparams.update(saved)
    assert torch.equal(voc.denoise(wav, lens, v=0.05)[0], want)


def test_run_inference_denoise_c(tmp_path):
    """denoise_c > 0 filters between the generator and the int16 conversion, in the plain and in the pipelined path; 0.0 (the default)
    writes the same bytes as a run without the argument"""
    from dict_tts_amd import model
    from scipy.io import wavfile
    acoustic = model.PortaSpeech_dict(hparams={})
    acoustic.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(1234, n_phone=6).items()}, strict=True)
    voc, st = _voc(), synth.biaobei_struct()
    batches = []
    for k, n in enumerate((2, 1)):
        b = {key: T(v) for key, v in synth.make_batch(st["sentences"][10 * k:10 * k + n], 100 + k).items()}
        b["item_name"], b["text"] = [f"{k}_{i}" for i in range(n)], [f"utt {k} {i}" for i in range(n)]
        batches.append(b)
    enc = [f"p{i}" for i in range(185)]

    def run(tag, **kw):
        torch.manual_seed(7)   # z_p is drawn from the CPU generator, in batch order
        rows = infer.run_inference(acoustic, voc, batches, str(tmp_path / tag), enc, **kw)
        return [open(os.path.join(tmp_path, tag, "wavs", r["wav_fn_pred"] + ".wav"), "rb").read() for r in rows]

    torch.manual_seed(7)
    floats = [w for b in batches for w in infer.infer_batch(acoustic, voc, b)[1]]
    sp = spectral.Spectral()
    for pipeline in (False, True):
        plain = run(f"plain{pipeline}", pipeline=pipeline)
        assert run(f"zero{pipeline}", pipeline=pipeline, denoise_c=0.0) == plain
        filtered = run(f"filtered{pipeline}", pipeline=pipeline, denoise_c=0.01)
        assert len(filtered) == len(floats) == 3 and filtered != plain
        for data, w in zip(filtered, floats):
            pcm = np.frombuffer(data[44:], np.int16)
            want, want_len = sp.denoise(T(w).cuda(), v=0.01)
            assert want_len.cpu().tolist() == [len(w)] == [len(pcm)]
            want = infer.wav_to_int16(want[0].cpu().numpy())
            assert np.max(np.abs(pcm.astype(np.int32) - want.astype(np.int32))) <= 1 and want.any()
