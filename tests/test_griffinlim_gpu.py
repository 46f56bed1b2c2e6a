"""Griffin-Lim on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM), ``Spectral.griffin_lim`` and the
``vocoder.GriffinLim`` plugin against the restatement of the reference's loop on torch.stft / torch.istft (tests/griffinlim_ref.py).

Accuracy is judged as tests/test_spectral_gpu.py judges the filter: in units of the error of the reference's OWN arithmetic (the float32
restatement against the float64 one on the same inputs), of which the kernels may take FACTOR = 4.  Every compared figure is printed before
it is asserted.

Measured on the MI355X (LABNOTES.md "Griffin-Lim"): one projection keeps |S'| within 2.0 - 2.4 ulp of A and S' |X64| within 0.59 - 1.26 of
A e32 of A X64; iterated error ratios 0.26 - 0.77 (perturbed start, 1 / 4 / 16 iterations) and 0.34 - 0.89 (random start, 1 / 2); d_16 / d_0 =
0.22 - 0.29 with a largest step ratio of 0.981; mel input within 0.075 of its bound.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import griffinlim_ref as gr
from dict_tts_amd import abi, infer, spectral, synth, vocoder

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SENTINEL = 777.0
NAMES = list(gr.CONFIGS)
EDGE_FRAMES = (1, 2, 31, 32, 33, 63, 64, 65, 128, 129)   # around ISTFT_TILE = 32 and both forward tiles (64 and 128 frames)
EDGE_CONFIGS = {**{k: gr.hparams(k) for k in NAMES}, "n1024_hop200": {**gr.hparams("n1024"), "hop_size": 200}}   # 200 does not divide 1024
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _sp(name):
    return spectral.Spectral(EDGE_CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _case(name, start):
    return gr.case(name, start)


@functools.lru_cache(maxsize=None)
def _gpu(name, start, n_iter):
    """-> (wav [hop (T - 1)], spec [T, bins]) of the case as host arrays"""
    c = _case(name, start)
    wav, lens, spec = _sp(name).griffin_lim(mag=T(c["A"][None]).cuda(), init=T(c["init"][None]).cuda(), n_iter=n_iter, return_spec=True)
    assert lens.cpu().tolist() == [c["hop"] * (c["T"] - 1)] and wav.shape == (1, c["hop"] * (c["T"] - 1))
    return wav[0].cpu().numpy(), spec[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(name, start, n_iter):
    """-> (y64, y32): the float64 restatement and the reference arithmetic"""
    c = _case(name, start)
    return gr.griffin_lim(c["A"], c["init"], c["window"], c["hop"], n_iter), gr.griffin_lim_f32(c["A"], c["init"], c["window"], c["hop"], n_iter)


# ---- 1
@pytest.mark.parametrize("name", NAMES)
def test_zero_iterations_is_the_existing_inverse_bit_for_bit(name):
    c, sp = _case(name, "random"), _sp(name)
    A, I = T(c["A"][None]).cuda(), T(c["init"][None]).cuda()
    wav, lens = sp.griffin_lim(mag=A, init=I, n_iter=0)
    want, want_lens = sp.istft(torch.view_as_complex(torch.view_as_real(I) * A[..., None]))
    print(f"{name}: {wav.shape[1]} samples, peak {wav.abs().max().item():.3f}")
    assert wav.shape == want.shape and wav.abs().max().item() > 0.01
    assert torch.equal(wav, want) and torch.equal(lens, want_lens)
    assert np.array_equal(_gpu(name, "random", 0)[0], want[0].cpu().numpy())


# ---- 2
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("start", ["random", "perturbed"])
def test_one_projection_on_every_bin(name, start):
    """S' = A X / |X| checked without the division: |S'| = A within 4 ulp, and S' |X64| = A X64 within FACTOR x A x the float32 torch.stft's
    own max-abs error on the same waveform.  No bin is left out: where |X64| is small both sides are."""
    c = _case(name, start)
    y0, _ = _gpu(name, start, 0)
    _, S1 = _gpu(name, start, 1)
    A = c["A"].astype(np.float64)
    X64 = gr.stft(y0, c["window"], c["hop"]).numpy()
    e32 = float(np.max(np.abs(gr.stft(y0, c["window"], c["hop"], torch.float32).numpy() - X64)))
    S = S1.astype(np.complex128)
    mag_err = np.abs(np.abs(S) - A) / np.spacing(c["A"]).astype(np.float64)
    lhs = np.abs(S * np.abs(X64) - A * X64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(A > 0, lhs / (A * e32), 0.0)
    print(f"{name}/{start}: | |S'| - A | up to {mag_err.max():.2f} ulp;  |S' |X64| - A X64| / (A e32) up to {ratio.max():.3f} (e32 = {e32:.3e}, "
          f"peak |X64| {np.abs(X64).max():.1f}, smallest |X64| {np.abs(X64).min():.2e})")
    assert S1.shape == A.shape and np.isfinite(S1.view(np.float32)).all()
    assert (mag_err <= 4.0).all(), float(mag_err.max())
    assert (lhs <= FACTOR * A * e32).all(), float(ratio.max())
    assert not S1[:, 0].imag.any() and not S1[:, -1].imag.any()


# ---- 3
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("start,n_iter", [("perturbed", 1), ("perturbed", 4), ("perturbed", 16), ("random", 1), ("random", 2)])
def test_iterated_accuracy_in_units_of_the_reference_arithmetic(name, start, n_iter):
    """(the random start stops at two iterations: near-empty bins make the phase ill-conditioned, and any two float32 paths part ways)"""
    y64, y32 = _ref(name, start, n_iter)
    got, _ = _gpu(name, start, n_iter)
    e_ref, e_gpu = float(np.max(np.abs(y32 - y64))), float(np.max(np.abs(got - y64)))
    print(f"{name}/{start}/n_iter={n_iter}: max-abs error gpu {e_gpu:.3e}  float32 restatement {e_ref:.3e}  ratio {e_gpu / e_ref:.2f}")
    assert got.shape == y64.shape and np.isfinite(got).all()
    assert e_gpu <= FACTOR * e_ref, (e_gpu, e_ref)


# ---- 4
@pytest.mark.parametrize("name", NAMES)
def test_consistency_falls_at_every_iteration(name):
    """the Griffin-Lim property on the device's own transforms: d_i = || |stft(y_i)| - A || / || A ||, every y_i from a call of its own"""
    c, sp = _case(name, "random"), _sp(name)
    A = T(c["A"]).to(torch.float64)
    d = []
    for i in range(17):
        X, _ = sp.stft(T(_gpu(name, "random", i)[0]).cuda())
        d.append(float(torch.linalg.norm(X[0].cpu().to(torch.complex128).abs() - A) / torch.linalg.norm(A)))
    print(f"{name}: d_0 .. d_16 = " + " ".join(f"{v:.4f}" for v in d) + f";  d_16 / d_0 = {d[16] / d[0]:.3f}, largest step ratio "
          f"{max(b / a for a, b in zip(d, d[1:])):.4f}")
    assert all(b < a for a, b in zip(d, d[1:])), d
    assert d[16] < 0.5 * d[0], d


# ---- 5: the rules of the launchers restated (csrc/stft_core.h, csrc/melspec.hip, csrc/istft.hip), to know which paths a batch took
def _skew_shift(hop):
    def degree(ps):
        worst = 1
        for w in range(4):
            for k in range(1 << min(ps, 8)):
                on_bank = [0] * 32
                for t in range(32):
                    a = (32 * w + t) * hop + k
                    on_bank[(a + (a >> ps)) % 32] += 1
                worst = max(worst, max(on_bank))
        return worst
    best, deg = 31, 1 << 30
    for ps in (31, 8, 7, 6, 5):
        d = degree(ps)
        if d < deg:
            best, deg = ps, d
    return best


def _tile_frames(waves, hop, n_fft, ps):
    tt = 32 * waves
    while tt > 1 and ((tt - 1) * hop + n_fft + (((tt - 1) * hop + n_fft) >> ps) + 1) * 4 > 160 * 1024:
        tt -= 1
    return tt


def _split(tiles, blocks, want):
    s = 1
    while s < blocks and tiles * s < want:
        s *= 2
    return s


@functools.lru_cache(maxsize=None)
def _paths(n_fft, hop, B, cap):
    """-> (waves of the forward tile, forward csplit, inverse csplit) of a batch of B utterances of cap rows"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    ps, frames = _skew_shift(hop), 1 + hop * (cap - 1) // hop
    tt4 = _tile_frames(4, hop, n_fft, ps)
    waves = 2 if 2 * B * ((frames + tt4 - 1) // tt4) <= cus else 4
    tt = _tile_frames(waves, hop, n_fft, ps)
    return waves, _split(B * ((frames + tt - 1) // tt), n_fft // 64, 4 * cus), _split(B * ((cap + 31) // 32), n_fft // 64, 16 * cus)


@functools.lru_cache(maxsize=None)
def _edge_inputs(name):
    sp = _sp(name)
    rng = np.random.default_rng(sp.n_fft + sp.hop)
    cap = max(EDGE_FRAMES)
    A = (0.5 * np.abs(rng.standard_normal((len(EDGE_FRAMES), cap, sp.n_bins)))).astype(np.float32)
    init = np.exp(2j * np.pi * rng.random(A.shape)).astype(np.complex64)
    return A, init


def _c_run(sp, A, init, frames, n_iter=2, reps=1, extra=5):
    """the C call on a batch that repeats (A, init, frames) reps times, out (wav_ld = hop (cap - 1) + extra) and spec_out pre-filled with
    the sentinel -> (out, out_lens, spec) as host arrays"""
    sp._plan()
    dev = torch.device("cuda")
    A, init = T(np.tile(A, (reps, 1, 1))).to(dev), T(np.tile(init, (reps, 1, 1))).to(dev)
    fr = torch.tensor(list(frames) * reps, dtype=torch.int32, device=dev)
    B, cap, bins = A.shape
    wav_ld = sp.hop * (cap - 1) + extra
    out = torch.full((B, wav_ld), SENTINEL, dtype=torch.float32, device=dev)
    out_lens = torch.full((B,), -1, dtype=torch.int32, device=dev)
    spec = torch.full((B, cap, bins, 2), SENTINEL, dtype=torch.float32, device=dev)
    sp.ctx.griffin_lim(B, cap, sp.hop, n_iter, wav_ld, out.data_ptr(), torch.cuda.current_stream().cuda_stream, mag=A.data_ptr(),
                       init=torch.view_as_real(init).data_ptr(), frames=fr.data_ptr(), out_lens=out_lens.data_ptr(), spec_out=spec.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_lens.cpu().numpy(), spec.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _edge_batch(name):
    A, init = _edge_inputs(name)
    return _c_run(_sp(name), A, init, EDGE_FRAMES)


@pytest.mark.parametrize("name", list(EDGE_CONFIGS))
def test_edge_frame_counts_and_batch_invariance(name):
    sp = _sp(name)
    A, init = _edge_inputs(name)
    out, out_lens, spec = _edge_batch(name)
    hop, nb, cap = sp.hop, len(EDGE_FRAMES), max(EDGE_FRAMES)
    assert out_lens.tolist() == [hop * (f - 1) for f in EDGE_FRAMES] and out_lens[0] == 0
    for b, f in enumerate(EDGE_FRAMES):
        assert np.all(out[b, out_lens[b]:] == SENTINEL) and not np.any(out[b, :out_lens[b]] == SENTINEL), b
        assert np.isfinite(out[b, :out_lens[b]]).all() and (f < 2 or np.abs(out[b, :out_lens[b]]).max() > 1e-3), b
        assert np.all(spec[b, f:] == SENTINEL) and not np.any(spec[b, :f] == SENTINEL), b          # rows past frames[b] untouched
        mag = np.hypot(spec[b, :f, :, 0].astype(np.float64), spec[b, :f, :, 1])
        assert np.all(np.abs(mag - A[b, :f]) <= 4.0 * np.spacing(A[b, :f])), b                      # the last S is a projection
    paths = {_paths(sp.n_fft, hop, nb, cap)}
    # the shim: same bits, zeros instead of the sentinel
    wav, lens, sspec = sp.griffin_lim(mag=T(A).cuda(), init=T(init).cuda(), frames=list(EDGE_FRAMES), n_iter=2, return_spec=True)
    assert lens.cpu().tolist() == out_lens.tolist() and wav.shape == (nb, hop * (cap - 1))
    wav, sspec = wav.cpu().numpy(), torch.view_as_real(sspec).cpu().numpy()
    for b, f in enumerate(EDGE_FRAMES):
        assert np.array_equal(wav[b, :out_lens[b]], out[b, :out_lens[b]]) and not wav[b, out_lens[b]:].any(), b
        assert np.array_equal(sspec[b, :f], spec[b, :f]) and not sspec[b, f:].any(), b
    # alone, with its own frame count as the capacity
    for b, f in enumerate(EDGE_FRAMES):
        o1, l1, s1 = _c_run(sp, A[b:b + 1, :f], init[b:b + 1, :f], (f,))
        paths.add(_paths(sp.n_fft, hop, 1, f))
        assert l1.tolist() == [out_lens[b]] and np.array_equal(o1[0, :l1[0]], out[b, :out_lens[b]]) and np.all(o1[0, l1[0]:] == SENTINEL), b
        assert np.array_equal(s1[0], spec[b, :f]), b
    # and in the batch repeated eight times
    big, big_lens, big_spec = _c_run(sp, A, init, EDGE_FRAMES, reps=8)
    paths.add(_paths(sp.n_fft, hop, 8 * nb, cap))
    for r in range(8):
        sl = slice(r * nb, (r + 1) * nb)
        assert np.array_equal(big[sl], out) and np.array_equal(big_lens[sl], out_lens) and np.array_equal(big_spec[sl], spec), r
    print(f"{name}: (forward waves, forward csplit, inverse csplit) reached: {sorted(paths)}")
    assert {p[0] for p in paths} == {2, 4}, paths                  # both tile sizes of the projection
    # the projection's split of a tile's bin blocks over workgroups (n_fft 512 has 8 blocks: every batch here gives each its own workgroup)
    assert len({p[1] for p in paths}) > 1 or sp.n_fft == 512, paths


# ---- 6
def test_mel_input_against_the_float64_product():
    """A = max(1e-10, sum_j P[k][j] 10^mel[j]).  Bound per output, u = 2^-24: the n_mels terms are summed by one FMA chain — n_mels roundings,
    each at most u of the partial sum, which sum |terms| bounds in any order: n_mels u sum |terms|; the product inside an FMA is exact (1 u
    kept for it all the same); the exponential is the device library's exp10f, documented to 1 ulp = 2 u of each term; P is given in
    float32 on both sides, and the comparison's own conversion of the float64 product costs 1 u.  That is n_mels + 4 with 4 u to spare:
    (n_mels + 8) u sum_j |P[k][j]| 10^mel[j], the constant an exponential of up to 4 ulp would need."""
    sp = spectral.Spectral(gr.hparams("n1024"))
    rng = np.random.default_rng(4)
    frames, cap = (37, 20), 37
    mel = np.clip(rng.normal(-2.0, 1.5, (2, cap, 80)), -5.0, 1.0).astype(np.float32)
    mel[0, 5] = -5.0               # the project's floor on a whole frame
    mel[1, :, 40:] = -5.0
    ones = torch.ones(2, cap, sp.n_bins, dtype=torch.complex64, device="cuda")
    _, lens, spec = sp.griffin_lim(mel=T(mel).cuda(), frames=list(frames), init=ones, n_iter=0, return_spec=True)
    P = sp.inv_mel_basis.astype(np.float64)
    assert sp.inv_mel_basis.shape == (513, 80) and lens.cpu().tolist() == [256 * 36, 256 * 19]
    spec = spec.cpu().numpy()
    floored = 0
    for b, f in enumerate(frames):
        A = spec[b, :f].real
        assert not spec[b, :f].imag.any() and not spec[b, f:].any()
        e = 10.0 ** mel[b, :f].astype(np.float64)
        raw = e @ P.T
        # (the floor is the float32 nearest to 1e-10, as any fp32 maximum has it: rows of P outside fmin .. fmax are zero, bound 0)
        want, bound = np.maximum(float(np.float32(1e-10)), raw), (80 + 8) * 2.0 ** -24 * (e @ np.abs(P).T)
        err = np.abs(A.astype(np.float64) - want)
        floored += int(np.sum(raw < 1e-10))
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        print(f"utterance {b}: error / bound up to {ratio.max():.3f}; {int(np.sum(raw < 1e-10))} of {raw.size} outputs at the floor, "
              f"{int(np.sum(A == np.float32(1e-10)))} on the device")
        assert (err <= bound).all(), float(ratio.max())
        assert (A >= np.float32(1e-10)).all()
    assert floored > 0 and (sp.inv_mel_basis < 0).any()
    # mel input is magnitude input of that A, bit for bit
    A = T(np.ascontiguousarray(spec.real)).cuda()
    init = torch.polar(torch.ones(2, cap, sp.n_bins), 2 * np.pi * torch.rand(2, cap, sp.n_bins, generator=torch.Generator().manual_seed(1))).cuda()
    got = sp.griffin_lim(mel=T(mel).cuda(), frames=list(frames), init=init, n_iter=3, return_spec=True)
    want = sp.griffin_lim(mag=A, frames=list(frames), init=init, n_iter=3, return_spec=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and got[0].abs().max().item() > 0


def test_random_start_follows_the_torch_seed():
    sp, c = _sp("n512"), _case("n512", "random")
    A = T(c["A"][None]).cuda()
    torch.manual_seed(5)
    a, _ = sp.griffin_lim(mag=A, n_iter=2)
    torch.manual_seed(5)
    b, _ = sp.griffin_lim(mag=A, n_iter=2)
    c2, _ = sp.griffin_lim(mag=A, n_iter=2)
    assert torch.equal(a, b) and not torch.equal(a, c2)


# ---- 7
def test_misuse_is_refused_with_the_value_named():
    ctx = abi.Context()
    try:
        stream = torch.cuda.current_stream().cuda_stream
        mag = torch.rand(1, 4, 513, device="cuda")
        mel = torch.zeros(1, 4, 80, device="cuda")
        init = torch.ones(1, 4, 513, 2, device="cuda")
        spec = torch.zeros(1, 4, 513, 2, device="cuda")
        out = torch.full((1, 800), SENTINEL, device="cuda")
        ptr = dict(mag=mag.data_ptr(), init=init.data_ptr(), spec_out=spec.data_ptr())
        call = lambda B=1, cap=4, hop=256, n_iter=1, wav_ld=800, **kw: ctx.griffin_lim(B, cap, hop, n_iter, wav_ld, out.data_ptr(), stream, **{**ptr, **kw})
        with pytest.raises(abi.DttsError, match=r"\(-1\).*DTTS_PART_ISTFT"):
            call()
        ctx.load_state_dict("istft", {"window": spectral.centred_hann(1024, 1024)})
        ctx.finalize(abi.PART_ISTFT)
        with pytest.raises(abi.DttsError, match=r"\(-1\).*istft\.inv_mel_basis"):     # DTTS_E_STATE: the plan has no inverse mel basis
            call(mag=None, mel=mel.data_ptr(), n_mels=80)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*n_iter = -1"):
            call(n_iter=-1)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mag_dev = 0x[0-9a-f]+ and mel_dev = 0x[0-9a-f]+ \(exactly one"):
            call(mel=mel.data_ptr(), n_mels=80)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mag_dev = \(nil\) and mel_dev = \(nil\)"):
            call(mag=None)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*wav_ld = 767 samples, spec_cap = 4 rows at hop 256 give 768"):
            call(wav_ld=767)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*init_dev = 0x[0-9a-f]+ is not aligned to 8"):
            call(init=init.data_ptr() + 4)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*spec_out_dev = 0x[0-9a-f]+ is not aligned to 8"):
            call(spec_out=spec.data_ptr() + 4)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*mag_dev = 0x[0-9a-f]+ is not aligned to 4"):
            call(mag=mag.data_ptr() + 2)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*hop = 1024.*falls to 0 "):   # the envelope criterion, as DTTS_OUT_SPECTRAL's
            call(hop=1024, cap=1)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*hop = 0"):
            call(hop=0)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*B = 0"):
            call(B=0)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*spec_cap = 0"):
            call(cap=0)
        ctx.load_state_dict("istft", {"window": spectral.centred_hann(1024, 1024), "inv_mel_basis": np.zeros((512, 80), np.float32)})
        with pytest.raises(abi.DttsError, match=r"\(-22\).*istft\.inv_mel_basis must be \[n_fft / 2 \+ 1 = 513\].*512 x 80"):
            ctx.finalize(abi.PART_ISTFT)
        ctx.load_state_dict("istft", {"window": spectral.centred_hann(1024, 1024), "inv_mel_basis": np.zeros((513, 40), np.float32)})
        ctx.finalize(abi.PART_ISTFT)
        with pytest.raises(abi.DttsError, match=r"\(-22\).*n_mels = 80, istft\.inv_mel_basis has 40"):
            call(mag=None, mel=mel.data_ptr(), n_mels=80)
        a = abi.GriffinLimArgs(C.sizeof(abi.GriffinLimArgs) - 8, 1, 4, 256, 1, 800, 0, 0, mag.data_ptr(), None, None, None, out.data_ptr(), None, None)
        assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_GRIFFIN_LIM, C.byref(a), stream) == -22
        assert f"size = {C.sizeof(abi.GriffinLimArgs) - 8}" in ctx.last_error()
        call(init=None, spec_out=None)                                                # and the good call goes through: zero phase
        torch.cuda.synchronize()
        assert bool((out[0, 768:] == SENTINEL).all()) and not bool((out[0, :768] == SENTINEL).any()) and out[0, :768].abs().max().item() > 0
    finally:
        ctx.close()


def test_edges_in_a_red_zone_context():
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    try:
        sp = spectral.Spectral(EDGE_CONFIGS["n1024"], ctx=ctx)
        A, init = _edge_inputs("n1024")
        out, out_lens, spec = _c_run(sp, A, init, EDGE_FRAMES)
        assert ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, ctx.last_error()
        ref_out, ref_lens, ref_spec = _edge_batch("n1024")
        assert np.array_equal(out, ref_out) and np.array_equal(out_lens, ref_lens) and np.array_equal(spec, ref_spec)
    finally:
        ctx.close()


def test_plugin_and_run_inference(tmp_path):
    from dict_tts_amd import model
    from scipy.io import wavfile
    g = vocoder.GriffinLim({"griffin_lim_iters": 16})
    assert (g.hop, g.n_iter) == (256, 16)
    rng = np.random.default_rng(3)
    mels = np.clip(rng.normal(-2.0, 1.0, (2, 33, 80)), -5.0, 0.5).astype(np.float32)
    lens = torch.tensor([20, 33], dtype=torch.int32, device="cuda")
    torch.manual_seed(11)
    one = g.spec2wav(mels[1])
    assert one.shape == (256 * 32,) and one.dtype == np.float32 and np.isfinite(one).all() and np.abs(one).max() > 1e-3
    torch.manual_seed(11)
    wav = g.forward_batch(T(mels).cuda(), lens)
    assert wav.shape == (2, 33 * 256) and g.ctx is g.spectral.ctx
    assert not wav[0, 19 * 256:].any().item() and not wav[1, 32 * 256:].any().item()        # the zero tail: one hop less than len * hop
    assert wav[0, :19 * 256].abs().max().item() > 1e-3 and wav[1, :32 * 256].abs().max().item() > 1e-3
    for norm in (False, True):
        pcm = g.to_int16(wav, lens, norm=norm).cpu().numpy()
        for b, n in enumerate((20 * 256, 33 * 256)):
            assert np.array_equal(pcm[b, :n], infer.wav_to_int16(wav[b, :n].cpu().numpy(), norm)) and not pcm[b, n:].any(), (norm, b)
    den, den_lens = g.denoise(wav, lens, v=0.01)                                               # through the same Spectral and context
    assert den.shape == wav.shape and den_lens.cpu().tolist() == [20 * 256, 33 * 256] and not torch.equal(den, wav)
    # the inference harness with no checkpoint anywhere near the vocoder
    acoustic = model.PortaSpeech_dict(hparams={})
    acoustic.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(1234, n_phone=6).items()}, strict=True)
    b = {key: T(v) for key, v in synth.make_batch(synth.biaobei_struct()["sentences"][:2], 100).items()}
    b["item_name"], b["text"] = ["0_0", "0_1"], ["utt 0", "utt 1"]
    for pipeline in (False, True):
        torch.manual_seed(7)
        rows = infer.run_inference(acoustic, g, [b], str(tmp_path / f"p{pipeline}"), [f"p{i}" for i in range(185)], pipeline=pipeline)
        torch.manual_seed(7)
        mel_lens = infer._model_forward(acoustic, b, None)["mel_lens"].cpu().tolist()
        assert len(rows) == 2
        for r, n in zip(rows, mel_lens):
            sr, pcm = wavfile.read(os.path.join(tmp_path, f"p{pipeline}", "wavs", r["wav_fn_pred"] + ".wav"))
            assert sr == 22050 and pcm.dtype == np.int16 and pcm.shape == (n * 256,) and pcm.any() and not pcm[(n - 1) * 256:].any()
