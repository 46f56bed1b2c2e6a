"""The speaker encoder on the GPU (dict_tts_amd/speaker_encoder.py, csrc/spkenc.hip) against the float64 restatement tests/spkenc_ref.py,
which tests/test_spkenc_cpu.py anchors on float64 torch.  Seeded synthetic weights (synth.voice_encoder_state_dict).

Error gates: the GPU's error against float64 <= 8 x the error of the float32 torch form of the same stage on the CPU, fed the same inputs,
both measured here; the reference figure is the maximum over the module's cases.
  (a) the LSTM stage from identical float32 mels (the GPU's own): max |delta| of the partials' unit embeddings;
  (b) the mel front end from the waveform, normalised by the utterance's largest mel value (float32 torch.stft -> power -> filterbank);
  (c) embed_batch end to end against float32 torch.stft -> float32 nn.LSTM.
Both sides form the same exact fp32 products and differ in summation order and in the transcendental functions, which moves the rounding
error by a single-digit factor: 8 is the project's margin for that situation (tests/test_disc_gpu.py).  The ratios are printed.
forward(mels) is held layer by layer in the same way: every layer's hidden sequence against the float32 single-layer nn.LSTM chain.

Measured on an MI355X (LABNOTES.md "Speaker encoder"): (a) 0.70 - 1.88 x, (b) 0.48 - 1.10 x, (c) 0.28 - 1.57 x; forward(mels) layers 0 / 1 / 2
at most 1.04 / 0.68 / 0.85 x, its embeddings 1.50 x; saturation 1.98 x."""
import numpy as np
import pytest
import torch

import spkenc_ref as R
import spkenc_shapes as S
from dict_tts_amd import abi, synth
from dict_tts_amd import speaker_encoder as E

pytestmark = pytest.mark.gpu
MARGIN = 8.0
NAMES = list(S.UTTERANCES)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def host(out):
    torch.cuda.synchronize()
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in out.items()}


@pytest.fixture(scope="module")
def sd():
    return synth.voice_encoder_state_dict(S.SEED)


@pytest.fixture(scope="module")
def enc(sd):
    return E.VoiceEncoder.from_checkpoint({"model_state": sd})


@pytest.fixture(scope="module")
def utt(sd, enc):
    """every utterance of spkenc_shapes alone on the GPU with all stages, its float64 restatement (from the waveform, and from the GPU's
    float32 mel) and the float32 torch forms, once per module"""
    sd64 = R.f64(sd)
    out = {}
    for name in NAMES:
        w = S.wav(name)
        got = host(enc.embed_batch(torch.from_numpy(w)[None], [len(w)], stages=True))
        P = int(got["n_partials"][0])
        ref = R.embed_utterance(sd64, w)
        F = ref["mel"].shape[0]
        gmel = got["mel"][0, :F]
        slices = np.stack([gmel[s:s + S.PART] for s in ref["starts"]])
        lstm64, _ = R.forward(sd64, slices)
        lstm32, _ = R.torch_forward(sd64, slices)
        wpad = np.pad(w, (0, max(0, (ref["starts"][-1] + S.PART) * S.HOP - len(w))))
        out[name] = {"got": got, "P": P, "F": F, "ref": ref, "lstm64": lstm64, "lstm32": lstm32, "mel32": R.torch_mel(wpad),
                     "e2e32": R.torch_embed_utterance(sd64, w)}
    return out


def test_counts_frames_and_untouched_rows(utt):
    for name in NAMES:
        u = utt[name]
        g = u["got"]
        assert u["P"] == S.PARTIALS[name] == len(u["ref"]["starts"]), name
        assert u["F"] == 1 + max(S.UTTERANCES[name], (u["ref"]["starts"][-1] + S.PART) * S.HOP) // S.HOP
        assert np.all(np.isfinite(g["mel"][0, :u["F"]])) and np.all(np.isnan(g["mel"][0, u["F"]:])), name
        assert np.all(np.isfinite(g["partials"][0, :u["P"]])) and np.all(np.isnan(g["partials"][0, u["P"]:])), name
        for h in g["hseq"]:
            assert np.all(np.isfinite(h[0, :u["P"]])) and np.all(np.isnan(h[0, u["P"]:])), name
        assert np.all(np.isfinite(g["embed"])) and abs(np.linalg.norm(g["embed"][0].astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_gate_a_lstm_stage_from_identical_mels(utt, name):
    e_ref = max(np.abs(u["lstm32"] - u["lstm64"]).max() for u in utt.values())
    u = utt[name]
    err = np.abs(u["got"]["partials"][0, :u["P"]].astype(np.float64) - u["lstm64"]).max()
    own = np.abs(u["lstm32"] - u["lstm64"]).max()
    print(f"(a) {name}: GPU {err:.3e}, torch float32 {own:.3e} (max over cases {e_ref:.3e}): {err / e_ref:.2f} x")
    assert err <= MARGIN * e_ref, (name, err, e_ref)


@pytest.mark.parametrize("name", NAMES)
def test_gate_b_mel_front_end(utt, name):
    rel = lambda m, u: np.abs(m - u["ref"]["mel"]).max() / u["ref"]["mel"].max()
    e_ref = max(rel(u["mel32"], u) for u in utt.values())
    u = utt[name]
    err = rel(u["got"]["mel"][0, :u["F"]].astype(np.float64), u)
    print(f"(b) {name}: GPU {err:.3e}, torch float32 {rel(u['mel32'], u):.3e} (max over cases {e_ref:.3e}): {err / e_ref:.2f} x")
    assert err <= MARGIN * e_ref, (name, err, e_ref)


@pytest.mark.parametrize("name", NAMES)
def test_gate_c_end_to_end(utt, name):
    e_ref = max(np.abs(u["e2e32"]["embed"] - u["ref"]["embed"]).max() for u in utt.values())
    u = utt[name]
    err = np.abs(u["got"]["embed"][0].astype(np.float64) - u["ref"]["embed"]).max()
    own = np.abs(u["e2e32"]["embed"] - u["ref"]["embed"]).max()
    print(f"(c) {name}: GPU {err:.3e}, torch float32 {own:.3e} (max over cases {e_ref:.3e}): {err / e_ref:.2f} x")
    assert err <= MARGIN * e_ref, (name, err, e_ref)


# ---- forward(mels): every layer's hidden sequence
_FWD = {}


def fwd_ref(sd, N, T, scale=1.0, mel_scale=0.05):
    key = (N, T, scale)
    if key not in _FWD:
        w = R.f64(sd if scale == 1.0 else synth.voice_encoder_state_dict(S.SEED, scale=scale))
        m = S.mels(N, T, scale=mel_scale)
        _FWD[key] = (m, R.forward(w, m), R.torch_forward(w, m))
    return _FWD[key]


@pytest.mark.parametrize("N,T", S.FORWARD_CASES)
def test_forward_layer_by_layer(sd, enc, N, T):
    cases = [fwd_ref(sd, n, t) for n, t in S.FORWARD_CASES]
    e_layer = [max(np.abs(c[2][1][l] - c[1][1][l]).max() for c in cases) for l in range(3)]
    e_emb = max(np.abs(c[2][0] - c[1][0]).max() for c in cases)
    m, (emb64, hs64), _ = fwd_ref(sd, N, T)
    got = host(enc.forward(torch.from_numpy(m), stages=True))
    assert got["n_partials"].tolist() == [1] * N
    for l in range(3):
        err = np.abs(got["hseq"][l][:, 0].astype(np.float64) - hs64[l]).max()
        print(f"forward N {N} T {T} layer {l}: GPU {err:.3e}, torch float32 max over cases {e_layer[l]:.3e}: {err / e_layer[l]:.2f} x")
        assert err <= MARGIN * e_layer[l], (N, T, l, err, e_layer[l])
    err = np.abs(got["partials"][:, 0].astype(np.float64) - emb64).max()
    print(f"forward N {N} T {T} embeddings: GPU {err:.3e}, torch float32 max over cases {e_emb:.3e}: {err / e_emb:.2f} x")
    assert err <= MARGIN * e_emb
    plain = enc(torch.from_numpy(m))
    assert plain.shape == (N, 256) and np.array_equal(bits(plain), bits(got["partials"][:, 0]))
    # an utterance of one partial: the mean of one row, normalised again
    assert np.abs(got["embed"].astype(np.float64) - emb64).max() <= MARGIN * e_emb + 2e-7


def test_saturation(sd):
    """weights x 8 and mels x 400: pre-activations reach the hundreds; every output is finite and inside gate (a)"""
    cases = [(1, 160), (S.M + 1, 3)]
    big = synth.voice_encoder_state_dict(S.SEED, scale=8.0)
    enc8 = E.VoiceEncoder.from_checkpoint(big)
    refs = [fwd_ref(sd, n, t, scale=8.0, mel_scale=20.0) for n, t in cases]
    e_emb = max(np.abs(c[2][0] - c[1][0]).max() for c in refs)
    w0 = R.f64(big)
    pre = refs[0][0][0].astype(np.float64) @ w0["lstm.weight_ih_l0"].T
    assert np.abs(pre).max() > 100.0
    for (n, t), (m, (emb64, hs64), _) in zip(cases, refs):
        got = host(enc8.forward(torch.from_numpy(m), stages=True))
        assert all(np.all(np.isfinite(h)) for h in got["hseq"]) and np.all(np.isfinite(got["partials"])) and np.all(np.isfinite(got["embed"]))
        err = np.abs(got["partials"][:, 0].astype(np.float64) - emb64).max()
        print(f"saturation N {n} T {t}: GPU {err:.3e}, torch float32 max over cases {e_emb:.3e}: {err / e_emb:.2f} x")
        assert err <= MARGIN * e_emb, (n, t, err, e_emb)


def test_dead_relu_gives_nan_and_the_next_call_is_clean(sd, enc, utt):
    dead = dict(sd)
    dead["linear.weight"] = np.zeros((256, 256), np.float32)
    dead["linear.bias"] = -np.ones(256, np.float32)
    w = S.wav("L31520")
    got = host(E.VoiceEncoder.from_checkpoint(dead).embed_batch(torch.from_numpy(w)[None], return_partials=True))
    assert got["n_partials"].tolist() == [2] and np.all(np.isnan(got["embed"])) and np.all(np.isnan(got["partials"][0, :2]))
    again = host(enc.embed_batch(torch.from_numpy(w)[None]))
    assert np.all(np.isfinite(again["embed"])) and np.array_equal(bits(again["embed"]), bits(utt["L31520"]["got"]["embed"]))


def test_mixed_batch_reads_nothing_past_lens_and_equals_alone(enc, utt):
    """a mixed batch with NaN behind every utterance, lens on the device: every utterance's bits are those of the utterance alone, at both
    tile sizes; unwritten stage rows stay NaN"""
    wavs, lens = S.batch(S.MIXED)
    dl = torch.from_numpy(lens).cuda()
    for tile_m in (0, 16, 32):
        got = host(enc.embed_batch(torch.from_numpy(wavs), dl, stages=True, tile_m=tile_m))
        for b, name in enumerate(S.MIXED):
            one, P, F = utt[name]["got"], utt[name]["P"], utt[name]["F"]
            assert got["n_partials"][b] == P
            assert np.array_equal(bits(got["embed"][b]), bits(one["embed"][0])), (tile_m, name)
            assert np.array_equal(bits(got["partials"][b, :P]), bits(one["partials"][0, :P])), (tile_m, name)
            assert np.array_equal(bits(got["mel"][b, :F]), bits(one["mel"][0, :F])), (tile_m, name)
            assert np.all(np.isnan(got["mel"][b, F:])) and np.all(np.isnan(got["partials"][b, P:]))
            for l in range(3):
                assert np.array_equal(bits(got["hseq"][l][b, :P]), bits(one["hseq"][l][0, :P])), (tile_m, name, l)
                assert np.all(np.isnan(got["hseq"][l][b, P:]))


def test_chunked_batch_equals_alone(enc, utt):
    """34 utterances of 33 partials need 1.1 GiB of workspace, above the 1 GiB cap: the batch runs as two chunks of 17, every row with the
    bits of the utterance alone"""
    B = 34
    w = S.wav("Pp1")
    P = abi.spkenc_max_partials(len(w), S.FRAME_STEP)
    assert B * P * (S.PART * (1024 + 2 * 256) * 4) > 1 << 30
    got = host(enc.embed_batch(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(w, (B, len(w)))))))
    assert got["n_partials"].tolist() == [S.M + 1] * B
    one = bits(utt["Pp1"]["got"]["embed"][0])
    for b in range(B):
        assert np.array_equal(bits(got["embed"][b]), one), b


def test_every_batch_position_and_host_lens(enc, utt):
    others = ("L200", "L25600")
    for pos in range(3):
        names = list(others)
        names.insert(pos, "L31520")
        wavs, lens = S.batch(names, pad=5)
        got = host(enc.embed_batch(torch.from_numpy(wavs), lens.tolist(), return_partials=True))
        for b, name in enumerate(names):
            assert np.array_equal(bits(got["embed"][b]), bits(utt[name]["got"]["embed"][0])), (pos, name)
    w = S.wav("L31520")
    e, parts, slices = enc.embed_utterance(w.astype(np.float16).astype(np.float32), return_partials=True)
    e16 = enc.embed_utterance(w.astype(np.float16))                          # float16 input: converted, the same values
    assert e.dtype == np.float32 and e.shape == (256,) and parts.shape == (2, 256) and len(slices) == 2
    assert np.array_equal(bits(e), bits(e16))
    assert np.array_equal(bits(enc.embed_utterance(w)), bits(utt["L31520"]["got"]["embed"][0]))
    spk = enc.embed_speaker([S.wav("L25600"), w])
    raw = np.mean([utt["L25600"]["got"]["embed"][0], utt["L31520"]["got"]["embed"][0]], axis=0)
    assert np.array_equal(bits(spk), bits(raw / np.linalg.norm(raw, 2)))
    sim = E.similarity(torch.from_numpy(utt["L25600"]["got"]["embed"]).cuda(), torch.from_numpy(utt["L31520"]["got"]["embed"]).cuda())
    assert sim.is_cuda and abs(float(sim[0]) - float(np.dot(utt["L25600"]["ref"]["embed"], utt["L31520"]["ref"]["embed"]))) < 1e-5


def test_partials_equal_forward_on_the_sliced_mel(enc, utt):
    u = utt["Pp1"]
    mel = torch.from_numpy(u["got"]["mel"][0]).cuda()
    slices = torch.stack([mel[s:s + S.PART] for s in u["ref"]["starts"]])
    assert np.array_equal(bits(enc(slices)), bits(u["got"]["partials"][0, :u["P"]]))
    m2, frames = enc.wav_to_mel_spectrogram(torch.from_numpy(S.wav("Pp1"))[None])
    F = int(frames[0])
    assert F == 1 + S.UTTERANCES["Pp1"] // S.HOP and np.array_equal(bits(m2[0, :F]), bits(u["got"]["mel"][0, :F]))


def test_memory_safety_and_grown_workspace(sd, enc, utt):
    """debug_redzone = 1: every workspace buffer between red zones and 0xFF before each call; no launch damages a zone, no stale word
    reaches an output; a call after the workspace grew equals the call before"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    dbg = E.VoiceEncoder.from_checkpoint(sd, ctx=ctx)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    small = torch.from_numpy(S.wav("L31520"))[None]
    wavs, lens = S.batch(S.MIXED)
    first = host(dbg.embed_batch(small, stages=True))
    assert ctx.debug_check(stream()) == 0, ctx.last_error()
    big = host(dbg.embed_batch(torch.from_numpy(wavs), torch.from_numpy(lens).cuda(), stages=True))      # the workspace grows
    assert ctx.debug_check(stream()) == 0, ctx.last_error()
    second = host(dbg.embed_batch(small, stages=True))
    assert ctx.debug_check(stream()) == 0, ctx.last_error()
    fwd = host(dbg.forward(torch.from_numpy(S.mels(S.M + 1, 3)), stages=True))
    assert ctx.debug_check(stream()) == 0, ctx.last_error()
    assert np.array_equal(bits(fwd["partials"]), bits(enc.forward(torch.from_numpy(S.mels(S.M + 1, 3)), stages=True)["partials"]))
    for k in ("embed", "partials", "mel"):
        assert np.array_equal(bits(first[k]), bits(second[k])), k
        assert np.array_equal(bits(first[k]), bits(utt["L31520"]["got"][k])), k
    for b, name in enumerate(S.MIXED):
        assert np.array_equal(bits(big["embed"][b]), bits(utt[name]["got"]["embed"][0])), name
    ctx.close()


def test_pad_modes_differ_in_the_edge_frames_only(sd, utt):
    refl = E.VoiceEncoder.from_checkpoint(sd, pad_mode="reflect")
    w = S.wav("L25600")
    got = host(refl.embed_batch(torch.from_numpy(w)[None], stages=True))
    a, b = utt["L25600"]["got"]["mel"][0, :161], got["mel"][0, :161]
    assert np.array_equal(bits(a[2:-2]), bits(b[2:-2]))
    for f in (0, 1, -2, -1):
        assert not np.array_equal(a[f], b[f]), f
    want = R.mel(w, "reflect")
    e_ref = np.abs(R.torch_mel(w, "reflect") - want).max() / want.max()
    err = np.abs(b.astype(np.float64) - want).max() / want.max()
    print(f"reflect mel: GPU {err:.3e}, torch float32 {e_ref:.3e}: {err / e_ref:.2f} x")
    assert err <= MARGIN * e_ref


def test_embeddings_hand_over_to_the_acoustic_model_on_the_device(enc):
    """a synthetic use_spk_embed acoustic model given embed_batch(...)['embed'] on the device gives the mel bits it gives for the same values
    from the host"""
    import speaker_ref as sr
    from dict_tts_amd import model
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    m = model.PortaSpeech_dict(hparams=dict(sr.FORMS["embed"]["hparams"]))
    m.load_state_dict({k: T(v) for k, v in sr.g11_state_dict("embed").items()}, strict=True)
    batch = {k: T(v) for k, v in sr.g11_batch().items()}
    B = batch["word_tokens"].shape[0]
    names = [("L31520", "L25600", "L200", "L31519")[i % 4] for i in range(B)]
    wavs, lens = S.batch(names)
    embed = enc.embed_batch(torch.from_numpy(wavs), torch.from_numpy(lens).cuda())["embed"]
    assert embed.is_cuda and embed.shape == (B, 256)
    dm = tuple(batch[k] for k in ("keys", "values", "key_map", "pinyin", "pinyin_map"))
    run = lambda spk, z: m((batch["word_tokens"], None), batch["pron_modified"], (None, None, None), None, None, dm, infer=True, z_p=z, spk_embed=spk)
    T_mel = run(embed, None)["mel_out"].shape[1]
    z = T(synth.noise(sr.SEED, B, T_mel // 4, "spkenc.handover.z"))
    dev, hst = run(embed, z), run(embed.cpu().numpy(), z)
    assert dev["mel_out"].shape == hst["mel_out"].shape and torch.equal(dev["mel_out"].cpu(), hst["mel_out"].cpu())
    assert torch.equal(dev["mel2word"].cpu(), hst["mel2word"].cpu())


def test_finalize_names_what_is_wrong(sd):
    """DTTS_E_NOENT names the first missing tensor, DTTS_E_INVAL the tensor whose shape is not the encoder's"""
    from dict_tts_amd import melspec
    full = {**sd, "mel_basis": melspec.mel_filterbank(16000, 400, 40, 0, 8000).astype(np.float32), "window": melspec.hann_window(400).astype(np.float32)}
    ctx = abi.Context()
    ctx.load_state_dict("spkenc", {k: v for k, v in full.items() if k != "lstm.weight_hh_l2"})
    with pytest.raises(abi.DttsError, match=r"\(-2\).*missing tensor spkenc\.lstm\.weight_hh_l2"):
        ctx.finalize(abi.PART_SPKENC)
    ctx.close()
    ctx = abi.Context()
    ctx.load_state_dict("spkenc", {**full, "mel_basis": np.zeros((80, 201), np.float32)})
    with pytest.raises(abi.DttsError, match=r"\(-22\).*spkenc\.mel_basis is \[80, 201\].*\[40, 201\]"):
        ctx.finalize(abi.PART_SPKENC)
    x = torch.zeros(1, 64, device="cuda")
    e, n = torch.zeros(1, 256, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(abi.DttsError, match=r"before dtts_finalize_weights\(DTTS_PART_SPKENC\)"):
        ctx.spkenc(1, torch.cuda.current_stream().cuda_stream, wav=x.data_ptr(), wav_ld=64, embed=e.data_ptr(), n_partials=n.data_ptr())
    ctx.close()


def test_embed_speaker_tool_writes_what_forward_takes(sd, enc, utt, tmp_path, monkeypatch, capsys):
    """tools/embed_speaker.py --ckpt pretrained.pt a.wav --out spk.npy (in this process): float32 [1, 256], the utterance's embedding"""
    import importlib.util
    import os
    import sys
    from scipy.io import wavfile
    ckpt, wav, out = str(tmp_path / "pretrained.pt"), str(tmp_path / "a.wav"), str(tmp_path / "spk.npy")
    torch.save({"model_state": {k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt)
    wavfile.write(wav, 22050, S.wav("L31520"))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "embed_speaker.py")
    spec = importlib.util.spec_from_file_location("embed_speaker_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["embed_speaker.py", "--ckpt", ckpt, wav, "--out", out])
    tool.main()
    assert '"finite": true' in capsys.readouterr().out
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (1, 256)
    assert np.array_equal(bits(got[0]), bits(utt["L31520"]["got"]["embed"][0]))     # the samples taken as 16 kHz, as the binariser takes them
