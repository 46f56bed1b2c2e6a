"""The speaker encoder without a GPU: the float64 restatement tests/spkenc_ref.py against float64 torch (the executable anchor: nn.LSTM,
torch.stft), the partial slices by hand, the loader, normalize_volume and the refusals of dict_tts_amd/speaker_encoder.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import spkenc_ref as R
import spkenc_shapes as S
from dict_tts_amd import abi, synth
from dict_tts_amd import speaker_encoder as E


@pytest.fixture(scope="module")
def sd():
    return synth.voice_encoder_state_dict(S.SEED)


def test_state_dict_is_torchs(sd):
    ref = torch.nn.LSTM(40, 256, 3, batch_first=True).state_dict()
    lin = torch.nn.Linear(256, 256).state_dict()
    want = {**{"lstm." + k: tuple(v.shape) for k, v in ref.items()}, **{"linear." + k: tuple(v.shape) for k, v in lin.items()}}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want == E.state_dict_shapes()
    assert all(v.dtype == np.float32 and np.abs(v).max() <= 1.0 / 16 for v in sd.values())
    big = synth.voice_encoder_state_dict(S.SEED, scale=8.0)
    assert all(np.array_equal(big[k], sd[k] * np.float32(8)) for k in sd)


@pytest.mark.parametrize("N,T", [(1, 1), (3, 2), (2, 160)])
def test_restated_lstm_against_float64_torch(sd, N, T):
    """the restatement's LSTM + linear + norm against torch.nn.LSTM(40, 256, 3, batch_first=True).double() of the same state dict"""
    m = S.mels(N, T)
    lstm = torch.nn.LSTM(40, 256, 3, batch_first=True).double()
    lstm.load_state_dict({k[5:]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("lstm.")})
    lin = torch.nn.Linear(256, 256).double()
    lin.load_state_dict({k[7:]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("linear.")})
    with torch.no_grad():
        out, (hidden, _) = lstm(torch.from_numpy(m).double())
        y = torch.relu(lin(hidden[-1]))
        want = (y / torch.norm(y, dim=1, keepdim=True)).numpy()
    got, hs = R.forward(R.f64(sd), m)
    assert np.abs(hs[2] - out.numpy()).max() <= 1e-12
    assert np.abs(got - want).max() <= 1e-12
    # and the layer-by-layer torch form the GPU gates use is the same network
    got2, hs2 = R.torch_forward(R.f64(sd), m, torch.float64)
    assert np.abs(got2 - want).max() <= 1e-12 and np.abs(hs2[2] - out.numpy()).max() <= 1e-12


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("name", ["L25600", "L31519"])
def test_restated_mel_against_float64_torch_stft(name, pad_mode):
    w = S.wav(name)
    got, want = R.mel(w, pad_mode), R.torch_mel(w, pad_mode, torch.float64)
    assert got.shape == want.shape == (1 + len(w) // 160, 40)
    assert np.abs(got - want).max() <= 1e-12 * want.max()


def test_pad_modes_differ_in_the_edge_frames_only():
    w = S.wav("L25600")                    # frame f covers samples 160 f - 200 .. 160 f + 199: frames 0, 1, 159, 160 reach outside 0 .. 25599
    a, b = R.mel(w, "constant"), R.mel(w, "reflect")
    assert np.array_equal(a[2:-2], b[2:-2])
    for f in (0, 1, -2, -1):
        assert not np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("n,count", [(0, 1), (1, 1), (25600, 1), (31519, 1), (31520, 2), (S.len_for_partials(S.M - 1) - 1, S.M - 2),
                                     (S.len_for_partials(S.M - 1), S.M - 1), (S.len_for_partials(S.M), S.M), (S.len_for_partials(S.M + 1), S.M + 1)])
def test_partial_slices_by_hand(n, count):
    wav_slices, mel_slices = E.VoiceEncoder.compute_partial_slices(n)
    assert len(wav_slices) == len(mel_slices) == count
    for i, (ws, ms) in enumerate(zip(wav_slices, mel_slices)):
        assert (ms.start, ms.stop) == (77 * i, 77 * i + 160) and (ws.start, ws.stop) == (160 * ms.start, 160 * ms.stop)
    assert R.partial_starts(n) == [m.start for m in mel_slices]
    # the library's bounds (what the device tables are sized by) hold for this length
    assert abi.spkenc_max_partials(max(n, 1), 77) >= count
    assert abi.spkenc_frames_ld(max(n, 1), 77) >= 1 + max(n, wav_slices[-1].stop) // 160


def test_partial_slices_coverage_and_rate():
    assert len(E.VoiceEncoder.compute_partial_slices(25600)[0]) == 1            # the second slice would cover 13280 / 25600 = 0.519
    assert len(E.VoiceEncoder.compute_partial_slices(25600, min_coverage=0.5)[0]) == 2
    assert E.frame_step_of(1.3) == 77 and E.frame_step_of(1.0) == 100
    assert len(E.VoiceEncoder.compute_partial_slices(41600, rate=1.0)[0]) == 2
    with pytest.raises(ValueError, match="min_coverage"):
        E.VoiceEncoder.compute_partial_slices(100, min_coverage=0.0)
    with pytest.raises(ValueError, match="rate"):
        E.VoiceEncoder.compute_partial_slices(100, rate=0.1)


def test_loader_names_order_wrapper_and_refusals(sd):
    enc = E.VoiceEncoder.from_checkpoint({"model_state": {k: torch.from_numpy(v) for k, v in sd.items()}, "step": 1})
    assert set(enc.weights) == set(sd) and all(np.array_equal(enc.weights[k], sd[k]) for k in sd)
    assert all(np.array_equal(E.VoiceEncoder().load_state_dict(sd).weights[k], sd[k]) for k in sd)
    missing = {k: v for k, v in sd.items() if k != "lstm.bias_hh_l1"}
    with pytest.raises(KeyError, match="lstm.bias_hh_l1"):
        E.VoiceEncoder.from_checkpoint(missing)
    with pytest.raises(ValueError, match=r"lstm\.weight_ih_l0 is \[1024, 80\].*\[1024, 40\]"):
        E.VoiceEncoder.from_checkpoint({**sd, "lstm.weight_ih_l0": np.zeros((1024, 80), np.float32)})
    with pytest.raises(ValueError, match="pad_mode"):
        E.VoiceEncoder(pad_mode="edge")
    with pytest.raises(abi.DttsError, match="no weights"):
        E.VoiceEncoder().forward(S.mels(1, 1))


def test_gate_order_is_i_f_g_o(sd):
    """swapping two gate blocks of a layer changes the result: the restatement (and so the kernels it gates) reads i, f, g, o"""
    m = S.mels(2, 3)
    base, _ = R.forward(R.f64(sd), m)
    for a, b in ((0, 1), (1, 2), (2, 3)):
        sw = {k: v.copy() for k, v in sd.items()}
        for key in ("lstm.weight_ih_l1", "lstm.weight_hh_l1", "lstm.bias_ih_l1", "lstm.bias_hh_l1"):
            blk = sw[key].reshape((4, 256) + sw[key].shape[1:])
            blk[[a, b]] = blk[[b, a]]
        got, _ = R.forward(R.f64(sw), m)
        assert np.abs(got - base).max() > 1e-6, (a, b)


def test_normalize_volume():
    t = np.arange(16000)
    quiet = (0.001 * np.sin(2 * np.pi * 220 * t / 16000)).astype(np.float32)
    loud = (0.5 * np.sin(2 * np.pi * 220 * t / 16000)).astype(np.float32)
    dbfs = lambda w: 20 * np.log10(np.sqrt(np.mean((w.astype(np.float64) * 32767) ** 2)) / 32767)
    up = E.normalize_volume(quiet, -30, increase_only=True)
    assert abs(dbfs(np.asarray(up)) + 30) < 1e-4
    assert E.normalize_volume(loud, -30, increase_only=True) is not None and np.array_equal(E.normalize_volume(loud, -30, increase_only=True), loud)
    assert abs(dbfs(np.asarray(E.normalize_volume(loud, -30))) + 30) < 1e-4
    with pytest.raises(ValueError):
        E.normalize_volume(loud, -30, increase_only=True, decrease_only=True)
    out = E.preprocess_wav(quiet)                      # no resampling without source_sr: host only
    assert out.dtype == np.float32 and abs(dbfs(out) + 30) < 1e-3
    assert np.array_equal(E.preprocess_wav(loud, source_sr=16000), loud)


def test_trim_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="webrtcvad"):
        E.preprocess_wav(np.zeros(100, np.float32), trim=True)


def test_float16_and_argument_checks(sd):
    """float16 input is accepted up to the device (the first thing that needs one is the context); wrong shapes are refused before it"""
    enc = E.VoiceEncoder.from_checkpoint(sd)
    with pytest.raises(ValueError, match=r"\[N, T, 40\]"):
        enc.forward(np.zeros((2, 3, 41), np.float32))
    with pytest.raises(ValueError, match="lens has 1 entries"):
        enc.embed_batch(np.zeros((2, 100), np.float16), [100])
    if not torch.cuda.is_available():
        with pytest.raises(abi.DttsError, match="needs a ROCm GPU"):
            enc.embed_utterance(np.zeros(100, np.float16))
    a = torch.tensor([[3.0, 4.0], [1.0, 0.0]])
    assert torch.allclose(E.similarity(a, torch.tensor([[3.0, 4.0], [0.0, 1.0]])), torch.tensor([1.0, 0.0]))


def test_argument_block_is_checked_before_the_handle():
    """the refusals of dtts_text2mel_fetch(DTTS_OUT_SPKENC) are reachable without a device: a NULL handle is the last thing looked at"""
    lib = abi.load_library()
    call = lambda a: (lib.dtts_text2mel_fetch(None, abi.OUT_SPKENC, C.byref(a), None), lib.dtts_last_error(None).decode())
    ok = dict(B=1, wav=256, wav_ld=100, embed=256, n_partials=256)
    a = abi.spkenc_args(**ok)
    a.size -= 8
    assert call(a)[0] == -22 and "size" in call(a)[1]
    for bad, word in ((dict(B=0), "B = 0"), (dict(wav_ld=0), "wav_ld = 0"), (dict(mode=2), "mode = 2"), (dict(frame_step=0), "frame_step = 0"),
                      (dict(min_coverage=0.0), "min_coverage"), (dict(pad_mode=3), "pad_mode = 3"), (dict(tile_m=8), "tile_m = 8"),
                      (dict(embed=None), "null"), (dict(wav=258), "not aligned"), (dict(mode=abi.SPKENC_FROM_MELS, lens=256), "lens_dev"),
                      (dict(mode=abi.SPKENC_FROM_MELS, wav_ld=abi.SPKENC_MAX_T + 1), "frames per sequence")):
        rc, msg = call(abi.spkenc_args(**{**ok, **bad}))
        assert rc == -22 and word in msg, (bad, rc, msg)
    a = abi.spkenc_args(**ok)
    a.reserved = 1
    assert call(a)[0] == -22 and "reserved" in call(a)[1]
    rc, msg = call(abi.spkenc_args(**ok))
    assert rc == -22 and "null handle" in msg
    assert C.sizeof(abi.SpkencArgs) == 112
