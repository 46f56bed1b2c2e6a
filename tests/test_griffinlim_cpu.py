"""CPU tests of Griffin-Lim's pieces that need no device: the restatement (tests/griffinlim_ref.py) against the float64 oracle of the
transforms (tests/istft_ref.py) and against the property that makes it Griffin-Lim, ``_mel_to_linear`` and the inverse mel basis against
their definitions, and every argument refusal of ``Spectral.griffin_lim`` / ``vocoder.GriffinLim`` that happens before a context exists."""
import numpy as np
import pytest
import torch

import griffinlim_ref as gr
import istft_ref as ir
from dict_tts_amd import infer, melspec, spectral, vocoder


@pytest.mark.parametrize("name", list(gr.CONFIGS))
def test_restated_transforms_equal_the_oracle(name):
    n_fft, hop, win, T = gr.CONFIGS[name]
    c = gr.case(name, "random")
    w, x = c["window"], c["x"]
    assert len(x) == hop * (T - 1) and 0.2 < float(np.sqrt(np.mean(x.astype(np.float64) ** 2))) < 0.32
    X = gr.stft(x, w, hop).numpy()
    want = ir.stft(x, w, hop)
    assert X.shape == want.shape == (T, n_fft // 2 + 1) and np.max(np.abs(X - want)) <= 1e-12 * np.abs(want).max()
    S = c["A"].astype(np.float64) * c["init"].astype(np.complex128)   # no signal has this spectrum, and its real bins have imaginary parts
    assert np.abs(S[:, 0].imag).max() > 0 and np.abs(S[:, -1].imag).max() > 0
    y = gr.istft(S, w, hop).numpy()
    assert y.shape == (hop * (T - 1),) and np.max(np.abs(y - ir.istft(S, w, hop))) <= 1e-12
    assert gr.istft(S[:1], w, hop).shape == (0,)
    assert np.array_equal(gr.griffin_lim(c["A"], c["init"], w, hop, 0), y)
    # one projection keeps every magnitude and the phase of X; a zero of X takes the phase zero
    X1 = gr.stft(y, w, hop)
    S1 = gr.project(torch.as_tensor(c["A"].astype(np.float64)), X1).numpy()
    assert np.max(np.abs(np.abs(S1) - c["A"])) <= 1e-12 * c["A"].max()
    assert np.max(np.abs(S1 * np.abs(X1.numpy()) - c["A"] * X1.numpy())) <= 1e-12 * c["A"].max() * np.abs(X1.numpy()).max()
    Z = gr.project(torch.as_tensor(np.array([[2.0, 3.0]])), torch.as_tensor(np.array([[0j, -4.0 + 0j]]))).numpy()
    assert np.array_equal(Z, np.array([[2.0 + 0j, -3.0 + 0j]]))
    y1, S1b = gr.griffin_lim(c["A"], c["init"], w, hop, 1, return_spec=True)
    assert np.array_equal(S1b, S1) and np.array_equal(y1, gr.istft(S1, w, hop).numpy())
    # the reference's spelling of the projection is the same function
    y1r = gr.griffin_lim(c["A"], c["init"], w, hop, 1, reference_spelling=True)
    assert np.max(np.abs(y1r - y1)) <= 1e-12


@pytest.mark.parametrize("start,total", [("random", 0.5), ("perturbed", 0.2)])
def test_restatement_has_the_griffin_lim_property(start, total):
    """the consistency || |STFT(y_i)| - A || / || A || falls at every iteration (Griffin & Lim 1984), in both precisions"""
    c = gr.case("n512", start)
    for f in (gr.griffin_lim, gr.griffin_lim_f32):
        d = [gr.consistency(f(c["A"], c["init"], c["window"], c["hop"], i), c["A"], c["window"], c["hop"]) for i in range(9)]
        assert all(b < a for a, b in zip(d, d[1:])), d
        assert d[8] < total * d[0] * 2, d


def test_mel_to_linear_follows_its_definition():
    hp = gr.hparams("n1024")
    P = spectral.inverse_mel_basis(hp, 1024)
    basis = melspec.mel_filterbank(22050, 1024, 80, 80, 7600).astype(np.float32)
    assert P.shape == (513, 80) and P.dtype == np.float32
    assert np.array_equal(P, np.linalg.pinv(basis.astype(np.float64)).astype(np.float32))
    B64, P64 = basis.astype(np.float64), P.astype(np.float64)
    assert np.max(np.abs(B64 @ P64 @ B64 - B64)) <= 1e-6 * np.abs(B64).max()      # Moore-Penrose, within the rounding of P
    assert (P < 0).any()                                                          # which is why _mel_to_linear needs its floor
    rng = np.random.default_rng(0)
    mel = np.clip(rng.normal(-2.0, 1.5, (7, 80)), -5.0, 1.0)
    mel[3] = -5.0                                                                 # the project's floor, log10(1e-5)
    A = gr.mel_to_linear(mel, P)
    want = np.maximum(1e-10, np.dot(P64, (10.0 ** mel).T)).T                      # utils/audio.py:95, on [n_mels, T]
    assert A.shape == (7, 513) and np.max(np.abs(A - want)) <= 1e-12 * want.max()
    assert (A == 1e-10).any() and (A > 1e-10).any()
    with pytest.raises(ValueError, match="fmax = 12000"):
        spectral.inverse_mel_basis({**hp, "fmax": 12000}, 1024)
    with pytest.raises(ValueError, match="audio_num_mel_bins = 200"):
        spectral.inverse_mel_basis({**hp, "audio_num_mel_bins": 200}, 1024)
    with pytest.raises(ValueError, match="needs the hparams fmin"):
        spectral.inverse_mel_basis({**hp, "fmin": None}, 1024)


def test_shim_refuses_bad_arguments_without_a_device():
    sp = spectral.Spectral(gr.hparams("n1024"))
    A = torch.zeros(1, 4, 513)
    with pytest.raises(ValueError, match="exactly one of mag= and mel="):
        sp.griffin_lim()
    with pytest.raises(ValueError, match="exactly one of mag= and mel="):
        sp.griffin_lim(mag=A, mel=torch.zeros(1, 4, 80))
    with pytest.raises(ValueError, match="n_iter = -1"):
        sp.griffin_lim(mag=A, n_iter=-1)
    with pytest.raises(ValueError, match=r"mag must be a float32 cuda tensor \[B, T, 513\]"):
        sp.griffin_lim(mag=A)
    with pytest.raises(ValueError, match=r"mel must be a float32 cuda tensor \[B, T, 80\]"):
        sp.griffin_lim(mel=np.zeros((4, 80), np.float32))
    assert sp.ctx is None and sp.inv_mel_basis is None      # nothing was built for a refused call


def test_plugin_is_built_from_hparams_alone():
    assert vocoder.VOCODERS["GriffinLim"] is vocoder.GriffinLim is vocoder.VOCODERS["griffinlim"]
    assert vocoder.get_vocoder_cls({"vocoder": "dict_tts_amd.vocoder.GriffinLim"}) is vocoder.GriffinLim
    g = vocoder.GriffinLim()                                # no checkpoint, no GPU: the Biaobei defaults
    assert (g.hop, g.n_iter, g.n_mels, g.ctx) == (256, 60, 80, None) and not hasattr(g, "overflowed")
    g = vocoder.GriffinLim({**gr.hparams("n512"), "griffin_lim_iters": 16})
    assert (g.hop, g.n_iter, g.spectral.n_fft) == (128, 16, 512)
    assert vocoder.GriffinLim(n_iter=3).n_iter == 3
    with pytest.raises(ValueError, match="griffin_lim_iters = -2"):
        vocoder.GriffinLim({"griffin_lim_iters": -2})
    with pytest.raises(ValueError, match="fft_size = 768"):
        vocoder.GriffinLim({"fft_size": 768})
    # to_int16 is plain torch: the numpy rule of save_wav (utils/audio.py:11-16), truncation included, per utterance
    g = vocoder.GriffinLim()
    rng = np.random.default_rng(1)
    wav = (0.4 * rng.standard_normal((2, 3 * 256))).clip(-0.99, 0.99).astype(np.float32)
    lens = torch.tensor([2, 3], dtype=torch.int32)
    for norm in (False, True):
        got = g.to_int16(torch.from_numpy(wav), lens, norm=norm).numpy()
        assert got.dtype == np.int16 and not got[0, 2 * 256:].any()
        for b, n in enumerate((2 * 256, 3 * 256)):
            assert np.array_equal(got[b, :n], infer.wav_to_int16(wav[b, :n], norm)), (norm, b)
    assert np.array_equal(g.to_int16(torch.from_numpy(wav)).numpy(), infer.wav_to_int16(wav))
