"""What the fetch units share, on the GPU (run with `-m gpu` on an MI355X).

The library keeps ONE list of workspace arenas; the red-zone mode (dtts_config.debug_redzone) reaches an arena only through it.  The
vocoder's arena is pinned by tests/test_gpu_parity.py; here every unit that needs no weights runs once in a red-zone context of its own,
at the smallest case of its shapes module that reaches the kernels (the pitch and loudness modules also list signals too short for a
frame or a block), and the damage dtts_debug_poke does is found in that unit's workspace.

And ONE table of parts: a part marked "rebuilt by every finalize that names it" takes the tensors loaded last."""
import numpy as np
import pytest
import torch

import dtw_shapes as ds
import losses_shapes as ls
import pitch_shapes as ps
import wavprep_shapes as ws
from dict_tts_amd import abi, dtw, losses, melspec, model, pitch, synth, wavprep

pytestmark = pytest.mark.gpu


def _run_losses(ctx):
    pred, tgt, _ = ls.mel_inputs(min(ls.MEL_CASES, key=lambda c: c["T"]))
    losses.ValidationLosses(hparams={}, ctx=ctx).mel(pred, tgt)


def _run_dtw(ctx):
    x, y = ds.inputs(min(ds.CASES, key=lambda c: c["N"] * c["M"] * c["F"]))
    dtw.DTW(ctx)(x[None], y[None])


def _run_pitch(ctx):
    ex = pitch.PitchAC(ctx)
    c = min((c for c in ps.CASES if c["p"] is ps.P0 and ex.frames(c["L"]) >= 1), key=lambda c: c["L"])
    assert ex(c["x"][None])["f0"].shape[1] >= 1


def _run_loudness(ctx):
    c = min((c for c in ws.LD_CASES if c["kind"] == "ok"), key=lambda c: c["L"])
    wavprep.Loudness(c["rate"], ctx=ctx).measure(c["x"][None])


@pytest.mark.parametrize("workspace,run", [("loss", _run_losses), ("dtw", _run_dtw), ("pitch", _run_pitch), ("loudness", _run_loudness)])
def test_every_unit_workspace_is_enrolled_in_red_zone_mode(workspace, run):
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    try:
        s = torch.cuda.current_stream().cuda_stream
        run(ctx)
        assert ctx.debug_check(s) == 0, ctx.last_error()
        ctx.debug_poke(s)
        assert ctx.debug_check(s) == 1
        assert f" {workspace} workspace buffer #0" in ctx.last_error(), ctx.last_error()
    finally:
        ctx.close()


def test_a_rebuilt_part_takes_the_tensors_loaded_last():
    """PART_MELSPEC finalised twice, with different windows, in the context of a model built from the synthetic weights (a part built
    once and ready beside one that is rebuilt): the second plan is in effect, bit for bit what a fresh context computes with it, and not
    what the first plan computes"""
    first = dict(audio_sample_rate=22050, fft_size=1024, hop_size=256, win_size=1024, audio_num_mel_bins=80, fmin=80, fmax=7600)
    second = {**first, "win_size": 800}
    wav = (0.3 * np.random.default_rng(5).standard_normal((2, 256 * 9 + 77))).astype(np.float32)
    fresh = {}
    for name, hp in (("first", first), ("second", second)):
        ms = melspec.MelSpectrogram(hp)
        fresh[name] = ms(wav)[0].cpu().numpy()
        ms.ctx.close()
    assert not np.array_equal(fresh["first"], fresh["second"])
    m = model.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.dict_tts_state_dict(1234).items()})
    try:
        melspec.MelSpectrogram(first, ctx=m.ctx)
        got = melspec.MelSpectrogram(second, ctx=m.ctx)(wav)[0].cpu().numpy()
        assert np.array_equal(got.view(np.int32), fresh["second"].view(np.int32))
        m.ctx.finalize(abi.PART_ACOUSTIC)   # built once: naming it again rebuilds nothing (its host tensors are gone) and is no error
    finally:
        m.ctx.close()
