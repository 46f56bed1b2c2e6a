"""The acoustic model's validation losses on the device: what the reference's ``DictTTSTask.validation_step`` reports
(tasks/tts/dict_tts.py:44-79,127-136) for the teacher-forced posterior pass of ``dict_tts_amd.model.PortaSpeech_dict`` —

  * the masked mel losses of ``mel_loss: "ssim:0.5|l1:0.5"`` (tasks/tts/tts_base.py:182-222, modules/commons/ssim.py),
  * the word-duration losses ``wdur`` / ``sdur`` of add_dur_loss in eval mode (tasks/tts/ps_flow.py:99-139),
  * ``kl * lambda_kl`` clamped at 0.002, and ``total_loss``

— computed by dict_tts_amd/csrc/losses.hip (dtts_text2mel_fetch(DTTS_OUT_LOSSES)): no ``F.conv2d``, nothing leaves the device, no gradients.
The SSIM window moments and the quotient are fp64 (the reference's float32 path forms E[x^2] - E[x]^2 of values near 6 against
C2 = 9e-4); every sum is fp64 in a fixed order.

Masking is the reference's: a frame counts iff its TARGET row is not all zero (``weights_nonzero_speech``), and the SSIM image is the batch
tensor as given: zero outside [0, T) x [0, n_mel), pad rows inside read as they are.  An utterance's sums therefore depend on the batch's
T, not on what else the batch holds.
"""
from math import exp

import numpy as np
import torch

from . import abi
from . import hparams as hparams_mod
from .unit import DeviceUnit

SSIM_WINDOW, SSIM_SIGMA, SSIM_BIAS = 11, 1.5, 6.0
KL_FLOOR = 0.002   # tasks/tts/dict_tts.py:74
# egs/egs_bases/tts/ps_flow.yaml:56-62 (the Dict-TTS configs inherit them)
LOSS_DEFAULTS = {"mel_loss": "ssim:0.5|l1:0.5", "lambda_kl": 1.0, "lambda_sent_dur": 0.0, "dur_scale": "log", "dur_level": "word"}


def ssim_window():
    """create_window(11, 1) of modules/commons/ssim.py as float32 [11, 11]: the Gaussian of sigma 1.5 evaluated in double and stored as
    float32, divided by its float32 sum, then the float32 outer product.  (The sum is the correctly rounded one, which is what torch's
    reduction returns for these eleven values; tests/golden/g13_losses.npz holds the reference's own window.)"""
    g = np.array([exp(-(x - SSIM_WINDOW // 2) ** 2 / float(2 * SSIM_SIGMA ** 2)) for x in range(SSIM_WINDOW)], np.float32)
    g = g / np.float32(g.astype(np.float64).sum())
    return (g[:, None] * g[None, :]).astype(np.float32)


def parse_mel_loss(spec):
    """``hparams['mel_loss']`` -> {name: lambda} by the rule of tasks/tts/tts_base.py:57-67 ("ssim:0.5|l1:0.5"; a name without a weight
    gets 1.0; empty items are skipped).  ``gdl`` is not implemented; any other unknown name is refused (the reference would fail later,
    in add_mel_loss)."""
    out = {}
    for item in str(spec).split("|"):
        if item == "":
            continue
        if ":" in item:
            name, lbd = item.split(":")
            lbd = float(lbd)
        else:
            name, lbd = item, 1.0
        if name == "gdl":
            raise NotImplementedError("mel_loss 'gdl' (the gradient difference loss) is not implemented on the MI355X path")
        if name not in ("l1", "mse", "ssim"):
            raise ValueError(f"mel_loss {name!r}: the reference's add_mel_loss knows l1, mse, ssim and gdl")
        out[name] = lbd
    return out


def _ratio(num, den):
    return num / den   # 0 / 0 = NaN, as the reference's masked means give it


class ValidationLosses(DeviceUnit):
    """mel(), dur(), run_model(), validation_step(): the reference's eval-mode loss figures, as float64 cuda tensors.

    hparams: the reference's keys mel_loss, lambda_kl, lambda_sent_dur, dur_scale, dur_level (None: the global hparams when set, else
    the ps_flow.yaml values).  ctx: an existing ``abi.Context`` (e.g. the model's), or None for one of its own; it is created on the
    first call, so that argument errors surface without a GPU.  mel_disc: an optional ``mel_discriminator.MelDiscriminator`` (the
    checkpoint's own multi-window discriminator); with it validation_step also reports ``a`` / ``r`` / ``f``, the adversarial terms of
    ``_training_step`` (tasks/tts/dict_tts.py:96-118), outside total_loss, which stays the reference's validation total.  Without it every
    output is what it was."""

    def __init__(self, hparams=None, ctx=None, mel_disc=None):
        if hparams is None:
            hparams = hparams_mod.hparams or {}
        hp = {**LOSS_DEFAULTS, **{k: v for k, v in dict(hparams).items() if k in LOSS_DEFAULTS}}
        self.loss_and_lambda = parse_mel_loss(hp["mel_loss"])
        self.lambda_kl = float(hp["lambda_kl"])
        self.lambda_sent_dur = float(hp["lambda_sent_dur"])
        if hp["dur_scale"] not in ("log", "linear"):
            raise ValueError(f"dur_scale = {hp['dur_scale']!r} (supported: 'log', 'linear')")
        self.dur_scale = hp["dur_scale"]
        if hp["dur_level"] != "word":
            raise NotImplementedError(f"dur_level = {hp['dur_level']!r}: only word-level durations are implemented (Dict-TTS has no phoneme durations)")
        if self.lambda_sent_dur > 0 and self.dur_scale != "linear":
            raise ValueError("lambda_sent_dur > 0 needs dur_scale = 'linear' (the reference asserts it, tasks/tts/ps_flow.py:111)")
        self.ctx = ctx
        self.mel_disc = mel_disc

    # -- the two halves ------------------------------------------------------------------------------------
    def mel(self, mel_out, target, bias=SSIM_BIAS, ssim_map=False):
        """mel_out, target: [B, T, n_mel] float32 (n_mel 1 .. 128).  -> dict of float64 cuda tensors: l1, mse, ssim (the reference's batch
        figures, sum_b sums / sum_b count), l1_utt, mse_utt, ssim_utt [B] (NaN for an utterance whose target is all zero), sums [B, 3]
        (sum w |p - t|, sum w (p - t)^2, sum w (1 - ssim)) and count [B] int64; with ssim_map=True also ssim_map [B, T, n_mel] float32,
        the unweighted map."""
        mel_out, target = torch.as_tensor(mel_out), torch.as_tensor(target)
        if mel_out.dim() != 3 or mel_out.shape != target.shape:
            raise ValueError(f"mel_out and target must both be [B, T, n_mel] (got {tuple(mel_out.shape)} and {tuple(target.shape)})")
        B, T, n_mel = mel_out.shape
        if B < 1 or T < 1:
            raise ValueError(f"B = {B}, T = {T}: an empty batch has no losses")
        if not 1 <= n_mel <= 128:
            raise ValueError(f"n_mel = {n_mel} (supported: 1 .. 128)")
        ctx = self._context()
        dev = self.device
        p = mel_out.to(device=dev, dtype=torch.float32).contiguous()
        t = target.to(device=dev, dtype=torch.float32).contiguous()
        sums = torch.empty(B, 3, dtype=torch.float64, device=dev)
        count = torch.empty(B, dtype=torch.int64, device=dev)
        smap = torch.empty(B, T, n_mel, dtype=torch.float32, device=dev) if ssim_map else None
        ctx.losses(B, torch.cuda.current_stream().cuda_stream, pred=p.data_ptr(), tgt=t.data_ptr(), T=T, n_mel=n_mel, mel_sums=sums.data_ptr(),
                   mel_count=count.data_ptr(), bias=bias, ssim_map=None if smap is None else smap.data_ptr())
        out = mel_figures(sums, count)
        if smap is not None:
            out["ssim_map"] = smap
        return out

    def dur(self, dur_pred, mel2word, word_lengths, dur_scale=None):
        """dur_pred [B, T_w] float32 (ret['dur']: log domain for dur_scale 'log'), mel2word [B, T_mel] int64 (1-based word per frame, 0 =
        padding), word_lengths [B].  -> dict: wdur (the eval form: over the words whose doubly-logged ground truth is > 0), sdur (mean
        over the batch of the sentence-level difference), wdur_train (the training-mode form, over the words within word_lengths), float64
        cuda scalars; sums [B, 5]; dur_gt [B, T_w] int32, the frames per word."""
        scale = self.dur_scale if dur_scale is None else dur_scale
        if scale not in ("log", "linear"):
            raise ValueError(f"dur_scale = {scale!r} (supported: 'log', 'linear')")
        dur_pred, mel2word, word_lengths = torch.as_tensor(dur_pred), torch.as_tensor(mel2word), torch.as_tensor(word_lengths)
        if dur_pred.dim() != 2 or mel2word.dim() != 2 or mel2word.shape[0] != dur_pred.shape[0]:
            raise ValueError(f"dur_pred must be [B, T_w] and mel2word [B, T_mel] (got {tuple(dur_pred.shape)} and {tuple(mel2word.shape)})")
        B, T_w = dur_pred.shape
        if word_lengths.reshape(-1).shape[0] != B:
            raise ValueError(f"word_lengths has {word_lengths.numel()} entries for a batch of {B}")
        if B < 1 or not 1 <= T_w <= abi.LOSS_MAX_WORDS:
            raise ValueError(f"B = {B}, T_w = {T_w} (supported: B >= 1, T_w in 1 .. {abi.LOSS_MAX_WORDS})")
        ctx = self._context()
        dev = self.device
        dp = dur_pred.to(device=dev, dtype=torch.float32).contiguous()
        m2w = mel2word.to(device=dev, dtype=torch.int64).contiguous()
        wl = word_lengths.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        sums = torch.empty(B, 5, dtype=torch.float64, device=dev)
        gt = torch.empty(B, T_w, dtype=torch.int32, device=dev)
        ctx.losses(B, torch.cuda.current_stream().cuda_stream, dur_pred=dp.data_ptr(), mel2word=m2w.data_ptr() if m2w.numel() else None,
                   word_len=wl.data_ptr(), T_w=T_w, T_mel=m2w.shape[1], dur_scale=0 if scale == "log" else 1, dur_sums=sums.data_ptr(),
                   dur_gt=gt.data_ptr())
        out = dur_figures(sums)
        out["dur_gt"] = gt
        return out

    # -- the task's eval-mode run_model / validation_step --------------------------------------------------
    def run_model(self, model, sample):
        """DictTTSTask.run_model(model, sample, return_output=True) in eval mode (tasks/tts/dict_tts.py:44-79) for this repository's
        ``PortaSpeech_dict``, under torch.no_grad(): -> (losses, output).  losses: kl = clamp(kl * lambda_kl, min=0.002), every mel
        loss of ``mel_loss`` times its lambda, wdur and sdur (the eval forms).  sample: the collater's keys word_tokens, pron_modified,
        mel2word, word_lengths, keys, values, key_map, pinyin, pinyin_map, mels, and spk_embed / spk_ids when the model has speakers;
        one extra key, eps, is handed to the posterior pass as its noise."""
        use_spk_id = bool(getattr(model, "hparams", {}).get("use_spk_id", False))
        spk = sample.get("spk_embed") if not use_spk_id else sample.get("spk_ids")
        with torch.no_grad():
            output = model((sample["word_tokens"], sample.get("txt_tokens")), sample["pron_modified"], (None, None, None),
                           ph2word=sample.get("ph2word"), word_len=torch.as_tensor(sample["word_lengths"]).max(),
                           dict_msg=(sample["keys"], sample["values"], sample["key_map"], sample["pinyin"], sample["pinyin_map"]),
                           mel2word=sample["mel2word"], mel2ph=sample.get("mel2ph"), tgt_mels=sample["mels"], spk_embed=spk, infer=False,
                           forward_post_glow=False, two_stage=True, eps=sample.get("eps"))
        losses = {"kl": torch.clamp(output["kl"].to(torch.float64) * self.lambda_kl, min=KL_FLOOR)}
        m = self.mel(output["mel_out"], sample["mels"])
        for name, lbd in self.loss_and_lambda.items():
            losses[name] = m[name] * lbd
        d = self.dur(output["dur"], sample["mel2word"], sample["word_lengths"])
        losses["wdur"] = d["wdur"]
        losses["sdur"] = d["sdur"]
        return losses, output

    def adversarial(self, mel_out, target, mel_lengths=None):
        """the checkpoint's discriminator on the predicted mels next to the recordings': ``MelDiscriminator.scores(target, mel_out, lens)``
        (clips at hop win / 2, every utterance at its own length; ``a_batch`` / ``r_batch`` / ``f_batch`` are what validation_step reports).
        mel_lengths None: the frames of the target whose bins are not all zero, as the mel losses mask them."""
        if self.mel_disc is None:
            raise ValueError("ValidationLosses was built without mel_disc=")
        target = torch.as_tensor(target)
        if mel_lengths is None:
            mel_lengths = target.abs().sum(-1).ne(0).sum(-1)
        return self.mel_disc.scores(target, torch.as_tensor(mel_out), mel_lengths)

    def validation_step(self, model, sample):
        """-> {'losses': {name: float}, 'total_loss': float, 'nsamples': sample['nsamples'] (or the batch size)}: the first half of
        DictTTSTask.validation_step (tasks/tts/dict_tts.py:127-136), scalars on the host as utils.tensors_to_scalars leaves them"""
        losses, output = self.run_model(model, sample)
        vals = torch.stack([v.reshape(()) for v in losses.values()]).cpu().tolist()   # one device-to-host copy
        out = {"losses": dict(zip(losses.keys(), vals)), "total_loss": float(sum(vals))}
        if self.mel_disc is not None:
            adv = self.adversarial(output["mel_out"], sample["mels"], sample.get("mel_lengths"))
            out["losses"].update(zip(("a", "r", "f"), torch.stack([adv[k + "_batch"] for k in ("a", "r", "f")]).cpu().tolist()))
        n = sample.get("nsamples")
        out["nsamples"] = int(n) if n is not None else int(torch.as_tensor(sample["word_tokens"]).shape[0])
        return out


def mel_figures(sums, count):
    """sums [B, 3] float64 and count [B] int64 as the library returns them -> the figures ValidationLosses.mel documents"""
    sums, count = torch.as_tensor(sums, dtype=torch.float64), torch.as_tensor(count, dtype=torch.int64)
    cnt = count.to(torch.float64)
    tot, n = sums.sum(dim=0), cnt.sum()
    out = {"sums": sums, "count": count}
    for i, name in enumerate(("l1", "mse", "ssim")):
        out[name] = _ratio(tot[i], n)
        out[name + "_utt"] = _ratio(sums[:, i], cnt)
    return out


def dur_figures(sums):
    """sums [B, 5] float64 as the library returns them -> wdur (eval), sdur, wdur_train"""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    tot = sums.sum(dim=0)
    return {"wdur": _ratio(tot[2], tot[3]), "sdur": sums[:, 4].abs().mean(), "wdur_train": _ratio(tot[0], tot[1]), "sums": sums}
