"""The acoustic checkpoint's multi-window mel discriminator as a measurement on the device: ``DictTTSTask.build_disc_model()``'s
modules/fastspeech/multi_window_disc.py::Discriminator (windows of 32 / 64 / 128 frames, three 3 x 3 stride-2 Conv2d blocks and a linear
head each), saved by the trainer as ``state_dict['mel_disc']``, and the ``a`` / ``r`` / ``f`` terms of tasks/tts/dict_tts.py::_training_step
(lines 96-118) — computed by dict_tts_amd/csrc/meldisc.hip (dtts_text2mel_fetch(DTTS_OUT_MELDISC)).

The module is evaluated in eval mode: ``Dropout2d`` is the identity, ``disc_norm: bn`` is the affine of its running statistics (eps 0.8:
the second positional argument of ``nn.BatchNorm2d(H, 0.8)``), ``disc_norm: in`` takes instance statistics per (clip, channel) as it does in
training, ``disc_norm: sn`` is ``weight_orig / sigma`` of the stored ``u`` / ``v``.  ``forward`` is the reference's interface (one start per
window shared by the batch); ``scores`` is the measurement: every utterance as if alone at its own length, clips at a fixed hop.  No
gradients; the conditional discriminator (``cond_disc``), which the Dict-TTS task never builds, is refused by name.
"""
import glob
import os
import re

import numpy as np
import torch

from . import abi
from .unit import DeviceUnit
from .discriminators import fold_spectral_norm

WINS = abi.MELDISC_WINS
BN_EPS = 0.8          # nn.BatchNorm2d(out_filters, 0.8): eps, not momentum
NORMS = ("in", "bn", "sn")
# egs/datasets/audio/*/dict_tts.yaml and egs/egs_bases/tts/ps_flow.yaml
HP_DEFAULTS = {"disc_win_num": 3, "mel_disc_hidden_size": 128, "disc_norm": "in", "disc_reduction": "stack", "audio_num_mel_bins": 80}


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def mel_disc_of(path_or_state):
    """a work directory (its newest model_ckpt_steps_*.ckpt), a checkpoint path, a loaded checkpoint, its ``state_dict`` or the ``mel_disc``
    child itself -> the ``mel_disc`` child (flat keys ``discriminator.conv_layers...``); KeyError when the checkpoint carries none"""
    st = path_or_state
    if isinstance(st, (str, bytes)) or hasattr(st, "__fspath__"):
        st = os.fspath(st)
        if os.path.isdir(st):
            ckpts = sorted(glob.glob(f"{st}/model_ckpt_steps_*.ckpt"), key=lambda x: int(re.findall(r"model_ckpt_steps_(\d+)\.ckpt", x)[0]))
            if not ckpts:
                raise FileNotFoundError(f"no model_ckpt_steps_*.ckpt under {st}")
            st = ckpts[-1]
        st = torch.load(st, map_location="cpu", weights_only=False)
    if "state_dict" in st:
        st = st["state_dict"]
    if "mel_disc" in st:
        return st["mel_disc"]
    if any(k.startswith("mel_disc.") for k in st):
        return {k[len("mel_disc."):]: v for k, v in st.items() if k.startswith("mel_disc.")}
    if any(k.startswith(("discriminator.", "cond_disc.")) for k in st):
        return st
    raise KeyError("the checkpoint carries no mel_disc (only Dict-TTS checkpoints saved by the training task do)")


def fold_state_dict(state, dtype=np.float32):
    """``state_dict.mel_disc`` (numpy arrays or tensors) -> the plain weights the library takes (include/dicttts_hip.h, DTTS_PART_MELDISC):
    ``<w>.conv.<l>.{weight,bias}`` (spectral norm folded in its eval form), ``<w>.norm.<l>.{weight,bias}`` (InstanceNorm2d's affine),
    ``<w>.affine.<l>.{scale,shift}`` (BatchNorm2d in eval mode: scale = weight / sqrt(running_var + 0.8), shift = bias - running_mean * scale),
    ``<w>.adv.{weight,bias}``.  dtype=np.float64 folds the float32 parameters in float64, as ``module.double()`` of the reference does."""
    sd = {k: _np(v) for k, v in state.items()}
    for k in sd:
        if k.startswith("cond_disc."):
            raise ValueError(f"mel_disc holds {k}: a conditional discriminator (cond_size > 0), which the Dict-TTS task never builds and this "
                             f"module does not implement")
    out = {}
    w = 0
    while f"discriminator.conv_layers.{w}.adv_layer.weight" in sd:
        src = f"discriminator.conv_layers.{w}"
        for l in range(3):
            c = f"{src}.model.{l}.0"
            if c + ".weight" in sd:
                wt = sd[c + ".weight"].astype(dtype)
            elif c + ".weight_orig" in sd:
                for s in ("weight_u", "weight_v"):
                    if f"{c}.{s}" not in sd:
                        raise KeyError(f"mel_disc lacks {c}.{s}")
                wt = fold_spectral_norm(sd[c + ".weight_orig"], sd[c + ".weight_u"], sd[c + ".weight_v"], dtype)
            else:
                raise KeyError(f"mel_disc lacks {c}.weight (or its weight_orig / weight_u / weight_v)")
            if c + ".bias" not in sd:
                raise KeyError(f"mel_disc lacks {c}.bias")
            out[f"{w}.conv.{l}.weight"] = wt
            out[f"{w}.conv.{l}.bias"] = sd[c + ".bias"].astype(dtype)
            n = f"{src}.model.{l}.3"
            if n + ".running_var" in sd:
                for s in ("weight", "bias", "running_mean"):
                    if f"{n}.{s}" not in sd:
                        raise KeyError(f"mel_disc lacks {n}.{s}")
                scale = sd[n + ".weight"].astype(dtype) / np.sqrt(sd[n + ".running_var"].astype(dtype) + dtype(BN_EPS))
                out[f"{w}.affine.{l}.scale"] = scale.astype(dtype)
                out[f"{w}.affine.{l}.shift"] = (sd[n + ".bias"].astype(dtype) - sd[n + ".running_mean"].astype(dtype) * scale).astype(dtype)
            elif n + ".weight" in sd:
                if n + ".bias" not in sd:
                    raise KeyError(f"mel_disc lacks {n}.bias")
                out[f"{w}.norm.{l}.weight"] = sd[n + ".weight"].astype(dtype)
                out[f"{w}.norm.{l}.bias"] = sd[n + ".bias"].astype(dtype)
        out[f"{w}.adv.weight"] = sd[f"{src}.adv_layer.weight"].astype(dtype)
        if f"{src}.adv_layer.bias" not in sd:
            raise KeyError(f"mel_disc lacks {src}.adv_layer.bias")
        out[f"{w}.adv.bias"] = sd[f"{src}.adv_layer.bias"].astype(dtype)
        w += 1
    if w == 0:
        raise KeyError("mel_disc lacks discriminator.conv_layers.0.adv_layer.weight")
    return out


def describe(weights):
    """the plain weights -> (win_num, hidden, norm, per_row): what the tensor shapes say"""
    n = 0
    while f"{n}.conv.0.weight" in weights:
        n += 1
    H = int(np.shape(weights["0.conv.0.weight"])[0])
    norm = "in" if "0.norm.1.weight" in weights else ("bn" if "0.affine.1.scale" in weights else "sn")
    per_row = int(np.size(weights["0.adv.weight"])) == H * 10
    return n, H, norm, per_row


def check_hparams(hp, weights):
    """-> the four options, from hparams (None: what the tensors say) cross-checked against the tensor shapes; every mismatch and every
    unsupported value is named"""
    n, H, norm, per_row = describe(weights)
    hp = dict(hp or {})
    bins = hp.get("audio_num_mel_bins", 80)
    if int(bins) != abi.MELDISC_MELS:
        raise ValueError(f"audio_num_mel_bins = {bins}: the reference's discriminator is built with freq_length = 80 and its heads are sized for it")
    if n > abi.MELDISC_MAX_WIN:
        raise ValueError(f"mel_disc holds {n} windows; disc_win_num is 1 .. 3 ([32, 64, 128][:n])")
    if H % 32 or not 32 <= H <= abi.MELDISC_MAX_HIDDEN:
        raise ValueError(f"mel_disc_hidden_size = {H} (supported: the multiples of 32 up to {abi.MELDISC_MAX_HIDDEN})")
    want = {"disc_win_num": n, "mel_disc_hidden_size": H}
    for key, have in want.items():
        if key in hp and int(hp[key]) != have:
            raise ValueError(f"{key} = {hp[key]} but the checkpoint's mel_disc has {have}")
    if "disc_win_num" in hp and not 1 <= int(hp["disc_win_num"]) <= 3:
        raise ValueError(f"disc_win_num = {hp['disc_win_num']} (supported: 1 .. 3)")
    if "disc_norm" in hp:
        if hp["disc_norm"] not in NORMS:
            raise ValueError(f"disc_norm = {hp['disc_norm']!r} (supported: 'in', 'bn', 'sn')")
        if hp["disc_norm"] != norm:
            raise ValueError(f"disc_norm = {hp['disc_norm']!r} but the checkpoint's mel_disc holds the tensors of {norm!r}")
    red = hp.get("disc_reduction", "none" if per_row else "stack")
    if red not in abi.MELDISC_REDUCTIONS:
        raise ValueError(f"disc_reduction = {red!r} (supported: 'stack', 'sum', 'none')")
    if (red == "none") != per_row:
        raise ValueError(f"disc_reduction = {red!r} but the checkpoint's adv_layer is {'per time row (none)' if per_row else 'over the whole map (stack / sum)'}")
    for w in range(n):
        size = int(np.size(weights[f"{w}.adv.weight"]))
        need = H * 10 if per_row else H * (WINS[w] // 8) * 10
        if size != need:
            raise ValueError(f"discriminator.conv_layers.{w}.adv_layer.weight has {size} inputs; the {WINS[w]}-frame window's head has {need}")
    return n, H, norm, red


def hop_starts(length, win, hop=None):
    """the measurement's starts of one window: 0, hop, 2 hop, ... <= length - win (hop None: win / 2)"""
    hop = win // 2 if hop is None else int(hop)
    if hop < 1:
        raise ValueError(f"hop = {hop} frames (must be at least 1)")
    return list(range(0, int(length) - win + 1, hop))


def figures(sums, counts, n_win):
    """the library's sums over [2B] signals (recordings, then predictions) -> the reference's figures.  sums f64 [2B, 3, 2], counts i64
    [2B, 3] -> dict: ``r`` = mean (1 - D(mel_g))^2, ``f`` = mean D(mel_p)^2, ``a`` = mean (1 - D(mel_p))^2 as [B, n_win] (NaN where no clip
    of the window fits the utterance); ``<name>_win`` [n_win]: sums over the batch divided by counts over the batch; ``<name>_batch``: the
    mean of those over the windows that have a clip at all (NaN when none has)."""
    T = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    sums, counts = T(sums).to(torch.float64)[:, :n_win], T(counts).to(torch.float64)[:, :n_win]
    B = sums.shape[0] // 2
    out = {}
    for name, sl, q in (("r", slice(0, B), 0), ("f", slice(B, 2 * B), 1), ("a", slice(B, 2 * B), 0)):
        out[name] = sums[sl, :, q] / counts[sl]
        pooled = sums[sl, :, q].sum(0) / counts[sl].sum(0)
        out[name + "_win"] = pooled
        out[name + "_batch"] = pooled[~torch.isnan(pooled)].mean() if bool((~torch.isnan(pooled)).any()) else pooled.sum()
    return out


class MelDiscriminator(DeviceUnit):
    """``MelDiscriminator(weights, reduction)``: plain folded weights (``fold_state_dict``'s names) -> ``forward`` / ``scores``.

    ctx: an existing ``abi.Context`` (e.g. the model's), or None for one of its own; it is created on the first call, so that argument
    errors surface without a GPU."""

    PREFIX, PART = "meldisc", abi.PART_MELDISC

    def __init__(self, weights, reduction=None, hparams=None, ctx=None):
        hp = dict(hparams or {})
        if reduction is not None:
            hp["disc_reduction"] = reduction
        self.win_num, self.hidden, self.norm, self.reduction = check_hparams(hp, weights)
        self.weights = {k: np.ascontiguousarray(np.asarray(v, np.float32)) for k, v in weights.items()}
        self.ctx = ctx

    @classmethod
    def from_checkpoint(cls, path_or_state, hparams=None, ctx=None):
        """a Dict-TTS work directory, checkpoint path, loaded checkpoint, ``state_dict`` or ``mel_disc`` child -> MelDiscriminator.
        hparams: the task's (disc_win_num, mel_disc_hidden_size, disc_norm, disc_reduction, audio_num_mel_bins), cross-checked against the
        tensor shapes; a work directory's config.yaml is read when hparams is None."""
        if hparams is None and isinstance(path_or_state, (str, bytes, os.PathLike)) and os.path.isdir(path_or_state):
            cfg = os.path.join(os.fspath(path_or_state), "config.yaml")
            if os.path.exists(cfg):
                from .vocoder import load_config_chain
                hparams = {k: v for k, v in load_config_chain(cfg).items() if k in HP_DEFAULTS}
        return cls(fold_state_dict(mel_disc_of(path_or_state)), hparams=hparams, ctx=ctx)

    def _check_mel(self, x, what):
        x = torch.as_tensor(x)
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3:
            raise ValueError(f"{what} must be [B, T, 80] (got {tuple(x.shape)})")
        if x.shape[2] != abi.MELDISC_MELS:
            raise ValueError(f"audio_num_mel_bins = {x.shape[2]}: the reference's discriminator is built with freq_length = 80")
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{what} is empty: {tuple(x.shape)}")
        return x

    def _run(self, mel, lens, starts, clips_ld, flags, hop=(0, 0, 0), hidden=False):
        """mel [n, T, 80] on the device, lens i32 [n] device or None, starts i32 [n_win, n, clips_ld] device or None -> raw outputs"""
        ctx, dev = self._context(), self.device
        n, T = mel.shape[0], mel.shape[1]
        if n > 65535 or T > (1 << 20) or n * clips_ld > (1 << 24):
            raise ValueError(f"{n} signals of {T} frames with {clips_ld} clips each (supported: 65535 signals, 2^20 frames, 2^24 clips per window)")
        out = {"sums": torch.full((n, 3, 2), float("nan"), dtype=torch.float64, device=dev),
               "counts": torch.zeros((n, 3), dtype=torch.int64, device=dev),
               "status": torch.zeros(n, dtype=torch.int32, device=dev),
               "d": torch.full((self.win_num, n, clips_ld, abi.MELDISC_D_LD), float("nan"), dtype=torch.float32, device=dev)}
        h = [None] * 9
        if hidden:
            out["h"] = []
            for w in range(self.win_num):
                for l in range(3):
                    t = torch.full((n, clips_ld, WINS[w] >> (l + 1), 80 >> (l + 1), self.hidden), float("nan"), dtype=torch.float32, device=dev)
                    out["h"].append(t)
                    h[3 * w + l] = t.data_ptr()
        ptr = lambda t: None if t is None else t.data_ptr()
        ctx.meldisc(n, torch.cuda.current_stream().cuda_stream, mel=mel.data_ptr(), T_ld=T, n_win=self.win_num, clips_ld=clips_ld, sums=out["sums"].data_ptr(),
                    counts=out["counts"].data_ptr(), status=out["status"].data_ptr(), reduction=abi.MELDISC_REDUCTIONS[self.reduction], flags=flags,
                    hop=hop, lens=ptr(lens), starts=ptr(starts), d=out["d"].data_ptr(), h=h)
        return out

    # -- the reference's interface -----------------------------------------------------------------------------
    def forward(self, x, start_frames_wins=None):
        """Discriminator.forward(x, start_frames_wins=...) in eval mode.  x [B, T, 80] (padding: zero frames).  -> {'y', 'h',
        'start_frames_wins'} with the reference's shapes: y [B, 1, n_win] (stack), [B, 1] (sum) or [B, sum win / 8] (none), None when
        some window is longer than the longest utterance; h: the outputs of the three blocks of every window that ran, [B, H, t, f];
        start_frames_wins: per window a list of B equal starts (None where the window did not fit).  x_len is the number of frames
        whose bins do not sum to 0; without start_frames_wins one start per window is drawn with numpy.random.randint(0, x_len.max() -
        win + 1), as ``clip`` draws it."""
        x = self._check_mel(x, "x")
        B, T = x.shape[0], x.shape[1]
        if start_frames_wins is None:
            start_frames_wins = [None] * self.win_num
        start_frames_wins = list(start_frames_wins)
        if len(start_frames_wins) < self.win_num:
            raise ValueError(f"start_frames_wins has {len(start_frames_wins)} entries for {self.win_num} windows")
        x_len_max = int(torch.as_tensor(x).sum(-1).ne(0).sum(-1).max())
        starts = np.full((self.win_num, B, 1), -1, np.int32)
        ran = []
        for w in range(self.win_num):
            t_end = x_len_max - WINS[w]
            if t_end < 0:
                continue
            if start_frames_wins[w] is None:
                start_frames_wins[w] = [int(np.random.randint(low=0, high=t_end + 1))] * B
            s = int(start_frames_wins[w][0])
            if s < 0 or s + WINS[w] > T:
                raise ValueError(f"start_frames_wins[{w}] = {s}: a {WINS[w]}-frame clip from there leaves the {T} frames of x")
            starts[w] = s
            ran.append(w)
        ret = {"y": None, "h": [], "start_frames_wins": start_frames_wins}
        if not ran:
            return ret
        self._context()
        xd = x.to(device=self.device, dtype=torch.float32).contiguous()
        raw = self._run(xd, None, torch.from_numpy(starts).to(self.device), 1, 0, hidden=True)
        for w in ran:
            for l in range(3):
                ret["h"].append(raw["h"][3 * w + l][:, 0].permute(0, 3, 1, 2))
        if len(ran) != self.win_num:
            return ret
        d = raw["d"][:, :, 0]                                   # [n_win, B, 16]
        if self.reduction == "stack":
            ret["y"] = d[:, :, 0].permute(1, 0)[:, None, :].contiguous()
        elif self.reduction == "sum":
            y = d[0, :, 0]
            for w in range(1, self.win_num):
                y = y + d[w, :, 0]
            ret["y"] = y[:, None]
        else:
            ret["y"] = torch.cat([d[w, :, :WINS[w] // 8] for w in range(self.win_num)], dim=-1)
        return ret

    __call__ = forward

    # -- the measurement ---------------------------------------------------------------------------------------
    def scores(self, mel_g, mel_p, lens=None, hop=None, starts=None, return_d=False):
        """mel_g (recordings), mel_p (predictions) [B, T, 80] float32, lens [B] valid frames of both or None (= T).  Every utterance is
        scored as if alone at its own length: for window w the clips start at 0, hop, 2 hop, ... <= len - win (hop: None = win / 2, an int,
        or one per window); ``starts`` (per window a list of starts, applied to every utterance; a start whose clip leaves the utterance
        is skipped) overrides hop.  Nothing behind an utterance's length is read.  -> dict of float64 device tensors ``r``, ``f``, ``a``
        [B, n_win] (NaN where no clip fits), ``<name>_win`` [n_win] and ``<name>_batch`` (sums and counts pooled over the batch, not means
        of means), the raw ``sums`` [2B, 3, 2], ``counts`` [2B, 3] and ``status`` [2B]; return_d=True adds ``d`` f32 [n_win, 2B, clips, 16]
        (NaN where there is no clip) and ``clip_starts``."""
        g, p = self._check_mel(mel_g, "mel_g"), self._check_mel(mel_p, "mel_p")
        if g.shape != p.shape:
            raise ValueError(f"mel_g and mel_p must have one shape (got {tuple(g.shape)} and {tuple(p.shape)})")
        B, T = g.shape[0], g.shape[1]
        if lens is not None:
            lens = torch.as_tensor(lens).reshape(-1)
            if lens.shape[0] != B:
                raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
            if not lens.is_cuda:
                for b, n in enumerate(lens.tolist()):
                    if n < 0 or n > T:
                        raise ValueError(f"lens[{b}] = {n} frames for mels of {T}")
        hops = [0, 0, 0]
        st = None
        if starts is not None:
            if len(starts) < self.win_num:
                raise ValueError(f"starts has {len(starts)} entries for {self.win_num} windows")
            clips_ld = max(1, max(len(starts[w]) for w in range(self.win_num)))
            arr = np.full((self.win_num, 2 * B, clips_ld), -1, np.int32)
            for w in range(self.win_num):
                for j, s in enumerate(starts[w]):
                    if int(s) < 0:
                        raise ValueError(f"starts[{w}][{j}] = {s}")
                    arr[w, :, j] = int(s)
            st = arr
        else:
            per = [hop] * self.win_num if hop is None or np.isscalar(hop) else list(hop)
            clips_ld = 1
            for w in range(self.win_num):
                hops[w] = WINS[w] // 2 if per[w] is None else int(per[w])
                clips_ld = max(clips_ld, len(hop_starts(T, WINS[w], hops[w])))
        self._context()
        dev = self.device
        mel = torch.cat([g.to(device=dev, dtype=torch.float32), p.to(device=dev, dtype=torch.float32)], dim=0).contiguous()
        ld = None if lens is None else torch.cat([lens, lens]).to(device=dev, dtype=torch.int32).contiguous()
        raw = self._run(mel, ld, None if st is None else torch.from_numpy(st).to(dev), clips_ld, abi.MELDISC_WITHIN_LEN, hop=hops)
        out = {"sums": raw["sums"], "counts": raw["counts"], "status": raw["status"]}
        out.update(figures(raw["sums"], raw["counts"], self.win_num))
        if return_d:
            out["d"] = raw["d"]
        return out
